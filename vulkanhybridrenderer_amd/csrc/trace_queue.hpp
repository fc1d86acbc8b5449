// The work-queue machinery of the ray-tracing units: the node step's instruction wrappers and packed slab tests, the shared descent of a
// tile ("the cut"), the cost ordering of a launch's blocks, one pass of a wave over its ray queue (wave_queue_walk<>) and what the queue
// kernels' launchers share on the host.  Device and host helpers only: no kernel and no launcher lives here.  (Until the ray-tracing unit
// was split by render path these were three stretches of kernels_trace.hip.)
#pragma once

#include <algorithm>
#include <type_traits>

#include "trace_device.hpp"

namespace vhr {

// Slab test of one child box, (lo, hi) pairs per axis, as three packed FMAs against precomputed 1/d and -o/d.
// Box tests only cull (boxes are padded, NaNs drop out of min/max), so they are outside the exact-arithmetic
// contract: 1/d may come from v_rcp_f32 and the FMA may round differently from (lo - o) * inv without changing
// any result.
typedef float f2v __attribute__((ext_vector_type(2)));

// v_min / v_max / v_min3 / v_max3 spelled as instructions: fminf / fmaxf lower to llvm.minnum / maxnum, which under the
// kernel's IEEE mode get a canonicalising v_max_f32 x, x, x in front of every operand the compiler cannot prove quiet
// (14 extra instructions per node here).  The hardware ops already return the non-NaN operand, which is all the
// cull needs (and no NaN can arise: see cull_reciprocal).
__device__ __forceinline__ float hw_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float hw_max(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float hw_min3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float hw_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// A comparison as the 64-bit lane mask it is, and a select on such a mask.  Spelled out because a ballot of a bool the compiler holds as a
// lane mask comes back through a vector register when it is handed to an asm statement (v_cndmask 0 / 1 + v_cmp_ne: two instructions per
// mask, four per node visit, r5); masks combine on the scalar unit.  (Lanes that are switched off read 0.)
__device__ __forceinline__ unsigned long long cmp_le_mask(float a, float b) { unsigned long long m; asm("v_cmp_le_f32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b)); return m; }
__device__ __forceinline__ unsigned long long cmp_gt_i32_mask_s(int uniform_a, int b) { unsigned long long m; asm("v_cmp_gt_i32_e64 %0, %1, %2" : "=s"(m) : "s"(uniform_a), "v"(b)); return m; }
__device__ __forceinline__ unsigned long long cmp_eq_i32_mask_s(int uniform_a, int b) { unsigned long long m; asm("v_cmp_eq_i32_e64 %0, %1, %2" : "=s"(m) : "s"(uniform_a), "v"(b)); return m; }
__device__ __forceinline__ int select_mask(int if_clear, int if_set, unsigned long long m) { int d; asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(d) : "v"(if_clear), "v"(if_set), "s"(m)); return d; }

__device__ __forceinline__ bool box_test_pk(f2v bx, f2v by, f2v bz, f3 inv, f3 noi, float tmin, float tlimit, float &tnear) {
    const f2v tx = __builtin_elementwise_fma(bx, f2v{ inv.x, inv.x }, f2v{ noi.x, noi.x });
    const f2v ty = __builtin_elementwise_fma(by, f2v{ inv.y, inv.y }, f2v{ noi.y, noi.y });
    const f2v tz = __builtin_elementwise_fma(bz, f2v{ inv.z, inv.z }, f2v{ noi.z, noi.z });
    const float tn = hw_max3(hw_min(tx.x, tx.y), hw_min(ty.x, ty.y), hw_max(hw_min(tz.x, tz.y), tmin));
    const float tf = hw_min3(hw_max(tx.x, tx.y), hw_max(ty.x, ty.y), hw_min(hw_max(tz.x, tz.y), tlimit));
    tnear = tn;
    return tn <= tf;
}

constexpr int kQueueBlock = 64;
constexpr int kStackSentinel = int(0x80000000u);   // not a node (>= 0) and not a leaf code the builder can emit
constexpr int kReflRays = 128;                      // rays of a wave's queue in the kernels whose waves own a 16x8-pixel tile

// One box in centre / half-extent form (a cut entry, build_tile_cut) against one ray: `ainv` = |1/d|.  The three centre terms are one packed
// FMA + one plain one, an axis's (near, far) pair is ONE packed FMA (-h and +h through neg_lo on the same register) that needs no min / max:
// 5 FMAs + 4 min / max + the compare instead of box_test_pk's 3 + 10 + 1.  Culling only: the box is the (lo, hi) box grown by a few ulp.
__device__ __forceinline__ unsigned long long box_test_ch1(float cx, float cy, float cz, float hx, float hy, float hz, f3 inv, f3 ainv, f3 noi, float tmin, float tlimit) {
    const f2v cxy = __builtin_elementwise_fma(f2v{ cx, cy }, f2v{ inv.x, inv.y }, f2v{ noi.x, noi.y });
    const float ciz = __builtin_fmaf(cz, inv.z, noi.z);
    const f2v x = __builtin_elementwise_fma(f2v{ -hx, hx }, f2v{ ainv.x, ainv.x }, f2v{ cxy.x, cxy.x });
    const f2v y = __builtin_elementwise_fma(f2v{ -hy, hy }, f2v{ ainv.y, ainv.y }, f2v{ cxy.y, cxy.y });
    const f2v z = __builtin_elementwise_fma(f2v{ -hz, hz }, f2v{ ainv.z, ainv.z }, f2v{ ciz, ciz });
    const float tn = hw_max3(x.x, y.x, hw_max(z.x, tmin));
    const float tf = hw_min3(x.y, y.y, hw_min(z.y, tlimit));
    return cmp_le_mask(tn, tf);
}

// A refilled ray against the tile's cut (build_tile_cut): the subtrees it hits go on its (empty) stack, the deepest -- the one closest to the
// origins -- on top; those that do not fit the LDS levels are remembered in `emask`.  Written without branches like the node step: the link is
// stored above the top whatever the test says (a slot above the top may hold anything) and the test's mask is the carry that moves the top.
// 13 vector instructions per entry (r5; 19 with box_test_pk and a predicated push); the masks are lane masks in scalar registers (cmp_le_mask).  Ends with the top entry popped into `cur`.
__device__ __forceinline__ void cut_to_stack(const float4 (*cut)[2], const uint32_t cut_n, int *stack, const uint32_t stack_levels, f3 inv, f3 noi, float tmin_v, float tlimit,
                                             int &cur, int &sp, uint32_t &emask) {
    const f3 ainv = f3{ fabsf(inv.x), fabsf(inv.y), fabsf(inv.z) };
    emask = 0;
    sp = 0;
    for (uint32_t e = 0; e < cut_n; ++e) {
        const float4 b0 = cut[e][0], b1 = cut[e][1];              // (cx, cy, cz, hx), (hy, hz, link, -): LDS broadcasts
        const unsigned long long hit = box_test_ch1(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, inv, ainv, noi, tmin_v, tlimit);
        const unsigned long long fits = cmp_gt_i32_mask_s(int(stack_levels) - 2, sp);          // sp + 2 < stack_levels (so sp + 1 <= stack_levels - 1: the store below stays inside the lane's rows)
        stack[(uint32_t(sp) + 1u) * kQueueBlock] = __float_as_int(b1.z);
        {
            unsigned long long carry_out;
            asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(sp), "=s"(carry_out) : "v"(sp), "s"(hit & fits));
        }
        if (hit & ~fits) emask = uint32_t(select_mask(int(emask), int(emask | (1u << e)), hit & ~fits));      // (wave-uniform and rare: a ray that hits more entries than the LDS levels hold)
    }
    if (sp > 0) { cur = stack[uint32_t(sp) * kQueueBlock]; --sp; } else cur = kStackSentinel;
}

// Both child boxes of a centre / half-extent node (BvhNodeCH) against one ray: `ainv` = |1/d|.  The centre terms of the two boxes
// share one packed FMA per axis; a box's (near, far) pair of an axis is ONE packed FMA (-h and +h through neg_lo on the same
// register), so no per-axis min / max is needed: 9 FMAs + 8 min / max per node instead of 6 + 20.  Culling only (see BvhNodeCH).
template <typename V4>
__device__ __forceinline__ void box_pair_ch(const V4 q0, const V4 q1, const V4 q2, f3 inv, f3 ainv, f3 noi, float tmin, float tlimit,
                                            float &tn0, float &tn1, float &tf0, float &tf1) {
    const f2v cix = __builtin_elementwise_fma(f2v{ q0.x, q0.y }, f2v{ inv.x, inv.x }, f2v{ noi.x, noi.x });
    const f2v ciy = __builtin_elementwise_fma(f2v{ q0.z, q0.w }, f2v{ inv.y, inv.y }, f2v{ noi.y, noi.y });
    const f2v ciz = __builtin_elementwise_fma(f2v{ q1.x, q1.y }, f2v{ inv.z, inv.z }, f2v{ noi.z, noi.z });
    const f2v x0 = __builtin_elementwise_fma(f2v{ -q1.z, q1.z }, f2v{ ainv.x, ainv.x }, f2v{ cix.x, cix.x });
    const f2v y0 = __builtin_elementwise_fma(f2v{ -q1.w, q1.w }, f2v{ ainv.y, ainv.y }, f2v{ ciy.x, ciy.x });
    const f2v z0 = __builtin_elementwise_fma(f2v{ -q2.x, q2.x }, f2v{ ainv.z, ainv.z }, f2v{ ciz.x, ciz.x });
    const f2v x1 = __builtin_elementwise_fma(f2v{ -q2.y, q2.y }, f2v{ ainv.x, ainv.x }, f2v{ cix.y, cix.y });
    const f2v y1 = __builtin_elementwise_fma(f2v{ -q2.z, q2.z }, f2v{ ainv.y, ainv.y }, f2v{ ciy.y, ciy.y });
    const f2v z1 = __builtin_elementwise_fma(f2v{ -q2.w, q2.w }, f2v{ ainv.z, ainv.z }, f2v{ ciz.y, ciz.y });
    tn0 = hw_max3(x0.x, y0.x, hw_max(z0.x, tmin));
    tn1 = hw_max3(x1.x, y1.x, hw_max(z1.x, tmin));
    tf0 = hw_min3(x0.y, y0.y, hw_min(z0.y, tlimit));
    tf1 = hw_min3(x1.y, y1.y, hw_min(z1.y, tlimit));
}
template <typename V4>
__device__ __forceinline__ void box_pair_ch(const V4 q0, const V4 q1, const V4 q2, f3 inv, f3 ainv, f3 noi, float tmin, float tlimit,
                                            bool &h0, bool &h1, float &tn0, float &tn1) {
    float tf0, tf1;
    box_pair_ch(q0, q1, q2, inv, ainv, noi, tmin, tlimit, tn0, tn1, tf0, tf1);
    h0 = tn0 <= tf0;
    h1 = tn1 <= tf1;
}

// Both child boxes of a 32-byte node (BvhNode16, r3c): centres and half extents are HALVES, child 0 in the low and child 1 in the high half of
// each word, and v_fma_mix_f32 widens the half operand inside the instruction -- 18 plain FMAs, no unpacking (a packed fp32 FMA
// occupies the SIMD twice as long as a plain one: the 9 packed FMAs of the fp32 form are the same lane operations).  `noi` is
// -(o - scene centre) / d: the centres are relative to the scene centre.  Culling only (see BvhNode16).
#define VHR_MIX(name, mods, b_open, b_close, sel)                                                                                      \
    __device__ __forceinline__ float name(uint32_t h, float b, float c) {                                                             \
        float r;                                                                                                                       \
        asm("v_fma_mix_f32 %0, " mods "%1, " b_open "%2" b_close ", %3 op_sel:[" sel ",0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(b), "v"(c));      \
        return r;                                                                                                                      \
    }
VHR_MIX(mix_lo, "", "", "", "0")
VHR_MIX(mix_hi, "", "", "", "1")
// h * |b| + c and -h * |b| + c: the ray's |1 / d| as an operand modifier of the instruction (no register copy of it)
VHR_MIX(mix_lo_abs, "", "|", "|", "0")
VHR_MIX(mix_hi_abs, "", "|", "|", "1")
VHR_MIX(mix_lo_neg_abs, "-", "|", "|", "0")
VHR_MIX(mix_hi_neg_abs, "-", "|", "|", "1")
#undef VHR_MIX

__device__ __forceinline__ void box_pair_ch16(const uint32_t cx, const uint32_t cy, const uint32_t cz, const uint32_t hx, const uint32_t hy, const uint32_t hz,
                                              f3 inv, f3 noi, float tmin, float tlimit, float &tn0, float &tn1, float &tf0, float &tf1) {
    const float cx0 = mix_lo(cx, inv.x, noi.x), cx1 = mix_hi(cx, inv.x, noi.x);
    const float cy0 = mix_lo(cy, inv.y, noi.y), cy1 = mix_hi(cy, inv.y, noi.y);
    const float cz0 = mix_lo(cz, inv.z, noi.z), cz1 = mix_hi(cz, inv.z, noi.z);
    tn0 = hw_max3(mix_lo_neg_abs(hx, inv.x, cx0), mix_lo_neg_abs(hy, inv.y, cy0), hw_max(mix_lo_neg_abs(hz, inv.z, cz0), tmin));
    tn1 = hw_max3(mix_hi_neg_abs(hx, inv.x, cx1), mix_hi_neg_abs(hy, inv.y, cy1), hw_max(mix_hi_neg_abs(hz, inv.z, cz1), tmin));
    tf0 = hw_min3(mix_lo_abs(hx, inv.x, cx0), mix_lo_abs(hy, inv.y, cy0), hw_min(mix_lo_abs(hz, inv.z, cz0), tlimit));
    tf1 = hw_min3(mix_hi_abs(hx, inv.x, cx1), mix_hi_abs(hy, inv.y, cy1), hw_min(mix_hi_abs(hz, inv.z, cz1), tlimit));
}
__device__ __forceinline__ void box_pair_ch16(const uint32_t cx, const uint32_t cy, const uint32_t cz, const uint32_t hx, const uint32_t hy, const uint32_t hz,
                                              f3 inv, f3 noi, float tmin, float tlimit, bool &h0, bool &h1, float &tn0, float &tn1) {
    float tf0, tf1;
    box_pair_ch16(cx, cy, cz, hx, hy, hz, inv, noi, tmin, tlimit, tn0, tn1, tf0, tf1);
    h0 = tn0 <= tf0;
    h1 = tn1 <= tf1;
}

// One visit's worth of a 48-byte node (BvhNode48): three 16-byte loads, the half extents widened back to fp32 words (first of a
// pair = the word itself, second = one shift), links from the third load.  Feeds box_pair_ch unchanged.
struct Node48Words { float4 q0, q1, q2; int2 links; };
__device__ __forceinline__ Node48Words load_node48(const BvhNode48 *nodes, int cur) {
    // `cur` is the node's BYTE offset (index * 48: what the 48-byte nodes' inner links hold, r3 -- one v_mul_lo_u32, a quarter-rate
    // instruction, less per visit)
    const float4 *np = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(nodes) + uint32_t(cur));
    const float4 r0 = np[0], r1 = np[1], r2 = np[2];
    Node48Words n;
    n.q0 = r0;
    n.q1 = make_float4(r1.x, r1.y, r1.z, __uint_as_float(__float_as_uint(r1.z) << 16));
    n.q2 = make_float4(r1.w, __uint_as_float(__float_as_uint(r1.w) << 16), r2.x, __uint_as_float(__float_as_uint(r2.x) << 16));
    n.links = int2{ __float_as_int(r2.y), __float_as_int(r2.z) };
    return n;
}

// 1/d for the slab test.  A zero (or denormal) component must not become inf: fma(lo, inf, -o*inf) is NaN on one
// side of the slab only, which would cull boxes the ray is inside of.  1e30 keeps lo * inv finite for any scene
// coordinate and classifies "parallel to the slab" correctly: inside -> (-huge, +huge), outside -> both beyond tmax.
// (The exact direction d itself is untouched: Moeller-Trumbore never sees this value.)
__device__ __forceinline__ float cull_reciprocal(float d) {
    // v_rcp_f32 (1 ulp) instead of the correctly rounded division (12 instructions, three of them per ray): at scene scale
    // (boxes reach t of a few tens) an ulp of 1/d moves a slab distance by ~1e-5, two orders below the boxes' padding
    const float r = __builtin_amdgcn_rcpf(d);
    return fabsf(d) < 1e-30f ? copysignf(1e30f, d) : r;
}

// Rank of this lane among the set bits of a wave mask: v_mbcnt_lo / v_mbcnt_hi (no per-lane (1 << lane) - 1 mask to keep in registers)
__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
}

// raygen.rgen:32-53 for one (pixel, kind): the ray direction, exact arithmetic
__device__ __forceinline__ f3 ray_direction(const vhr_trace_params &tp, uint32_t seed, uint32_t kind, f3 L, f3 N) {
    uint32_t rng = seed;
    float rnd1 = random01(rng), rnd2 = random01(rng);                                        // rgen:32-33
    if (kind == 0) {                                                                         // rgen:34-41
        const f3 cone_dir = normalize3(uniform_sample_cone(rnd1, rnd2, tp.cone_cos_max));
        return onb_transform(L, cone_dir);
    }
    for (uint32_t i = 0; i < kind; ++i) { rnd1 = random01(rng); rnd2 = random01(rng); }       // rgen:46-48
    return onb_transform(N, cosine_hemisphere(rnd1, rnd2));                                  // rgen:49-51
}

// Every wave owns one 8x8-pixel tile and runs its own queue; a block is WAVES such waves side by side (a CU
// accepts at most 16 workgroups, so single-wave blocks cap occupancy at 4 waves per SIMD: measured).  Waves of a
// block share nothing and never synchronise with each other.
template <int WAVES>
__device__ __forceinline__ void tile_pixel(uint32_t block_tile, uint32_t tiles_x, uint32_t wave, uint32_t local, uint32_t row_begin, uint32_t tile_rows,
                                           uint32_t &x, uint32_t &y, uint32_t col_begin = 0u) {
    const uint32_t by = block_tile / tiles_x, bx = block_tile - by * tiles_x;
    x = col_begin + (bx * WAVES + wave) * 8u + (local & 7u);
    y = row_begin + by * tile_rows + (local >> 3);          // tile_rows < 8: the lanes of the tile's missing rows stay out of range
}

// orders this wave's LDS writes before its later LDS reads by other lanes (no cross-wave communication exists)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The shared descent ("the cut"): the rays of a tile all start within centimetres of each other, and each of them would spend most of its
// ~16 node visits walking from the root down to the boxes around that spot -- every box on the way contains the origin, so every ray
// hits it whatever its direction.  The wave therefore makes that descent ONCE per tile (uniformly: follow the inner child whose
// box contains the bounding box of the tile's ray origins, keep the other child) and leaves a CUT of the tree in LDS: up to
// kCutMax subtrees that together cover all geometry.  A ray then starts by testing the cut's boxes (a short uniform loop over
// LDS broadcasts, every refilled lane busy) and walks only the subtrees it hits.  Box tests only cull, so results are unchanged.
constexpr int kCutMax = 16;          // (12 and 24 entries measured flat around 16)

// An upper bound of |onb_transform(n, v)| / |v|, i.e. of the largest singular value of the Frisvad basis (c0, c1, n) that
// common.glsl:80-93 builds around the G-buffer normal.  The normal is a rounded half vector, not a unit vector, and near
// n.z = -1 the basis amplifies that error by 1 / (1 + n.z): AO directions are NOT unit vectors, so the reach of an AO ray is
// tmax * |d|, not tmax.  Gershgorin on the Gram matrix of the three columns, 2 % of slack for this function's own rounding
// and for |v| of the cosine-hemisphere sample (1 within a few ulp).
__device__ __forceinline__ float onb_norm_bound(f3 n) {
    f3 c0, c1;
    if (n.z < -0.9999999f) {
        c0 = f3{ 0.0f, -1.0f, 0.0f };
        c1 = f3{ -1.0f, 0.0f, 0.0f };
    } else {
        const float a = 1.0f / (1.0f + n.z);
        const float b = ((-n.x) * n.y) * a;
        c0 = f3{ 1.0f - (n.x * n.x) * a, b, -n.x };
        c1 = f3{ b, 1.0f - (n.y * n.y) * a, -n.y };
    }
    const float g00 = dot3(c0, c0), g11 = dot3(c1, c1), g22 = dot3(n, n);
    const float g01 = fabsf(dot3(c0, c1)), g02 = fabsf(dot3(c0, n)), g12 = fabsf(dot3(c1, n));
    const float row = fmaxf(fmaxf(g00 + g01 + g02, g01 + g11 + g12), g02 + g12 + g22);
    const float bound = sqrtf(row) * 1.02f;
    return bound == bound ? bound : 3.0e38f;            // a NaN normal prunes nothing
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) v4f *uniform_f4_ptr;         // constant address space + uniform address = SMEM loads
typedef const __attribute__((address_space(4))) v4i *uniform_i4_ptr;

// The same descent written on wave-uniform values (rounds 2-4): every comparison and every move of a box is a vector instruction for the whole
// wave, ~100 per level.  Kept for the closest-hit walks and the raytraced path, whose launches are not bound by vector issue (and whose kernels
// the lane-parallel form below does not compile for: the backend's verifier rejects a private-to-flat cast next to it).
__device__ __forceinline__ uint32_t build_tile_cut_uniform(const DeviceScene &sc, f3 omin, f3 omax, float4 (*s_cut)[2], uint32_t lane, float reach = 3.0e38f,
                                                   const int max_entries = kCutMax, const int link_bytes = int(sizeof(BvhNode48)), const f3 centre = f3{ 0.0f, 0.0f, 0.0f }) {
    // ---- bounds of the origins (wave reduction), then the descent; every lane computes the same thing ----
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        omin.x = fminf(omin.x, __shfl_xor(omin.x, off)); omin.y = fminf(omin.y, __shfl_xor(omin.y, off)); omin.z = fminf(omin.z, __shfl_xor(omin.z, off));
        omax.x = fmaxf(omax.x, __shfl_xor(omax.x, off)); omax.y = fmaxf(omax.y, __shfl_xor(omax.y, off)); omax.z = fmaxf(omax.z, __shfl_xor(omax.z, off));
        reach = fmaxf(reach, __shfl_xor(reach, off));
    }
    // wave-uniform from here on, and told so: the descent then runs on scalar registers and scalar branches
    auto uni = [](float f) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f))); };
    omin = f3{ uni(omin.x), uni(omin.y), uni(omin.z) }; omax = f3{ uni(omax.x), uni(omax.y), uni(omax.z) };
    box_bounds(sc, omin, omax);                          // "bvh_frame": the nodes' boxes are in the frame
    reach = uni(reach);
    const float reach2 = reach * reach;                 // inf for "no pruning" (and for anything that overflows)
    // The cut while it is being built: entry e lives in lane e (box, link).
    float e_lx = 0.0f, e_hx = 0.0f, e_ly = 0.0f, e_hy = 0.0f, e_lz = 0.0f, e_hz = 0.0f;
    int e_link = 0;
    uint32_t cut_n = 0;
    auto gap2_of = [&](float lx, float hx, float ly, float hy, float lz, float hz) {
        const float gx = fmaxf(fmaxf(lx - omax.x, omin.x - hx), 0.0f), gy = fmaxf(fmaxf(ly - omax.y, omin.y - hy), 0.0f),
                    gz = fmaxf(fmaxf(lz - omax.z, omin.z - hz), 0.0f);
        return (gx * gx + gy * gy) + gz * gz;
    };
    auto put = [&](uint32_t slot, float lx, float hx, float ly, float hy, float lz, float hz, int link) {
        if (lane == slot) { e_lx = lx; e_hx = hx; e_ly = ly; e_hy = hy; e_lz = lz; e_hz = hz; e_link = link; }
    };
    auto add_entry = [&](float lx, float hx, float ly, float hy, float lz, float hz, int link) {
        const float g2 = gap2_of(lx, hx, ly, hy, lz, hz);
        if (g2 > reach2) return;                                                             // out of every ray's reach
        put(cut_n, lx, hx, ly, hy, lz, hz, link);
        ++cut_n;
    };
    int node = 0;
    float fb[6] = { -3.0e38f, 3.0e38f, -3.0e38f, 3.0e38f, -3.0e38f, 3.0e38f };          // box of `node` (the root: everything)
    bool open = true;                                                                      // `node` still waits for its entry
    for (int it = 0; it < max_entries - 2; ++it) {
        // a uniform address in the constant address space: the node arrives through the scalar cache (s_load), not through the
        // vector memory path the walk itself is bound by
        const uniform_f4_ptr np = (uniform_f4_ptr)(uintptr_t)(sc.nodes + node);
        const v4f q0 = np[0], q1 = np[1], q2 = np[2];
        const v4i vl = ((uniform_i4_ptr)np)[3];
        const int2 links = int2{ vl.x, vl.y };
        const bool in0 = q0.x <= omin.x && omax.x <= q0.y && q0.z <= omin.y && omax.y <= q0.w && q1.x <= omin.z && omax.z <= q1.y;
        const bool in1 = q1.z <= omin.x && omax.x <= q1.w && q2.x <= omin.y && omax.y <= q2.y && q2.z <= omin.z && omax.z <= q2.w;
        const bool follow0 = links.x >= 0 && in0, follow1 = !follow0 && links.y >= 0 && in1;
        if (!(follow0 || follow1)) {                                                      // the descent ends here: both children join the cut
            add_entry(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, links.x);
            add_entry(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, links.y);
            open = false;
            break;
        }
        if (follow0) {
            add_entry(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, links.y);
            fb[0] = q0.x; fb[1] = q0.y; fb[2] = q0.z; fb[3] = q0.w; fb[4] = q1.x; fb[5] = q1.y;
            node = links.x;
        } else {
            add_entry(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, links.x);
            fb[0] = q1.z; fb[1] = q1.w; fb[2] = q2.x; fb[3] = q2.y; fb[4] = q2.z; fb[5] = q2.w;
            node = links.y;
        }
    }
    if (open) add_entry(fb[0], fb[1], fb[2], fb[3], fb[4], fb[5], node);                  // the budget ran out: the subtree itself
    if (lane < cut_n) {
        // centre / half extent (box_test_ch1), the centre relative to `centre` (the walkers of the half-precision nodes keep their ray origins
        // relative to the scene's centre): c +- h contains [lo, hi] -- h carries 4 ulp of the magnitudes involved, the roundings of c, of
        // hi - c and of the shift are below one each.  The root's "everything" box (+-3e38) stays finite: c = 0, h = 3e38 (1 + 2.4e-7).
        auto ch = [](float lo, float hi, float shift, float &c, float &h) {
            const float mid = 0.5f * lo + 0.5f * hi;
            c = mid - shift;
            h = fmaxf(hi - mid, mid - lo);
            h += (fabsf(mid) + fabsf(shift) + h) * 2.4e-7f;
        };
        float cx, cy, cz, hx, hy, hz;
        ch(e_lx, e_hx, centre.x, cx, hx); ch(e_ly, e_hy, centre.y, cy, hy); ch(e_lz, e_hz, centre.z, cz, hz);
        s_cut[lane][0] = make_float4(cx, cy, cz, hx);
        s_cut[lane][1] = make_float4(hy, hz, __int_as_float(e_link >= 0 ? e_link * link_bytes : e_link), 0.0f);
    }
    wave_lds_sync();
    return cut_n;
}

// One entry of a tile's cut (build_tile_cut): what a lane knows about itself, and the store of a child's box in centre / half-extent form.
struct CutLane {
    f3 omin, omax;
    float reach2, shift;
    uint32_t axis;
    bool lo_lane;
    uint32_t my_child, lane;
    int link_bytes;
};
__device__ __forceinline__ void cut_add_entry(const CutLane cl, float4 (*s_cut)[2], uint32_t &cut_n, const float word, const int child, const int link) {
    if (cl.reach2 < 3.0e38f) {                                                               // (uniform; launches without shadow rays only)
        const int b0 = 6 * child;
        auto lane_word = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
        const float lx = lane_word(word, b0), hx = lane_word(word, b0 + 1), ly = lane_word(word, b0 + 2), hy = lane_word(word, b0 + 3), lz = lane_word(word, b0 + 4),
                    hz = lane_word(word, b0 + 5);
        const float gx = fmaxf(fmaxf(lx - cl.omax.x, cl.omin.x - hx), 0.0f), gy = fmaxf(fmaxf(ly - cl.omax.y, cl.omin.y - hy), 0.0f),
                    gz = fmaxf(fmaxf(lz - cl.omax.z, cl.omin.z - hz), 0.0f);
        if ((gx * gx + gy * gy) + gz * gz > cl.reach2) return;                                // out of every ray's reach
    }
    // centre / half extent (box_test_ch1), the centre relative to `centre` (the walkers of the half-precision nodes keep their ray origins
    // relative to the scene's centre): c +- h contains [lo, hi] -- h carries 4 ulp of the magnitudes involved, the roundings of c, of
    // hi - c and of the shift are below one each.  The root's "everything" box (+-3e38) stays finite: c = 0, h = 3e38 (1 + 2.4e-7).
    const float other = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(word), 0xB1, 0xf, 0xf, true));      // quad_perm [1, 0, 3, 2]: the pair's other word
    const float mid = 0.5f * word + 0.5f * other;                                          // (lo lanes: word = lo, other = hi)
    const float c = mid - cl.shift;
    float h = fmaxf(other - mid, mid - word);
    h += (fabsf(mid) + fabsf(cl.shift) + h) * 2.4e-7f;
    // (the cut is an LDS array at every call site; said so, so that the stores are ds_write and not flat stores behind an address-space test)
    typedef __attribute__((address_space(3))) float lds_float;
    lds_float *const entry = (lds_float *)(&s_cut[0][0]) + cut_n * 8u;                       // (cx, cy, cz, hx), (hy, hz, link, -)
    if (cl.lo_lane && cl.my_child == uint32_t(child)) { entry[cl.axis] = c; entry[3u + cl.axis] = h; }
    if (cl.lane == 0u) entry[6] = __int_as_float(link >= 0 ? link * cl.link_bytes : link);
    ++cut_n;
}

// The shared descent of a tile (see CUT above): `omin` / `omax` are this lane's contribution to the bounds of the tile's ray
// origins (+-3e38 for lanes without one).  Leaves the cut in s_cut[0 .. n) -- centre / half extent: (cx, cy, cz, hx), (hy, hz, link, -) --
// and returns n, wave-uniform.  Entries are in path order: the deeper an entry, the closer its box to the origins.
// `reach` (this lane's contribution, 0 for lanes without rays; +inf = no pruning): an upper bound of how far any of the tile's
// rays can get from its origin, tmax * |d|.  A subtree whose box lies farther than that from the bounds of the origins cannot
// hold a hit of any of them and is left out of the cut -- decided once per tile instead of by a box test per ray.
// `link_bytes`: inner links of the finished cut are multiplied by it (48 for the walkers of the 48-byte nodes, whose links are byte offsets).
__device__ __forceinline__ uint32_t build_tile_cut(const DeviceScene &sc, f3 omin, f3 omax, float4 (*s_cut)[2], uint32_t lane, float reach = 3.0e38f,
                                                   const int max_entries = kCutMax, const int link_bytes = int(sizeof(BvhNode48)), const f3 centre = f3{ 0.0f, 0.0f, 0.0f }) {
    // ---- bounds of the origins (wave reduction), then the descent; every lane computes the same thing ----
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        omin.x = fminf(omin.x, __shfl_xor(omin.x, off)); omin.y = fminf(omin.y, __shfl_xor(omin.y, off)); omin.z = fminf(omin.z, __shfl_xor(omin.z, off));
        omax.x = fmaxf(omax.x, __shfl_xor(omax.x, off)); omax.y = fmaxf(omax.y, __shfl_xor(omax.y, off)); omax.z = fmaxf(omax.z, __shfl_xor(omax.z, off));
        reach = fmaxf(reach, __shfl_xor(reach, off));
    }
    auto uni = [](float f) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f))); };
    omin = f3{ uni(omin.x), uni(omin.y), uni(omin.z) }; omax = f3{ uni(omax.x), uni(omax.y), uni(omax.z) };
    box_bounds(sc, omin, omax);                          // "bvh_frame": the nodes' boxes are in the frame
    reach = uni(reach);
    const float reach2 = reach * reach;                 // inf for "no pruning" (and for anything that overflows)
    // The descent is wave-uniform, but this chip's scalar unit has no float arithmetic: written on uniform values, every comparison, every
    // min / max and every move of a box is a vector instruction for the whole wave -- about a hundred per level, 800 per tile, a seventh of the
    // any-hit launch's instructions (r5).  So the lanes take a WORD of the 64-byte node each: lane w (of every sixteen) loads word w -- child 0's
    // box in words 0-5 as (lo, hi) pairs per axis, child 1's in 6-11, the links in 12 and 13 -- and tests it against its own bound of the
    // origins; the answers come back as a lane mask, the links by v_readlane, and everything that steers the descent is scalar.  An entry's
    // centre / half-extent form is computed by the three even lanes that hold its lo words (the hi word comes from the neighbour by DPP) and
    // stored straight to the cut in LDS.  ~20 vector instructions per level.
    const uint32_t w = lane & 15u;
    const bool is_hi = (w & 1u) != 0u;
    const uint32_t axis = (w % 6u) >> 1;
    const bool lo_lane = lane < 12u && !is_hi;          // the lanes that hold a box's lo words (one sixteen of the wave writes)
    const uint32_t my_child = w >= 6u ? 1u : 0u;
    // a lo word passes iff word <= omin[axis], a hi word iff omax[axis] <= word, i.e. -word <= -omax[axis]: one comparison with the sign flipped
    const uint32_t flip = is_hi ? 0x80000000u : 0u;
    const float ref = is_hi ? -(axis == 0u ? omax.x : axis == 1u ? omax.y : omax.z) : (axis == 0u ? omin.x : axis == 1u ? omin.y : omin.z);
    const float shift = axis == 0u ? centre.x : axis == 1u ? centre.y : centre.z;
    const uint32_t word_offset = w * 4u;
    uint32_t cut_n = 0;
    const CutLane cl{ omin, omax, reach2, shift, axis, lo_lane, my_child, lane, link_bytes };
    // `word`: a node's words, one per lane; `child`'s box joins the cut with `link`
#define add_entry(word, child, link) cut_add_entry(cl, s_cut, cut_n, word, child, link)
    int node = 0;
    float pword = is_hi ? 3.0e38f : -3.0e38f;                                              // the words `node`'s own box came in: for the root, "everything" as child 0
    int pchild = 0;
    bool open = true;                                                                      // `node` still waits for its entry
    const char *const base = reinterpret_cast<const char *>(sc.nodes);
    for (int it = 0; it < max_entries - 2; ++it) {
        const float word = *reinterpret_cast<const float *>(base + (uint32_t(node) * uint32_t(sizeof(BvhNode)) + word_offset));
        const uint32_t inside = uint32_t(cmp_le_mask(__uint_as_float(__float_as_uint(word) ^ flip), ref));      // bit w: word w keeps the origins inside
        const bool in0 = (inside & 0x3fu) == 0x3fu, in1 = (inside & 0xfc0u) == 0xfc0u;
        const int link0 = __builtin_amdgcn_readlane(__float_as_int(word), 12), link1 = __builtin_amdgcn_readlane(__float_as_int(word), 13);
        const bool follow0 = link0 >= 0 && in0, follow1 = !follow0 && link1 >= 0 && in1;
        if (!(follow0 || follow1)) {                                                      // the descent ends here: both children join the cut
            add_entry(word, 0, link0);
            add_entry(word, 1, link1);
            open = false;
            break;
        }
        if (follow0) { add_entry(word, 1, link1); pchild = 0; node = link0; }
        else { add_entry(word, 0, link0); pchild = 1; node = link1; }
        pword = word;
    }
    if (open) {                                                                            // the budget ran out: the subtree itself
        if (pchild == 0) add_entry(pword, 0, node); else add_entry(pword, 1, node);
    }
#undef add_entry
    wave_lds_sync();
    return cut_n;
}

// "raygen_cost_order": the blocks of an earlier launch sorted by cost, heaviest first, by ONE block of the ray-tracing launch (its first: it starts at
// once and has the whole launch to finish its own tile afterwards).  A block's cost is its longest-lived wave's lifetime; the blocks fall into 8
// classes of cost relative to the maximum, and a stable counting sort puts the heaviest class first -- inside a class the blocks keep their
// row-major order (neighbouring tiles share nodes; a full sort gives that up: round 2's "longest tiles first").  Whatever the lifetimes hold, the
// result is a permutation of 0 .. n_blocks - 1: the order is a speed hint, never correctness.  `lds`: 8 * 64 * WAVES words of scratch.
template <int WAVES>
__device__ __forceinline__ void order_blocks_by_cost(const uint32_t *__restrict__ wave_cost, const uint32_t n_blocks, uint32_t *__restrict__ order, uint32_t *lds) {
    constexpr uint32_t NT = 64u * WAVES, C = 8u;
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + NT - 1u) / NT, b0 = min(t * per, n_blocks), b1 = min(b0 + per, n_blocks);     // a contiguous chunk per thread
    auto cost = [&](uint32_t b) { uint32_t c = 0; for (uint32_t w = 0; w < uint32_t(WAVES); ++w) c = max(c, wave_cost[b * uint32_t(WAVES) + w]); return c; };
    uint32_t mx = 0;
    for (uint32_t b = b0; b < b1; ++b) mx = max(mx, cost(b));
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, uint32_t(__shfl_xor(int(mx), off)));
    if ((t & 63u) == 0u) lds[t >> 6] = mx;
    __syncthreads();
    for (uint32_t w = 0; w < uint32_t(WAVES); ++w) mx = max(mx, lds[w]);
    __syncthreads();
    const float scale = float(C) / float(max(1u, mx));
    auto cls = [&](uint32_t c) { return (C - 1u) - min(C - 1u, uint32_t(float(c) * scale)); };    // 0 = the heaviest (any deterministic map will do)
    uint32_t mine[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) mine[c] = 0;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t k = cls(cost(b));
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) mine[c] += k == c ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) lds[c * NT + t] = mine[c];
    __syncthreads();
    for (uint32_t off = 1; off < C * NT; off <<= 1) {         // inclusive scan over (class-major, thread-minor)
        uint32_t v[C];
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) { const uint32_t i = c * NT + t; v[c] = i >= off ? lds[i - off] : 0u; }
        __syncthreads();
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) lds[c * NT + t] += v[c];
        __syncthreads();
    }
    uint32_t pos[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) pos[c] = lds[c * NT + t] - mine[c];       // inclusive -> exclusive
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t k = cls(cost(b));
        uint32_t p = 0;
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) { p = k == c ? pos[c] : p; pos[c] += k == c ? 1u : 0u; }
        // (rotated by one: the LIGHTEST block goes to the front -- the next launch's first block, which does this sort before its own tile)
        order[p + 1u == n_blocks ? 0u : p + 1u] = b;
    }
    __syncthreads();                                        // the scratch is the waves' traversal stacks from here on
}

// "raygen_cost_order", what a queue kernel's launch gets: wave_cost != nullptr -> every wave leaves its lifetime there (index = its block's tiles *
// WAVES + wave); block_order != nullptr -> block b works on the tiles of block block_order[b] (the launch before last's blocks, longest-lived
// first); order_out != nullptr -> the launch's first block sorts the previous launch's `order_blocks` blocks by `cost_prev` into it before its own tile
struct CostOrderArgs {
    uint32_t *wave_cost = nullptr;
    const uint32_t *block_order = nullptr;
    const uint32_t *cost_prev = nullptr;
    uint32_t *order_out = nullptr;
    uint32_t order_blocks = 0;
};

// ---------------------------------------------------------------------------------------------
// One pass of a wave over its ray queue (`total` rays; fetch(r, pix, origin, direction) delivers the r-th one and the id of
// its pixel, commit(pix, triangle, u, v) takes its result, kNoHit = miss).  Lanes pull rays whenever `refill_threshold` of
// them are idle and walk the BVH "while-while" with the node step of raygen_queue_kernel: packed-FMA slabs against 1/d and
// -o/d, near child first, far child pushed, boxes culled against the closest t so far (tn <= tbest keeps equal-t candidates:
// decision vi), early exit of the node loop, LDS stack + scratch spill.  Leaves: every triangle, Moeller-Trumbore against the
// full [tmin, tmax] interval, closest = min t then smaller flat index; with `any_hit` (wave-uniform) the first accepted
// triangle ends the ray (gl_RayFlagsTerminateOnFirstHitEXT -- the boolean does not depend on the order).  A candidate goes through three
// steps: mt_candidate with decision (vi), then the ray's candidate filter -- filter(pix, triangle, u, v), the protocol of trace_device.hpp;
// true: the candidate does not exist for this ray -- then the commit.  PER_RAY (the batched ray query, ray_query_kernel): every ray brings
// its own interval -- fetch(r, pix, origin, direction, tmin, tmax), the ray's tmax seeds the cull -- and commit(pix, triangle, u, v, t)
// is also told the hit's t; `tmin` / `tmax` are then unused.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kNoHit = 0xffffffffu;

// what a walk did (STATS builds only): node visits, leaf visits and triangle tests summed over lanes, and the trips of the two inner loops
// counted once per wave (the slowest lane's) -- lane utilisation = (nodes + triangles) / (64 x wave_trips), as for raygen_queue_kernel
struct WalkCounters { uint32_t nodes = 0, leaves = 0, triangles = 0, wave_trips = 0, refills = 0; };

struct NoFlag { __device__ __forceinline__ void operator()(uint32_t) const {} };
template <bool SPILL, bool DEFER, bool STATS = false, bool PER_RAY = false, typename Fetch, typename Commit, typename Flag = NoFlag,
          typename Filter = NoFilter>
__device__ __forceinline__ void wave_queue_walk(const DeviceScene &sc, int *stack, const uint32_t stack_levels, const uint32_t lane,
                                                const uint32_t total, const uint32_t refill_threshold, const uint32_t early_exit,
                                                const float tmin, const float tmax, const bool any_hit, uint32_t &overflow,
                                                const float4 (*cut)[2], const uint32_t cut_n, Fetch fetch, Commit commit, WalkCounters *wc = nullptr,
                                                Flag flag = Flag{}, Filter filter = Filter{}) {
    f3 ro = f3{ 0, 0, 0 }, rd = f3{ 0, 0, 1 }, rinv = f3{ 0, 0, 0 }, noi = f3{ 0, 0, 0 }, ainv = f3{ 0, 0, 0 };
    float tbest = 0.0f, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = kNoHit, best_flat = 0;
    int cur = 0, sp = 0;
    uint32_t pix = 0, next = 0;
    uint32_t emask = 0;                                   // cut entries this lane's ray hits that did not fit its LDS stack
    bool has = false;
    // volatile: keeps the array in scratch.  Left alone, the compiler promotes it to 32 VGPRs with indirect indexing, which
    // pushes the kernels over their register budget (55 spilled VGPRs, 38 spilled SGPRs, 1.5x slower: measured)
    volatile int spill[SPILL ? kSpillStack : 1];
    float tmin_v = tmin;
    asm volatile("" : "+v"(tmin_v));
    float ray_tmin = tmin, ray_tmax = tmax;               // the interval of the lane's ray (PER_RAY: its own, else the launch's)
    for (;;) {
        const unsigned long long idle = __ballot(!has);
        const uint32_t n_idle = uint32_t(__popcll(idle));
        if (next < total && (n_idle >= refill_threshold || n_idle == 64u)) {                 // wave-uniform
            const uint32_t r = next + lane_rank(idle);
            next += n_idle;
            if (STATS && lane == 0) ++wc->refills;
            if (!has && r < total) {
                if constexpr (PER_RAY) { fetch(r, pix, ro, rd, ray_tmin, ray_tmax); tmin_v = ray_tmin; }
                else fetch(r, pix, ro, rd);
                f3 bo, bd;
                box_ray(sc, ro, rd, bo, bd);                  // "bvh_frame": the slab tests' ray (ro, rd stay the triangle tests')
                rinv = f3{ cull_reciprocal(bd.x), cull_reciprocal(bd.y), cull_reciprocal(bd.z) };
                noi = f3{ -(bo.x * rinv.x), -(bo.y * rinv.y), -(bo.z * rinv.z) };
                ainv = f3{ fabsf(rinv.x), fabsf(rinv.y), fabsf(rinv.z) };
                tbest = ray_tmax; best_tri = kNoHit; best_flat = 0; best_u = 0.0f; best_v = 0.0f;
                cur = 0; sp = 0;
                // the ray against the tile's cut: the (t, flat index) order of the commit makes the result independent of the order the subtrees are walked in
                if (cut_n) cut_to_stack(cut, cut_n, stack, stack_levels, rinv, noi, tmin_v, ray_tmax, cur, sp, emask);
                has = true;
            }
        }
        if (!__any(has)) break;
        // ---- inner nodes ----
        const uint32_t walkers_in = uint32_t(__popcll(__ballot(has && cur >= 0)));
        uint32_t my_nodes = 0, my_tris = 0;               // (STATS) this lane's trips of the two inner loops in this round
        while (has && cur >= 0) {
            if (uint32_t(__popcll(__ballot(true))) * 16u <= walkers_in * early_exit) break;
            if (STATS) ++my_nodes;
            // (the 48-byte fp32 nodes: the 32-byte half-precision ones were measured here too -- r3c, and r4 with the walk as a kernel of its
            // own at 58 registers -- and make no difference to this walk)
            const Node48Words nw = load_node48(sc.nodes48, cur);
            const int2 links = nw.links;
            float tn0, tn1;
            bool h0, h1;
            box_pair_ch(nw.q0, nw.q1, nw.q2, rinv, ainv, noi, tmin_v, tbest, h0, h1, tn0, tn1);
            const bool both = h0 && h1, none = !(h0 || h1);
            const bool first0 = tn0 <= tn1;
            const int nearc = first0 ? links.x : links.y, farc = first0 ? links.y : links.x;
            int *const row = stack + min(uint32_t(sp), stack_levels + 1u) * kQueueBlock;
            int top = row[0];
            row[kQueueBlock] = farc;
            if (__any(uint32_t(sp) >= stack_levels)) {
                if (SPILL && uint32_t(sp) > stack_levels) top = spill[(uint32_t(sp) - 1u - stack_levels) & uint32_t(kSpillStack - 1)];
                if (uint32_t(sp) >= stack_levels) {
                    if (SPILL && uint32_t(sp) - stack_levels < uint32_t(kSpillStack)) spill[uint32_t(sp) - stack_levels] = farc;
                    else overflow |= both ? 1u : 0u;
                }
            }
            cur = both ? nearc : (none ? top : (h0 ? links.x : links.y));
            sp += (both ? 1 : 0) - (none ? 1 : 0);
        }
        // ---- leaf ----
        if (has && cur < 0 && cur != kStackSentinel) {
            const uint32_t vv = ~uint32_t(cur);
            const uint32_t first = vv >> 2, count = (vv & 3u) + 1u;
            bool done = false;
            if (STATS) ++wc->leaves;
            for (uint32_t i = 0; i < count; ++i) {
                const float4 *tp = reinterpret_cast<const float4 *>(sc.tris + first + i);
                const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                float t, uu, ww;
                if (STATS) ++my_tris;
                const f3 v0 = f3{ ta.x, ta.y, ta.z }, e1 = f3{ ta.w, tb.x, tb.y }, e2 = f3{ tb.z, tb.w, tc.x };
                if (mt_candidate(ro, rd, v0, e1, e2, ray_tmin, ray_tmax, t, uu, ww)) {
                    // decision (vi): a candidate that contradicts itself is decided again in binary64.  DEFER (the mirror ray's kernels, where about one ray of a
                    // 1080p frame has one): not here, where the walk's registers are all alive -- the ray's pixel is flagged and computed again by the per-pixel
                    // code when the tile is shaded (redo_pixel_reflection); the walk goes on as if the candidate had missed.  !DEFER (the raytraced path,
                    // whose shadow rays leave the hit point itself: 6 % of its rays have one): inline.
                    if (!solution_consistent(ro, rd, v0, e1, e2, t, uu, ww)) {
                        if (DEFER) { flag(pix); continue; }
                        if (!mt_binary64(ro, rd, v0, e1, e2, ray_tmin, ray_tmax, t, uu, ww)) continue;
                    }
                    if constexpr (!std::is_same_v<Filter, NoFilter>) { if (filter(pix, first + i, uu, ww)) continue; }
                    const uint32_t flat = __float_as_uint(tc.w);
                    if (best_tri == kNoHit || t < tbest || (t == tbest && flat < best_flat)) {
                        tbest = t; best_tri = first + i; best_flat = flat; best_u = uu; best_v = ww;
                    }
                    if (any_hit) { done = true; break; }
                }
            }
            if (done) {
                cur = kStackSentinel;
                emask = 0;
            } else {
                cur = stack[min(uint32_t(sp), stack_levels + 1u) * kQueueBlock];             // pop (the sentinel if nothing is pending)
                if (SPILL && __any(uint32_t(sp) > stack_levels)) {
                    if (uint32_t(sp) > stack_levels) cur = spill[(uint32_t(sp) - 1u - stack_levels) & uint32_t(kSpillStack - 1)];
                }
                --sp;
            }
        }
        if (has && cur == kStackSentinel && emask) {          // overflowed cut entries: the next subtree
            const int e = __ffs(int(emask)) - 1;
            emask &= emask - 1u;
            cur = __float_as_int(cut[e][1].z);
            sp = 0;                                           // (the pop of the empty stack left it at -1)
        }
        if (has && cur == kStackSentinel) {
            has = false;
            if constexpr (PER_RAY) commit(pix, best_tri, best_u, best_v, tbest);
            else commit(pix, best_tri, best_u, best_v);
        }
        if (STATS) {
            wc->nodes += my_nodes; wc->triangles += my_tris;
            uint32_t tn = my_nodes, tt = my_tris;
            for (int off = 32; off > 0; off >>= 1) { tn = max(tn, uint32_t(__shfl_xor(int(tn), off))); tt = max(tt, uint32_t(__shfl_xor(int(tt), off))); }
            wc->wave_trips += tn + tt;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// What the launchers of the queue kernels share (host).
// ---------------------------------------------------------------------------------------------
// The walk's parameters by the options in force.  `levels`: the LDS part of the traversal stack, sized by the tree actually built (depth <=
// kMaxBvhDepth): less LDS, more waves per CU; deeper entries spill to scratch (`spill`: the SPILL instantiation) unless the whole stack fits
// the configured levels.  `lds_bytes`: a block's dynamic LDS -- the kernels index s_dyn by the same (levels + 3) rows per wave.
struct QueueLaunch {
    uint32_t levels, threshold, early_exit;
    size_t lds_bytes;
    bool spill;
};
static QueueLaunch queue_launch(const vhr_context *ctx, const int lds_levels_option, const int early_exit_option, const uint32_t waves_per_block) {
    QueueLaunch q;
    q.levels = std::max<uint32_t>(1u, std::min<uint32_t>(ctx->bvh_depth + 1u, uint32_t(std::max(1, ctx->options[lds_levels_option]))));
    q.threshold = uint32_t(std::max(1, std::min(64, ctx->options[kOptRefillThreshold])));
    q.early_exit = uint32_t(std::max(0, std::min(15, ctx->options[early_exit_option])));
    q.lds_bytes = size_t(q.levels + 3) * kQueueBlock * sizeof(int) * waves_per_block;
    q.spill = q.levels < ctx->bvh_depth + 1u;
    return q;
}

// The grid of a launch whose waves own one tile_w x 8 pixel tile each, two waves to a block.
struct TileGrid {
    uint32_t tiles_x, tiles_total;
    dim3 grid, block;
};
static TileGrid tile_grid(const uint32_t columns, const uint32_t rows, const uint32_t tile_w) {
    TileGrid g;
    g.tiles_x = (columns + tile_w - 1u) / tile_w;
    g.tiles_total = g.tiles_x * ((rows + 7u) / 8u);
    g.grid = dim3((g.tiles_total + 1u) / 2u);
    g.block = dim3(kQueueBlock * 2);
    return g;
}

// Ray statistics (vhr_set_ray_statistics) around a path's launches: `count` RayStats cleared on the stream before them, copied to the context
// behind them -- [0] the path's own, [1] the hybrid path's mirror-ray launch.  The end also reports a launch that failed, in the launcher's words.
static int ray_stats_begin(vhr_context *ctx, const bool on, const uint32_t count = 1u) {
    if (on && hipMemsetAsync(ctx->d_ray_stats, 0, count * sizeof(RayStats), ctx->stream) != hipSuccess)
        return ctx->fail(VHR_ERROR_DEVICE, "hipMemsetAsync(ray stats) failed");
    return VHR_OK;
}
static int ray_stats_end(vhr_context *ctx, const bool on, const char *launch_failed, const uint32_t count = 1u) {
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, launch_failed);
    if (on && (hipMemcpyAsync(&ctx->h_ray_stats, ctx->d_ray_stats, sizeof(RayStats), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
               (count > 1u && hipMemcpyAsync(&ctx->h_refl_stats, ctx->d_ray_stats + 1, sizeof(RayStats), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)))
        return ctx->fail(VHR_ERROR_DEVICE, "hipMemcpyAsync(ray stats) failed");
    return VHR_OK;
}

// A run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{}); nested for several flags.
template <typename F>
static void with_bool(const bool flag, F &&f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}
// A launch's candidate filter (kFilterNone / kFilterAlpha / kFilterMask, trace_device.hpp) likewise: the mask instantiation only where a mask of
// the launch ACTS on the masks the primitives carry (vhr_context::ray_mask_acts; the alpha rule is then its runtime bit), else the alpha
// instantiation or the plain kernels, as before masks existed.
static int launch_filter(const bool mask_acts, const bool alpha) { return mask_acts ? kFilterMask : (alpha ? kFilterAlpha : kFilterNone); }
template <typename F>
static void with_filter(const int filter, F &&f) {
    if (filter == kFilterMask) f(std::integral_constant<int, kFilterMask>{});
    else if (filter == kFilterAlpha) f(std::integral_constant<int, kFilterAlpha>{});
    else f(std::integral_constant<int, kFilterNone>{});
}

// "raygen_cost_order": the cost / order pointers of a queue-kernel launch of `n_blocks` blocks of `wv` waves (see vhr_context::CostOrder).
// 1 (default) = launches of at least 2 048 blocks (a full round of waves or more), 2 = any launch (tests); the two launches an order connects must
// have been issued on the same stream -- the order is written and read in stream order, nothing else guards it.
static void prepare_cost_order(vhr_context *ctx, vhr_context::CostOrder &co, const uint32_t n_blocks, const uint32_t wv, const uint32_t key, CostOrderArgs &out,
                               const vhr_context::CostOrder::Shape &shape) {
    const int mode = ctx->options[kOptRaygenCostOrder];
    if (!mode) return;
    if (co.stream != ctx->stream) {
        // another stream than the last launch's (frames in flight switched on or off, say): whatever of that stream is still in flight may be
        // writing an order -- wait once, forget both
        if (co.capacity) (void)hipDeviceSynchronize();
        co.stream = ctx->stream;
        co.order_blocks[0] = co.order_blocks[1] = co.cost_blocks[0] = co.cost_blocks[1] = 0;
    }
    if (n_blocks < (mode >= 2 ? 2u : 2048u)) return;
    const uint32_t n_waves = n_blocks * wv;
    if (n_waves > co.capacity) {
        (void)hipDeviceSynchronize();              // (first use / a larger launch: nothing may still read the old buffers)
        for (int i = 0; i < 2; ++i) { (void)hipFree(co.cost[i]); (void)hipFree(co.order[i]); co.cost[i] = co.order[i] = nullptr; }
        co.capacity = 0;
        co.order_blocks[0] = co.order_blocks[1] = co.cost_blocks[0] = co.cost_blocks[1] = 0;
        bool ok = true;
        for (int i = 0; i < 2; ++i)
            ok = ok && hipMalloc(reinterpret_cast<void **>(&co.cost[i]), size_t(n_waves) * 4) == hipSuccess &&
                 hipMalloc(reinterpret_cast<void **>(&co.order[i]), size_t(n_waves) * 4) == hipSuccess;
        if (!ok) return;
        co.capacity = n_waves;
    }
    const uint32_t prev = co.slot, slot = prev ^ 1u;
    co.slot = slot;
    out.wave_cost = co.cost[slot];
    if (co.order_blocks[slot] == n_blocks && co.order_key[slot] == key) out.block_order = co.order[slot];
    if (co.cost_blocks[prev] == n_blocks && co.cost_key[prev] == key) {       // the previous launch had this shape: its blocks get ordered
        out.cost_prev = co.cost[prev]; out.order_out = co.order[prev]; out.order_blocks = n_blocks;
        co.order_blocks[prev] = n_blocks; co.order_key[prev] = key;
    } else {
        co.order_blocks[prev] = 0;
    }
    co.cost_blocks[slot] = n_blocks; co.cost_key[slot] = key;
    co.cost_waves[slot] = n_waves;
    co.shape[slot] = shape;
}

}  // namespace vhr
