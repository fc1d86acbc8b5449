// K1 + K2 of the hybrid render path: software BVH2 ray tracing for gfx950.
//
// Replaces, for the hybrid render path's "Raytrace Pass" (hybrid_render_path.cpp:101-136):
//   data/shaders/hybrid_render_path/raygen.rgen:14-66        -> raygen_kernel, raygen_queue_kernel; the mirror ray: reflection_kernel, reflection_queue_kernel
//   data/shaders/hybrid_render_path/miss.rmiss:6-8            -> payload 1.0 when the any-hit walk finds nothing
//   data/shaders/hybrid_render_path/reflection_miss.rmiss:6-8 -> payload 0 when the closest-hit walk finds nothing
//   vkCmdTraceRaysKHR (raytracing_execution_context.cpp:4-13) -> launch_raygen
// The walkers, the triangle test and reflection_hit.rchit are in trace_device.hpp, the queue machinery in trace_queue.hpp; the other
// render paths, the stand-in passes and the batched ray query, which this file also held until it was split, are in kernels_raytraced.hip,
// kernels_forward.hip, kernels_standin.hip and kernels_ray_query.hip.  All five are built with the same flags.
//
// Compiled with -ffp-contract=off: ray setup and Moeller-Trumbore follow the exact-arithmetic contract of
// device_math.hpp so visibility results are bit-reproducible.
#define VHR_TRACE_UNIT unit_trace      // this unit's copy of the sRGB decode table (trace_device.hpp)
#include <cstring>

#include "trace_queue.hpp"
#include "svgf_temporal.hpp"

namespace vhr {

#ifndef VHR_REDO_INLINE
#define VHR_REDO_INLINE __attribute__((noinline))
#endif
#ifndef VHR_K1_WAVES_MIN
#define VHR_K1_WAVES_MIN 8          // waves per SIMD the any-hit queue kernel is allocated for (7: <= 72 registers, 8: <= 64; redo_pixel_visibility() inherits it)
#endif
constexpr uint32_t kRedoPixel = 0x80000000u;   // raygen_queue_kernel's visibility word: the pixel is computed again by redo_pixel_visibility (decision (vi))

// ---------------------------------------------------------------------------------------------
// K1: raygen.rgen:14-66
// ---------------------------------------------------------------------------------------------
struct RaygenArgs {
    DeviceScene scene;
    vhr_per_frame_data pfd;
    vhr_trace_params tp;
    const void *normals;     // RGBA16F
    const float *depth;      // D32F
    void *shadow_ao;         // RG16F
    void *reflections;       // RGBA16F or nullptr
    uint32_t width, height;  // launch size == image size
    uint32_t row_begin, row_end;
    uint32_t col_begin, col_end;     // screen tiles (vhr_set_tile): the columns the queue kernels trace -- col_begin a multiple of the tile
                                     // width, [0, width) otherwise; the per-pixel kernels trace whole rows (a superset)
    RayStats *stats;         // nullptr = off
    // "fuse_temporal": the queue kernel's tile epilogue runs svgf.comp for the tile's pixels (the dispatch the SVGF pass records next)
    uint32_t fuse_temporal;  // 0 = off
    TemporalArgs temporal;
    CostOrderArgs co;        // "raygen_cost_order" (the default queue kernel, the mirror-ray queue kernel)
    RayMaskArgs masks;       // ray cull masks: read by the kFilterMask instantiations only (last, so that no other argument moves)
};

// raygen.rgen:26-55 for one covered pixel: its shadow ray and its AO rays one after another (the walker with the whole of decision (vi): traverse<> ->
// ray_triangle).  STRIDE: the stack's (kTraceBlock: the per-pixel kernels' LDS columns; 1: a private array).
// FILTER (in every kernel of this file): kFilterAlpha ("alpha_test_rays" on a scene that can discard) -- a candidate gbuf_discarded names does not exist
// for the ray; kFilterMask (a ray-class mask that acts: vhr_context::ray_mask_acts) -- a candidate whose primitive's mask shares no bit with the ray's class mask
// does not exist, and by a.masks.alpha the alpha rule applies behind it.
template <int STRIDE, int FILTER = kFilterNone>
__device__ __forceinline__ void pixel_visibility(const RaygenArgs &a, const uint32_t x, const uint32_t y, const float depth, int *stack, uint32_t &overflow,
                                                 f3 &P, f3 &N, f3 &origin, float &shadow_payload, float &ao_payload) {
    const uint32_t W = a.width, H = a.height;
    const float u = (float(x) + 0.5f) / float(W);                                        // rgen:15-16
    const float v = (float(y) + 0.5f) / float(H);
    uint32_t rng = seed_thread((y * H + x) * a.pfd.frame_index);                         // rgen:17 (LaunchSize.y)
    P = get_world_space_position(a.pfd, depth, u, v);                                    // rgen:26
    const f3 L = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1],
                      a.pfd.directional_light.direction[2] };                            // rgen:27
    const f4 nid = load_rgba16f(a.normals, W, x, y);                                     // rgen:28
    N = f3{ nid.x, nid.y, nid.z };
    origin = P + N * a.tp.normal_bias;                                                   // rgen:29
    Hit hit;

    float rnd1 = random01(rng);                                                          // rgen:32-33
    float rnd2 = random01(rng);
    shadow_payload = 1.0f;
    if (a.tp.shadow_enable) {
        const f3 cone_dir = normalize3(uniform_sample_cone(rnd1, rnd2, a.tp.cone_cos_max));   // rgen:34
        const f3 dir = onb_transform(L, cone_dir);                                       // rgen:35,40
        // rgen:37-41 issues this trace four times with identical arguments; once is equivalent
        const bool occluded = traverse<true, STRIDE>(a.scene, origin, dir, a.tp.tmin, a.tp.tmax, stack, hit, overflow, ray_filter<FILTER>(a.scene, a.masks, a.masks.shadow));
        shadow_payload = occluded ? 0.0f : 1.0f;                                         // miss.rmiss:7
    }
    ao_payload = 0.0f;                                                                   // rgen:44-55
    for (uint32_t i = 0; i < a.tp.ao_spp; ++i) {
        rnd1 = random01(rng);
        rnd2 = random01(rng);
        const f3 rnd_dir = cosine_hemisphere(rnd1, rnd2);
        const f3 dir = onb_transform(N, rnd_dir);
        const bool occluded = traverse<true, STRIDE>(a.scene, origin, dir, a.tp.tmin, a.tp.ao_tmax, stack, hit, overflow, ray_filter<FILTER>(a.scene, a.masks, a.masks.ao));
        ao_payload += occluded ? 0.0f : 1.0f;
    }
    if (a.tp.ao_spp) ao_payload /= float(a.tp.ao_spp); else ao_payload = 1.0f;
}

// Decision (vi) in the any-hit queue kernel: a pixel one of whose rays met a candidate that contradicts itself is computed again, whole, by the per-pixel
// kernel's code (binary64 decisions inline) when its tile is done -- a call, so that the queue kernel's loops carry none of this (inlined in its leaf
// test the binary64 arithmetic cost the kernel 13 registers = a wave per SIMD, 1.3-1.5 % of the frame: profiles/r6_decision_vi_cost.txt).  `a` points at
// the launch's arguments where they lie in memory (the address of a by-value argument would copy all of it to every lane's scratch).  At 1080p:
// none to three pixels of a frame on the BASELINE stand-ins, up to ~70 on sponza_hard_rot (profiles/r6_decision_vi_cost.txt).
template <int FILTER = kFilterNone>
__device__ VHR_REDO_INLINE float2 redo_pixel_visibility(const RaygenArgs *a, const uint32_t x, const uint32_t y) {
    int st[kTraceStack];
    uint32_t overflow = 0;
    f3 P, N, origin;
    float shadow_payload, ao_payload;
    pixel_visibility<1, FILTER>(*a, x, y, a->depth[size_t(y) * a->width + x], st, overflow, P, N, origin, shadow_payload, ao_payload);
    return float2{ shadow_payload, ao_payload };
}

// raygen.rgen:14-66 for one pixel
template <int FILTER = kFilterNone>
__device__ __forceinline__ void raygen_pixel(const RaygenArgs &a, const uint32_t x, const uint32_t y, int *stack, uint32_t &overflow, bool &covered, bool &second_ray) {
    const uint32_t W = a.width;
    const float depth = a.depth[size_t(y) * W + x];                                      // rgen:19
    if (depth == 0.0f) {                                                                 // rgen:20-24
        store_rg16f(a.shadow_ao, W, x, y, 1.0f, 1.0f);
        if (a.reflections) store_rgba16f(a.reflections, W, x, y, 0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    covered = true;
    f3 P, N, origin;
    float shadow_payload, ao_payload;
    pixel_visibility<kTraceBlock, FILTER>(a, x, y, depth, stack, overflow, P, N, origin, shadow_payload, ao_payload);
    store_rg16f(a.shadow_ao, W, x, y, shadow_payload, ao_payload);                       // rgen:57

    if (a.reflections) {
        f4 payload = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
        if (a.tp.reflections) {                                                          // rgen:60-65
            const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
            const f3 I = normalize3(P - cam);
            const float ni2 = 2.0f * dot3(N, I);
            const f3 rdir = I - N * ni2;                                                 // reflect(I, N)
            payload = trace_reflection<kTraceBlock>(a.scene, a.pfd, a.tp, origin, rdir, stack, overflow, second_ray, ray_filter<FILTER>(a.scene, a.masks, a.masks.reflection));
        }
        store_rgba16f(a.reflections, W, x, y, payload.x, payload.y, payload.z, payload.w);
    }
}

template <int FILTER = kFilterNone>
__global__ __launch_bounds__(kTraceBlock) void raygen_kernel(const RaygenArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_stack[kTraceStack * kTraceBlock];
    int *stack = s_stack + threadIdx.x;
    uint32_t x, y;
    pixel_of_thread(x, y, a.row_begin);
    uint32_t overflow = 0;
    bool covered = false, second_ray = false;
    if (x < a.width && y < a.row_end) raygen_pixel<FILTER>(a, x, y, stack, overflow, covered, second_ray);
    if (a.stats) {
        const unsigned long long cov = __ballot(covered), ovf = __ballot(overflow != 0), sec = __ballot(second_ray);
        if ((threadIdx.x & 63u) == 0) {
            if (cov) atomicAdd(&a.stats->covered_pixels, (unsigned long long)__popcll(cov));
            if (ovf) atomicAdd(&a.stats->stack_overflows, (unsigned long long)__popcll(ovf));
            if (sec) atomicAdd(&a.stats->second_bounce_rays, (unsigned long long)__popcll(sec));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K1 (work-queue form): the same visibility rays as raygen_kernel, scheduled for wave64 occupancy.
//
// raygen.rgen traces its rays one after another per pixel, so on a SIMD machine every lane of a wave waits
// for the slowest lane of EACH ray (measured: 43 % of VALU lanes active).  Here a 16x16-pixel block first
// compacts its covered pixels (wave ballot + one LDS atomic per wave), which defines a block-local queue of
// `covered * (1 + ao_spp)` any-hit rays, kind-major (all shadow rays, then AO sample 0, AO sample 1, ...) so
// that rays in flight together are of one kind.  Lanes pull rays from the queue whenever at least
// `refill_threshold` lanes of the wave are idle -- one LDS atomic per refill, ranks from the idle ballot
// ("wavefront-ballot compaction") -- regenerate the ray from (pixel, kind) with raygen.rgen's exact arithmetic
// (the RNG state is recomputed from the seed), and walk the BVH one node or leaf per loop trip.  Visibility
// results are integers accumulated in LDS (order independent), so the output is bit-identical to the
// sequential form: shadow = !any_hit, ao = float(visible) / float(spp).  The mirror ray (closest hit +
// shading, a different register budget) runs in reflection_kernel.
// ---------------------------------------------------------------------------------------------
// raygen_queue_kernel<WAVES, COMPACT, SPILL, STATS>: every wave owns one 8x8-pixel tile (tile_rows < 8: fewer rows) and runs its own queue of
// `covered x (1 + ao_spp)` rays, kind-major, the shadow rays last.  COMPACT: the walk reads the 32-byte half-precision nodes (BvhNode16, two loads
// per visit; trees whose boxes do not fit the half range walk the 48-byte fp32 nodes instead).  SPILL: stack entries beyond the LDS levels
// live in scratch.  STATS: in-kernel counters and timers (vhr_set_ray_statistics).  Per covered pixel the wave keeps 5 words in LDS -- the ray
// origin and the G-buffer normal as the halves it is -- and recomputes the pixel's seed and the ray's direction at refill with raygen.rgen's
// exact arithmetic.
// FILTER: kFilterAlpha ("alpha_test_rays"): the leaf test asks gbuf_discarded about every consistent candidate before it ends the ray (DESIGN.md
// section 4b); kFilterMask: it first tests the primitive's mask byte against the class mask of the lane's ray kind.
template <int WAVES, bool COMPACT, bool SPILL, bool STATS, bool FUSE = false, int FILTER = kFilterNone>
__global__ __launch_bounds__(kQueueBlock *WAVES) __attribute__((amdgpu_waves_per_eu(VHR_K1_WAVES_MIN, 8))) void raygen_queue_kernel(const RaygenArgs a, const uint32_t stack_levels, const uint32_t refill_threshold,
                                                                          const uint32_t block_tiles_x, const uint32_t early_exit, const uint32_t tile_rows, const uint32_t steal_threshold, const Stamps st) {
    vhr_stamp(st);
    RayStats *const stats = STATS ? a.stats : nullptr;    // !STATS: counters and timers below are dead code (fewer VGPRs)
    extern __shared__ int s_dyn[];                    // per wave: (stack_levels + 3) x 64 ints
    const unsigned long long t_start = stats ? __builtin_readcyclecounter() : 0ull;
    unsigned long long t_setup = 0, t_refill = 0, t_nodes = 0, t_leaves = 0, n_refills = 0;
    __shared__ uint32_t s_vis_all[WAVES][kQueueBlock];    // bit k: the pixel's ray of kind k (0 = shadow, 1.. = AO) found an occluder
    __shared__ float s_ray_all[WAVES][5][kQueueBlock];    // per covered pixel: ray origin (3), the normal's half bits (2)
    __shared__ uint8_t s_list_all[WAVES][kQueueBlock];    // compacted covered pixels
    __shared__ float4 s_cut_all[WAVES][kCutMax][2];       // (lo.x, hi.x, lo.y, hi.y), (lo.z, hi.z, link, -)
    // (the compiler cannot know that threadIdx.x >> 6 is the same in every lane of a wave: said explicitly, what derives
    // from it -- the LDS bases, the wave's tile -- stays in scalar registers)
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t (&s_vis)[kQueueBlock] = s_vis_all[wave];
    float (&s_ray)[5][kQueueBlock] = s_ray_all[wave];
    uint8_t (&s_list)[kQueueBlock] = s_list_all[wave];
    float4 (&s_cut)[kCutMax][2] = s_cut_all[wave];
    // LDS stack rows: [0] = sentinel (what a pop of the empty stack returns), [1 .. stack_levels] = entries
    // 0 .. stack_levels-1, [stack_levels+1, +2] = dummies that absorb the accesses of entries living in scratch
    const unsigned long long t_cost0 = a.co.wave_cost ? __builtin_readcyclecounter() : 0ull;
    if constexpr (!STATS) {
        // "raygen_cost_order": the launch's first block orders the previous launch's blocks for the next one (8 * 64 * WAVES words <= the block's
        // (stack_levels + 3) * 64 * WAVES words of stack: the host asks for it only with >= 5 stack levels)
        if (a.co.order_out && blockIdx.x == 0u) order_blocks_by_cost<WAVES>(a.co.cost_prev, a.co.order_blocks, a.co.order_out, reinterpret_cast<uint32_t *>(s_dyn));
    }
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    const uint32_t W = a.width, H = a.height;
    uint32_t x, y;
    // "raygen_cost_order": the blocks that lived longest two launches ago start first (a launch ends with its last wave; a long-lived wave that
    // starts late is what the launch's end waits for)
    const uint32_t block_tile = a.co.block_order ? a.co.block_order[blockIdx.x] : blockIdx.x;
    tile_pixel<WAVES>(block_tile, block_tiles_x, wave, lane, a.row_begin, tile_rows, x, y, a.col_begin);
    const bool in_range = x < a.col_end && y < a.row_end && (lane >> 3) < tile_rows;
    bool covered = false;
    float depth = 0.0f;
    if (in_range) {
        depth = a.depth[size_t(y) * W + x];                                                  // rgen:19
        covered = depth != 0.0f;
        if (!covered) store_rg16f(a.shadow_ao, W, x, y, 1.0f, 1.0f);                         // rgen:20-21
    }
    s_vis[lane] = 0;
    const uint32_t first_kind = a.tp.shadow_enable ? 0u : 1u;
    const uint32_t last_kind = a.tp.ao_spp;           // kinds first_kind .. last_kind
    // without shadow rays the queue holds AO rays only and the cut is pruned to their reach (with them in the queue, letting the AO rays skip
    // the entries beyond their reach was measured: the test per entry costs sponza_proc what it saves bistro_proc, r4)
    const bool ao_only = first_kind != 0u;
    // A pixel's visibility word holds one "blocked" bit per ray kind (what lets several lanes share a ray: "raygen_steal") while the kinds fit a
    // word; with more than 30 AO samples it holds bit 0 for the shadow ray and, from bit 8 up, the COUNT of AO rays that escaped, and a ray is
    // walked by the one lane that fetched it.  Bit 31 (kRedoPixel) in either form: decision (vi) wants the pixel computed again (below).
    const bool kind_bits = last_kind <= 30u;
    const f3 L = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1], a.pfd.directional_light.direction[2] };
    f3 omin = f3{ 3.0e38f, 3.0e38f, 3.0e38f }, omax = f3{ -3.0e38f, -3.0e38f, -3.0e38f };   // bounds of the tile's ray origins
    float ao_reach = 0.0f;                                                                   // bound of tmax * |d| over this pixel's AO rays
    if (covered) {
        // ---- raygen.rgen:15-29 once per pixel (shared by all of the pixel's rays) ----
        const float u = (float(x) + 0.5f) / float(W);
        const float v = (float(y) + 0.5f) / float(H);
        const f3 P = get_world_space_position(a.pfd, depth, u, v);                           // rgen:26
        const uint2 nraw = reinterpret_cast<const uint2 *>(a.normals)[size_t(y) * W + x];    // rgen:28 (R16G16B16A16: nx ny | nz id)
        const f3 N = f3{ half_bits_to_float(uint16_t(nraw.x & 0xffffu)), half_bits_to_float(uint16_t(nraw.x >> 16)), half_bits_to_float(uint16_t(nraw.y & 0xffffu)) };
        const f3 origin = P + N * a.tp.normal_bias;                                          // rgen:29
        s_ray[0][lane] = origin.x; s_ray[1][lane] = origin.y; s_ray[2][lane] = origin.z;
        s_ray[3][lane] = __uint_as_float(nraw.x); s_ray[4][lane] = __uint_as_float(nraw.y);
        if (ao_only) ao_reach = a.tp.ao_tmax * onb_norm_bound(N);      // (wave-uniform condition)
        omin = origin; omax = origin;
    }
    const unsigned long long cov_mask = __ballot(covered);
    const uint32_t ncov = uint32_t(__popcll(cov_mask));
    if (covered) s_list[lane_rank(cov_mask)] = uint8_t(lane);
    wave_lds_sync();
    const uint32_t total = (a.scene.node_count == 0) ? 0u : ncov * (1u + last_kind - first_kind);
    uint32_t cut_n = 0;
    if (total) cut_n = build_tile_cut(a.scene, omin, omax, s_cut, lane, ao_only ? ao_reach : 3.0e38f, kCutMax, COMPACT ? int(sizeof(BvhNode16)) : int(sizeof(BvhNode48)),
                                      COMPACT ? f3{ a.scene.centre[0], a.scene.centre[1], a.scene.centre[2] } : f3{ 0.0f, 0.0f, 0.0f });
    const uint32_t n_cut_entries = cut_n;
    uint32_t emask = 0;                               // cut entries this lane's ray hits that did not fit its LDS stack
    if (stats) t_setup = __builtin_readcyclecounter() - t_start;

    f3 ro = f3{ 0, 0, 0 }, rd = f3{ 0, 0, 1 }, rinv = f3{ 0, 0, 0 }, noi = f3{ 0, 0, 0 }, ainv = f3{ 0, 0, 0 };
    float tmax = 0.0f;
    int cur = 0, sp = 0;
    int sbase = 0;                                    // "raygen_steal": stack rows 1 .. sbase have been taken by other lanes (row sbase holds a sentinel)
    uint32_t pix = 0, kind = 0;
    bool has = false;
    uint32_t next = 0;                                // queue head: wave-uniform, lives in a register
    uint32_t overflow = 0;
    uint32_t n_nodes = 0, n_leaves = 0, n_tris = 0, n_wave_trips = 0, n_drain_trips = 0;      // statistics (only flushed when stats)
    uint32_t n_drain_le4 = 0, n_drain_le8 = 0, n_drain_le16 = 0;
    // Stack entries beyond the LDS levels spill to a small private (scratch) array: any-hit walks rarely hold more than
    // a dozen pending subtrees, so the LDS part can be much shallower than the tree -- more waves per CU -- without
    // giving up the guarantee that kTraceStack entries can never overflow (the builder bounds the depth).
    int spill[SPILL ? kSpillStack : 1];
    const float tmin = a.tp.tmin;
    float tmin_v = tmin;                              // one VGPR copy for the asm-operand min/max of the slab test
    asm volatile("" : "+v"(tmin_v));
    for (;;) {
        // ---- refill idle lanes from the tile's ray queue (ranks from the idle ballot) ----
        const unsigned long long idle = __ballot(!has);
        const uint32_t n_idle = uint32_t(__popcll(idle));
        const unsigned long long t0 = stats ? __builtin_readcyclecounter() : 0ull;
        const bool queue_dry = next >= total;         // (before this trip's refill: the steal below reads the idle ballot taken above)
        if (next < total && (n_idle >= refill_threshold || n_idle == 64u)) {     // wave-uniform condition
            __builtin_amdgcn_s_setprio(0);            // (see below)
            ++n_refills;
            const uint32_t r = next + lane_rank(idle);
            next += n_idle;
            if (!has && r < total) {
                // k = r / ncov without the integer division (~25 instructions): the queue is kind-major, k < kinds
                uint32_t k = 0, rr = r;
                while (rr >= ncov) { rr -= ncov; ++k; }
                kind = last_kind - k;                 // the shadow rays (kind 0) at the END of the queue (r2: the AO rays' long drains overlap them)
                pix = s_list[rr];
                ro = f3{ s_ray[0][pix], s_ray[1][pix], s_ray[2][pix] };
                const uint32_t nxy = __float_as_uint(s_ray[3][pix]), nzw = __float_as_uint(s_ray[4][pix]);
                const uint32_t px = x - (lane & 7u) + (pix & 7u), py = y - (lane >> 3) + (pix >> 3);     // the tile's origin + the pixel's place in it
                rd = ray_direction(a.tp, seed_thread((py * H + px) * a.pfd.frame_index), kind, L,                            // rgen:17
                                   f3{ half_bits_to_float(uint16_t(nxy & 0xffffu)), half_bits_to_float(uint16_t(nxy >> 16)), half_bits_to_float(uint16_t(nzw & 0xffffu)) });
                tmax = kind == 0 ? a.tp.tmax : a.tp.ao_tmax;                                 // rgen:40,52
                f3 bo, bd;
                box_ray(a.scene, ro, rd, bo, bd);             // "bvh_frame": the slab tests' ray (ro, rd stay the triangle tests')
                rinv = f3{ cull_reciprocal(bd.x), cull_reciprocal(bd.y), cull_reciprocal(bd.z) };
                // COMPACT boxes are relative to the scene centre: shift the origin used by the slab test (only)
                const f3 oc = COMPACT ? f3{ bo.x - a.scene.centre[0], bo.y - a.scene.centre[1], bo.z - a.scene.centre[2] } : bo;
                noi = f3{ -(oc.x * rinv.x), -(oc.y * rinv.y), -(oc.z * rinv.z) };
                if (!COMPACT) ainv = f3{ fabsf(rinv.x), fabsf(rinv.y), fabsf(rinv.z) };
                sbase = 0;
                cut_to_stack(s_cut, cut_n, stack, stack_levels, rinv, noi, tmin_v, tmax, cur, sp, emask);      // (its boxes are relative to the centre `noi` is)
                has = true;
            }
        }
        // ---- the queue is dry: idle lanes take pending subtrees off the busy lanes' stacks ----
        // Any hit = OR over the subtrees a ray touches, in any order and by any lane: a lane with nothing left to fetch takes the top stack entry
        // of a busy lane and walks it for the same ray (the ray's registers come over by ds_bpermute).  One entry per busy lane and trip: the
        // walkers of a long ray double from trip to trip.  A lane whose ray another lane has meanwhile found blocked stops.
        if (steal_threshold && kind_bits && queue_dry && n_idle >= steal_threshold && n_idle != 64u) {         // wave-uniform
            if (has && ((s_vis[pix] >> kind) & 1u)) has = false;                                  // (the idle ballot above is one trip old for such a lane: it steals next trip)
            const bool donor = has && sp > sbase && uint32_t(sbase) < stack_levels;               // rows sbase + 1 .. sp are its own; row sbase + 1 is in LDS
            const unsigned long long dmask = __ballot(donor);
            if (dmask) {
                if (donor) s_list[lane_rank(dmask)] = uint8_t(lane);                              // (the list of covered pixels is not needed any more: the queue is dry)
                wave_lds_sync();
                const uint32_t nd = uint32_t(__popcll(dmask));
                const uint32_t r = lane_rank(idle);
                const bool thief = ((idle >> lane) & 1ull) && r < nd;
                const uint32_t d = thief ? uint32_t(s_list[r]) : lane;
                const int drow = __shfl(sbase, int(d)) + 1;                                       // the donor's LOWEST entry: the far child pushed first, the largest subtree it holds
                const int link = (stack - lane + d)[(thief ? uint32_t(drow) : 0u) * kQueueBlock];
                const float t_ox = __shfl(ro.x, int(d)), t_oy = __shfl(ro.y, int(d)), t_oz = __shfl(ro.z, int(d));
                const float t_dx = __shfl(rd.x, int(d)), t_dy = __shfl(rd.y, int(d)), t_dz = __shfl(rd.z, int(d));
                const float t_ix = __shfl(rinv.x, int(d)), t_iy = __shfl(rinv.y, int(d)), t_iz = __shfl(rinv.z, int(d));
                const float t_nx = __shfl(noi.x, int(d)), t_ny = __shfl(noi.y, int(d)), t_nz = __shfl(noi.z, int(d));
                const float t_ax = COMPACT ? 0.0f : __shfl(ainv.x, int(d)), t_ay = COMPACT ? 0.0f : __shfl(ainv.y, int(d)), t_az = COMPACT ? 0.0f : __shfl(ainv.z, int(d));
                const float t_tmax = __shfl(tmax, int(d));
                const uint32_t t_pk = uint32_t(__shfl(int(pix | (kind << 8)), int(d)));
                wave_lds_sync();
                if (donor && lane_rank(dmask) < n_idle) {                                         // its lowest entry has a taker: a sentinel in its place ends the donor's walk there
                    ++sbase;
                    stack[uint32_t(sbase) * kQueueBlock] = kStackSentinel;
                }
                if (thief) {
                    ro = f3{ t_ox, t_oy, t_oz }; rd = f3{ t_dx, t_dy, t_dz }; rinv = f3{ t_ix, t_iy, t_iz }; noi = f3{ t_nx, t_ny, t_nz };
                    if (!COMPACT) ainv = f3{ t_ax, t_ay, t_az };
                    tmax = t_tmax; pix = t_pk & 0xffu; kind = t_pk >> 8;
                    cur = link; sp = 0; sbase = 0; emask = 0;
                    has = true;
                }
                if (stats) ++n_refills;
            }
        }
        if (!__any(has)) break;                       // nothing in flight and (since all lanes were idle) nothing left to fetch
#ifdef VHR_K1_COUNT_TRIPS
        if (stats) ++n_drain_trips;                   // (scratch builds: the statistics' drain counter counts the outer loop's trips instead)
#endif
        // The walk is a chain of dependent round trips, the refill a block of arithmetic that nothing waits for: a wave in the walk goes first when
        // both want the SIMD (r3c: -1.4 % on sponza_proc, nothing on bistro_proc)
        __builtin_amdgcn_s_setprio(3);
        const unsigned long long t1 = stats ? __builtin_readcyclecounter() : 0ull;
        // ---- inner nodes: descend until this lane holds a leaf or its ray has run out of subtrees ----
        // The step is written without branches (selects + one unconditional LDS write and read per trip): divergent
        // if/else chains here cost more scalar exec-mask bookkeeping than the box tests themselves.  The write goes to
        // slot `sp` (level stack_levels - 1 at most: the builder bounds the depth), the read takes the current top.
        // Early exit: lanes leave this loop one by one (ray finished, or a leaf reached) and then idle until the LAST
        // walker leaves it.  With few leaf visits per any-hit ray that wait dominates (measured: 3.7 refills per 192-ray
        // tile, 44 % of the lanes active), so once the walkers have shrunk to a fraction of those that entered, the
        // loop is left: waiting lanes test their leaves, finished ones are refilled, the walkers resume where they were.
        bool found = false;
        const uint32_t nodes_before = n_nodes, tris_before = n_tris;
        const uint32_t walkers_in = uint32_t(__popcll(__ballot(has && cur >= 0)));
        while (has && cur >= 0) {
            if (uint32_t(__popcll(__ballot(true))) * 16u <= walkers_in * early_exit) break;   // ballot(true) = the walkers left; early_exit in 0..15 sixteenths, so the first trip always runs
            ++n_nodes;
            float tn0, tn1, tf0, tf1;
            int2 links;
            if (COMPACT) {
                // `cur` is the node's BYTE offset (index * 32); two 16-byte loads per visit
                const uint4 *np = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(a.scene.nodes16) + uint32_t(cur));
                const uint4 c0 = np[0], c1 = np[1];
                box_pair_ch16(c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, rinv, noi, tmin_v, tmax, tn0, tn1, tf0, tf1);
                links = int2{ int(c1.z), int(c1.w) };
            } else {
                const Node48Words nw = load_node48(a.scene.nodes48, cur);
                links = nw.links;
                box_pair_ch(nw.q0, nw.q1, nw.q2, rinv, ainv, noi, tmin_v, tmax, tn0, tn1, tf0, tf1);
            }
            // The hit tests as lane masks in scalar registers (cmp_le_mask): what combines them is scalar work, what uses them takes them as they are.
            const unsigned long long h0 = cmp_le_mask(tn0, tf0), h1 = cmp_le_mask(tn1, tf1);
            // Child 0 is entered if it is hit and child 1 is not, or is not nearer; the child NOT entered goes to the stack slot (a
            // meaningful entry only when both are hit).  Three selects and two carries per visit (r3; the (near, far) form took ten
            // vector instructions: masks are scalar work, selects are not).
            const unsigned long long enter0 = h0 & (~h1 | cmp_le_mask(tn0, tn1));
            const int nearc = select_mask(links.y, links.x, enter0), farc = select_mask(links.x, links.y, enter0);
            // One address serves both accesses: row min(sp, L+1) holds the top entry (sp - 1; the sentinel when the stack
            // is empty), the row after it is where entry sp goes.  The write is harmless when !both (above the top).
            int *const row = stack + min(uint32_t(sp), stack_levels + 1u) * kQueueBlock;
            int top = row[0];
            row[kQueueBlock] = farc;
            // deep entries: behind a wave-uniform test, so that the hot path keeps plain ds_read / ds_write (an
            // if-converted "LDS or scratch" access becomes a flat load plus ten instructions of pointer selection)
            if (__any(uint32_t(sp) >= stack_levels)) {
                if (SPILL && uint32_t(sp) > stack_levels) top = spill[(uint32_t(sp) - 1u - stack_levels) & uint32_t(kSpillStack - 1)];
                if (uint32_t(sp) >= stack_levels) {
                    if (SPILL && uint32_t(sp) - stack_levels < uint32_t(kSpillStack)) spill[uint32_t(sp) - stack_levels] = farc;
                    else overflow |= uint32_t((h0 & h1) >> lane) & 1u;            // cannot happen (builder depth bound); counted
                }
            }
            cur = select_mask(top, nearc, h0 | h1);                               // no child hit: popping the empty stack yields the sentinel
            {   // sp += h0 + h1 - 1: +1 both, 0 one, -1 none (with the sentinel) -- two add-with-carry, the hit masks as the carries
                int t;
                unsigned long long carry_out;
                asm("v_addc_co_u32_e64 %0, %1, %2, -1, %3" : "=v"(t), "=s"(carry_out) : "v"(sp), "s"(h0));
                asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(sp), "=s"(carry_out) : "v"(t), "s"(h1));
            }
        }
#ifdef VHR_K1_COUNT_IDLE
        // (scratch builds, profiles/r6_k1_postponed_leaf.txt) who sat out how many trips of this pass through the node loop: lanes holding a leaf -- what a
        // postponed-leaf step could have kept walking -- and lanes without a ray.  [drain_le4, drain_le8, drain_le16] = lane-trips of walkers, holders, the rest.
        if (stats) {
            const uint32_t mine = n_nodes - nodes_before;
            uint32_t tot = mine;
            for (int off = 32; off > 0; off >>= 1) tot = max(tot, uint32_t(__shfl_xor(int(tot), off)));
            const bool holder = has && cur < 0 && cur != kStackSentinel;
            uint32_t w = mine, hl = holder ? tot - mine : 0u, fr = holder ? 0u : tot - mine;
            for (int off = 32; off > 0; off >>= 1) { w += uint32_t(__shfl_xor(int(w), off)); hl += uint32_t(__shfl_xor(int(hl), off)); fr += uint32_t(__shfl_xor(int(fr), off)); }
            n_drain_le4 += w; n_drain_le8 += hl; n_drain_le16 += fr;
        }
#endif
        const unsigned long long t2 = stats ? __builtin_readcyclecounter() : 0ull;
        // ---- leaf ----
        // one memory round trip per triangle: its three loads are issued together and the test has no early return (with
        // ray_triangle() the compiler sinks the load of v0 behind the `det == 0` return: two dependent round trips per test).
        // (r3c-r5 the NEXT triangle's loads were in flight while this one was tested: -1.3 % on sponza_proc, +0.7 % on bistro_proc.  With the
        // consistency test of decision (vi) the triangle's nine floats live to the end of the test, and next to a second triangle's nine the
        // kernel needed 68 registers -- a wave per SIMD; without the prefetch 59.  Measured equal: 0.4558 / 0.4569 ms.  Verifying candidates
        // outside the loop on a triangle fetched again kept the prefetch at 62 registers and cost more: 0.469 ms -- a found ray is no rarity.)
        auto test_leaf = [&](const int code) {
            const uint32_t vv = ~uint32_t(code);
            const uint32_t first = vv >> 2, count = (vv & 3u) + 1u;
            ++n_leaves;
            const BvhTri *const leaf = a.scene.tris + first;
            for (uint32_t i = 0; i < count; ++i) {
                ++n_tris;
                const float4 ta = reinterpret_cast<const float4 *>(leaf + i)[0], tb = reinterpret_cast<const float4 *>(leaf + i)[1];
                const float tcx = reinterpret_cast<const float *>(leaf + i)[8];
                const f3 v0 = f3{ ta.x, ta.y, ta.z }, e1 = f3{ ta.w, tb.x, tb.y }, e2 = f3{ tb.z, tb.w, tcx };
                float ct, cu, cv;
                // (the consistency test behind the candidates only: few tests get this far, and a wave whose lanes all failed skips it)
                if (mt_candidate(ro, rd, v0, e1, e2, tmin, tmax, ct, cu, cv)) {
                    if (solution_consistent(ro, rd, v0, e1, e2, ct, cu, cv)) {
                        // the candidate filter ray_filter<FILTER>(a.scene, a.masks, kind == 0 ? a.masks.shadow : a.masks.ao) spelled out: the object costs STATS builds a spilled VGPR
                        if constexpr (FILTER == kFilterAlpha) { if (gbuf_discarded(a.scene, first + i, cu, cv)) continue; }      // GbufDiscard
                        if constexpr (FILTER == kFilterMask) {          // RayMaskReject, the ray's class by its kind
                            if ((uint32_t(a.masks.prim_masks[leaf[i].prim]) & (kind == 0 ? a.masks.shadow : a.masks.ao)) == 0u) continue;
                            if (a.masks.alpha && gbuf_discarded(a.scene, first + i, cu, cv)) continue;
                        }
                        found = true;
                        break;
                    }
                    // decision (vi): a candidate that contradicts itself is decided again in binary64 -- not here: the pixel is marked and computed
                    // again when the tile is done (redo_pixel_visibility), the walk goes on as if the candidate had missed
                    atomicOr(&s_vis[pix], kRedoPixel);
                }
            }
        };
        if (has && cur < 0 && cur != kStackSentinel) {
            test_leaf(cur);
            if (!found) {                                                          // pop (the sentinel if nothing is pending)
                cur = stack[min(uint32_t(sp), stack_levels + 1u) * kQueueBlock];
                if (SPILL && __any(uint32_t(sp) > stack_levels)) {
                    if (uint32_t(sp) > stack_levels) cur = spill[(uint32_t(sp) - 1u - stack_levels) & uint32_t(kSpillStack - 1)];
                }
                --sp;
            }
        }
        if (has && !found && cur == kStackSentinel && emask) {                 // overflowed cut entries: next subtree
            const int e = __ffs(int(emask)) - 1;
            emask &= emask - 1u;
            cur = __float_as_int(s_cut[e][1].z);
            sp = 0;                                   // the pop of the empty stack left it at -1
            sbase = 0;                                // (every row is this lane's own again)
        }
        const bool finished = found || cur == kStackSentinel;
        if (has && finished) {
            has = false;
            if (kind_bits) { if (found) atomicOr(&s_vis[pix], 1u << kind); }                  // miss.rmiss:7 leaves 1.0 where nothing is found
            else if (kind == 0) { if (found) atomicOr(&s_vis[pix], 1u); }
            else if (!found) atomicAdd(&s_vis[pix], 256u);
        }
        if (stats) {       // wave-level trip counts of the two inner loops = the slowest lane's (for lane utilisation)
            const unsigned long long t3 = __builtin_readcyclecounter();
            t_refill += t1 - t0; t_nodes += t2 - t1; t_leaves += t3 - t2;
            uint32_t tn = n_nodes - nodes_before, tt = n_tris - tris_before;
            for (int off = 32; off > 0; off >>= 1) { tn = max(tn, uint32_t(__shfl_xor(int(tn), off))); tt = max(tt, uint32_t(__shfl_xor(int(tt), off))); }
            n_wave_trips += tn + tt;
            if (next >= total) {
#ifndef VHR_K1_COUNT_TRIPS
                n_drain_trips += tn + tt;    // trips made after the tile's queue ran dry (nothing left to refill with)
#endif
                const uint32_t live = uint32_t(__popcll(__ballot(has)));   // rays still in flight after this round of trips
#ifndef VHR_K1_COUNT_IDLE
                if (live <= 4u) n_drain_le4 += tn + tt;
                if (live <= 8u) n_drain_le8 += tn + tt;
                if (live <= 16u) n_drain_le16 += tn + tt;
#endif
            }
        }
    }
    wave_lds_sync();
    float shadow_payload = 1.0f, ao_payload = 1.0f;                                          // rgen:20-21 for a pixel without geometry
    uint32_t n_redo = 0;
    if (covered) {
        const uint32_t vis = s_vis[lane];
        shadow_payload = (vis & 1u) ? 0.0f : 1.0f;
        if (a.tp.ao_spp) ao_payload = float(a.scene.node_count == 0 ? a.tp.ao_spp : (kind_bits ? a.tp.ao_spp - uint32_t(__popc(vis >> 1)) : (vis >> 8))) / float(a.tp.ao_spp);   // rgen:55: the AO rays that escaped
        if (vis & kRedoPixel) {                           // decision (vi): one of this pixel's rays met a candidate that contradicts itself
            static_assert(offsetof(RaygenArgs, scene) == 0, "the launch's arguments start with `a`");
            const float2 again = redo_pixel_visibility<FILTER>(reinterpret_cast<const RaygenArgs *>((const void *)__builtin_amdgcn_kernarg_segment_ptr()), x, y);
            shadow_payload = again.x; ao_payload = again.y;
            n_redo = 1;
        }
        store_rg16f(a.shadow_ao, W, x, y, shadow_payload, ao_payload);                       // rgen:57
    }
    if (a.co.wave_cost && lane == 0) a.co.wave_cost[block_tile * uint32_t(WAVES) + wave] = uint32_t(min(__builtin_readcyclecounter() - t_cost0, 0xffffffffull));
    // ---- "fuse_temporal": svgf.comp for this tile's pixels, right here ----
    // svgf.comp reads of the CURRENT frame only the pixel's own texels; everything else it gathers is the previous frame's.  So the
    // wave that has just finished a tile can run it for the tile: the visibility goes from LDS into the filter (rounded to the halves
    // the image holds, which is also what is stored), the normals are the ones the set-up loaded, and the gathers of 16 200 x 2 waves
    // spread over the launch instead of forming a kernel of their own that waits on memory.
    if constexpr (FUSE) {                             // (an instantiation of its own: the epilogue's registers and code stay out of the plain launch)
        if (a.fuse_temporal) {                                                               // (uniform)
            const TemporalArgs &t = a.temporal;
            if (in_range && x >= t.col_begin && x < t.limit_x && y >= t.row_begin && y < t.row_end && y < t.limit_y) {
                const uint2 nraw = reinterpret_cast<const uint2 *>(a.normals)[size_t(y) * W + x];
                const float2 cur = unpack_rg16f(pack_rg16f(shadow_payload, ao_payload));     // what the RG16F image holds
                svgf_temporal_pixel(t, x, y, unpack_rgba16f(nraw), cur.x, cur.y);
            }
        }
    }
    if (stats) {
        const unsigned long long ovf = __ballot(overflow != 0);
        if (lane == 0) {
            if (cov_mask) atomicAdd(&stats->covered_pixels, (unsigned long long)__popcll(cov_mask));
            if (ovf) atomicAdd(&stats->stack_overflows, (unsigned long long)__popcll(ovf));
            atomicAdd(&stats->wave_iterations, (unsigned long long)n_wave_trips);
            atomicAdd(&stats->drain_iterations, (unsigned long long)n_drain_trips);
            atomicAdd(&stats->drain_le4, (unsigned long long)n_drain_le4);
            atomicAdd(&stats->drain_le8, (unsigned long long)n_drain_le8);
            atomicAdd(&stats->drain_le16, (unsigned long long)n_drain_le16);
            atomicAdd(&stats->cycles_total, __builtin_readcyclecounter() - t_start);
            atomicAdd(&stats->cycles_setup, t_setup);
            atomicAdd(&stats->cycles_refill, t_refill);
            atomicAdd(&stats->cycles_nodes, t_nodes);
            atomicAdd(&stats->cycles_leaves, t_leaves);
            atomicAdd(&stats->refills, n_refills);
            atomicAdd(&stats->waves, 1ull);
            atomicAdd(&stats->cut_entries, (unsigned long long)n_cut_entries);
        }
        const unsigned long long redo = __ballot(n_redo != 0);
        if (redo && lane == 0) atomicAdd(&stats->pending_rays, (unsigned long long)__popcll(redo));
        // wave-reduced first: 64 same-address atomics per wave serialise at the memory side (the diagnostic launch took 3.4 ms)
        for (int off = 32; off > 0; off >>= 1) { n_nodes += uint32_t(__shfl_xor(int(n_nodes), off)); n_leaves += uint32_t(__shfl_xor(int(n_leaves), off)); n_tris += uint32_t(__shfl_xor(int(n_tris), off)); }
        if (lane == 0) {
            atomicAdd(&stats->node_visits, (unsigned long long)n_nodes);
            atomicAdd(&stats->leaf_visits, (unsigned long long)n_leaves);
            atomicAdd(&stats->triangle_tests, (unsigned long long)n_tris);
        }
    }
}

// Mirror ray of raygen.rgen:59-65 (closest hit, reflection_hit.rchit / reflection_miss.rmiss) for one pixel of the image
template <int STRIDE, int FILTER = kFilterNone>
__device__ __forceinline__ f4 reflection_payload(const RaygenArgs &a, const uint32_t x, const uint32_t y, int *stack, bool &second_ray) {
    const uint32_t W = a.width, H = a.height;
    f4 payload = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const float depth = a.depth[size_t(y) * W + x];
    if (depth != 0.0f && a.tp.reflections) {
        const float u = (float(x) + 0.5f) / float(W), v = (float(y) + 0.5f) / float(H);
        const f3 P = get_world_space_position(a.pfd, depth, u, v);
        const f4 nid = load_rgba16f(a.normals, W, x, y);
        const f3 N = f3{ nid.x, nid.y, nid.z };
        const f3 origin = P + N * a.tp.normal_bias;
        const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
        const f3 I = normalize3(P - cam);
        const float ni2 = 2.0f * dot3(N, I);
        const f3 rdir = I - N * ni2;
        uint32_t overflow = 0;
        payload = trace_reflection<STRIDE>(a.scene, a.pfd, a.tp, origin, rdir, stack, overflow, second_ray, ray_filter<FILTER>(a.scene, a.masks, a.masks.reflection));
    }
    return payload;
}
template <int FILTER = kFilterNone>
__device__ __forceinline__ void reflection_pixel(const RaygenArgs &a, const uint32_t x, const uint32_t y, int *stack, bool &second_ray) {
    const f4 payload = reflection_payload<kTraceBlock, FILTER>(a, x, y, stack, second_ray);
    store_rgba16f(a.reflections, a.width, x, y, payload.x, payload.y, payload.z, payload.w);
}

// Decision (vi) in the mirror ray's queue kernel: a pixel whose ray (first or second bounce) met a candidate whose fp32 solution contradicts itself is
// computed again, whole, by the per-pixel kernel's code (binary64 decisions inline) when its tile is shaded -- a call, so that the queue's walk carries
// none of this: inlined in its leaf test the binary64 arithmetic made the two-bounce kernel spill 45 registers (launch +13 %), a list of the candidates
// per ray decided by a call at the ray's commit still cost +7 % (profiles/r6_decision_vi_cost.txt).  `a` points at the launch's arguments where they lie
// in memory (the address of a by-value argument would copy all of it to every lane's scratch: 1.4 KB a lane, and the launch took four times as long for
// the waves the scratch ring then had room for).  About one pixel of a 1080p frame on the BASELINE stand-ins, ~70-100 on sponza_hard_rot.  `second`: a second-bounce ray was
// traced (the launch's ray count).
struct RedoReflection { f4 payload; uint32_t second; };
template <int FILTER = kFilterNone>
__device__ __attribute__((noinline)) RedoReflection redo_pixel_reflection(const RaygenArgs *a, const uint32_t x, const uint32_t y) {
    int st[kTraceStack];
    bool second_ray = false;
    const f4 payload = reflection_payload<1, FILTER>(*a, x, y, st, second_ray);
    return RedoReflection{ payload, second_ray ? 1u : 0u };
}

// ... one pixel per thread
template <int FILTER = kFilterNone>
__global__ __launch_bounds__(kTraceBlock) void reflection_kernel(const RaygenArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_refl_stack[kTraceStack * kTraceBlock];
    int *stack = s_refl_stack + threadIdx.x;
    uint32_t x, y;
    pixel_of_thread(x, y, a.row_begin);
    bool second_ray = false;
    if (x < a.width && y < a.row_end) reflection_pixel<FILTER>(a, x, y, stack, second_ray);
    if (a.stats) {
        const unsigned long long sec = __ballot(second_ray);
        if ((threadIdx.x & 63u) == 0 && sec) atomicAdd(&a.stats->second_bounce_rays, (unsigned long long)__popcll(sec));
    }
}

// ---------------------------------------------------------------------------------------------
// Mirror ray, work-queue form (the default for one bounce): closest-hit traversal with the node step of raygen_queue_kernel.
//
// Every wave owns a 16x8-pixel tile = a queue of up to 128 mirror rays.  Phase 1 (whole wave, twice): raygen.rgen:15-29,60-63
// per pixel -- origin and reflect(I, N) parked in LDS, covered pixels compacted with a ballot.  Phase 2: lanes pull rays from
// the queue whenever `refill_threshold` of them are idle and walk the BVH "while-while": the branch-free inner-node step
// (packed-FMA slabs against 1/d and -o/d, near child first, far child pushed, boxes culled against the closest t so far),
// then the leaf's <= 4 Moeller-Trumbore tests with the (t, flat index) order of decision (vi).  A finished ray leaves its
// hit record (triangle, u, v) in the LDS slot its origin came from.  Phase 3 (whole wave, twice): reflection_hit.rchit on
// the records -- the texture fetches and the BRDF run with all lanes active instead of inside the divergent walk.
// Results are those of reflection_kernel bit for bit: the same rays, the same intersection arithmetic, the same shader.
// ---------------------------------------------------------------------------------------------
// raygen.rgen:15-16, 26-29, 60-61 for one covered pixel: the mirror ray's origin and direction
__device__ __forceinline__ void mirror_ray_of_pixel(const RaygenArgs &a, f3 cam, uint32_t x, uint32_t y, float depth, f3 &origin, f3 &rdir) {
    const uint32_t W = a.width, H = a.height;
    const float u = (float(x) + 0.5f) / float(W), v = (float(y) + 0.5f) / float(H);          // rgen:15-16
    const f3 P = get_world_space_position(a.pfd, depth, u, v);                               // rgen:26
    const f4 nid = load_rgba16f(a.normals, W, x, y);                                         // rgen:28
    const f3 N = f3{ nid.x, nid.y, nid.z };
    origin = P + N * a.tp.normal_bias;                                                       // rgen:29
    const f3 I = normalize3(P - cam);                                                        // rgen:60
    const float ni2 = 2.0f * dot3(N, I);
    rdir = I - N * ni2;                                                                      // rgen:61 reflect(I, N)
}

// FILTER: the walk's candidate filter is GbufDiscard ("alpha_test_rays") or RayMaskReject ("reflection_ray_mask"); phase 3's redo applies it as well.
template <bool SPILL, int BOUNCES, bool STATS = false, int FILTER = kFilterNone>
__global__ __launch_bounds__(kQueueBlock * 2) __attribute__((amdgpu_waves_per_eu(7, 7))) void reflection_queue_kernel(
    const RaygenArgs a, const uint32_t stack_levels, const uint32_t refill_threshold, const uint32_t tiles_x, const uint32_t tiles_total,
    const uint32_t early_exit, const Stamps st) {
    vhr_stamp(st);
    extern __shared__ int s_dyn[];                        // per wave: (stack_levels + 3) x 64 ints, see raygen_queue_kernel
    // rows 0-2 origin -> hit record (triangle, u, v), rows 3-5 direction; two bounces: rows 6-8 second origin -> second record,
    // and rows 3-5 are rewritten with the second direction between the two walks.
    // A wave's tile is 8 x 8 pixels, one ray per lane (r5; 16 x 8 before).  The launch waits on the latency of its walks -- 4 KB of LDS padding per
    // workgroup, 5.5 -> 4.5 waves per SIMD, cost it 16-23 % -- and its LDS, not its registers, set the occupancy: with 128 rays per wave 14 080 B
    // per workgroup of two waves (11 workgroups per CU = 5.5 waves per SIMD; two bounces 17 152 B = 4.5 waves).  With 64 rays 10 880 / 12 416 B:
    // 7 / 6.5 waves (69-72 registers admit 7).  One bounce 261-265 -> 244-250 us (sponza_proc 1080p), 444-450 -> 435 us (bistro_proc); two bounces
    // 626 -> 508 us, 963 -> 854 us.  (Recomputing a ray from its pixel at the queue's fetch instead of parking it in LDS -- 9 344 B -- was equal
    // or slower than parking it: the ~120 instructions per ray eat what the last half wave per SIMD buys; 8 waves at 64 registers bought nothing.)
    constexpr int ROWS = BOUNCES > 1 ? 9 : 6;
    constexpr uint32_t SUBS = 1u;                         // 8-pixel-wide sub-tiles per wave (the loops below are written for any number)
    constexpr int RAYS = 64 * int(SUBS);
    __shared__ float s_ray_all[2][ROWS][RAYS];
    __shared__ uint8_t s_list_all[2][RAYS];               // compacted covered pixels
    __shared__ float4 s_cut_all[2][kCutMax][2];           // the tile's shared descent (build_tile_cut), once per walk
    __shared__ uint32_t s_redo_all[2][RAYS / 32];         // decision (vi): bit p = pixel p is computed again in phase 3 (redo_pixel_reflection)
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    // "raygen_cost_order" for this launch (see raygen_queue_kernel): the first block sorts the previous launch's blocks before its own tiles
    const unsigned long long t_cost0 = a.co.wave_cost ? __builtin_readcyclecounter() : 0ull;
    if (a.co.order_out && blockIdx.x == 0u) order_blocks_by_cost<2>(a.co.cost_prev, a.co.order_blocks, a.co.order_out, reinterpret_cast<uint32_t *>(s_dyn));
    const uint32_t block = a.co.block_order ? a.co.block_order[blockIdx.x] : blockIdx.x;
    const uint32_t tile = block * 2u + wave;
    if (tile >= tiles_total) return;                      // waves of a block share nothing and never synchronise
    float (&s_ray)[ROWS][RAYS] = s_ray_all[wave];
    uint8_t (&s_list)[RAYS] = s_list_all[wave];
    uint32_t (&s_redo)[RAYS / 32] = s_redo_all[wave];
    if (lane < uint32_t(RAYS / 32)) s_redo[lane] = 0u;
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    const uint32_t W = a.width;
    const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };

    // ---- phase 1: per-pixel ray setup, whole wave ----
    unsigned long long covered_mask[SUBS];
    uint32_t ncov = 0;
    f3 omin = f3{ 3.0e38f, 3.0e38f, 3.0e38f }, omax = f3{ -3.0e38f, -3.0e38f, -3.0e38f };   // bounds of this walk's ray origins
    auto grow = [&](f3 o) {
        omin = f3{ fminf(omin.x, o.x), fminf(omin.y, o.y), fminf(omin.z, o.z) };
        omax = f3{ fmaxf(omax.x, o.x), fmaxf(omax.y, o.y), fmaxf(omax.z, o.z) };
    };
#pragma unroll
    for (uint32_t sub = 0; sub < SUBS; ++sub) {
        const uint32_t x = a.col_begin + tile_x * (8u * SUBS) + sub * 8u + (lane & 7u), y = a.row_begin + tile_y * 8u + (lane >> 3);
        const bool in_range = x < a.col_end && y < a.row_end;
        const float depth = in_range ? a.depth[size_t(y) * W + x] : 0.0f;                    // rgen:19
        const bool covered = depth != 0.0f;
        if (in_range && !covered) store_rgba16f(a.reflections, W, x, y, 0.0f, 0.0f, 0.0f, 0.0f);   // rgen:22
        const uint32_t p = sub * 64u + lane;
        if (covered) {
            f3 origin, rdir;
            mirror_ray_of_pixel(a, cam, x, y, depth, origin, rdir);
            s_ray[0][p] = origin.x; s_ray[1][p] = origin.y; s_ray[2][p] = origin.z;
            s_ray[3][p] = rdir.x; s_ray[4][p] = rdir.y; s_ray[5][p] = rdir.z;
            grow(origin);
        }
        const unsigned long long m = __ballot(covered);
        covered_mask[sub] = m;
        if (covered) s_list[ncov + lane_rank(m)] = uint8_t(p);
        ncov += uint32_t(__popcll(m));
    }
    wave_lds_sync();
    uint32_t total = a.scene.node_count == 0 ? 0u : ncov;
    const bool traced = total != 0;

    // ---- phase 2: the queue (once per bounce) ----
    uint32_t overflow = 0, second_rays = 0;
    WalkCounters wc;
    const unsigned long long t_walk0 = STATS ? __builtin_readcyclecounter() : 0ull;
    unsigned long long t_walk = 0;
#pragma unroll 1
    for (int bounce = 0; bounce < BOUNCES; ++bounce) {
    const int orow = bounce ? 6 : 0;                      // where this bounce's origins sit and its hit records go
    // (first bounce only: the second bounce's origins are scattered over the scene, their descent ends at once -- measured: no gain)
    const uint32_t cut_n = total && bounce == 0 ? build_tile_cut_uniform(a.scene, omin, omax, s_cut_all[wave], lane) : 0u;
    const unsigned long long tw0 = STATS ? __builtin_readcyclecounter() : 0ull;
    wave_queue_walk<SPILL, true, STATS>(
        a.scene, stack, stack_levels, lane, total, refill_threshold, early_exit, a.tp.tmin, a.tp.tmax, false, overflow, s_cut_all[wave], cut_n,
        [&](uint32_t r, uint32_t &pix, f3 &ro, f3 &rd) {
            pix = s_list[r];
            ro = f3{ s_ray[orow][pix], s_ray[orow + 1][pix], s_ray[orow + 2][pix] };
            rd = f3{ s_ray[3][pix], s_ray[4][pix], s_ray[5][pix] };
        },
        [&](uint32_t pix, uint32_t tri, float u, float v) {                                  // the hit record replaces the ray's origin
            s_ray[orow][pix] = __uint_as_float(tri); s_ray[orow + 1][pix] = u; s_ray[orow + 2][pix] = v;
        }, &wc,
        [&](uint32_t pix) { atomicOr(&s_redo[pix >> 5], 1u << (pix & 31u)); },                    // decision (vi): the pixel is computed again in phase 3
        ray_filter<FILTER>(a.scene, a.masks, a.masks.reflection));
    wave_lds_sync();
    if (STATS) t_walk += __builtin_readcyclecounter() - tw0;
    if constexpr (BOUNCES > 1) if (bounce == 0) {
        // ---- second-bounce rays (trace_reflection's arithmetic), whole wave: a mirror ray from every first hit ----
        uint32_t n2 = 0;
#pragma unroll
        for (uint32_t sub = 0; sub < SUBS; ++sub) {
            const uint32_t p = sub * 64u + lane;
            const bool was_covered = traced && ((covered_mask[sub] >> lane) & 1ull);
            const uint32_t tri = was_covered ? __float_as_uint(s_ray[0][p]) : kNoHit;
            const bool hit1 = tri != kNoHit;
            if (hit1) {
                Hit h;
                h.t = 0.0f; h.u = s_ray[1][p]; h.v = s_ray[2][p]; h.tri_index = tri; h.flat = 0;
                f3 hp, hn;
                hit_position_normal(a.scene, h, hp, hn);
                const f3 rdir = f3{ s_ray[3][p], s_ray[4][p], s_ray[5][p] };
                const f3 nn = normalize3(hn);
                const float ni = dot3(nn, rdir);
                const f3 nf = ni < 0.0f ? nn : -nn;
                const f3 d2 = rdir - nn * (2.0f * ni);
                const f3 o2 = hp + nf * a.tp.normal_bias;
                s_ray[6][p] = o2.x; s_ray[7][p] = o2.y; s_ray[8][p] = o2.z;
                s_ray[3][p] = d2.x; s_ray[4][p] = d2.y; s_ray[5][p] = d2.z;
            }
            const unsigned long long m = __ballot(hit1);
            if (hit1) s_list[n2 + lane_rank(m)] = uint8_t(p);
            n2 += uint32_t(__popcll(m));
        }
        wave_lds_sync();
        total = n2;
        second_rays = n2;
    }
    }

    // ---- phase 3: reflection_hit.rchit / reflection_miss.rmiss on the records, whole wave ----
    uint32_t n_redo = 0;
    int redo_second = 0;
#pragma unroll
    for (uint32_t sub = 0; sub < SUBS; ++sub) {
        if (!((covered_mask[sub] >> lane) & 1ull)) continue;
        const uint32_t x = a.col_begin + tile_x * (8u * SUBS) + sub * 8u + (lane & 7u), y = a.row_begin + tile_y * 8u + (lane >> 3);
        const uint32_t p = sub * 64u + lane;
        f4 payload = f4{ 0.0f, 0.0f, 0.0f, 0.0f };                                           // reflection_miss.rmiss:7
        const uint32_t tri = traced ? __float_as_uint(s_ray[0][p]) : kNoHit;
        if (traced && ((s_redo[p >> 5] >> (p & 31u)) & 1u)) {                                // decision (vi): this pixel's ray asked for binary64
            static_assert(offsetof(RaygenArgs, scene) == 0, "the launch's arguments start with `a`");
            const RedoReflection again = redo_pixel_reflection<FILTER>(reinterpret_cast<const RaygenArgs *>((const void *)__builtin_amdgcn_kernarg_segment_ptr()), x, y);
            payload = again.payload;
            ++n_redo;
            if (BOUNCES > 1) redo_second += int(again.second) - int(tri != kNoHit);          // (the launch's count of second-bounce rays)
        } else if (tri != kNoHit) {
            Hit h;
            h.t = 0.0f; h.u = s_ray[1][p]; h.v = s_ray[2][p]; h.tri_index = tri; h.flat = 0;
            if constexpr (BOUNCES > 1) {
                f4 second = f4{ 0.0f, 0.0f, 0.0f, 0.0f };                                    // reflection_miss.rmiss:7
                const uint32_t tri2 = __float_as_uint(s_ray[6][p]);
                if (tri2 != kNoHit) {
                    Hit h2;
                    h2.t = 0.0f; h2.u = s_ray[7][p]; h2.v = s_ray[8][p]; h2.tri_index = tri2; h2.flat = 0;
                    second = shade_reflection_hit(a.scene, a.pfd, h2);
                }
                payload = shade_reflection_hit(a.scene, a.pfd, h, &second);
            } else {
                payload = shade_reflection_hit(a.scene, a.pfd, h);
            }
        }
        store_rgba16f(a.reflections, W, x, y, payload.x, payload.y, payload.z, payload.w);   // rgen:65
    }
    if (a.stats) {
        for (int off = 32; off > 0; off >>= 1) { n_redo += uint32_t(__shfl_xor(int(n_redo), off)); redo_second += __shfl_xor(redo_second, off); }
        second_rays = uint32_t(int(second_rays) + redo_second);
        if (lane == 0) {
            if (overflow) atomicAdd(&a.stats->stack_overflows, 1ull);
            if (second_rays) atomicAdd(&a.stats->second_bounce_rays, (unsigned long long)second_rays);
            if (n_redo) atomicAdd(&(a.stats + 1)->pending_rays, (unsigned long long)n_redo);
        }
    }
    if constexpr (STATS) {
        // the mirror-ray launch's own counters: the second RayStats of the buffer (vhr_get_reflection_statistics)
        RayStats *const rs = a.stats + 1;
        uint32_t n_nodes = wc.nodes, n_leaves = wc.leaves, n_tris = wc.triangles;
        for (int off = 32; off > 0; off >>= 1) { n_nodes += uint32_t(__shfl_xor(int(n_nodes), off)); n_leaves += uint32_t(__shfl_xor(int(n_leaves), off)); n_tris += uint32_t(__shfl_xor(int(n_tris), off)); }
        if (lane == 0) {
            atomicAdd(&rs->node_visits, (unsigned long long)n_nodes);
            atomicAdd(&rs->leaf_visits, (unsigned long long)n_leaves);
            atomicAdd(&rs->triangle_tests, (unsigned long long)n_tris);
            atomicAdd(&rs->wave_iterations, (unsigned long long)wc.wave_trips);
            atomicAdd(&rs->unique_rays, (unsigned long long)(ncov + second_rays));
            atomicAdd(&rs->covered_pixels, (unsigned long long)ncov);
            atomicAdd(&rs->second_bounce_rays, (unsigned long long)second_rays);
            atomicAdd(&rs->refills, (unsigned long long)wc.refills);
            atomicAdd(&rs->waves, 1ull);
            atomicAdd(&rs->cycles_total, __builtin_readcyclecounter() - t_walk0);          // set-up + walks + shading, this wave
            atomicAdd(&rs->cycles_nodes, t_walk);                                           // the walks alone (both bounces)
        }
    }
    if (a.co.wave_cost && lane == 0) a.co.wave_cost[tile] = uint32_t(min(__builtin_readcyclecounter() - t_cost0, 0xffffffffull));
}

// "alpha_test_rays", read at every launch: the alpha instantiations run only where the switch is on AND some primitive of the scene can discard
// (vhr_update_geometry looked); everywhere else the launches are the ones they were before the switch existed.
static bool alpha_rays(const vhr_context *ctx) { return ctx->alpha_test_rays != 0 && ctx->scene_can_discard; }


// The shadow / AO launch itself, by the options in force (everything launch_raygen decided is in `a`).  `alpha`: alpha_rays() as launch_raygen
// saw it, `filter`: the launch's launch_filter() (a launch held back for "fuse_temporal" has neither).
static void issue_raygen(vhr_context *ctx, const RaygenArgs &a_in, const uint32_t width, const uint32_t height, const bool alpha = false, const int filter = kFilterNone) {
    RaygenArgs a = a_in;
    a.co = CostOrderArgs{};
    (void)height;
    ctx->time_begin(kKernelRaygen);
    if (alpha) ++ctx->alpha_launches;
    if (filter == kFilterMask) ++ctx->mask_launches;
    if (ctx->options[kOptRaygenVariant] == 0) {
        with_filter(filter, [&](auto al) { launch(ctx, raygen_kernel<decltype(al)::value>, dim3((width + 15) / 16, (a.row_end - a.row_begin + 15) / 16), dim3(kTraceBlock), 0, a); });
    } else {
        const uint32_t rows_traced = a.row_end - a.row_begin;
        // rows of a wave's tile: 8, or ("raygen_tile_rows" 0 = auto, the default) 6 for a launch whose 8x8 tiles would fill less than 70 % of the
        // chip's wave slots -- a single partial round of waves lasts as long as its slowest wave, and a wave with three quarters of the rays
        // lives shorter: the 540 x 570 rectangle of a 1080p / 8 screen tile 97.7 -> 89.9 us (4 rows: 90.2); whole frames and larger tiles keep
        // 8 rows (a 990 x 570 tile: 122 us either way, 128 with 4 rows)
        uint32_t tile_rows = uint32_t(std::max(0, std::min(8, ctx->options[kOptRaygenTileRows])));
        if (tile_rows == 0u) {
            const uint64_t tiles8 = uint64_t((a.col_end - a.col_begin + 7) / 8) * ((rows_traced + 7) / 8), slots = uint64_t(ctx->cu_count) * 32u;
            tile_rows = tiles8 * 10u < slots * 7u ? 6u : 8u;
        }
        const uint32_t tiles_x = (a.col_end - a.col_begin + 7) / 8, tiles_y = (rows_traced + tile_rows - 1) / tile_rows;
        const int waves = ctx->options[kOptWavesPerBlock];
        const uint32_t wv = waves >= 4 ? 4u : (waves >= 2 ? 2u : 1u);
        const QueueLaunch q = queue_launch(ctx, kOptLdsStackLevels, kOptEarlyExit, wv);
        const bool compact = ctx->options[kOptCompactNodes] != 0 && ctx->nodes16_valid;      // the 32-byte half-precision nodes (two loads per visit instead of three)
        const uint32_t n_blocks = ((tiles_x + wv - 1u) / wv) * tiles_y;
        {   // "raygen_cost_order" (see vhr_context::CostOrder)
            const uint32_t key = (tiles_x * 2654435761u) ^ (tiles_y * 40503u) ^ (wv << 28) ^ (tile_rows << 24) ^ (a.row_begin * 97u) ^ (a.col_begin * 193u);
            if (!a.stats && q.levels >= 5u) prepare_cost_order(ctx, ctx->cost_order_raygen, n_blocks, wv, key, a.co, { tiles_x, (tiles_x + wv - 1u) / wv, wv, 8u, tile_rows, a.col_begin, a.row_begin });
        }
        const uint32_t steal = uint32_t(std::max(0, std::min(63, ctx->options[kOptRaygenSteal])));
        auto go = [&](auto kernel) { launch(ctx, kernel, dim3(n_blocks), dim3(kQueueBlock * wv), q.lds_bytes, a, q.levels, q.threshold, (tiles_x + wv - 1u) / wv, q.early_exit, tile_rows, steal); };
        auto by_flags = [&](auto waves_c) {
            constexpr int WV = decltype(waves_c)::value;
            with_bool(q.spill, [&](auto sp) {
                constexpr bool SP = decltype(sp)::value;
                if (a.fuse_temporal && compact && !a.stats && filter == kFilterNone) {   // "fuse_temporal": svgf.comp in the tiles' epilogues (the default node form only)
                    go(raygen_queue_kernel<WV, true, SP, false, true>);
                    return;
                }
                with_bool(compact, [&](auto co) {
                    with_bool(a.stats != nullptr, [&](auto st) { with_filter(filter, [&](auto al) {
                        go(raygen_queue_kernel<WV, decltype(co)::value, SP, decltype(st)::value, false, decltype(al)::value>);
                    }); });
                });
            });
        };
        if (wv == 4u) by_flags(std::integral_constant<int, 4>{});
        else if (wv == 2u) by_flags(std::integral_constant<int, 2>{});
        else by_flags(std::integral_constant<int, 1>{});
    }
    ctx->time_end(kKernelRaygen);
}

// "fuse_temporal": a TraceRays whose shadow / AO launch was held back (launch_raygen) is issued now -- with svgf.comp fused into the
// tiles' epilogues if `fuse` is the dispatch the SVGF pass has just recorded for the very images this launch works on, alone otherwise.
// Called by flush_recorded (with or without `fuse`) and, without, by everything that enqueues on or waits for the stream in between
// (vhr::launch, sync_streams, image copies, pass epilogues and external callbacks, the end of vhr_graph_execute).
struct DeferredRaygen { RaygenArgs a; uint32_t width, height; };
int flush_deferred_raygen(vhr_context *ctx, const TemporalArgs *fuse) {
    if (!ctx->deferred_raygen) return VHR_OK;
    DeferredRaygen d;
    std::memcpy(&d, ctx->deferred_raygen_blob.data(), sizeof(d));
    ctx->deferred_raygen = false;                      // (first: the launch below goes through vhr::launch, which would flush again)
    if (fuse) { d.a.fuse_temporal = 1u; d.a.temporal = *fuse; }
    PassDescription *const running = ctx->cur_pass;
    ctx->cur_pass = ctx->deferred_pass;               // the stamps (and the time) are the ray-tracing pass's
    issue_raygen(ctx, d.a, d.width, d.height);
    if (ctx->deferred_pass && ctx->deferred_pass->stamped_in_kernel) {
        ctx->pending_end = &ctx->d_stamps[ctx->deferred_pass->stamp_index].end;      // stored by the next kernel on the stream
        ctx->deferred_pass->timed = true;
    }
    ctx->cur_pass = running;
    ctx->deferred_pass = nullptr;
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "raygen kernel launch failed");
    return VHR_OK;
}
bool deferred_raygen_matches(const vhr_context *ctx, const TemporalArgs &t) {
    if (!ctx->deferred_raygen) return false;
    DeferredRaygen d;
    std::memcpy(&d, ctx->deferred_raygen_blob.data(), sizeof(d));
    // the dispatch reads this launch's two images and covers exactly the pixels the launch covers (whole-image work)
    return t.raytraced == d.a.shadow_ao && static_cast<const void *>(t.normals) == d.a.normals && t.width == d.a.width && t.height == d.a.height &&
           t.col_begin == 0 && t.row_begin == 0 && t.limit_x == d.a.width && t.row_end >= d.a.height && t.limit_y >= d.a.height &&
           d.a.col_begin == 0 && d.a.row_begin == 0 && d.a.col_end == d.a.width && d.a.row_end == d.a.height;
}

int launch_raygen(vhr_context *ctx, const vhr_per_frame_data &pfd, uint32_t width, uint32_t height, const Image &normals,
                  const Image &depth, Image &shadow_ao, Image *reflections) {
    if (width != normals.width || height != normals.height || width != depth.width || height != depth.height ||
        width != shadow_ao.width || height != shadow_ao.height || (reflections && (reflections->width != width || reflections->height != height)))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "TraceRays: launch size must equal the extent of the pass images");
    RaygenArgs a;
    a.fuse_temporal = 0u;
    a.temporal = TemporalArgs{};
    a.co = CostOrderArgs{};
    a.scene = ctx->device_scene();
    a.pfd = pfd;
    a.tp = ctx->trace_params;
    a.normals = normals.ptr;
    a.depth = static_cast<const float *>(depth.ptr);
    a.shadow_ao = shadow_ao.ptr;
    a.reflections = reflections ? reflections->ptr : nullptr;
    a.width = width;
    a.height = height;
    const uint32_t owned_begin = std::min(ctx->row_begin, height), owned_end = std::min(ctx->row_end, height);
    a.row_begin = owned_begin;
    a.row_end = owned_end;
    // screen tiles: the owned columns, on 16-pixel tile boundaries (a few columns more than owned are harmless: rays are per pixel)
    const uint32_t owned_col_begin = std::min(ctx->col_begin, width), owned_col_end = std::min(ctx->col_end, width);
    a.col_begin = owned_col_begin & ~15u;
    a.col_end = owned_col_end;
    a.stats = ctx->ray_stats_enabled ? ctx->d_ray_stats : nullptr;
    ctx->raytraced_pixels = 0;                 // ray statistics are the hybrid path's again
    ctx->alpha_launches = 0;
    ctx->mask_launches = 0;
    if (a.row_end <= a.row_begin || a.col_end <= a.col_begin) return VHR_OK;
    if (ctx->options[kOptTraceOverlap]) {      // strips / tiles: trace the margin the denoiser recomputes too (no exchange of raw visibility)
        a.row_begin = owned_begin > ctx->overlap ? owned_begin - ctx->overlap : 0u;
        a.row_end = uint32_t(std::min<uint64_t>(height, uint64_t(owned_end) + ctx->overlap));
        a.col_begin = (owned_col_begin > ctx->overlap ? owned_col_begin - ctx->overlap : 0u) & ~15u;
        a.col_end = uint32_t(std::min<uint64_t>(width, uint64_t(owned_col_end) + ctx->overlap));
    }
    if (const int rc = ray_stats_begin(ctx, a.stats != nullptr, 2u)) return rc;      // [0] shadow / AO launch, [1] mirror-ray launch
    // "fuse_temporal" (opt-in): hold the launch back until the next pass shows its first command -- if that is svgf.comp on this launch's
    // images, the queue kernel runs it in its tiles' epilogues (flush_deferred_raygen).  Only the default kernel has that epilogue, only
    // whole-image work on one stream qualifies, and only a pass nobody hooked an epilogue to (its owner expects the image when it runs).
    // With "alpha_test_rays" in force the launch is not held back: the epilogue has no alpha instantiation, the SVGF pass runs its own dispatch.
    // The ray-class masks likewise: where the shadow or the AO mask acts the launch filters and is not held back.  (The per-pixel kernel of
    // "raygen_variant" 0 traces the mirror ray too: one launch, one filter for the three classes.)
    const bool alpha = alpha_rays(ctx);
    a.masks = RayMaskArgs{ nullptr, uint32_t(ctx->shadow_ray_mask), uint32_t(ctx->ao_ray_mask), uint32_t(ctx->reflection_ray_mask), alpha ? 1u : 0u };
    const bool mirror_acts = a.reflections && a.tp.reflections && ctx->ray_mask_acts(a.masks.reflection);
    const bool visibility_acts = ctx->ray_mask_acts(a.masks.shadow) || ctx->ray_mask_acts(a.masks.ao) || (ctx->options[kOptRaygenVariant] == 0 && mirror_acts);
    if (visibility_acts || mirror_acts) {
        if (const int rc = ensure_device_prim_masks(ctx)) return rc;
        a.masks.prim_masks = ctx->d_prim_masks;
    }
    const int filter = launch_filter(visibility_acts, alpha);
    {
        // (the epilogue exists in the queue kernel on the 32-byte nodes only: issue_raygen)
        const bool default_kernel = ctx->options[kOptRaygenVariant] != 0 && ctx->options[kOptCompactNodes] != 0 && ctx->nodes16_valid;
        const bool whole = a.row_begin == 0 && a.row_end == height && a.col_begin == 0 && a.col_end == width;
        const bool mirror = a.reflections && a.tp.reflections;
        if (ctx->options[kOptFuseTemporal] && filter == kFilterNone && ctx->may_defer_raygen && default_kernel && whole && !mirror && !a.stats && ctx->frames_in_flight == 1 &&
            (ctx->in_kernel_stamps() || !ctx->options[kOptPassTimestamps]) && a.scene.node_count != 0) {
            a.fuse_temporal = 0u;
            DeferredRaygen d;
            std::memset(static_cast<void *>(&d), 0, sizeof(d));
            d.a = a; d.width = width; d.height = height;
            ctx->deferred_raygen_blob.resize(sizeof(d));
            std::memcpy(ctx->deferred_raygen_blob.data(), &d, sizeof(d));
            ctx->deferred_raygen = true;
            ctx->deferred_pass = ctx->cur_pass;
            return VHR_OK;
        }
    }
    issue_raygen(ctx, a, width, height, alpha, filter);
    // The mirror ray's launch (raygen.rgen:59-65): not denoised, so owned rows (and columns) only.  It runs BEHIND the shadow / AO launch: beside it
    // (a second stream) the two take as long as one after the other, and with walk and shading in two launches the walk is no faster
    // (profiles/r4_reflection_concurrent.txt, r4d/r4e logs in profiles/r4_reflection_split.txt).
    if (ctx->options[kOptRaygenVariant] != 0 && a.reflections && a.tp.reflections) {
        RaygenArgs m = a;
        m.row_begin = owned_begin;
        m.row_end = owned_end;
        m.col_begin = owned_col_begin & ~15u;
        m.col_end = owned_col_end;
        // "reflection_async": on a stream of its own, behind the shadow / AO launch and beside whatever the caller's stream does next (the SVGF
        // pass, which reads nothing of it).  One stream and event pair per context; the caller's stream joins at the next external pass, at the
        // end of the frame, and wherever the library waits or hands images out.
        hipStream_t const main_stream = ctx->stream;
        PassDescription *const main_pass = ctx->cur_pass;
        bool on_own_stream = false;
        if (ctx->options[kOptReflectionAsync] && ctx->frames_in_flight == 1 && !m.stats) {
            bool ok = true;
            if (!ctx->refl_stream)
                ok = hipStreamCreateWithFlags(&ctx->refl_stream, hipStreamNonBlocking) == hipSuccess &&
                     hipEventCreateWithFlags(&ctx->refl_ready, VHR_JOIN_EVENT_FLAGS) == hipSuccess &&
                     hipEventCreateWithFlags(&ctx->refl_done, VHR_JOIN_EVENT_FLAGS) == hipSuccess;
            if (ok && ctx->refl_pending) ok = ctx->join_refl() == VHR_OK;                    // (one launch at a time on that stream)
            ok = ok && hipEventRecord(ctx->refl_ready, ctx->stream) == hipSuccess && hipStreamWaitEvent(ctx->refl_stream, ctx->refl_ready, 0) == hipSuccess;
            if (ok) {
                on_own_stream = true;
                ctx->stream = ctx->refl_stream;
                ctx->cur_pass = nullptr;             // the pass's time stamps stay on the caller's stream
                ctx->no_stamps = true;
            }
        }
        ctx->time_begin(kKernelReflection);
        if (alpha) ++ctx->alpha_launches;
        const int mirror_filter = launch_filter(mirror_acts, alpha);
        if (mirror_filter == kFilterMask) ++ctx->mask_launches;
        if (m.tp.reflections <= 2 && ctx->options[kOptReflectionVariant] != 0) {
            const QueueLaunch q = queue_launch(ctx, kOptReflectionLdsStackLevels, kOptReflectionEarlyExit, 2u);
            const TileGrid g = tile_grid(m.col_end - m.col_begin, owned_end - owned_begin, 8u);      // (reflection_queue_kernel: 8 x 8 pixels per wave)
            m.co = CostOrderArgs{};
            if (q.levels >= 5u && !m.stats)                // "raygen_cost_order" for the mirror-ray launch (its own lifetimes and orders)
                prepare_cost_order(ctx, ctx->cost_order_reflection, (g.tiles_total + 1u) / 2u, 2u,
                                   (g.tiles_x * 2654435761u) ^ (g.tiles_total * 40503u) ^ (uint32_t(m.tp.reflections) << 28) ^ (m.row_begin * 97u) ^ (m.col_begin * 193u), m.co,
                                   { g.tiles_x, g.tiles_x, 1u, 8u, 8u, m.col_begin, m.row_begin });
            with_bool(q.spill, [&](auto sp) { with_bool(m.tp.reflections == 2, [&](auto two) { with_bool(m.stats != nullptr, [&](auto st) {
                constexpr bool SP = decltype(sp)::value, ST = decltype(st)::value;
                constexpr int B = decltype(two)::value ? 2 : 1;
                with_filter(mirror_filter, [&](auto al) {
                    launch(ctx, reflection_queue_kernel<SP, B, ST, decltype(al)::value>, g.grid, g.block, q.lds_bytes, m, q.levels, q.threshold, g.tiles_x, g.tiles_total, q.early_exit);
                });
            }); }); });
        } else {
            with_filter(mirror_filter, [&](auto al) { launch(ctx, reflection_kernel<decltype(al)::value>, dim3((width + 15) / 16, (owned_end - owned_begin + 15) / 16), dim3(kTraceBlock), 0, m); });
        }
        ctx->time_end(kKernelReflection);
        if (on_own_stream) {
            ctx->no_stamps = false;
            ctx->cur_pass = main_pass;
            const bool rec = hipEventRecord(ctx->refl_done, ctx->refl_stream) == hipSuccess;
            ctx->stream = main_stream;
            ctx->refl_pending = true;
            ctx->refl_writes = m.reflections;
            ctx->refl_reads[0] = m.normals; ctx->refl_reads[1] = m.depth;
            if (!rec) return ctx->fail(VHR_ERROR_DEVICE, "hipEventRecord(mirror-ray stream) failed");
        }
    }
    return ray_stats_end(ctx, a.stats != nullptr, "raygen kernel launch failed", 2u);
}

}  // namespace vhr
