// What happens to a tree after kernels_bvh.hip has built it, on the device: the refit (vhr_refit_geometry), the partial refit
// (vhr_refit_geometry_partial), the settle pass of "object_motion_vectors", the three passes of vhr_rebuild_geometry around the build, and the
// tree's SAH cost.  Exact arithmetic like the builder's (compiled without FMA contraction): a refit's records and boxes are the host twin's
// (csrc/bvh_build.cpp) bit for bit.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vhr_internal.hpp"
#include "bvh_math.hpp"
#include "bvh_device.hpp"

namespace vhr {
namespace {

// ---- refit (vhr_refit_geometry): the topology stays, the records and the boxes follow the vertices and the transforms ----
struct RefitFrame { float r[9]; uint32_t on; float magnitude; };      // magnitude: the world magnitude the tree's padding was built with (0 on the world axes)
struct RefitCounters { unsigned long long non_finite, records_outside, children_outside, differing, beyond; };      // differing: "object_motion_vectors" only; beyond: the part of non_finite that is finite and beyond the frame's magnitude
// the leaf pass: record k re-derived in its slot from (prim, tri) with bvh_math::world_record; three 16-byte loads' worth of gather per corner,
// three 16-byte stores
// one record from its primitive's transform and its three vertices (absolute indices `vi`): the one place a refit of either kind derives a
// record; `now`: what it stored; returns the coordinates met that the tree cannot hold: non-finite ones in the low 16 bits and, in a frame, those
// beyond f.magnitude in the high 16 (at most 9 each per record: a wave's sum keeps them apart)
__device__ __forceinline__ uint32_t refit_write_record(float4 *slot, const float4 &q2, const vhr_primitive &pr, const vhr_vertex *__restrict__ vertices, const uint32_t vi[3],
                                                       const RefitFrame &f, float4 now[3]) {
    float v0[3], e1[3], e2[3];
    const uint32_t bad = bvh_math::world_record(pr.transform, vertices[vi[0]].pos, vertices[vi[1]].pos, vertices[vi[2]].pos, v0, e1, e2) +
                         (bvh_math::coordinates_beyond(v0, e1, e2, f.magnitude, f.on != 0u) << 16);
    now[0] = float4{ v0[0], v0[1], v0[2], e1[0] };
    now[1] = float4{ e1[1], e1[2], e2[0], e2[1] };
    now[2] = float4{ e2[2], q2.y, q2.z, q2.w };
    slot[0] = now[0]; slot[1] = now[1]; slot[2] = now[2];
    return bad;
}
// a wave's sum of refit_write_record's results into the two counters (non_finite counts both kinds: vhr_get_refit_statistics out[5])
__device__ __forceinline__ void count_unholdable(RefitCounters *counters, uint32_t bad) {
    atomicAdd(&counters->non_finite, (unsigned long long)((bad & 0xffffu) + (bad >> 16)));
    if (bad >> 16) atomicAdd(&counters->beyond, (unsigned long long)(bad >> 16));
}
// "object_motion_vectors" (the MOTION instantiations; vhr_context::d_prev_saved has the rules): per record its state before the last successful
// refit, the whole 48 bytes in the same slot, and the number of the refit that last saved it.  `epoch`: the number of the refit that is running.
struct RefitMotion { BvhTri *prev; uint32_t *saved; uint32_t epoch; };
__device__ __forceinline__ uint32_t motion_differs(const float4 a[3], const float4 b[3]) {      // in any of the nine words, as bits
    uint32_t x = (__float_as_uint(a[0].x) ^ __float_as_uint(b[0].x)) | (__float_as_uint(a[0].y) ^ __float_as_uint(b[0].y)) | (__float_as_uint(a[0].z) ^ __float_as_uint(b[0].z)) |
                 (__float_as_uint(a[0].w) ^ __float_as_uint(b[0].w));
    x |= (__float_as_uint(a[1].x) ^ __float_as_uint(b[1].x)) | (__float_as_uint(a[1].y) ^ __float_as_uint(b[1].y)) | (__float_as_uint(a[1].z) ^ __float_as_uint(b[1].z)) |
         (__float_as_uint(a[1].w) ^ __float_as_uint(b[1].w));
    x |= __float_as_uint(a[2].x) ^ __float_as_uint(b[2].x);
    return x != 0u ? 1u : 0u;
}
// record k is about to be rewritten (`slot` still holds its old words, q2 the third of them): its previous state into `was`, saved first unless a
// failed attempt of this refit has saved it already (the slot then holds that attempt's values, the previous array the state to keep)
__device__ __forceinline__ void motion_save(const RefitMotion &m, uint32_t k, const float4 *slot, const float4 &q2, float4 was[3]) {
    float4 *pslot = reinterpret_cast<float4 *>(m.prev + k);
    if (m.saved[k] != m.epoch) {
        was[0] = slot[0]; was[1] = slot[1]; was[2] = q2;
        pslot[0] = was[0]; pslot[1] = was[1]; pslot[2] = was[2];
        m.saved[k] = m.epoch;
    } else {
        was[0] = pslot[0]; was[1] = pslot[1]; was[2] = pslot[2];
    }
}
template <bool MOTION>
__global__ __launch_bounds__(256) void k0_refit_records_kernel(const vhr_vertex *__restrict__ vertices, const uint32_t *__restrict__ indices,
                                                               const vhr_primitive *__restrict__ primitives, uint32_t primitive_count, uint32_t n,
                                                               BvhTri *__restrict__ tris, RefitCounters *__restrict__ counters, const RefitMotion motion, const RefitFrame f) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t bad = 0, differs = 0;
    if (k < n) {
        float4 *slot = reinterpret_cast<float4 *>(tris + k);
        const float4 q2 = slot[2];                                   // (e2.z, prim, tri, flat)
        const uint32_t p = __float_as_uint(q2.y), local = __float_as_uint(q2.z);
        if (p < primitive_count) {
            const vhr_primitive &pr = primitives[p];
            uint32_t vi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) vi[c] = pr.vertex_offset + indices[pr.index_offset + 3u * local + uint32_t(c)];
            float4 was[3], now[3];
            if constexpr (MOTION) motion_save(motion, k, slot, q2, was);
            bad = refit_write_record(slot, q2, pr, vertices, vi, f, now);
            if constexpr (MOTION) differs = motion_differs(was, now);
        } else {
            bad = 1u;                                                // (not a record of this scene: cannot happen, never dereferenced)
        }
    }
    for (int off = 32; off > 0; off >>= 1) bad += uint32_t(__shfl_xor(int(bad), off));
    if ((threadIdx.x & 63u) == 0u && bad) count_unholdable(counters, bad);
    if constexpr (MOTION) {
        for (int off = 32; off > 0; off >>= 1) differs += uint32_t(__shfl_xor(int(differs), off));
        if ((threadIdx.x & 63u) == 0u && differs) atomicAdd(&counters->differing, (unsigned long long)differs);
    }
}
// The partial refit's mark and leaf pass, one thread per record: a record with its primitive in a primitive range or one of its three absolute
// vertex indices in a vertex range is dirty -- re-derived as above, and its leaf's node and that node's ancestors get their dirty bit (one
// vector atomicOr per step; the climb ends at the first bit somebody else has set, so every node is counted once).  A clean record costs its
// (prim, tri) words and three index reads, and no store.  MOTION: a clean record also costs its `saved` word; one the refit before this one
// saved has stopped and is settled (previous = current), one a failed whole-tree attempt of this refit saved keeps its previous and is compared.
// A pass that then FAILS (non-finite coordinates) has settled those records all the same: until the retry succeeds the context's differing count
// (vhr_get_object_motion_statistics out[1]) is the last successful refit's and no longer describes the arrays -- which nothing may trace meanwhile.
// The contract holds after the retry: the dirty set only grows, and a settled record it reaches is saved again from its unchanged slot.
constexpr uint32_t kNoParent = 0xffffffffu;
struct PartialCounters { unsigned long long dirty_records, dirty_nodes; };
template <bool MOTION>
__global__ __launch_bounds__(256) void k0_refit_mark_kernel(const vhr_vertex *__restrict__ vertices, const uint32_t *__restrict__ indices,
                                                            const vhr_primitive *__restrict__ primitives, uint32_t primitive_count, uint32_t n,
                                                            BvhTri *__restrict__ tris, const uint32_t *__restrict__ owner, const uint32_t *__restrict__ parent,
                                                            uint32_t *__restrict__ dirty, RefitDirty ranges, RefitCounters *__restrict__ counters,
                                                            PartialCounters *__restrict__ partial, const RefitMotion motion, const RefitFrame f) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t bad = 0, records = 0, nodes = 0, differs = 0;
    if (k < n) {
        float4 *slot = reinterpret_cast<float4 *>(tris + k);
        const float4 q2 = slot[2];                                   // (e2.z, prim, tri, flat)
        const uint32_t p = __float_as_uint(q2.y), local = __float_as_uint(q2.z);
        if (p < primitive_count) {
            const vhr_primitive &pr = primitives[p];
            uint32_t vi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) vi[c] = pr.vertex_offset + indices[pr.index_offset + 3u * local + uint32_t(c)];
            if (ranges.primitives.holds(p) || ranges.vertices.holds(vi[0]) || ranges.vertices.holds(vi[1]) || ranges.vertices.holds(vi[2])) {
                float4 was[3], now[3];
                if constexpr (MOTION) motion_save(motion, k, slot, q2, was);
                bad = refit_write_record(slot, q2, pr, vertices, vi, f, now);
                if constexpr (MOTION) differs = motion_differs(was, now);
                records = 1u;
                for (uint32_t node = owner[k]; node != kNoParent; node = parent[node]) {
                    const uint32_t bit = 1u << (node & 31u);
                    if (atomicOr(&dirty[node >> 5], bit) & bit) break;
                    ++nodes;
                }
            } else if constexpr (MOTION) {
                const uint32_t saved = motion.saved[k];
                float4 *pslot = reinterpret_cast<float4 *>(motion.prev + k);
                if (saved == motion.epoch - 1u) {
                    pslot[0] = slot[0]; pslot[1] = slot[1]; pslot[2] = q2;
                } else if (saved == motion.epoch) {
                    const float4 was[3] = { pslot[0], pslot[1], pslot[2] }, now[3] = { slot[0], slot[1], q2 };
                    differs = motion_differs(was, now);
                }
            }
        } else {
            bad = 1u;                                                // (not a record of this scene: cannot happen, never dereferenced)
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        bad += uint32_t(__shfl_xor(int(bad), off)); records += uint32_t(__shfl_xor(int(records), off)); nodes += uint32_t(__shfl_xor(int(nodes), off));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (bad) count_unholdable(counters, bad);
        if (records) atomicAdd(&partial->dirty_records, (unsigned long long)records);
        if (nodes) atomicAdd(&partial->dirty_nodes, (unsigned long long)nodes);
    }
    if constexpr (MOTION) {
        for (int off = 32; off > 0; off >>= 1) differs += uint32_t(__shfl_xor(int(differs), off));
        if ((threadIdx.x & 63u) == 0u && differs) atomicAdd(&counters->differing, (unsigned long long)differs);
    }
}
// the settle pass of a refit call with nothing pending (number `epoch`): what refit epoch - 1 saved has stopped
__global__ __launch_bounds__(256) void k0_motion_settle_kernel(const BvhTri *__restrict__ tris, uint32_t n, const RefitMotion motion) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n || motion.saved[k] != motion.epoch - 1u) return;
    const float4 *slot = reinterpret_cast<const float4 *>(tris + k);
    float4 *pslot = reinterpret_cast<float4 *>(motion.prev + k);
    pslot[0] = slot[0]; pslot[1] = slot[1]; pslot[2] = slot[2];
}
// ---- rebuild in place (vhr_rebuild_geometry; vhr_internal.hpp has the carry-over's rules) ----
// Three bandwidth-bound passes, one thread per element, nothing but loads, stores and one count.
// The finiteness pass: vertices written through VHR_UPDATE_DEVICE_MEMORY are unvalidated, and a NaN must not reach the builder's bin index.  A
// vertex is 56 bytes, so its position is 8-byte aligned and no more: one 8-byte and one 4-byte load (the other 44 bytes are not read).  The
// count is of coordinates, by their exponent bits (all ones: inf or NaN); reduced over the wave, one vector atomic per wave that met any.
__global__ __launch_bounds__(256) void k0_rebuild_finite_kernel(const vhr_vertex *__restrict__ vertices, uint32_t n, unsigned long long *__restrict__ non_finite) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    uint32_t bad = 0;
    if (v < n) {
        const float2 xy = *reinterpret_cast<const float2 *>(vertices[v].pos);
        const float z = vertices[v].pos[2];
        const uint32_t w[3] = { __float_as_uint(xy.x), __float_as_uint(xy.y), __float_as_uint(z) };
#pragma unroll
        for (int a = 0; a < 3; ++a) bad += (w[a] & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) bad += uint32_t(__shfl_xor(int(bad), off));
    if ((threadIdx.x & 63u) == 0u && bad) atomicAdd(non_finite, (unsigned long long)bad);
}
// The gather, before the old tree is freed: record k's 48 bytes to flat[record.flat] (the flat index is the record's last word).  A record a
// failed refit attempt of number `epoch` saved gives its previous record (its slot holds the attempt's values).  The references a presplit tree
// holds of one triangle carry the same words, so their stores to one flat slot do not race for the result.  A flat index outside the scene's
// triangles cannot happen and is never used as an address.
__global__ __launch_bounds__(256) void k0_rebuild_gather_kernel(const BvhTri *__restrict__ tris, uint32_t n, const RefitMotion motion, uint32_t flat_count,
                                                                BvhTri *__restrict__ flat) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const float4 *slot = reinterpret_cast<const float4 *>((motion.saved[k] == motion.epoch ? motion.prev : tris) + k);
    const float4 q0 = slot[0], q1 = slot[1], q2 = slot[2];
    const uint32_t f = __float_as_uint(q2.w);
    if (f >= flat_count) return;
    float4 *out = reinterpret_cast<float4 *>(flat + f);
    out[0] = q0; out[1] = q1; out[2] = q2;
}
// The scatter, after the build: slot k of the new tree takes previous = flat[its record's flat index] and saved = `epoch` if the nine words
// differ from its current record (motion_differs, as the refit counts them), else 0 -- which is what the settle pass of the next refit call and
// the invariant at vhr_context::d_prev_saved expect of refit number `epoch`.  Every word of both arrays is written.
__global__ __launch_bounds__(256) void k0_rebuild_scatter_kernel(const BvhTri *__restrict__ tris, uint32_t n, const BvhTri *__restrict__ flat, uint32_t flat_count,
                                                                 const RefitMotion motion, unsigned long long *__restrict__ differing) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t differs = 0;
    if (k < n) {
        const float4 *slot = reinterpret_cast<const float4 *>(tris + k);
        const float4 now[3] = { slot[0], slot[1], slot[2] };
        const uint32_t f = __float_as_uint(now[2].w);
        float4 was[3] = { now[0], now[1], now[2] };
        if (f < flat_count) {
            const float4 *src = reinterpret_cast<const float4 *>(flat + f);
            was[0] = src[0]; was[1] = src[1]; was[2] = src[2];
        }
        float4 *pslot = reinterpret_cast<float4 *>(motion.prev + k);
        pslot[0] = was[0]; pslot[1] = was[1]; pslot[2] = was[2];
        differs = motion_differs(was, now);
        motion.saved[k] = differs ? motion.epoch : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) differs += uint32_t(__shfl_xor(int(differs), off));
    if ((threadIdx.x & 63u) == 0u && differs) atomicAdd(differing, (unsigned long long)differs);
}
// one node (bvh_math::refit_slots): its two slots from its children's unpadded boxes, its own unpadded box for its parent
__device__ __forceinline__ void refit_node(uint32_t k, BvhNode *nodes, const BvhTri *tris, Box6 *self_box, const RefitFrame &f, bool single) {
    BvhNode nd = nodes[k];
    Box6 mine;
    bvh_math::refit_slots(nd, single, tris, reinterpret_cast<const float *>(self_box), f.r, f.on != 0u, bvh_math::frame_pad_of(f.magnitude), mine.lo, mine.hi);
    nodes[k] = nd;
    self_box[k] = mine;
}
// the upward pass, design (a): one launch per level, deepest first; nodes [begin, end) are one level (the plan checks that the tree is
// numbered level by level, as both builders number it)
__global__ __launch_bounds__(256) void k0_refit_level_kernel(BvhNode *__restrict__ nodes, const BvhTri *__restrict__ tris, Box6 *__restrict__ self_box,
                                                             uint32_t begin, uint32_t end, RefitFrame f, uint32_t single, const uint32_t *__restrict__ dirty) {
    const uint32_t i = begin + blockIdx.x * 256u + threadIdx.x;
    if (i >= end || !node_selected(dirty, i)) return;
    refit_node(i, nodes, tris, self_box, f, single != 0u);
}
// ... and the levels at the top, which have fewer nodes than a launch is worth: one workgroup, a barrier between levels
constexpr int kRefitTopLevels = 16;
constexpr uint32_t kRefitTopNodes = 1024;          // a level of at most this many nodes belongs to the top
struct RefitTop { uint32_t begin[kRefitTopLevels + 1]; int levels; };
__global__ __launch_bounds__(256) void k0_refit_top_kernel(BvhNode *__restrict__ nodes, const BvhTri *__restrict__ tris, Box6 *__restrict__ self_box,
                                                           RefitTop top, RefitFrame f, uint32_t single, const uint32_t *__restrict__ dirty) {
    for (int level = top.levels - 1; level >= 0; --level) {
        for (uint32_t i = top.begin[level] + threadIdx.x; i < top.begin[level + 1]; i += 256u)
            if (node_selected(dirty, i)) refit_node(i, nodes, tris, self_box, f, single != 0u);
        __threadfence_block();
        __syncthreads();
    }
}
// the check pass: what the walkers will meet, in exact comparisons -- every record's corners inside its leaf's slot, every inner child's two
// slots inside the slot its parent holds for it
__global__ __launch_bounds__(256) void k0_refit_check_kernel(const BvhNode *__restrict__ nodes, const BvhTri *__restrict__ tris, uint32_t count, RefitFrame f,
                                                             RefitCounters *__restrict__ counters, const uint32_t *__restrict__ dirty, uint8_t *__restrict__ status) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    int bad_records = 0, bad_children = 0;
    if (k < count && node_selected(dirty, k)) {
        const BvhNode nd = nodes[k];
        bvh_math::refit_check(nd, count == 1u, nodes, tris, f.r, f.on != 0u, bad_records, bad_children);
        // what this node added to the two counters at its last check (records: at most 8, four bits; children: at most 4): a dirty pass
        // counts new - old, like k0_check_forms_kernel
        const uint32_t old = dirty ? status[k] : 0u;
        status[k] = uint8_t(uint32_t(bad_records) | (uint32_t(bad_children) << 4));
        bad_records -= int(old & 15u);
        bad_children -= int(old >> 4);
    }
    for (int off = 32; off > 0; off >>= 1) { bad_records += __shfl_xor(bad_records, off); bad_children += __shfl_xor(bad_children, off); }
    if ((threadIdx.x & 63u) == 0u) {
        if (bad_records) atomicAdd(&counters->records_outside, (unsigned long long)(long long)bad_records);
        if (bad_children) atomicAdd(&counters->children_outside, (unsigned long long)(long long)bad_children);
    }
}
// vhr_get_bvh_sah_cost: per workgroup the sum over its nodes of child half area x (1 | triangles of the leaf), reduced in a fixed order (the
// host adds the workgroups' sums in index order: the same tree gives the same bits)
__global__ __launch_bounds__(256) void k0_sah_cost_kernel(const BvhNode *__restrict__ nodes, uint32_t count, double *__restrict__ partial) {
    __shared__ double s_wave[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    double sum = 0.0;
    if (k < count) {
        const BvhNode nd = nodes[k];
        sum = bvh_math::sah_term(nd.box0, nd.child0);
        if (!bvh_math::absent_child1(nd, count == 1u)) sum += bvh_math::sah_term(nd.box1, nd.child1);
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) partial[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

}  // namespace

// ---- refit on the device ----
// What a refit needs beyond what a build leaves behind, made at the first refit from the nodes' links (fetched once) and kept until the next
// build: the level ranges (checked, not assumed: the refit relies on parents-before-children only), the per-node unpadded boxes, counters;
// for the partial refit every node's parent, every record's leaf node, one dirty bit per node and what each node last added to the checks.
struct RefitPlan {
    std::vector<uint32_t> level_begin;        // nodes [level_begin[l], level_begin[l + 1]) are level l
    Box6 *d_self_box = nullptr;
    RefitCounters *d_counters = nullptr;      // + the 5 words of k0_check_forms_kernel + 12 of the scene bounds + PartialCounters behind it
    double *d_partial = nullptr;              // k0_sah_cost_kernel's sums, one per workgroup
    uint32_t *d_parent = nullptr;             // per node; kNoParent for the root
    uint32_t *d_owner = nullptr;              // per record: the node whose leaf holds it
    uint32_t *d_dirty = nullptr;              // one bit per node, all clear between refits
    uint16_t *d_form_status = nullptr;        // per node: its part of k0_check_forms_kernel's out[1..4] at its last check
    uint8_t *d_check_status = nullptr;        // per node: its part of k0_refit_check_kernel's two counters
    bool boxes_valid = false;                 // a whole-tree refit has filled d_self_box and the two status arrays
    bool dirty_stale = false;                 // a dirty pass ended early (an error after its mark kernel): d_dirty may hold bits
    unsigned long long totals[6] = { 0, 0, 0, 0, 0, 0 };      // form checks out[1..4], records outside, children outside: over all nodes
    hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    uint32_t launches = 0;                    // of the upward pass (reporting)
};
void free_refit_plan(vhr_context *ctx) {
    RefitPlan *p = ctx->refit_plan;
    if (!p) return;
    hipFree(p->d_self_box); hipFree(p->d_counters); hipFree(p->d_partial);
    hipFree(p->d_parent); hipFree(p->d_owner); hipFree(p->d_dirty); hipFree(p->d_form_status); hipFree(p->d_check_status);
    for (hipEvent_t e : p->ev) if (e) hipEventDestroy(e);
    delete p;
    ctx->refit_plan = nullptr;
}

// the counters of one refit as they lie in device memory
struct RefitReadback { RefitCounters c; unsigned long long checks[5]; uint32_t bounds[12]; PartialCounters partial; };

static int make_refit_plan(vhr_context *ctx) {
    if (ctx->refit_plan) return VHR_OK;
    const uint32_t n = ctx->node_count;
    std::vector<BvhNode> nodes(n);
    BVH_TRY("refit", hipMemcpy(nodes.data(), ctx->d_nodes, sizeof(BvhNode) * n, hipMemcpyDeviceToHost));
    std::vector<uint32_t> depth(n, 0u), parent(n, kNoParent), owner(ctx->tri_count, 0u);
    uint32_t levels = 1;
    for (uint32_t k = 0; k < n; ++k) {
        const int32_t links[2] = { nodes[k].child0, nodes[k].child1 };
        for (int32_t link : links) {
            if (link >= 0) {
                if (uint32_t(link) <= k || uint32_t(link) >= n) return ctx->fail(VHR_ERROR_GRAPH, "vhr_refit_geometry: the tree's nodes are not numbered parents before children");
                depth[uint32_t(link)] = depth[k] + 1u;
                parent[uint32_t(link)] = k;
                levels = std::max(levels, depth[k] + 2u);
            } else {
                const uint32_t first = bvh_math::leaf_first(link), count = bvh_math::leaf_count(link);
                if (uint64_t(first) + count > ctx->tri_count) return ctx->fail(VHR_ERROR_GRAPH, "vhr_refit_geometry: a leaf lies outside the triangle records");
                for (uint32_t i = 0; i < count; ++i) owner[first + i] = k;
            }
        }
        // one launch per level needs every level to be a contiguous range of nodes: both builders number breadth first, anything else is refused
        if (k && depth[k] < depth[k - 1]) return ctx->fail(VHR_ERROR_GRAPH, "vhr_refit_geometry: the tree's nodes are not numbered level by level");
    }
    // (the context gets the plan only when it is complete: a failed allocation leaves nothing half-made behind)
    RefitPlan *p = new RefitPlan();
    p->level_begin.assign(levels + 1u, 0u);
    for (uint32_t k = 0; k < n; ++k) ++p->level_begin[depth[k] + 1u];
    for (uint32_t l = 0; l < levels; ++l) p->level_begin[l + 1u] += p->level_begin[l];
    const size_t dirty_bytes = sizeof(uint32_t) * ((size_t(n) + 31u) / 32u);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->d_self_box), sizeof(Box6) * n);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_counters), sizeof(RefitReadback));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_partial), sizeof(double) * ((n + 255u) / 256u));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_parent), sizeof(uint32_t) * n);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_owner), sizeof(uint32_t) * std::max(ctx->tri_count, 1u));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_dirty), dirty_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_form_status), sizeof(uint16_t) * n);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->d_check_status), sizeof(uint8_t) * n);
    if (e == hipSuccess) e = hipMemcpy(p->d_parent, parent.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && ctx->tri_count) e = hipMemcpy(p->d_owner, owner.data(), sizeof(uint32_t) * ctx->tri_count, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(p->d_dirty, 0, dirty_bytes);
    if (e != hipSuccess) {
        ctx->refit_plan = p;
        free_refit_plan(ctx);
        return ctx->fail(VHR_ERROR_DEVICE, std::string("refit: allocating the plan: ") + hipGetErrorString(e));
    }
    ctx->refit_plan = p;
    return VHR_OK;
}

int device_bvh_sah_cost(vhr_context *ctx, double *cost) {
    *cost = 0.0;
    const uint32_t n = ctx->node_count, blocks = (n + 255u) / 256u;
    if (!n || !ctx->d_nodes) return VHR_OK;
    double *d_partial = ctx->refit_plan ? ctx->refit_plan->d_partial : nullptr;
    Scratch tmp;
    if (!d_partial) BVH_TRY("refit", tmp.alloc(&d_partial, blocks));
    hipLaunchKernelGGL(k0_sah_cost_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->d_nodes, n, d_partial);
    std::vector<double> partial(blocks);
    BvhNode root;
    BVH_TRY("refit", hipMemcpyAsync(partial.data(), d_partial, sizeof(double) * blocks, hipMemcpyDeviceToHost, ctx->stream));
    BVH_TRY("refit", hipMemcpyAsync(&root, ctx->d_nodes, sizeof(root), hipMemcpyDeviceToHost, ctx->stream));
    BVH_TRY("refit", hipStreamSynchronize(ctx->stream));
    BVH_TRY("refit", hipGetLastError());
    double sum = 0.0;
    for (double v : partial) sum += v;
    *cost = bvh_math::sah_cost(sum, root, n == 1u);
    return VHR_OK;
}

static dim3 refit_grid(uint32_t count) { return dim3((count + 255u) / 256u); }
static RefitFrame refit_frame(const vhr_context *ctx) {
    RefitFrame f;
    for (int i = 0; i < 9; ++i) f.r[i] = ctx->bvh_frame[i];
    f.on = ctx->bvh_frame_on ? 1u : 0u;
    f.magnitude = ctx->bvh_frame_magnitude;
    return f;
}
// the upward pass: the boxes, level by level from the deepest; the levels at the top in one launch.  `dirty`: nullptr = every node
static void refit_upward(vhr_context *ctx, RefitPlan *p, const RefitFrame &f, const uint32_t *dirty) {
    const uint32_t single = ctx->node_count == 1u ? 1u : 0u;
    const uint32_t levels = uint32_t(p->level_begin.size()) - 1u;
    uint32_t top_levels = 0;
    while (top_levels < levels && top_levels < uint32_t(kRefitTopLevels) && p->level_begin[top_levels + 1u] - p->level_begin[top_levels] <= kRefitTopNodes) ++top_levels;
    p->launches = 0;
    for (uint32_t l = levels; l-- > top_levels;) {
        const uint32_t begin = p->level_begin[l], end = p->level_begin[l + 1u];
        hipLaunchKernelGGL(k0_refit_level_kernel, refit_grid(end - begin), dim3(256), 0, ctx->stream, ctx->d_nodes, ctx->d_tris, p->d_self_box, begin, end, f, single, dirty);
        ++p->launches;
    }
    if (top_levels) {
        RefitTop top{};
        top.levels = int(top_levels);
        for (uint32_t l = 0; l <= top_levels; ++l) top.begin[l] = p->level_begin[l];
        hipLaunchKernelGGL(k0_refit_top_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->d_nodes, ctx->d_tris, p->d_self_box, top, f, single, dirty);
        ++p->launches;
    }
}
// the derived forms and their containment check for the nodes of `forms_dirty`, the refit's own check for those of `dirty` (nullptr = every
// node), with ctx->bvh_centre
static void refit_forms_and_checks(vhr_context *ctx, RefitPlan *p, const RefitFrame &f, const uint32_t *forms_dirty, const uint32_t *dirty) {
    const uint32_t n_nodes = ctx->node_count;
    RefitReadback *d = reinterpret_cast<RefitReadback *>(p->d_counters);
    hipStream_t s = ctx->stream;
    launch_forms(ctx, n_nodes, forms_dirty);
    launch_check_forms(ctx, n_nodes, d->checks, forms_dirty, p->d_form_status);
    hipLaunchKernelGGL(k0_refit_check_kernel, refit_grid(n_nodes), dim3(256), 0, s, ctx->d_nodes, ctx->d_tris, n_nodes, f, &d->c, dirty, p->d_check_status);
}
// the counters of a finished refit into the context: `forms_whole` / `checks_whole` say whether the form checks / the refit's own check ran over
// every node (their counters are then the totals) or over the dirty nodes (new - old, added to the totals)
static void refit_publish(vhr_context *ctx, RefitPlan *p, const RefitReadback &got, bool forms_whole, bool checks_whole, uint64_t records, uint64_t nodes, bool timed) {
    const uint32_t n_nodes = ctx->node_count;
    for (int i = 0; i < 4; ++i) p->totals[i] = (forms_whole ? 0ull : p->totals[i]) + got.checks[i + 1];      // (two's complement: a negative difference wraps back)
    p->totals[4] = (checks_whole ? 0ull : p->totals[4]) + got.c.records_outside;
    p->totals[5] = (checks_whole ? 0ull : p->totals[5]) + got.c.children_outside;
    ctx->bvh_form_checks[0] = 2ull * n_nodes;                    // boxes checked: two per node
    ctx->bvh_form_checks[1] = p->totals[0];
    ctx->bvh_form_checks[2] = p->totals[1];
    publish_half_nodes(ctx, n_nodes, p->totals[2], p->totals[3]);      // the rule of a build
    ctx->refit_stats[kRefitRecords] = records;
    ctx->refit_stats[kRefitNodes] = nodes;
    ctx->refit_stats[kRefitRecordsOutside] = p->totals[4];
    ctx->refit_stats[kRefitChildrenOutside] = p->totals[5];
    ctx->refit_stats[kRefitNonFinite] = got.c.non_finite;
    ctx->refit_beyond = got.c.beyond;
    ctx->motion_refit_differing = got.c.differing;
    ctx->refit_stats[kRefitHalfNodes] = ctx->nodes16_valid ? 1u : 0u;
    ctx->refit_stats[7] = p->launches;
    for (int i = 1; i < 4; ++i) ctx->refit_times_ms[i] = 0.0;
    if (timed) {                               // kernels only: the scene centre's read-back lies between ev[2] and ev[3]
        const int pairs[3][2] = { { 0, 1 }, { 1, 2 }, { 3, 4 } };
        for (int i = 0; i < 3; ++i) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, p->ev[pairs[i][0]], p->ev[pairs[i][1]]) == hipSuccess) ctx->refit_times_ms[i + 1] = ms;
        }
    }
}
// "object_motion_vectors": what the leaf pass of the refit that is about to run needs (prev == nullptr: the option is off, the plain kernels run)
static RefitMotion refit_motion(const vhr_context *ctx) {
    const bool on = ctx->object_motion_vectors && ctx->d_prev_tris && ctx->d_prev_saved;
    return RefitMotion{ on ? ctx->d_prev_tris : nullptr, on ? ctx->d_prev_saved : nullptr, ctx->motion_epoch + 1u };
}
static RefitReadback refit_counters_init() {
    RefitReadback init{};
    for (int a = 0; a < 3; ++a) { init.bounds[a] = init.bounds[6 + a] = 0xffffffffu; }
    return init;
}

// The refit proper; the caller (vhr_refit_geometry) has checked that there is a tree, that it is not a presplit one, and has waited for the
// context's streams.  Fills ctx->refit_stats / refit_times_ms[1..3] and the context's tree state (centre, form checks, nodes16_valid).
int device_refit_bvh(vhr_context *ctx) {
    hipStream_t s = ctx->stream;
    if (!ctx->sah_cost_built_valid) {           // the cost of the tree as built, before its boxes move
        VHR_TRY(device_bvh_sah_cost(ctx, &ctx->sah_cost_built));
        ctx->sah_cost_built_valid = true;
    }
    VHR_TRY(make_refit_plan(ctx));
    RefitPlan *p = ctx->refit_plan;
    const uint32_t n_nodes = ctx->node_count, n_tris = ctx->tri_count;
    const dim3 block(256);
    const bool timed = (ctx->kernel_timing_mask & (1u << kKernelRefit)) != 0;
    if (timed)
        for (hipEvent_t &e : p->ev) if (!e) BVH_TRY("refit", hipEventCreate(&e));
    const RefitFrame f = refit_frame(ctx);
    RefitReadback *d = reinterpret_cast<RefitReadback *>(p->d_counters);
    const RefitReadback init = refit_counters_init();
    RefitReadback got{};
    BVH_TRY("refit", hipMemcpyAsync(p->d_counters, &init, sizeof(init), hipMemcpyHostToDevice, s));
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[0], s));
    // 1. the records
    const RefitMotion motion = refit_motion(ctx);
    hipLaunchKernelGGL(motion.prev ? k0_refit_records_kernel<true> : k0_refit_records_kernel<false>, refit_grid(n_tris), block, 0, s, ctx->d_vertices, ctx->d_indices,
                       ctx->d_primitives, ctx->primitive_count, n_tris, ctx->d_tris, p->d_counters, motion, f);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[1], s));
    // 2. + 3. the boxes
    refit_upward(ctx, p, f, nullptr);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[2], s));
    // 4. the scene centre (one reduction and a read-back of 12 words: k0_forms_kernel takes the centre by value, like the build), the derived
    // forms, their containment check and the refit's own
    launch_node_bounds(ctx, n_nodes, d->bounds + 6);
    uint32_t h_bounds[12];
    BVH_TRY("refit", hipMemcpyAsync(h_bounds, d->bounds, sizeof(h_bounds), hipMemcpyDeviceToHost, s));
    BVH_TRY("refit", hipStreamSynchronize(s));
    BVH_TRY("refit", hipGetLastError());
    centre_from_bounds(h_bounds + 6, ctx->bvh_centre);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[3], s));
    refit_forms_and_checks(ctx, p, f, nullptr, nullptr);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[4], s));
    BVH_TRY("refit", hipMemcpyAsync(&got, p->d_counters, sizeof(got), hipMemcpyDeviceToHost, s));
    BVH_TRY("refit", hipStreamSynchronize(s));
    BVH_TRY("refit", hipGetLastError());
    p->boxes_valid = true;
    refit_publish(ctx, p, got, true, true, n_tris, n_nodes, timed);
    return VHR_OK;
}

bool device_refit_boxes_valid(const vhr_context *ctx) { return ctx->refit_plan && ctx->refit_plan->boxes_valid; }

// vhr_refit_geometry_partial's dirty path; same contract as device_refit_bvh.  The scene centre comes from the root's two slots: every other
// slot lies inside them (the containment the check pass counts violations of, which the padding guarantees for finite coordinates), so the
// whole-tree reduction gives the same bits.
int device_refit_bvh_partial(vhr_context *ctx, bool *ran_whole) {
    *ran_whole = false;
    VHR_TRY(make_refit_plan(ctx));
    RefitPlan *p = ctx->refit_plan;
    if (!p->boxes_valid) { *ran_whole = true; return device_refit_bvh(ctx); }
    hipStream_t s = ctx->stream;
    const uint32_t n_nodes = ctx->node_count, n_tris = ctx->tri_count;
    const dim3 block(256);
    const bool timed = (ctx->kernel_timing_mask & (1u << kKernelRefit)) != 0;
    if (timed)
        for (hipEvent_t &e : p->ev) if (!e) BVH_TRY("refit", hipEventCreate(&e));
    const RefitFrame f = refit_frame(ctx);
    RefitReadback *d = reinterpret_cast<RefitReadback *>(p->d_counters);
    const RefitReadback init = refit_counters_init();
    RefitReadback got{};
    BVH_TRY("refit", hipMemcpyAsync(p->d_counters, &init, sizeof(init), hipMemcpyHostToDevice, s));
    const size_t dirty_bytes = sizeof(uint32_t) * ((size_t(n_nodes) + 31u) / 32u);
    if (p->dirty_stale) BVH_TRY("refit", hipMemsetAsync(p->d_dirty, 0, dirty_bytes, s));      // (the last dirty pass did not reach its own clearing)
    p->dirty_stale = true;
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[0], s));
    // 1. mark, and the dirty records
    const RefitMotion motion = refit_motion(ctx);
    hipLaunchKernelGGL(motion.prev ? k0_refit_mark_kernel<true> : k0_refit_mark_kernel<false>, refit_grid(n_tris), block, 0, s, ctx->d_vertices, ctx->d_indices, ctx->d_primitives,
                       ctx->primitive_count, n_tris, ctx->d_tris, p->d_owner, p->d_parent, p->d_dirty, ctx->refit_dirty, &d->c, &d->partial, motion, f);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[1], s));
    // 2. + 3. the dirty nodes' boxes: the same launches, a one-bit test per node
    refit_upward(ctx, p, f, p->d_dirty);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[2], s));
    // 4. the scene centre from the root (the first of the two read-backs)
    BvhNode root;
    BVH_TRY("refit", hipMemcpyAsync(&root, ctx->d_nodes, sizeof(root), hipMemcpyDeviceToHost, s));
    BVH_TRY("refit", hipStreamSynchronize(s));
    BVH_TRY("refit", hipGetLastError());
    float centre[3];
    bvh_math::centre_of_root(root, centre);
    const bool centre_moved = std::memcmp(centre, ctx->bvh_centre, sizeof(centre)) != 0;
    for (int a = 0; a < 3; ++a) ctx->bvh_centre[a] = centre[a];
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[3], s));
    // (a centre that moved: every node's half-precision form hangs on it, so all forms and their checks again)
    refit_forms_and_checks(ctx, p, f, centre_moved ? nullptr : p->d_dirty, p->d_dirty);
    if (timed) BVH_TRY("refit", hipEventRecord(p->ev[4], s));
    BVH_TRY("refit", hipMemsetAsync(p->d_dirty, 0, dirty_bytes, s));
    BVH_TRY("refit", hipMemcpyAsync(&got, p->d_counters, sizeof(got), hipMemcpyDeviceToHost, s));
    BVH_TRY("refit", hipStreamSynchronize(s));
    BVH_TRY("refit", hipGetLastError());
    p->dirty_stale = false;
    refit_publish(ctx, p, got, centre_moved, false, got.partial.dirty_records, got.partial.dirty_nodes, timed);
    ctx->partial_stats[kPartialForms] = centre_moved ? n_nodes : got.partial.dirty_nodes;
    ctx->partial_stats[kPartialCentreMoved] = centre_moved ? 1u : 0u;
    return VHR_OK;
}

// A refit call with nothing pending while the last refit left records that differ from their previous ones: those objects have stopped.  The
// caller has waited for the context's streams (frames in flight read the previous array) and counts the call as a refit.
int device_motion_settle(vhr_context *ctx) {
    const RefitMotion motion = refit_motion(ctx);
    if (!motion.prev || !ctx->tri_count) return VHR_OK;
    hipLaunchKernelGGL(k0_motion_settle_kernel, refit_grid(ctx->tri_count), dim3(256), 0, ctx->stream, ctx->d_tris, ctx->tri_count, motion);
    BVH_TRY("refit", hipStreamSynchronize(ctx->stream));
    BVH_TRY("refit", hipGetLastError());
    return VHR_OK;
}

// ---- rebuild in place (vhr_rebuild_geometry): the three passes around device_build_bvh; the caller has waited for the context's streams ----
int device_count_non_finite_positions(vhr_context *ctx, uint64_t *count) {
    *count = 0;
    if (!ctx->vertex_count) return VHR_OK;
    Scratch tmp;
    unsigned long long *d_count, h_count = 0;
    BVH_TRY("rebuild", tmp.alloc(&d_count, size_t(1)));
    BVH_TRY("rebuild", hipMemsetAsync(d_count, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k0_rebuild_finite_kernel, refit_grid(ctx->vertex_count), dim3(256), 0, ctx->stream, ctx->d_vertices, ctx->vertex_count, d_count);
    BVH_TRY("rebuild", hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream));
    BVH_TRY("rebuild", hipStreamSynchronize(ctx->stream));
    BVH_TRY("rebuild", hipGetLastError());
    *count = h_count;
    return VHR_OK;
}

int device_rebuild_gather(vhr_context *ctx, uint32_t flat_count, BvhTri **d_flat) {
    *d_flat = nullptr;
    const RefitMotion motion = refit_motion(ctx);
    if (!motion.prev || !ctx->tri_count || !flat_count) return VHR_OK;
    BvhTri *flat = nullptr;
    BVH_TRY("rebuild", hipMalloc(reinterpret_cast<void **>(&flat), sizeof(BvhTri) * size_t(flat_count)));
    hipError_t e = hipMemsetAsync(flat, 0, sizeof(BvhTri) * size_t(flat_count), ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k0_rebuild_gather_kernel, refit_grid(ctx->tri_count), dim3(256), 0, ctx->stream, ctx->d_tris, ctx->tri_count, motion, flat_count, flat);
        e = hipStreamSynchronize(ctx->stream);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { hipFree(flat); BVH_TRY("rebuild", e); }
    *d_flat = flat;
    return VHR_OK;
}

int device_rebuild_scatter(vhr_context *ctx, const BvhTri *d_flat, uint32_t flat_count, uint64_t *differing) {
    *differing = 0;
    hipFree(ctx->d_prev_tris); hipFree(ctx->d_prev_saved);
    ctx->d_prev_tris = nullptr; ctx->d_prev_saved = nullptr;
    if (!ctx->tri_count) return VHR_OK;
    hipStream_t s = ctx->stream;
    Scratch tmp;
    unsigned long long *d_count, h_count = 0;
    BVH_TRY("rebuild", tmp.alloc(&d_count, size_t(1)));
    BVH_TRY("rebuild", hipMalloc(reinterpret_cast<void **>(&ctx->d_prev_tris), sizeof(BvhTri) * size_t(ctx->tri_count)));
    BVH_TRY("rebuild", hipMalloc(reinterpret_cast<void **>(&ctx->d_prev_saved), sizeof(uint32_t) * size_t(ctx->tri_count)));
    BVH_TRY("rebuild", hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
    const RefitMotion motion{ ctx->d_prev_tris, ctx->d_prev_saved, ctx->motion_epoch + 1u };
    hipLaunchKernelGGL(k0_rebuild_scatter_kernel, refit_grid(ctx->tri_count), dim3(256), 0, s, ctx->d_tris, ctx->tri_count, d_flat, flat_count, motion, d_count);
    BVH_TRY("rebuild", hipMemcpyAsync(&h_count, d_count, sizeof(h_count), hipMemcpyDeviceToHost, s));
    BVH_TRY("rebuild", hipStreamSynchronize(s));
    BVH_TRY("rebuild", hipGetLastError());
    *differing = h_count;
    return VHR_OK;
}

}  // namespace vhr
