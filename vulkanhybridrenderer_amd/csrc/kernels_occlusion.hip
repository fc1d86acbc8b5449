// vhr_occlusion_query: hemisphere occlusion masks at surface points, and the kernel of vhr_debug_occlusion_rays.  Built with the ray-tracing
// units' flags (the rays owe the host's copy in queries.cpp their bits: occlusion_rays.hpp).
#define VHR_TRACE_UNIT unit_occlusion      // names this unit's copy of the sRGB decode table (trace_device.hpp), which comes with the header;
                                           // no kernel here samples a texture (the alpha rule is out of this entry point's scope)
#include "trace_queue.hpp"
#include "occlusion_rays.hpp"

namespace vhr {

// ---------------------------------------------------------------------------------------------
// vhr_occlusion_query: `samples` cosine-distributed any-hit rays around the axis of each query point, one bit per ray.  No ray array exists:
// ray (i, j) is made from point i where the walk fetches it (occlusion_ray, occlusion_rays.hpp).  Launch 1 (occlusion_query_kernel) has
// ray_query_kernel's shape: every wave owns `wave_points` = max(1, 256 / samples) whole consecutive points, i.e. at most kOcclusionWaveRays
// rays, and runs wave_queue_walk over them (PER_RAY, any hit, no tile and no cut: a shared descent around the wave's origins was measured and
// not kept).  A ray's commit ORs its bit into its point's mask in wave-private LDS -- two words per point -- and the wave
// stores its masks once, as 8-byte words, when the walk is done.  Decision (vi) stays out
// of the loop (DEFER): a ray with a self-contradicting candidate is walked on as if it had missed and marks its POINT, and the wave appends
// each marked point once to the stream's list, whose capacity is therefore `count`.  Launch 2 (occlusion_redo_kernel) strides over the list,
// whose length only the device knows, computes all rays of a listed point again with traverse<true>, which decides in binary64 in place, and
// overwrites the point's mask.  Neither launch reads or writes anything of a frame.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kOcclusionWaveRays = 256;                               // rays per wave at most (kQueryWaveRays' figure)
constexpr uint32_t kOcclusionWavePoints = kOcclusionWaveRays;              // ... and points (samples == 1)
constexpr uint32_t kOcclusionMaskWords = kOcclusionWavePoints * 2u;        // a wave's masks in LDS, and behind them one mark bit per point
constexpr uint32_t kOcclusionLdsWords = kOcclusionMaskWords + kOcclusionWavePoints / 32u;
static_assert(VHR_OCCLUSION_MAX_SAMPLES == 64u, "a point's mask is one 64-bit word, and a ray's id keeps its sample in six bits");

struct OcclusionArgs {
    DeviceScene scene;
    const float4 *points;                 // 2 x float4 per point: (origin, tmin), (axis, tmax)
    unsigned long long *occluded;         // one mask per point
    uint32_t *redo_list;                  // capacity count
    OcclusionCounters *counters;
    uint32_t count, samples, seed;
    uint32_t wave_points;                 // max(1, kOcclusionWaveRays / samples)
    uint32_t samples_magic;               // 65536 / samples + 1: (r * magic) >> 16 == r / samples for r < 256 (the error r / 65536 stays below 1 / samples)
    RayMaskArgs masks;                    // the kFilterMask instantiations: masks.shadow = the cull_mask
};

__device__ __forceinline__ OcclusionRay occlusion_point(const OcclusionArgs &a, const uint32_t point) {
    const float4 p = a.points[size_t(point) * 2u], q = a.points[size_t(point) * 2u + 1u];
    return OcclusionRay{ f3{ p.x, p.y, p.z }, p.w, f3{ q.x, q.y, q.z }, q.w };
}

// FILTER: kFilterNone, or kFilterMask where the cull mask acts on the masks the primitives carry (no per-ray masks: the filter never asks for the ray's id)
template <bool SPILL, int FILTER = kFilterNone>
__global__ __launch_bounds__(kQueueBlock * 2) void occlusion_query_kernel(const OcclusionArgs a, const uint32_t stack_levels, const uint32_t refill_threshold,
                                                                          const uint32_t early_exit, const Stamps st) {
    vhr_stamp(st);
    extern __shared__ int s_dyn[];                        // per wave: (stack_levels + 3) x 64 ints, see raygen_queue_kernel
    __shared__ uint32_t s_masks[2][kOcclusionLdsWords];
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const uint64_t first = (uint64_t(blockIdx.x) * 2u + wave) * a.wave_points;
    if (first >= a.count) return;
    const uint32_t base = uint32_t(first), points = uint32_t(min(uint64_t(a.wave_points), uint64_t(a.count) - first));
    if (a.scene.node_count == 0) {                        // no geometry: nothing occludes
        for (uint32_t p = lane; p < points; p += 64u) a.occluded[base + p] = 0ull;
        return;
    }
    uint32_t *const mask = s_masks[wave], *const marks = mask + kOcclusionMaskWords;
    for (uint32_t w = lane; w < kOcclusionLdsWords; w += 64u) mask[w] = 0u;
    wave_lds_sync();
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    uint32_t overflow = 0;
    bool flagged = false;                                 // decision (vi) asked for binary64 on the lane's current ray
    wave_queue_walk<SPILL, true, false, true>(
        a.scene, stack, stack_levels, lane, points * a.samples, refill_threshold, early_exit, 0.0f, 0.0f, true, overflow, nullptr, 0u,
        [&](uint32_t r, uint32_t &ray, f3 &ro, f3 &rd, float &tmin, float &tmax) {
            const uint32_t p = (r * a.samples_magic) >> 16, j = r - p * a.samples;
            ray = (p << 6) | j;                           // what the commit is told: the point within the wave and the sample
            const OcclusionRay q = occlusion_ray(occlusion_point(a, base + p), base + p, j, a.samples, a.seed);
            ro = q.o; tmin = q.tmin;
            rd = q.d; tmax = q.tmax;
        },
        [&](uint32_t ray, uint32_t tri, float, float, float) {
            const uint32_t p = ray >> 6, j = ray & 63u;
            if (tri != kNoHit) atomicOr(&mask[p * 2u + (j >> 5)], 1u << (j & 31u));
            if (flagged) {
                atomicOr(&marks[p >> 5], 1u << (p & 31u));
                flagged = false;
            }
        }, nullptr,
        [&](uint32_t) { flagged = true; }, ray_filter<FILTER>(a.scene, a.masks, a.masks.shadow, nullptr));
    wave_lds_sync();
    uint32_t hits = 0;
    for (uint32_t p = lane; p < points; p += 64u) {
        const uint32_t lo = mask[p * 2u], hi = mask[p * 2u + 1u];
        a.occluded[base + p] = (unsigned long long)lo | ((unsigned long long)hi << 32);
        hits += uint32_t(__popc(lo) + __popc(hi));
        if ((marks[p >> 5] >> (p & 31u)) & 1u) a.redo_list[atomicAdd(&a.counters->redo_count, 1u)] = base + p;      // (rare: a plain vector atomic per listed point)
    }
    for (int off = 32; off > 0; off >>= 1) hits += uint32_t(__shfl_xor(int(hits), off));
    const bool wave_overflow = __any(overflow != 0u);
    if (lane == 0) {
        if (hits) atomicAdd(&a.counters->occluded, (unsigned long long)hits);
        if (wave_overflow) atomicAdd(&a.counters->overflows, 1u);
    }
}

// Decision (vi), second half, for the points launch 1 listed: every ray of the point through the per-pixel walker with the binary64 redo inside
// its leaf test.  The unit of the redo is the point -- its mask is one word, written whole -- so a point is listed once however many of its rays asked.
template <int FILTER = kFilterNone>
__global__ __launch_bounds__(kTraceBlock) void occlusion_redo_kernel(const OcclusionArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_stack[kTraceStack * kTraceBlock];
    const uint32_t n = a.counters->redo_count;            // written by launch 1
    uint32_t overflow = 0;
    int delta = 0;                                        // change of the occluded-ray count
    for (uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x; i < n; i += gridDim.x * kTraceBlock) {
        const uint32_t point = a.redo_list[i];
        const OcclusionRay pt = occlusion_point(a, point);
        const unsigned long long was = a.occluded[point];
        unsigned long long now = 0ull;
        for (uint32_t j = 0; j < a.samples; ++j) {
            const OcclusionRay q = occlusion_ray(pt, point, j, a.samples, a.seed);
            Hit best;
            best.t = best.u = best.v = 0.0f; best.tri_index = 0; best.flat = 0;
            if (traverse<true>(a.scene, q.o, q.d, q.tmin, q.tmax, s_stack + threadIdx.x, best, overflow, ray_filter<FILTER>(a.scene, a.masks, a.masks.shadow, nullptr)))
                now |= 1ull << j;
        }
        a.occluded[point] = now;
        delta += __popcll(now) - __popcll(was);
    }
    if (delta) atomicAdd(&a.counters->occluded, (unsigned long long)(long long)delta);
    if (overflow) atomicAdd(&a.counters->overflows, 1u);
}

int launch_occlusion_query(vhr_context *ctx, const vhr_ray *points, uint32_t count, uint32_t samples, uint32_t seed, uint32_t cull_mask, uint64_t *occluded) {
    if (count == 0) return VHR_OK;
    QueryScratch *const q = stream_scratch(ctx, ctx->oq_scratch, sizeof(OcclusionCounters), "vhr_occlusion_query");     // this stream's counters and list
    if (!q) return VHR_ERROR_DEVICE;
    if (q->capacity < count) {
        (void)hipFree(q->list);                     // (synchronises: a query still in flight is done with it)
        q->list = nullptr;
        q->capacity = 0;
        if (hipMalloc(reinterpret_cast<void **>(&q->list), size_t(count) * sizeof(uint32_t)) != hipSuccess)
            return ctx->fail(VHR_ERROR_DEVICE, "vhr_occlusion_query: device allocation failed");
        q->capacity = count;
    }
    OcclusionArgs a;
    a.scene = ctx->device_scene();
    a.points = reinterpret_cast<const float4 *>(points);
    a.occluded = reinterpret_cast<unsigned long long *>(occluded);
    a.redo_list = q->list;
    ctx->oq_last_counters = a.counters = static_cast<OcclusionCounters *>(q->counters);
    a.count = count;
    a.samples = samples;
    a.seed = seed;
    a.wave_points = std::max(1u, kOcclusionWaveRays / samples);
    a.samples_magic = 65536u / samples + 1u;
    const QueueLaunch ql = queue_launch(ctx, kOptLdsStackLevels, kOptEarlyExit, 2u);
    const uint64_t waves = (uint64_t(count) + a.wave_points - 1u) / a.wave_points;
    const dim3 grid(uint32_t((waves + 1u) / 2u));
    // the filtering kernels only where the cull mask acts on the masks the primitives carry
    const bool mask_acts = ctx->ray_mask_acts(cull_mask);
    a.masks = RayMaskArgs{ nullptr, cull_mask, cull_mask, cull_mask, 0u };
    if (mask_acts) {
        if (const int rc = ensure_device_prim_masks(ctx)) return rc;
        a.masks.prim_masks = ctx->d_prim_masks;
    }
    ctx->oq_mask_ran = mask_acts ? 1u : 0u;
    const uint32_t redo_blocks = std::min<uint32_t>((count + kTraceBlock - 1u) / kTraceBlock, uint32_t(ctx->cu_count) * 4u);
    with_bool(ql.spill, [&](auto sp) { with_bool(mask_acts, [&](auto mk) {
        constexpr int filter = decltype(mk)::value ? kFilterMask : kFilterNone;
        launch(ctx, occlusion_query_kernel<decltype(sp)::value, filter>, grid, dim3(kQueueBlock * 2), ql.lds_bytes, a, ql.levels, ql.threshold, ql.early_exit);
        if (a.scene.node_count != 0) launch(ctx, occlusion_redo_kernel<filter>, dim3(redo_blocks), dim3(kTraceBlock), 0, a);
    }); });
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "vhr_occlusion_query: kernel launch failed");
    return VHR_OK;
}

// ---------------------------------------------------------------------------------------------
// vhr_debug_occlusion_rays on a device context: the rays themselves, point-major, one per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void occlusion_rays_kernel(const float4 *points, const uint32_t count, const uint32_t samples, const uint32_t seed, float4 *out, const Stamps st) {
    vhr_stamp(st);
    const uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= uint64_t(count) * samples) return;
    const uint32_t i = uint32_t(k / samples), j = uint32_t(k - uint64_t(i) * samples);
    const float4 p = points[size_t(i) * 2u], q = points[size_t(i) * 2u + 1u];
    const OcclusionRay r = occlusion_ray(OcclusionRay{ f3{ p.x, p.y, p.z }, p.w, f3{ q.x, q.y, q.z }, q.w }, i, j, samples, seed);
    out[k * 2u] = make_float4(r.o.x, r.o.y, r.o.z, r.tmin);
    out[k * 2u + 1u] = make_float4(r.d.x, r.d.y, r.d.z, r.tmax);
}

int launch_occlusion_rays(vhr_context *ctx, const vhr_ray *points, uint32_t count, uint32_t samples, uint32_t seed, vhr_ray *out) {
    const uint64_t rays = uint64_t(count) * samples;
    PairArray a[2] = { { points, nullptr, size_t(count) * sizeof(vhr_ray) }, { nullptr, out, size_t(rays) * sizeof(vhr_ray) } };
    return run_pairs(ctx, "vhr_debug_occlusion_rays", a, [&] {
        launch(ctx, occlusion_rays_kernel, dim3(uint32_t((rays + 255u) / 256u)), dim3(256), 0, static_cast<const float4 *>(a[0].d), count, samples, seed, static_cast<float4 *>(a[1].d));
    });
}

}  // namespace vhr
