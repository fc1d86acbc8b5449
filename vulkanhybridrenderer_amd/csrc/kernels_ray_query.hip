// The batched ray query (vhr_ray_query) and the debug kernel that runs the walkers' triangle test on explicit pairs
// (vhr_debug_ray_triangle), with the face rule of vhr_ray_query_faces and its pairs kernel (vhr_debug_ray_facing).  (Split from the end of
// kernels_trace.hip; built with the same flags.)
#define VHR_TRACE_UNIT unit_ray_query      // names this unit's copy of the sRGB decode table (trace_device.hpp), which comes with the header:
                                           // gbuf_discarded (VHR_RAY_QUERY_ALPHA_TEST) samples base-colour textures here
#include "trace_queue.hpp"

namespace vhr {

// ---------------------------------------------------------------------------------------------
// vhr_debug_ray_triangle: decision (vi) as the walkers' triangle test computes it, on explicit (ray, triangle) pairs -- what tests/ hold against the oracle's
// orc_ray_triangle and against exact arithmetic (tests/golden/kat_decision_vi.json), without a scene or a tree in between.  17 floats per pair:
// o, d, v0, e1, e2, tmin, tmax; out: hit (0 / 1) and (t, u, v).  One pair per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ray_triangle_pairs_kernel(const float *pairs, const uint32_t n, uint32_t *hit, float *tuv, const Stamps st) {
    vhr_stamp(st);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *p = pairs + size_t(i) * 17u;
    float t = 0.0f, u = 0.0f, v = 0.0f;
    const bool h = ray_triangle(f3{ p[0], p[1], p[2] }, f3{ p[3], p[4], p[5] }, f3{ p[6], p[7], p[8] }, f3{ p[9], p[10], p[11] }, f3{ p[12], p[13], p[14] }, p[15], p[16], t, u, v);
    hit[i] = h ? 1u : 0u;
    tuv[size_t(i) * 3u] = h ? t : 0.0f; tuv[size_t(i) * 3u + 1u] = h ? u : 0.0f; tuv[size_t(i) * 3u + 2u] = h ? v : 0.0f;
}

int launch_ray_triangle_pairs(vhr_context *ctx, const float *pairs, uint32_t n, uint32_t *hit, float *tuv) {
    PairArray a[3] = { { pairs, nullptr, size_t(n) * 17u * sizeof(float) }, { nullptr, hit, size_t(n) * sizeof(uint32_t) }, { nullptr, tuv, size_t(n) * 3u * sizeof(float) } };
    return run_pairs(ctx, "vhr_debug_ray_triangle", a, [&] {
        launch(ctx, ray_triangle_pairs_kernel, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<const float *>(a[0].d), n, static_cast<uint32_t *>(a[1].d), static_cast<float *>(a[2].d));
    });
}

// ---------------------------------------------------------------------------------------------
// vhr_debug_ray_facing on a device context: ray_hit_kind (ray_facing.hpp) on explicit pairs, 9 floats each (d, e1, e2) and a flip byte (flips may
// be null: all 0) -> one byte, 0xFE front / 0xFF back.  One pair per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ray_facing_pairs_kernel(const float *pairs, const uint8_t *flips, const uint32_t n, uint8_t *out, const Stamps st) {
    vhr_stamp(st);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *p = pairs + size_t(i) * 9u;
    out[i] = uint8_t(ray_hit_kind(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], flips != nullptr && flips[i] != 0));
}

int launch_ray_facing_pairs(vhr_context *ctx, const float *pairs, const uint8_t *flips, uint32_t n, uint8_t *out) {
    PairArray a[3] = { { pairs, nullptr, size_t(n) * 9u * sizeof(float) }, { flips, nullptr, flips ? size_t(n) : 0u }, { nullptr, out, size_t(n) } };
    return run_pairs(ctx, "vhr_debug_ray_facing", a, [&] {
        launch(ctx, ray_facing_pairs_kernel, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<const float *>(a[0].d), static_cast<const uint8_t *>(a[1].d), n, static_cast<uint8_t *>(a[2].d));
    });
}

// ---------------------------------------------------------------------------------------------
// vhr_ray_query: batched rayQueryEXT on the scene's BVH (the reference's RayqueryRenderPath, rayquery_render_path/default.frag:36-45,
// asks the same of the TLAS from a fragment shader).  Launch 1 (ray_query_kernel): every wave owns kQueryWaveRays consecutive rays of
// the batch and runs wave_queue_walk over them (PER_RAY: each ray's own [tmin, tmax]; no tile, so no shared descent).  Decision (vi)
// stays out of the loop as in the mirror-ray kernel (DEFER): a ray with a self-contradicting candidate is walked on as if it had
// missed and its index is appended to a list at its commit.  Launch 2 (ray_query_redo_kernel) walks every listed ray again with
// traverse<>, which decides in binary64 in place, and overwrites its result; it strides over the list, whose length only the
// device knows.  Neither launch reads or writes anything of a frame.
// ---------------------------------------------------------------------------------------------
#ifndef VHR_QUERY_WAVE_RAYS
#define VHR_QUERY_WAVE_RAYS 256      // rays per wave of ray_query_kernel (a scratch build may change it)
#endif
constexpr uint32_t kQueryWaveRays = VHR_QUERY_WAVE_RAYS;

struct RayQueryArgs {
    DeviceScene scene;
    const float4 *rays;                   // 2 x float4 per ray: (origin, tmin), (direction, tmax)
    void *results;                        // vhr_ray_hit[count] or uint8_t[count] (any_hit)
    uint32_t *redo_list;                  // capacity count
    RayQueryCounters *counters;
    uint32_t count, any_hit;
    RayMaskArgs masks;                    // vhr_ray_query_masked (the kFilterMask instantiations): masks.shadow = its cull_mask
    const uint8_t *ray_masks;             // one byte per ray, ANDed with the cull mask, or null
    // vhr_ray_query_faces (the kFilterFace instantiations; the others never read these)
    const uint8_t *prim_flips;            // one byte per primitive (never null there)
    uint32_t face_cull;                   // VHR_FACE_CULL_*
};
static_assert(sizeof(vhr_ray) == 2 * sizeof(float4), "vhr_ray is two float4");

// `kind`: vhr_ray_hit::reserved -- 0 from every instantiation but kFilterFace, whose closest hits carry their hit kind there
__device__ __forceinline__ void ray_query_store(const RayQueryArgs &a, const uint32_t ray, const bool any_hit, const bool hit, const float t,
                                                const float u, const float v, const uint32_t prim, const uint32_t tri, const uint32_t kind = 0u) {
    if (any_hit) { static_cast<uint8_t *>(a.results)[ray] = hit ? 1u : 0u; return; }
    uint32_t *const r = static_cast<uint32_t *>(a.results) + size_t(ray) * 6u;      // vhr_ray_hit (results is 4-byte aligned)
    r[0] = hit ? __float_as_uint(t) : 0u; r[1] = hit ? __float_as_uint(u) : 0u; r[2] = hit ? __float_as_uint(v) : 0u;
    r[3] = hit ? prim : kNoHit; r[4] = hit ? tri : kNoHit; r[5] = hit ? kind : 0u;
}

// the hit kind of the committed triangle (kFilterFace, closest hit): the function the face filter culls by, on the record and the ray's direction
__device__ __forceinline__ uint32_t committed_hit_kind(const RayQueryArgs &a, const uint32_t ray, const uint32_t tri_index) {
    const BvhTri &bt = a.scene.tris[tri_index];
    const float4 q = a.rays[size_t(ray) * 2u + 1u];
    return ray_hit_kind(q.x, q.y, q.z, bt.e1[0], bt.e1[1], bt.e1[2], bt.e2[0], bt.e2[1], bt.e2[2], a.prim_flips[bt.prim] != 0);
}
// a launch's candidate filter: ray_filter<> (trace_device.hpp) for the three the hybrid path shares, the face rule built here.  `ray_masks`: null
// where `ray_mask` already holds the ray's own (the redo kernel)
template <int FILTER> __device__ __forceinline__ auto query_filter(const RayQueryArgs &a, const uint32_t ray_mask, const uint8_t *ray_masks) {
    if constexpr (FILTER == kFilterFace) return RayFaceReject{ &a.scene, a.masks.prim_masks, ray_masks, a.prim_flips, a.rays, ray_mask, a.masks.alpha, a.face_cull };
    else return ray_filter<FILTER>(a.scene, a.masks, ray_mask, ray_masks);
}

// FILTER: kFilterAlpha (VHR_RAY_QUERY_ALPHA_TEST) -- a candidate gbuf_discarded names does not exist; kFilterMask (vhr_ray_query_masked) -- nor does
// one whose primitive's mask shares no bit with the ray's mask, read at the candidate by ray id; kFilterFace (vhr_ray_query_faces) -- nor one on a
// triangle the ray's face cull mode removes, behind the mask test and before the alpha rule (both runtime there), and a closest hit is stored
// with its hit kind.  The walk's candidate filter (trace_device.hpp).
template <bool SPILL, int FILTER = kFilterNone>
__global__ __launch_bounds__(kQueueBlock * 2) void ray_query_kernel(const RayQueryArgs a, const uint32_t stack_levels, const uint32_t refill_threshold,
                                                                    const uint32_t early_exit, const Stamps st) {
    vhr_stamp(st);
    extern __shared__ int s_dyn[];                        // per wave: (stack_levels + 3) x 64 ints, see raygen_queue_kernel
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const uint64_t first = (uint64_t(blockIdx.x) * 2u + wave) * kQueryWaveRays;
    if (first >= a.count) return;
    const uint32_t base = uint32_t(first), total = uint32_t(min(uint64_t(kQueryWaveRays), uint64_t(a.count) - first));
    const bool any_hit = a.any_hit != 0u;
    if (a.scene.node_count == 0) {                        // no geometry: every ray misses
        for (uint32_t r = lane; r < total; r += 64u) ray_query_store(a, base + r, any_hit, false, 0.0f, 0.0f, 0.0f, 0u, 0u);
        return;
    }
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    uint32_t overflow = 0, hits = 0;
    bool flagged = false;                                 // decision (vi) asked for binary64 on the lane's current ray
    wave_queue_walk<SPILL, true, false, true>(
        a.scene, stack, stack_levels, lane, total, refill_threshold, early_exit, 0.0f, 0.0f, any_hit, overflow, nullptr, 0u,
        [&](uint32_t r, uint32_t &ray, f3 &ro, f3 &rd, float &tmin, float &tmax) {
            ray = base + r;
            const float4 p = a.rays[size_t(ray) * 2u], q = a.rays[size_t(ray) * 2u + 1u];
            ro = f3{ p.x, p.y, p.z }; tmin = p.w;
            rd = f3{ q.x, q.y, q.z }; tmax = q.w;
        },
        [&](uint32_t ray, uint32_t tri, float u, float v, float t) {
            const bool hit = tri != kNoHit;
            hits += hit ? 1u : 0u;
            uint32_t kind = 0u;
            if constexpr (FILTER == kFilterFace) { if (hit && !any_hit) kind = committed_hit_kind(a, ray, tri); }
            ray_query_store(a, ray, any_hit, hit, t, u, v, hit ? a.scene.tris[tri].prim : 0u, hit ? a.scene.tris[tri].tri : 0u, kind);
            if (flagged) {                                // (rare: a plain vector atomic per listed ray)
                a.redo_list[atomicAdd(&a.counters->redo_count, 1u)] = ray;
                flagged = false;
            }
        }, nullptr,
        [&](uint32_t) { flagged = true; }, query_filter<FILTER>(a, a.masks.shadow, a.ray_masks));
    for (int off = 32; off > 0; off >>= 1) hits += uint32_t(__shfl_xor(int(hits), off));
    const bool wave_overflow = __any(overflow != 0u);
    if (lane == 0) {
        if (hits) atomicAdd(&a.counters->hits, (unsigned long long)hits);
        if (wave_overflow) atomicAdd(&a.counters->overflows, 1u);
    }
}

// Decision (vi), second half, for the rays launch 1 listed: the per-pixel walker with the binary64 redo inside its leaf test.
template <int FILTER = kFilterNone>
__global__ __launch_bounds__(kTraceBlock) void ray_query_redo_kernel(const RayQueryArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_stack[kTraceStack * kTraceBlock];
    const uint32_t n = a.counters->redo_count;            // written by launch 1
    const bool any_hit = a.any_hit != 0u;
    uint32_t overflow = 0;
    int delta = 0;                                        // change of the hit count
    for (uint32_t i = blockIdx.x * kTraceBlock + threadIdx.x; i < n; i += gridDim.x * kTraceBlock) {
        const uint32_t ray = a.redo_list[i];
        const float4 p = a.rays[size_t(ray) * 2u], q = a.rays[size_t(ray) * 2u + 1u];
        const f3 o = f3{ p.x, p.y, p.z }, d = f3{ q.x, q.y, q.z };
        Hit best;
        best.t = best.u = best.v = 0.0f; best.tri_index = 0; best.flat = 0;
        bool hit, was;
        uint32_t ray_mask = a.masks.shadow;
        if constexpr (FILTER == kFilterMask || FILTER == kFilterFace) { if (a.ray_masks) ray_mask &= uint32_t(a.ray_masks[ray]); }
        const uint32_t id = FILTER == kFilterFace ? ray : 0u;          // (the face filter reads the ray's direction by it; the others ask for nothing)
        if (any_hit) {
            was = static_cast<const uint8_t *>(a.results)[ray] != 0u;
            hit = traverse<true>(a.scene, o, d, p.w, q.w, s_stack + threadIdx.x, best, overflow, query_filter<FILTER>(a, ray_mask, nullptr), id);
        } else {
            was = static_cast<const uint32_t *>(a.results)[size_t(ray) * 6u + 3u] != kNoHit;
            hit = traverse<false>(a.scene, o, d, p.w, q.w, s_stack + threadIdx.x, best, overflow, query_filter<FILTER>(a, ray_mask, nullptr), id);
        }
        uint32_t kind = 0u;
        if constexpr (FILTER == kFilterFace) { if (hit && !any_hit) kind = committed_hit_kind(a, ray, best.tri_index); }
        ray_query_store(a, ray, any_hit, hit, best.t, best.u, best.v, hit && !any_hit ? a.scene.tris[best.tri_index].prim : 0u,
                        hit && !any_hit ? a.scene.tris[best.tri_index].tri : 0u, kind);
        delta += int(hit) - int(was);
    }
    if (delta) atomicAdd(&a.counters->hits, (unsigned long long)(long long)delta);
    if (overflow) atomicAdd(&a.counters->overflows, 1u);
}

int launch_ray_query(vhr_context *ctx, const vhr_ray *rays, uint32_t count, bool any_hit, bool alpha_test, void *results, uint32_t cull_mask,
                     const uint8_t *ray_masks, int face_cull) {
    ctx->rq_mask_ran = 0;
    ctx->rq_face_ran = 0;
    if (count == 0) return VHR_OK;
    QueryScratch *const q = stream_scratch(ctx, ctx->rq_scratch, sizeof(RayQueryCounters), "vhr_ray_query");     // this stream's counters and list
    if (!q) return VHR_ERROR_DEVICE;
    if (q->capacity < count) {
        (void)hipFree(q->list);                     // (synchronises: a query still in flight is done with it)
        q->list = nullptr;
        q->capacity = 0;
        if (hipMalloc(reinterpret_cast<void **>(&q->list), size_t(count) * sizeof(uint32_t)) != hipSuccess)
            return ctx->fail(VHR_ERROR_DEVICE, "vhr_ray_query: device allocation failed");
        q->capacity = count;
    }
    RayQueryArgs a;
    a.scene = ctx->device_scene();
    a.rays = reinterpret_cast<const float4 *>(rays);
    a.results = results;
    a.redo_list = q->list;
    ctx->rq_last_counters = a.counters = static_cast<RayQueryCounters *>(q->counters);
    a.count = count;
    a.any_hit = any_hit ? 1u : 0u;
    const QueueLaunch ql = queue_launch(ctx, kOptLdsStackLevels, kOptEarlyExit, 2u);
    const dim3 grid(uint32_t((uint64_t(count) + 2u * kQueryWaveRays - 1u) / (2u * kQueryWaveRays)));
    // the flag on a scene none of whose primitives can discard asks for nothing: the plain kernels
    const bool alpha = alpha_test && ctx->scene_can_discard;
    // the mask likewise: the filtering kernels only where the cull mask acts on the masks the primitives carry, or with per-ray masks (one may be 0)
    const bool mask_acts = ray_masks != nullptr || ctx->ray_mask_acts(cull_mask);
    a.masks = RayMaskArgs{ nullptr, cull_mask, cull_mask, cull_mask, alpha ? 1u : 0u };
    a.ray_masks = ray_masks;
    if (mask_acts) {
        if (const int rc = ensure_device_prim_masks(ctx)) return rc;
        a.masks.prim_masks = ctx->d_prim_masks;
        ctx->rq_mask_ran = 1;
    }
    // vhr_ray_query_faces: the face instantiation where a cull mode is set, and in closest-hit mode whatever it is (the hit kind is reported);
    // terminate-on-first-hit with VHR_FACE_CULL_NONE is vhr_ray_query_masked's launch
    const bool face = face_cull > 0 || (face_cull == 0 && !any_hit);
    a.prim_flips = nullptr;
    a.face_cull = face ? uint32_t(face_cull) : 0u;
    if (face && ctx->primitive_count != 0) {
        if (const int rc = ensure_device_prim_flips(ctx)) return rc;
        a.prim_flips = ctx->d_prim_flips;
    }
    ctx->rq_face_ran = face ? 1u : 0u;
    const int filter = face ? kFilterFace : launch_filter(mask_acts, alpha);
    const uint32_t redo_blocks = std::min<uint32_t>((count + kTraceBlock - 1u) / kTraceBlock, uint32_t(ctx->cu_count) * 4u);
    ctx->time_begin(kKernelRayQuery);
    if (face) {
        with_bool(ql.spill, [&](auto sp) {
            launch(ctx, ray_query_kernel<decltype(sp)::value, kFilterFace>, grid, dim3(kQueueBlock * 2), ql.lds_bytes, a, ql.levels, ql.threshold, ql.early_exit);
        });
        if (a.scene.node_count != 0) launch(ctx, ray_query_redo_kernel<kFilterFace>, dim3(redo_blocks), dim3(kTraceBlock), 0, a);
    } else {
        with_bool(ql.spill, [&](auto sp) { with_filter(filter, [&](auto al) {
            launch(ctx, ray_query_kernel<decltype(sp)::value, decltype(al)::value>, grid, dim3(kQueueBlock * 2), ql.lds_bytes, a, ql.levels, ql.threshold, ql.early_exit);
        }); });
        if (a.scene.node_count != 0)
            with_filter(filter, [&](auto al) { launch(ctx, ray_query_redo_kernel<decltype(al)::value>, dim3(redo_blocks), dim3(kTraceBlock), 0, a); });
    }
    ctx->time_end(kKernelRayQuery);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "vhr_ray_query: kernel launch failed");
    return VHR_OK;
}

}  // namespace vhr
