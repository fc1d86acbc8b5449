// Query half of the C ABI (include/vhr_amd.h): batched ray queries, closest-point and k-nearest queries on the scene's tree, the surface points of their
// hits (vhr_resolve_hits), hemisphere occlusion masks at such points (vhr_occlusion_query), their host-memory staging and statistics, and the pair entry points that run one shared function (ray / triangle, facing, point / triangle) on a list of inputs.
#include <cstring>
#include <string>

#include "vhr_internal.hpp"
#include "closest_point.hpp"  // point_triangle's host copy (vhr_debug_point_triangle on a host-only context)
#include "occlusion_rays.hpp" // occlusion_ray's host copy (vhr_debug_occlusion_rays on a host-only context)
#include "ray_facing.hpp"     // ray_hit_kind's host copy (vhr_debug_ray_facing on a host-only context)
#include "surface_point.hpp"  // surface_geometry's host copy (vhr_resolve_hits on a host-only context)

using namespace vhr;

void vhr::free_query_scratch(vhr_context *ctx) {
    for (auto *all : { &ctx->rq_scratch, &ctx->pq_scratch, &ctx->nq_scratch, &ctx->sp_scratch, &ctx->oq_scratch })
        for (QueryScratch &q : *all) { hipFree(q.counters); hipFree(q.list); }
    hipFree(ctx->d_rq_staging);
}

QueryScratch *vhr::stream_scratch(vhr_context *ctx, std::vector<QueryScratch> &all, size_t counter_bytes, const char *who) {
    QueryScratch *q = nullptr;
    for (QueryScratch &e : all) if (e.stream == ctx->stream) q = &e;
    if (!q) {
        void *counters = nullptr;
        if (hipMalloc(&counters, counter_bytes) != hipSuccess) { ctx->fail(VHR_ERROR_DEVICE, std::string(who) + ": device allocation failed"); return nullptr; }
        all.push_back(QueryScratch{ ctx->stream, counters, nullptr, 0 });
        q = &all.back();
    }
    if (hipMemsetAsync(q->counters, 0, counter_bytes, ctx->stream) != hipSuccess) { ctx->fail(VHR_ERROR_DEVICE, std::string(who) + ": hipMemsetAsync failed"); return nullptr; }
    return q;
}

// A host-memory call, staged through the context's one buffer (it grows to the largest call so far; its old contents are not kept): the input,
// the output at the next 256-byte boundary and -- the ray query's per-ray masks -- a second input (or null) at the boundary behind that.  Copies
// in, has `enqueue(in, out, in2)` launch on the staged pointers, copies out and waits for ctx->stream, so no call finds another's data in the buffer.
template <typename Enqueue>
static int staged_call(vhr_context *ctx, const void *in, uint64_t in_bytes, const void *in2, uint64_t in2_bytes, void *out, uint64_t out_bytes, Enqueue &&enqueue) {
    const uint64_t out_offset = (in_bytes + 255u) & ~uint64_t(255u), in2_offset = (out_offset + out_bytes + 255u) & ~uint64_t(255u);
    const uint64_t staging = in2 ? in2_offset + in2_bytes : out_offset + out_bytes;
    if (ctx->rq_staging_bytes < staging) {
        (void)hipFree(ctx->d_rq_staging);
        ctx->d_rq_staging = nullptr;
        ctx->rq_staging_bytes = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->d_rq_staging, staging));
        ctx->rq_staging_bytes = staging;
    }
    char *const d = static_cast<char *>(ctx->d_rq_staging);
    HIP_TRY(ctx, hipMemcpyAsync(d, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (in2) HIP_TRY(ctx, hipMemcpyAsync(d + in2_offset, in2, in2_bytes, hipMemcpyHostToDevice, ctx->stream));
    VHR_TRY(enqueue(d, d + out_offset, in2 ? d + in2_offset : nullptr));
    HIP_TRY(ctx, hipMemcpyAsync(out, d + out_offset, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return VHR_OK;
}

// the counters of an entry point's last call: its stream may be the caller's, so wait for the device, then read
static int read_last_counters(vhr_context *ctx, void *out, const void *counters, size_t bytes) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out, counters, bytes, hipMemcpyDeviceToHost));
    return VHR_OK;
}

// The argument tests the entry points share.  Each keeps its own ORDER of them: which message wins when a call has two faults is behaviour.
static bool misaligned(const void *p, uint32_t count, uintptr_t boundary) { return count > 0 && reinterpret_cast<uintptr_t>(p) % boundary; }
static int invalid(vhr_context *ctx, const std::string &msg) { return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, msg); }

extern "C" {

// vhr_ray_query, vhr_ray_query_masked and vhr_ray_query_faces: one body.  `who` names the entry point in messages; `masked` = the second and the
// third (cull_mask checked, the filtering kernels where the mask acts or per-ray masks are given); face_cull = the third's VHR_FACE_CULL_* (checked
// behind cull_mask), -1 from the others.
static int ray_query_impl(vhr_context *ctx, const char *who_, const bool masked, const vhr_ray *rays, uint32_t count, uint32_t flags, uint32_t cull_mask,
                          const uint8_t *ray_masks, void *results, const int64_t face_cull = -1) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    const std::string who(who_);
    // the arguments first (the same answer on every context), then the device
    if (flags & ~uint32_t(VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT | VHR_RAY_QUERY_HOST_MEMORY | VHR_RAY_QUERY_ALPHA_TEST)) return invalid(ctx, who + ": unknown flag bits " + std::to_string(flags));
    if (count > 0 && (!rays || !results)) return invalid(ctx, who + ": rays and results must not be NULL when count > 0");
    if (misaligned(rays, count, 16u)) return invalid(ctx, who + ": rays must be 16-byte aligned");
    if (misaligned(results, count, 4u)) return invalid(ctx, who + ": results must be 4-byte aligned");
    if (masked && cull_mask > 0xFFu) return invalid(ctx, who + ": cull_mask " + std::to_string(cull_mask) + " exceeds 0xFF");
    if (face_cull > int64_t(VHR_FACE_CULL_FRONT))
        return invalid(ctx, who + ": face_cull " + std::to_string(face_cull) + " is none of VHR_FACE_CULL_NONE / BACK / FRONT (the two do not combine)");
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, who + ": host-only context: no device work");
    VHR_TRY(ctx->refuse_if_stale(who_));
    if (count == 0) return VHR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool any_hit = (flags & VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT) != 0, alpha_test = (flags & VHR_RAY_QUERY_ALPHA_TEST) != 0;
    ctx->rq_rays = count;
    if (!masked) { cull_mask = 0xFFu; ray_masks = nullptr; }
    const auto enqueue = [&](const void *r, void *out, const void *masks) {
        return vhr::launch_ray_query(ctx, static_cast<const vhr_ray *>(r), count, any_hit, alpha_test, out, cull_mask, static_cast<const uint8_t *>(masks), int(face_cull));
    };
    if (!(flags & VHR_RAY_QUERY_HOST_MEMORY)) return enqueue(rays, results, ray_masks);
    // host memory: the rays, the results and (vhr_ray_query_masked, vhr_ray_query_faces) the per-ray masks, one byte each
    return staged_call(ctx, rays, uint64_t(count) * sizeof(vhr_ray), ray_masks, count, results, uint64_t(count) * (any_hit ? 1u : sizeof(vhr_ray_hit)), enqueue);
}

int vhr_ray_query(vhr_context *ctx, const vhr_ray *rays, uint32_t count, uint32_t flags, void *results) {
    return ray_query_impl(ctx, "vhr_ray_query", false, rays, count, flags, 0xFFu, nullptr, results);
}

int vhr_ray_query_masked(vhr_context *ctx, const vhr_ray *rays, uint32_t count, uint32_t flags, uint32_t cull_mask, const uint8_t *ray_masks, void *results) {
    return ray_query_impl(ctx, "vhr_ray_query_masked", true, rays, count, flags, cull_mask, ray_masks, results);
}

int vhr_ray_query_faces(vhr_context *ctx, const vhr_ray *rays, uint32_t count, uint32_t flags, uint32_t cull_mask, const uint8_t *ray_masks,
                        uint32_t face_cull, void *results) {
    return ray_query_impl(ctx, "vhr_ray_query_faces", true, rays, count, flags, cull_mask, ray_masks, results, int64_t(face_cull));
}

// a device context runs the device's copy of ray_hit_kind, a host-only context the host's: one source (ray_facing.hpp)
int vhr_debug_ray_facing(vhr_context *ctx, const float *pairs, const uint8_t *flips, uint32_t count, uint8_t *out) {
    if (!ctx || (count && (!pairs || !out))) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_debug_ray_facing: null argument") : VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) return launch_ray_facing_pairs(ctx, pairs, flips, count, out);
    for (uint32_t i = 0; i < count; ++i) {
        const float *s = pairs + size_t(i) * 9u;
        out[i] = uint8_t(ray_hit_kind(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], flips != nullptr && flips[i] != 0));
    }
    return VHR_OK;
}

int vhr_get_ray_query_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ctx->host_only || ctx->rq_rays == 0 || !ctx->rq_last_counters) return VHR_OK;
    RayQueryCounters c;
    VHR_TRY(read_last_counters(ctx, &c, ctx->rq_last_counters, sizeof(c)));
    out[0] = ctx->rq_rays; out[1] = c.hits; out[2] = c.redo_count; out[3] = c.overflows;
    return VHR_OK;
}

// vhr_closest_point_query: the arguments first (the same answer on every context), then the device; staged like the ray query's host path
int vhr_closest_point_query(vhr_context *ctx, const vhr_point_query *points, uint32_t count, uint32_t flags, uint32_t cull_mask, void *results) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    const std::string who("vhr_closest_point_query");
    if (count > 0 && (!points || !results)) return invalid(ctx, who + ": points and results must not be NULL when count > 0");
    if (flags & ~uint32_t(VHR_POINT_QUERY_ANY_WITHIN | VHR_POINT_QUERY_HOST_MEMORY)) return invalid(ctx, who + ": unknown flag bits " + std::to_string(flags));
    if (misaligned(points, count, 16u)) return invalid(ctx, who + ": points must be 16-byte aligned");
    if (misaligned(results, count, 4u)) return invalid(ctx, who + ": results must be 4-byte aligned");
    if (cull_mask > 0xFFu) return invalid(ctx, who + ": cull_mask " + std::to_string(cull_mask) + " exceeds 0xFF");
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, who + ": host-only context: no device work");
    VHR_TRY(ctx->refuse_if_stale("vhr_closest_point_query"));
    if (count == 0) return VHR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool any_within = (flags & VHR_POINT_QUERY_ANY_WITHIN) != 0;
    ctx->pq_queries = count;
    const auto enqueue = [&](const void *p, void *out, const void *) { return vhr::launch_point_query(ctx, static_cast<const vhr_point_query *>(p), count, any_within, cull_mask, out); };
    if (!(flags & VHR_POINT_QUERY_HOST_MEMORY)) return enqueue(points, results, nullptr);
    return staged_call(ctx, points, uint64_t(count) * sizeof(vhr_point_query), nullptr, 0, results, uint64_t(count) * (any_within ? 1u : sizeof(vhr_ray_hit)), enqueue);
}

int vhr_get_point_query_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ctx->host_only || ctx->pq_queries == 0 || !ctx->pq_last_counters) return VHR_OK;
    PointQueryCounters c;
    VHR_TRY(read_last_counters(ctx, &c, ctx->pq_last_counters, sizeof(c)));
    out[0] = ctx->pq_queries; out[1] = c.found; out[2] = c.evaluations; out[3] = c.overflows;
    return VHR_OK;
}

// vhr_nearest_points_query: the closest-point query's checks in its order, then k; staged the same way, k records per query out
int vhr_nearest_points_query(vhr_context *ctx, const vhr_point_query *points, uint32_t count, uint32_t k, uint32_t flags, uint32_t cull_mask, vhr_ray_hit *results) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    const std::string who("vhr_nearest_points_query");
    if (count > 0 && (!points || !results)) return invalid(ctx, who + ": points and results must not be NULL when count > 0");
    if (flags & ~uint32_t(VHR_POINT_QUERY_HOST_MEMORY)) return invalid(ctx, who + ": unknown flag bits " + std::to_string(flags));
    if (misaligned(points, count, 16u)) return invalid(ctx, who + ": points must be 16-byte aligned");
    if (misaligned(results, count, 4u)) return invalid(ctx, who + ": results must be 4-byte aligned");
    if (cull_mask > 0xFFu) return invalid(ctx, who + ": cull_mask " + std::to_string(cull_mask) + " exceeds 0xFF");
    if (k == 0 || k > VHR_NEAREST_MAX_K) return invalid(ctx, who + ": k " + std::to_string(k) + " is not in 1 .. VHR_NEAREST_MAX_K (" + std::to_string(VHR_NEAREST_MAX_K) + ")");
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, who + ": host-only context: no device work");
    VHR_TRY(ctx->refuse_if_stale("vhr_nearest_points_query"));
    if (count == 0) return VHR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->nq_queries = count;
    const auto enqueue = [&](const void *p, void *out, const void *) {
        return vhr::launch_nearest_query(ctx, static_cast<const vhr_point_query *>(p), count, k, cull_mask, static_cast<vhr_ray_hit *>(out));
    };
    if (!(flags & VHR_POINT_QUERY_HOST_MEMORY)) return enqueue(points, results, nullptr);
    return staged_call(ctx, points, uint64_t(count) * sizeof(vhr_point_query), nullptr, 0, results, uint64_t(count) * k * sizeof(vhr_ray_hit), enqueue);
}

int vhr_get_nearest_query_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ctx->host_only || ctx->nq_queries == 0 || !ctx->nq_last_counters) return VHR_OK;
    NearestQueryCounters c;
    VHR_TRY(read_last_counters(ctx, &c, ctx->nq_last_counters, sizeof(c)));
    out[0] = ctx->nq_queries; out[1] = c.entries; out[2] = c.evaluations; out[3] = c.overflows;
    return VHR_OK;
}

// a device context runs the device's copy of point_triangle, a host-only context the host's: one source (closest_point.hpp)
int vhr_debug_point_triangle(vhr_context *ctx, const float *pairs, uint32_t count, float *out) {
    if (!ctx || (count && (!pairs || !out))) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_debug_point_triangle: null argument") : VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) return launch_point_triangle_pairs(ctx, pairs, count, out);
    for (uint32_t i = 0; i < count; ++i) {
        const float *s = pairs + size_t(i) * 12u;
        const PointTriangle r = point_triangle(s, s + 3, s + 6, s + 9);
        out[size_t(i) * 3u] = r.d2; out[size_t(i) * 3u + 1u] = r.u; out[size_t(i) * 3u + 2u] = r.v;
    }
    return VHR_OK;
}

// vhr_resolve_hits on a host-only context: the geometry part from the arrays the context keeps, by the source the kernel runs (surface_point.hpp)
static void resolve_hits_host(vhr_context *ctx, const vhr_ray_hit *hits, uint32_t count, vhr_surface_point *out) {
    ctx->sp_host_counters = SurfaceCounters{};
    const uint32_t primitive_count = ctx->has_geometry() ? ctx->primitive_count : 0u;
    for (uint32_t i = 0; i < count; ++i) {
        // (hits need 4-byte alignment only, which is vhr_ray_hit's own; out is 16-byte aligned)
        const vhr_ray_hit &h = hits[i];
        vhr_surface_point &o = out[i];
        std::memset(&o, 0, sizeof(o));
        if (!surface_hit_addressable(h.u, h.v, h.geometry_index, h.primitive_index, primitive_count)) continue;
        const vhr_primitive &prim = ctx->h_primitives[h.geometry_index];
        if (!(h.primitive_index < prim.index_count / 3u)) continue;
        const uint32_t *ix = ctx->h_indices.data() + (size_t(prim.index_offset) + 3u * size_t(h.primitive_index));
        const vhr_vertex *vx = ctx->h_vertices.data() + prim.vertex_offset;
        float M[9];
        normal_matrix3(prim.transform, M);
        const SurfaceGeometry s = surface_geometry(prim.transform, ctx->h_prim_flips[h.geometry_index] != 0, M, vx[ix[0]], vx[ix[1]], vx[ix[2]], h.u, h.v);
        for (int k = 0; k < 3; ++k) { o.position[k] = s.position[k]; o.geometric_normal[k] = s.geometric_normal[k]; o.shading_normal[k] = s.shading_normal[k]; }
        for (int k = 0; k < 2; ++k) { o.uv0[k] = s.uv0[k]; o.uv1[k] = s.uv1[k]; }
        o.flags = s.flags;
        ++ctx->sp_host_counters.valid;
    }
}

// vhr_resolve_hits: the arguments first (the same answer on every context), then the device; staged like the queries' host paths
int vhr_resolve_hits(vhr_context *ctx, const vhr_ray_hit *hits, uint32_t count, uint32_t flags, vhr_surface_point *out) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    const std::string who("vhr_resolve_hits");
    if (count > 0 && (!hits || !out)) return invalid(ctx, who + ": hits and out must not be NULL when count > 0");
    if (flags & ~uint32_t(VHR_SURFACE_MATERIAL | VHR_SURFACE_HOST_MEMORY)) return invalid(ctx, who + ": unknown flag bits " + std::to_string(flags));
    if (misaligned(hits, count, 4u)) return invalid(ctx, who + ": hits must be 4-byte aligned");
    if (misaligned(out, count, 16u)) return invalid(ctx, who + ": out must be 16-byte aligned");
    if (count == 0) return VHR_OK;
    const bool material = (flags & VHR_SURFACE_MATERIAL) != 0, host_memory = (flags & VHR_SURFACE_HOST_MEMORY) != 0;
    if (ctx->host_only && (material || !host_memory))
        return ctx->fail(VHR_ERROR_NO_DEVICE, who + ": host-only context: " + (material ? "no textures are sampled without a device (VHR_SURFACE_MATERIAL)" : "no device memory (VHR_SURFACE_HOST_MEMORY)"));
    VHR_TRY(ctx->refuse_if_stale("vhr_resolve_hits"));
    ctx->sp_hits = count;
    ctx->sp_material = material;
    if (ctx->host_only) { resolve_hits_host(ctx, hits, count, out); return VHR_OK; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto enqueue = [&](const void *h, void *o, const void *) { return vhr::launch_resolve_hits(ctx, static_cast<const vhr_ray_hit *>(h), count, material, static_cast<vhr_surface_point *>(o)); };
    if (!host_memory) return enqueue(hits, out, nullptr);
    return staged_call(ctx, hits, uint64_t(count) * sizeof(vhr_ray_hit), nullptr, 0, out, uint64_t(count) * sizeof(vhr_surface_point), enqueue);
}

int vhr_get_surface_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ctx->sp_hits == 0) return VHR_OK;
    SurfaceCounters c = ctx->sp_host_counters;
    if (!ctx->host_only) {
        if (!ctx->sp_last_counters) return VHR_OK;
        SurfaceCounters slots[kSurfaceCounterSlots];
        VHR_TRY(read_last_counters(ctx, slots, ctx->sp_last_counters, sizeof(slots)));
        c = SurfaceCounters{};
        for (const SurfaceCounters &slot : slots) { c.valid += slot.valid; c.discarded += slot.discarded; }
    }
    out[0] = ctx->sp_hits; out[1] = c.valid; out[2] = c.discarded; out[3] = ctx->sp_material ? 1u : 0u;
    return VHR_OK;
}

// vhr_occlusion_query: the arguments first, in the contract's order (the same answer on every context), then the device; staged like the queries' host paths
int vhr_occlusion_query(vhr_context *ctx, const vhr_ray *points, uint32_t count, uint32_t samples, uint32_t seed, uint32_t flags, uint32_t cull_mask, uint64_t *occluded) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    const std::string who("vhr_occlusion_query");
    if (count > 0 && (!points || !occluded)) return invalid(ctx, who + ": points and occluded must not be NULL when count > 0");
    if (flags & ~uint32_t(VHR_OCCLUSION_HOST_MEMORY)) return invalid(ctx, who + ": unknown flag bits " + std::to_string(flags));
    if (misaligned(points, count, 16u)) return invalid(ctx, who + ": points must be 16-byte aligned");
    if (misaligned(occluded, count, 8u)) return invalid(ctx, who + ": occluded must be 8-byte aligned");
    if (cull_mask > 0xFFu) return invalid(ctx, who + ": cull_mask " + std::to_string(cull_mask) + " exceeds 0xFF");
    if (samples == 0 || samples > VHR_OCCLUSION_MAX_SAMPLES)
        return invalid(ctx, who + ": samples " + std::to_string(samples) + " is not in 1 .. VHR_OCCLUSION_MAX_SAMPLES (" + std::to_string(VHR_OCCLUSION_MAX_SAMPLES) + ")");
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, who + ": host-only context: no device work");
    VHR_TRY(ctx->refuse_if_stale("vhr_occlusion_query"));
    if (count == 0) return VHR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->oq_points = count;
    const auto enqueue = [&](const void *p, void *out, const void *) {
        return vhr::launch_occlusion_query(ctx, static_cast<const vhr_ray *>(p), count, samples, seed, cull_mask, static_cast<uint64_t *>(out));
    };
    if (!(flags & VHR_OCCLUSION_HOST_MEMORY)) return enqueue(points, occluded, nullptr);
    return staged_call(ctx, points, uint64_t(count) * sizeof(vhr_ray), nullptr, 0, occluded, uint64_t(count) * sizeof(uint64_t), enqueue);
}

int vhr_get_occlusion_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (ctx->host_only || ctx->oq_points == 0 || !ctx->oq_last_counters) return VHR_OK;
    OcclusionCounters c;
    VHR_TRY(read_last_counters(ctx, &c, ctx->oq_last_counters, sizeof(c)));
    out[0] = ctx->oq_points; out[1] = c.occluded; out[2] = c.redo_count; out[3] = c.overflows;
    return VHR_OK;
}

// a device context runs the device's copy of occlusion_ray, a host-only context the host's: one source (occlusion_rays.hpp)
int vhr_debug_occlusion_rays(vhr_context *ctx, const vhr_ray *points, uint32_t count, uint32_t samples, uint32_t seed, vhr_ray *out) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (count && (!points || !out)) return invalid(ctx, "vhr_debug_occlusion_rays: null argument");
    if (samples == 0 || samples > VHR_OCCLUSION_MAX_SAMPLES)
        return invalid(ctx, "vhr_debug_occlusion_rays: samples " + std::to_string(samples) + " is not in 1 .. VHR_OCCLUSION_MAX_SAMPLES (" + std::to_string(VHR_OCCLUSION_MAX_SAMPLES) + ")");
    if (!ctx->host_only) return launch_occlusion_rays(ctx, points, count, samples, seed, out);
    for (uint32_t i = 0; i < count; ++i) {
        const vhr_ray &p = points[i];
        const OcclusionRay point{ f3{ p.origin[0], p.origin[1], p.origin[2] }, p.tmin, f3{ p.direction[0], p.direction[1], p.direction[2] }, p.tmax };
        for (uint32_t j = 0; j < samples; ++j) {
            const OcclusionRay r = occlusion_ray(point, i, j, samples, seed);
            vhr_ray &o = out[size_t(i) * samples + j];
            o.origin[0] = r.o.x; o.origin[1] = r.o.y; o.origin[2] = r.o.z; o.tmin = r.tmin;
            o.direction[0] = r.d.x; o.direction[1] = r.d.y; o.direction[2] = r.d.z; o.tmax = r.tmax;
        }
    }
    return VHR_OK;
}

int vhr_surface_point_layout(uint32_t out[8]) {
    if (!out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = sizeof(vhr_surface_point); out[1] = offsetof(vhr_surface_point, flags); out[2] = offsetof(vhr_surface_point, geometric_normal);
    out[3] = offsetof(vhr_surface_point, metallic); out[4] = offsetof(vhr_surface_point, shading_normal); out[5] = offsetof(vhr_surface_point, roughness);
    out[6] = offsetof(vhr_surface_point, base_color); out[7] = offsetof(vhr_surface_point, uv0);
    return 8;
}

int vhr_ray_query_struct_layout(uint32_t out[8]) {
    if (!out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = sizeof(vhr_ray); out[1] = offsetof(vhr_ray, tmin); out[2] = offsetof(vhr_ray, direction); out[3] = offsetof(vhr_ray, tmax);
    out[4] = sizeof(vhr_ray_hit); out[5] = offsetof(vhr_ray_hit, geometry_index); out[6] = offsetof(vhr_ray_hit, primitive_index);
    out[7] = offsetof(vhr_ray_hit, reserved);
    return 8;
}

int vhr_debug_ray_triangle(vhr_context *ctx, const float *pairs, uint32_t count, uint32_t *hit, float *tuv) {
    if (!ctx || (count && (!pairs || !hit || !tuv))) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_debug_ray_triangle: null argument") : VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return ctx->fail(VHR_ERROR_DEVICE, "vhr_debug_ray_triangle: host-only context");
    return launch_ray_triangle_pairs(ctx, pairs, count, hit, tuv);
}

}  // extern "C"
