// The "Forward Pass" stand-ins of the rayquery render path (inline shadow queries) and of the forward raster path (8x MSAA and its
// resolve).  (Split from kernels_trace.hip, where they followed the composition stand-in; built with the same flags.)
#define VHR_TRACE_UNIT unit_forward      // this unit's copy of the sRGB decode table (trace_device.hpp)
#include "trace_queue.hpp"

namespace vhr {

// ---------------------------------------------------------------------------------------------
// Stand-in for the rayquery render path's "Forward Pass" (rayquery_render_path.cpp:11-54, default.vert:19-28, default.frag:16-49):
// the visible surface of every pixel by a primary ray (gbuffer_kernel's camera ray: from the camera through the near-plane point of
// the pixel centre, tmin 1 in that parameterisation, no alpha layers -- the raster pass discards nothing), then the fragment stage:
// one terminate-on-first-hit query from in_pos towards the light (tmin 0.1, tmax 10000, every triangle opaque) and the shading of
// default.frag.  Writes swapchain texels (B8G8R8A8_SRGB, presentation orientation: row 0 = top, like composition_kernel), the
// reverse-Z depth in the G-buffer's orientation (clip.z / clip.w, like gbuffer_kernel) and, where asked for, three probes per pixel in
// Depth's row order: the committed primary hit (vhr_ray_hit), in_pos with w = 1 (0 for a miss) and the query's answer.  A miss writes
// (0, 0, 0, 0) and depth 0 (the clears of :16-17).
// ---------------------------------------------------------------------------------------------
struct RayqueryForwardArgs {
    DeviceScene scene;
    vhr_per_frame_data pfd;
    float projview[16];      // camera_proj * camera_view (the depth, as gbuffer_kernel computes it)
    uchar4 *out;             // RENDER_OUTPUT: B8G8R8A8_SRGB texels
    float *depth;            // "Depth", D32_SFLOAT
    uint32_t *hits;          // probes, nullptr = not asked for: vhr_ray_hit (6 words) per pixel
    float *positions;        // 4 floats per pixel
    uint8_t *shadowed;       // 1 = the inline query found an occluder
    uint32_t width, height;
    RayStats *stats;         // nullptr = off; covered_pixels counts the primary hits (= queries)
};

// the camera ray of a pixel (gbuffer_kernel): origin the camera, direction to the pixel centre's point on the near plane (reverse Z: depth 1)
__device__ __forceinline__ f3 rayquery_primary_dir(const vhr_per_frame_data &pfd, f3 cam, uint32_t x, uint32_t y, uint32_t W, uint32_t H) {
    const float u = (float(x) + 0.5f) / float(W), v = (float(y) + 0.5f) / float(H);
    return get_world_space_position(pfd, 1.0f, u, v) - cam;
}

// default.frag:16-48 once the inline query's answer is known
__device__ f3 rayquery_forward_shade(const DeviceScene &sc, const vhr_per_frame_data &pfd, const Hit &h, bool shadowed) {
    const BvhTri &bt = sc.tris[h.tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];                                  // :16
    const TriAttributes at = interpolate(sc, prim, bt.tri, h.u, h.v);                     // in_normal: object space, not renormalised (vert:23)
    f3 albedo;
    if (prim.material.base_color_texture == -1) {                                        // :17-23
        albedo = f3{ prim.material.base_color[0], prim.material.base_color[1], prim.material.base_color[2] };
    } else {
        const f4 t = sample_texture(sc, prim.material.base_color_texture, at.uvx, at.uvy);
        albedo = f3{ t.x, t.y, t.z };
    }
    const f3 normal = at.normal;
    f3 N = normal;                                                                       // :25-31
    if (prim.material.normal_map >= 0) {
        const f4 tg = interpolate_tangent(sc, prim, bt.tri, h.u, h.v);
        const f3 T = f3{ tg.x, tg.y, tg.z };
        const f4 tx = sample_texture(sc, prim.material.normal_map, at.uvx, at.uvy);
        const f3 tsn = normalize3(f3{ tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f });
        const f3 bitangent = cross3(tsn, T) * tg.w;                                      // sic
        const f3 tangent = normalize3(T - normal * dot3(T, normal));
        N = (tangent * tsn.x + bitangent * tsn.y) + normal * tsn.z;
    }
    const f3 light_dir = -f3{ pfd.directional_light.direction[0], pfd.directional_light.direction[1], pfd.directional_light.direction[2] };
    const f3 lc = f3{ pfd.directional_light.color[0], pfd.directional_light.color[1], pfd.directional_light.color[2] };
    const float in_shadow = shadowed ? 0.0f : 1.0f;                                      // :41-44
    const f3 ambient = albedo * 0.2f;                                                    // :46
    return ambient + mul3(mul3(albedo * fmaxf(dot3(N, light_dir), 0.0f), lc), f3{ in_shadow, in_shadow, in_shadow });   // :47 (no light.intensity)
}

// the pixel's outputs: texel (flipped presentation row), depth and the probes (Depth's rows); `hit` false = the clears
__device__ __forceinline__ void rayquery_forward_store(const RayqueryForwardArgs &a, const uint32_t x, const uint32_t y, const bool hit, const Hit &h,
                                                       const f3 cam, const f3 dir, const f3 position, const bool shadowed) {
    const uint32_t W = a.width, H = a.height;
    const size_t i = size_t(y) * W + x;
    uchar4 texel = make_uchar4(0, 0, 0, 0);
    float depth = 0.0f;
    if (hit) {
        const f3 c = rayquery_forward_shade(a.scene, a.pfd, h, shadowed);
        texel = make_uchar4(srgb8(c.z), srgb8(c.y), srgb8(c.x), 255);                      // out_color = vec4(.., 1.0) through the sRGB attachment
        const f3 P = cam + dir * h.t;
        const f4 clip = mat4_mul(a.projview, f4{ P.x, P.y, P.z, 1.0f });
        depth = clip.z / clip.w;
    }
    a.out[size_t(H - 1 - y) * W + x] = texel;
    a.depth[i] = depth;
    if (a.hits) {
        uint32_t *const r = a.hits + i * 6u;
        r[0] = hit ? __float_as_uint(h.t) : 0u; r[1] = hit ? __float_as_uint(h.u) : 0u; r[2] = hit ? __float_as_uint(h.v) : 0u;
        r[3] = hit ? a.scene.tris[h.tri_index].prim : kNoHit; r[4] = hit ? a.scene.tris[h.tri_index].tri : kNoHit; r[5] = 0u;
    }
    if (a.positions) {
        float *const p = a.positions + i * 4u;
        p[0] = hit ? position.x : 0.0f; p[1] = hit ? position.y : 0.0f; p[2] = hit ? position.z : 0.0f; p[3] = hit ? 1.0f : 0.0f;
    }
    if (a.shadowed) a.shadowed[i] = hit && shadowed ? 1u : 0u;
}

// Literal form (`variant_rayquery` 0): one pixel per thread, the two rays one after the other through traverse<> -- the cross-check.
__global__ __launch_bounds__(kTraceBlock) void rayquery_forward_kernel(const RayqueryForwardArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_rq_stack[kTraceStack * kTraceBlock];
    int *stack = s_rq_stack + threadIdx.x;
    uint32_t x, y;
    pixel_of_thread(x, y, 0);
    bool hit = false;
    uint32_t overflow = 0;
    if (x < a.width && y < a.height) {
        const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
        const f3 dir = rayquery_primary_dir(a.pfd, cam, x, y, a.width, a.height);
        Hit h;
        h.t = h.u = h.v = 0.0f; h.tri_index = 0; h.flat = 0;
        hit = traverse<false>(a.scene, cam, dir, 1.0f, 3.0e38f, stack, h, overflow);
        f3 position = f3{ 0.0f, 0.0f, 0.0f };
        bool shadowed = false;
        if (hit) {
            f3 unused_normal;
            hit_position_normal(a.scene, h, position, unused_normal);                    // in_pos (vert:22, interpolated)
            const f3 light_dir = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1], a.pfd.directional_light.direction[2] };
            Hit sh;
            shadowed = traverse<true>(a.scene, position, light_dir, 0.1f, 10000.0f, stack, sh, overflow);   // frag:36-44
        }
        rayquery_forward_store(a, x, y, hit, h, cam, dir, position, shadowed);
    }
    if (a.stats) {
        const unsigned long long cov = __ballot(hit), ovf = __ballot(overflow != 0);
        if ((threadIdx.x & 63u) == 0) {
            if (cov) atomicAdd(&a.stats->covered_pixels, (unsigned long long)__popcll(cov));
            if (ovf) atomicAdd(&a.stats->stack_overflows, (unsigned long long)__popcll(ovf));
        }
    }
}

// Work-queue form (default, `variant_rayquery` 1), raytraced_queue_kernel's schedule: a wave owns a 16x8-pixel tile and runs
// wave_queue_walk twice -- the primary rays (closest hit, each ray's t committed for the depth), then the inline query of every
// covered pixel (any hit) from the tile's shared descent around the hit points -- with the ray setup, in_pos and default.frag done by
// the whole wave in between and after.  Decision (vi) is decided inline in binary64 like the raytraced path's queue kernel (its shadow
// rays leave the surface itself): the same test as traverse<>, so the same rays give rayquery_forward_kernel's outputs bit for bit.
template <bool SPILL>
__global__ __launch_bounds__(kQueueBlock * 2) __attribute__((amdgpu_waves_per_eu(5, 6))) void rayquery_forward_queue_kernel(
    const RayqueryForwardArgs a, const uint32_t stack_levels, const uint32_t refill_threshold, const uint32_t tiles_x, const uint32_t tiles_total,
    const uint32_t early_exit, const Stamps st) {
    vhr_stamp(st);
    extern __shared__ int s_dyn[];                        // per wave: (stack_levels + 3) x 64 ints
    // rows 0-2: primary direction -> rows 0-3 primary hit record (triangle, u, v, t); rows 4-6: in_pos; row 7: the query's answer
    __shared__ float s_ray_all[2][8][kReflRays];
    __shared__ uint8_t s_list_all[2][kReflRays];
    __shared__ float4 s_cut_all[2][kCutMax][2];           // the tile's shared descent (build_tile_cut), once per walk
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const uint32_t tile = blockIdx.x * 2u + wave;
    if (tile >= tiles_total) return;                      // waves of a block share nothing and never synchronise
    float (&s_ray)[8][kReflRays] = s_ray_all[wave];
    uint8_t (&s_list)[kReflRays] = s_list_all[wave];
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    const uint32_t W = a.width, H = a.height;
    const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
    const f3 light_dir = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1], a.pfd.directional_light.direction[2] };

    // ---- primary rays, whole wave ----
    unsigned long long in_mask[2];
    uint32_t total = 0;
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        const uint32_t x = tile_x * 16u + sub * 8u + (lane & 7u), y = tile_y * 8u + (lane >> 3);
        const bool in_range = x < W && y < H;
        const uint32_t p = sub * 64u + lane;
        if (in_range) {
            const f3 dir = rayquery_primary_dir(a.pfd, cam, x, y, W, H);
            s_ray[0][p] = dir.x; s_ray[1][p] = dir.y; s_ray[2][p] = dir.z;
        }
        const unsigned long long m = __ballot(in_range);
        in_mask[sub] = m;
        if (in_range) s_list[total + lane_rank(m)] = uint8_t(p);
        total += uint32_t(__popcll(m));
    }
    wave_lds_sync();
    const bool traced = a.scene.node_count != 0;
    uint32_t overflow = 0;
    // ---- walk 1: closest hit of the primary rays; the commit keeps t (PER_RAY) for the depth ----
    uint32_t cut_n = traced && total ? build_tile_cut_uniform(a.scene, cam, cam, s_cut_all[wave], lane) : 0u;
    wave_queue_walk<SPILL, false, false, true>(
        a.scene, stack, stack_levels, lane, traced ? total : 0u, refill_threshold, early_exit, 0.0f, 0.0f, false, overflow, s_cut_all[wave], cut_n,
        [&](uint32_t r, uint32_t &pix, f3 &ro, f3 &rd, float &tmin, float &tmax) {
            pix = s_list[r];
            ro = cam;
            rd = f3{ s_ray[0][pix], s_ray[1][pix], s_ray[2][pix] };
            tmin = 1.0f; tmax = 3.0e38f;
        },
        [&](uint32_t pix, uint32_t tri, float u, float v, float t) {
            s_ray[0][pix] = __uint_as_float(tri); s_ray[1][pix] = u; s_ray[2][pix] = v; s_ray[3][pix] = t;
        });
    wave_lds_sync();
    // ---- in_pos of every covered pixel, whole wave (vert:22) ----
    uint32_t nhit = 0;
    f3 omin = f3{ 3.0e38f, 3.0e38f, 3.0e38f }, omax = f3{ -3.0e38f, -3.0e38f, -3.0e38f };   // bounds of the queries' origins
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        const uint32_t p = sub * 64u + lane;
        const bool inside = traced && ((in_mask[sub] >> lane) & 1ull);
        const uint32_t tri = inside ? __float_as_uint(s_ray[0][p]) : kNoHit;
        const bool hit = tri != kNoHit;
        if (hit) {
            Hit h;
            h.t = 0.0f; h.u = s_ray[1][p]; h.v = s_ray[2][p]; h.tri_index = tri; h.flat = 0;
            f3 position, unused_normal;
            hit_position_normal(a.scene, h, position, unused_normal);
            s_ray[4][p] = position.x; s_ray[5][p] = position.y; s_ray[6][p] = position.z;
            omin = f3{ fminf(omin.x, position.x), fminf(omin.y, position.y), fminf(omin.z, position.z) };
            omax = f3{ fmaxf(omax.x, position.x), fmaxf(omax.y, position.y), fmaxf(omax.z, position.z) };
        }
        const unsigned long long m = __ballot(hit);
        if (hit) s_list[nhit + lane_rank(m)] = uint8_t(p);
        nhit += uint32_t(__popcll(m));
    }
    wave_lds_sync();
    // ---- walk 2: the inline queries (frag:36-44), any hit; the answer (an occluder's triangle or kNoHit) lands in row 7 ----
    cut_n = nhit ? build_tile_cut_uniform(a.scene, omin, omax, s_cut_all[wave], lane) : 0u;
    wave_queue_walk<SPILL, false>(
        a.scene, stack, stack_levels, lane, nhit, refill_threshold, early_exit, 0.1f, 10000.0f, true, overflow, s_cut_all[wave], cut_n,
        [&](uint32_t r, uint32_t &pix, f3 &ro, f3 &rd) {
            pix = s_list[r];
            ro = f3{ s_ray[4][pix], s_ray[5][pix], s_ray[6][pix] };
            rd = light_dir;
        },
        [&](uint32_t pix, uint32_t tri, float, float) { s_ray[7][pix] = __uint_as_float(tri); });
    wave_lds_sync();
    // ---- default.frag and the stores, whole wave ----
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        if (!((in_mask[sub] >> lane) & 1ull)) continue;
        const uint32_t x = tile_x * 16u + sub * 8u + (lane & 7u), y = tile_y * 8u + (lane >> 3);
        const uint32_t p = sub * 64u + lane;
        const uint32_t tri = traced ? __float_as_uint(s_ray[0][p]) : kNoHit;
        const bool hit = tri != kNoHit;
        Hit h;
        h.t = hit ? s_ray[3][p] : 0.0f; h.u = hit ? s_ray[1][p] : 0.0f; h.v = hit ? s_ray[2][p] : 0.0f; h.tri_index = hit ? tri : 0u; h.flat = 0;
        const f3 position = hit ? f3{ s_ray[4][p], s_ray[5][p], s_ray[6][p] } : f3{ 0.0f, 0.0f, 0.0f };
        const bool shadowed = hit && __float_as_uint(s_ray[7][p]) != kNoHit;
        rayquery_forward_store(a, x, y, hit, h, cam, rayquery_primary_dir(a.pfd, cam, x, y, W, H), position, shadowed);
    }
    if (a.stats && lane == 0) {
        if (nhit) atomicAdd(&a.stats->covered_pixels, (unsigned long long)nhit);
        if (overflow) atomicAdd(&a.stats->stack_overflows, 1ull);
    }
}

int launch_rayquery_forward(vhr_context *ctx, const vhr_per_frame_data &pfd, Image &out, Image &depth, void *hits, float *positions, uint8_t *shadowed) {
    if (out.width != depth.width || out.height != depth.height) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_rayquery_forward: image extents differ");
    if (out.bpp != 4) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_rayquery_forward: the output storage image must have 4-byte texels (B8G8R8A8_SRGB)");
    if (depth.format != VHR_FORMAT_D32_SFLOAT) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_rayquery_forward: \"Depth\" must be D32_SFLOAT (rayquery_render_path.cpp:17)");
    if (reinterpret_cast<uintptr_t>(hits) % 4u || reinterpret_cast<uintptr_t>(positions) % 4u)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_rayquery_forward: primary_hits and positions must be 4-byte aligned");
    RayqueryForwardArgs a;
    a.scene = ctx->device_scene();
    a.pfd = pfd;
    host_mat4_mul(pfd.camera_proj, pfd.camera_view, a.projview);
    a.out = static_cast<uchar4 *>(out.ptr);
    a.depth = static_cast<float *>(depth.ptr);
    a.hits = static_cast<uint32_t *>(hits);
    a.positions = positions;
    a.shadowed = shadowed;
    a.width = depth.width;
    a.height = depth.height;
    a.stats = ctx->ray_stats_enabled ? ctx->d_ray_stats : nullptr;
    if (a.width == 0 || a.height == 0) return VHR_OK;
    if (const int rc = ray_stats_begin(ctx, a.stats != nullptr)) return rc;
    ctx->time_begin(kKernelRayqueryForward);
    if (ctx->options[kOptRayqueryVariant] != 0) {
        const QueueLaunch q = queue_launch(ctx, kOptLdsStackLevels, kOptEarlyExit, 2u);
        const TileGrid g = tile_grid(a.width, a.height, 16u);
        with_bool(q.spill, [&](auto sp) {
            launch(ctx, rayquery_forward_queue_kernel<decltype(sp)::value>, g.grid, g.block, q.lds_bytes, a, q.levels, q.threshold, g.tiles_x, g.tiles_total, q.early_exit);
        });
    } else {
        launch(ctx, rayquery_forward_kernel, dim3((a.width + 15) / 16, (a.height + 15) / 16), dim3(kTraceBlock), 0, a);
    }
    ctx->time_end(kKernelRayqueryForward);
    if (const int rc = ray_stats_end(ctx, a.stats != nullptr, "rayquery forward kernel launch failed")) return rc;
    ctx->raytraced_pixels = uint64_t(a.width) * a.height;      // ray statistics: one primary ray per pixel + one query per primary hit
    return VHR_OK;
}

// ---------------------------------------------------------------------------------------------
// Stand-in for the forward raster path's "Forward Pass" (forward_raster_render_path.cpp:52-96, forward_raster_render_path/default.vert
// + default.frag) with its multisampled attachments (render_graph.cpp:341, :399-423, :810-830, :921-945).  A ray caster, not a rasteriser:
// S = 8 sample rays per pixel (1 without MSAA), each the G-buffer stand-in's camera ray through the sample's point on the near plane (tmin 1).
// The visible triangle of a sample is its closest hit (ties: the smaller flat index) among the triangles whose FRAGMENT at this pixel is
// not discarded -- default.frag's alpha test on the attributes at the pixel centre (no sample shading, no `centroid`: the centre ray
// against the triangle's plane, extrapolated outside it), rejected inside the walk like the ALPHA walkers' candidates, so the answer is
// exact at any depth complexity.  Each distinct visible triangle of a pixel is shaded once, at the pixel centre, and its colour goes to
// every sample it covers; then the resolve.  Everything is in framebuffer rows (the pass contains RENDER_OUTPUT, so its viewport is
// flipped, pipeline.cpp:174-178): framebuffer row fy is row H - 1 - fy of the G-buffer stand-in's ray parameterisation.
// ---------------------------------------------------------------------------------------------
struct ForwardRasterArgs {
    DeviceScene scene;
    vhr_per_frame_data pfd;
    float projview[16];      // camera_proj * camera_view (the depth, as gbuffer_kernel computes it)
    uint32_t *out;           // RENDER_OUTPUT, resolved: B8G8R8A8_SRGB texels (bytes b g r a), one per pixel
    float *depth;            // "Depth", D32_SFLOAT, S per pixel
    uint32_t *msaa;          // "Forward Pass_MSAA": S = 8 texels per pixel (nullptr when S = 1)
    uint32_t *hits;          // probes, nullptr = not asked for: vhr_ray_hit (6 words) per sample
    uint8_t *fragments;      // fragments shaded per pixel
    uint32_t width, height;
    RayStats *stats;         // nullptr = off; counts stack overflows
};

// Vulkan's standard 8-sample locations: pixel units from the pixel's top-left corner, y down in framebuffer rows
__constant__ float c_msaa8_x[8] = { 0.5625f, 0.4375f, 0.8125f, 0.3125f, 0.1875f, 0.0625f, 0.6875f, 0.9375f };
__constant__ float c_msaa8_y[8] = { 0.3125f, 0.6875f, 0.5625f, 0.1875f, 0.8125f, 0.4375f, 0.9375f, 0.0625f };

// the camera ray of sample s of framebuffer pixel (x, fy): the G-buffer stand-in's ray (rayquery_primary_dir) through the sample's point.
// The sample's y offset sy runs down the framebuffer, so in the stand-in's (upward) parameterisation it is 1 - sy above row H - 1 - fy.
// S = 1: the pixel centre -- exactly rayquery_primary_dir(x, H - 1 - fy).
template <uint32_t S>
__device__ __forceinline__ f3 forward_sample_dir(const vhr_per_frame_data &pfd, f3 cam, uint32_t x, uint32_t fy, uint32_t s, uint32_t W, uint32_t H) {
    const float sx = S == 1 ? 0.5f : c_msaa8_x[s], sy = S == 1 ? 0.5f : c_msaa8_y[s];
    const float u = (float(x) + sx) / float(W), v = (float(H - 1u - fy) + (1.0f - sy)) / float(H);
    return get_world_space_position(pfd, 1.0f, u, v) - cam;
}

// the barycentrics of the point where the ray (o, d) meets the triangle's PLANE: Moeller-Trumbore's u and v without its bounds (a pixel
// centre outside the triangle extrapolates the attributes, as a rasteriser does); a ray parallel to the plane gets (0, 0)
__device__ __forceinline__ void plane_barycentrics(const DeviceScene &sc, uint32_t tri_index, f3 o, f3 d, float &u, float &v) {
    const float4 *tp = reinterpret_cast<const float4 *>(sc.tris + tri_index);
    const float4 ta = tp[0], tb = tp[1], tc = tp[2];
    const f3 v0 = f3{ ta.x, ta.y, ta.z }, e1 = f3{ ta.w, tb.x, tb.y }, e2 = f3{ tb.z, tb.w, tc.x };
    const f3 pvec = cross3(d, e2);
    const float det = dot3(e1, pvec);
    u = 0.0f; v = 0.0f;
    if (det == 0.0f) return;
    const float inv = 1.0f / det;
    const f3 tvec = o - v0;
    u = dot3(tvec, pvec) * inv;
    v = dot3(d, cross3(tvec, e1)) * inv;
}

// default.frag:19-27: the fragment of triangle tri_index at the pixel whose centre ray is (cam, cdir) is discarded
__device__ bool forward_discarded(const DeviceScene &sc, uint32_t tri_index, f3 cam, f3 cdir) {
    const BvhTri &bt = sc.tris[tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];
    if (prim.material.alpha_mask != 1) return false;
    if (prim.material.base_color_texture == -1) return prim.material.base_color[3] < prim.material.alpha_cutoff;   // :21-22
    float u, v;
    plane_barycentrics(sc, tri_index, cam, cdir, u, v);
    const TriAttributes at = interpolate(sc, prim, bt.tri, u, v);
    return sample_texture(sc, prim.material.base_color_texture, at.uvx, at.uvy).w < prim.material.alpha_cutoff;   // :24-27
}

// default.frag:19-53 for the fragment of triangle tri_index at the pixel whose centre ray is (cam, cdir): the texel through the sRGB
// attachment (B8G8R8A8_SRGB, bytes b g r a, alpha 1).  in_normal is object space and not renormalised (as in the rayquery path); the
// shadow-map term is overwritten with 1.0 (:47), so in_pos and the shadow map are unused.
__device__ uint32_t forward_raster_fragment(const DeviceScene &sc, const vhr_per_frame_data &pfd, uint32_t tri_index, f3 cam, f3 cdir) {
    float u, v;
    plane_barycentrics(sc, tri_index, cam, cdir, u, v);
    const BvhTri &bt = sc.tris[tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];
    const TriAttributes at = interpolate(sc, prim, bt.tri, u, v);
    f3 albedo;
    if (prim.material.base_color_texture == -1) {                                        // :21-26
        albedo = f3{ prim.material.base_color[0], prim.material.base_color[1], prim.material.base_color[2] };
    } else {
        const f4 t = sample_texture(sc, prim.material.base_color_texture, at.uvx, at.uvy);
        albedo = f3{ t.x, t.y, t.z };
    }
    const f3 normal = at.normal;
    f3 N = normal;                                                                       // :31-37
    if (prim.material.normal_map >= 0) {
        const f4 tg = interpolate_tangent(sc, prim, bt.tri, u, v);
        const f3 T = f3{ tg.x, tg.y, tg.z };
        const f4 tx = sample_texture(sc, prim.material.normal_map, at.uvx, at.uvy);
        const f3 tsn = normalize3(f3{ tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f });
        const f3 bitangent = cross3(tsn, T) * tg.w;                                      // sic
        const f3 tangent = normalize3(T - normal * dot3(T, normal));
        N = (tangent * tsn.x + bitangent * tsn.y) + normal * tsn.z;
    }
    const f3 light_dir = -f3{ pfd.directional_light.direction[0], pfd.directional_light.direction[1], pfd.directional_light.direction[2] };
    const f3 lc = f3{ pfd.directional_light.color[0], pfd.directional_light.color[1], pfd.directional_light.color[2] };
    const f3 c = albedo * VHR_PI_INVERSE + mul3(albedo * fmaxf(dot3(N, light_dir), 0.0f), lc);     // :49-51 (shadow = 1.0)
    return uint32_t(srgb8(c.z)) | (uint32_t(srgb8(c.y)) << 8) | (uint32_t(srgb8(c.x)) << 16) | (255u << 24);
}

// the resolve of an 8-sample texel: per channel the fp32 mean of the decoded samples, summed in sample order (colour from sRGB, alpha as
// UNORM), encoded as every sRGB store here (srgb8) and alpha as UNORM -- the library's definition (Vulkan leaves an sRGB resolve's
// arithmetic to the implementation)
__device__ __forceinline__ void resolve_add(float (&acc)[4], uint32_t texel) {
    acc[0] += c_srgb_lut[texel & 255u]; acc[1] += c_srgb_lut[(texel >> 8) & 255u]; acc[2] += c_srgb_lut[(texel >> 16) & 255u];
    acc[3] += float(texel >> 24) / 255.0f;
}
__device__ __forceinline__ uint32_t resolve_texel(const float (&acc)[4]) {
    return uint32_t(srgb8(acc[0] * 0.125f)) | (uint32_t(srgb8(acc[1] * 0.125f)) << 8) | (uint32_t(srgb8(acc[2] * 0.125f)) << 16) |
           (unorm8(acc[3] * 0.125f) << 24);
}

// reverse-Z clip.z / clip.w of the sample's hit (gbuffer_kernel's depth)
__device__ __forceinline__ float forward_depth(const ForwardRasterArgs &a, f3 cam, f3 dir, float t) {
    const f3 P = cam + dir * t;
    const f4 clip = mat4_mul(a.projview, f4{ P.x, P.y, P.z, 1.0f });
    return clip.z / clip.w;
}

// the sample_hits probe of one sample (vhr_ray_hit; zeros and kNoHit for a miss)
__device__ __forceinline__ void forward_store_hit(const ForwardRasterArgs &a, const size_t i, const bool hit, const uint32_t tri, const float t,
                                                  const float u, const float v) {
    uint32_t *const r = a.hits + i * 6u;
    r[0] = hit ? __float_as_uint(t) : 0u; r[1] = hit ? __float_as_uint(u) : 0u; r[2] = hit ? __float_as_uint(v) : 0u;
    r[3] = hit ? a.scene.tris[tri].prim : kNoHit; r[4] = hit ? a.scene.tris[tri].tri : kNoHit; r[5] = 0u;
}

// Literal form (`variant_standin_forward_raster` 0): one pixel per thread, its S sample rays one after the other through traverse<> with the
// discard as the candidate filter, then the fragments and the resolve -- the definition of the bits.
template <uint32_t S>
__global__ __launch_bounds__(kTraceBlock) void forward_raster_kernel(const ForwardRasterArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_fr_stack[kTraceStack * kTraceBlock];
    int *stack = s_fr_stack + threadIdx.x;
    uint32_t x, fy;
    pixel_of_thread(x, fy, 0);
    uint32_t overflow = 0;
    if (x < a.width && fy < a.height) {
        const uint32_t W = a.width, H = a.height;
        const size_t pix = size_t(fy) * W + x;
        const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
        const f3 cdir = forward_sample_dir<1>(a.pfd, cam, x, fy, 0, W, H);
        const DeviceScene *sc = &a.scene;
        const auto discarded = [sc, cam, cdir](uint32_t, uint32_t tri, float, float) { return forward_discarded(*sc, tri, cam, cdir); };
        uint32_t tris[S], texels[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            const f3 dir = forward_sample_dir<S>(a.pfd, cam, x, fy, s, W, H);
            Hit h;
            h.t = h.u = h.v = 0.0f; h.tri_index = 0; h.flat = 0;
            const bool hit = traverse<false, kTraceBlock>(a.scene, cam, dir, 1.0f, 3.0e38f, stack, h, overflow, discarded);
            tris[s] = hit ? h.tri_index : kNoHit;
            a.depth[pix * S + s] = hit ? forward_depth(a, cam, dir, h.t) : 0.0f;
            if (a.hits) forward_store_hit(a, pix * S + s, hit, h.tri_index, h.t, h.u, h.v);
        }
        uint32_t nfrag = 0;
        float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            uint32_t texel = 0u;                                                         // the clear (0, 0, 0, 0)
            if (tris[s] != kNoHit) {
                uint32_t owner = s;                                                      // the first sample of the same triangle
#pragma unroll
                for (uint32_t q = 0; q < s; ++q)
                    if (owner == s && tris[q] == tris[s]) owner = q;
                if (owner == s) { texels[s] = forward_raster_fragment(a.scene, a.pfd, tris[s], cam, cdir); ++nfrag; }
                texel = texels[owner];
            }
            texels[s] = texel;
            if (S == 1) a.out[pix] = texel;
            else { a.msaa[pix * S + s] = texel; resolve_add(acc, texel); }
        }
        if (S > 1) a.out[pix] = resolve_texel(acc);
        if (a.fragments) a.fragments[pix] = uint8_t(nfrag);
    }
    if (a.stats) {
        const unsigned long long ovf = __ballot(overflow != 0);
        if ((threadIdx.x & 63u) == 0 && ovf) atomicAdd(&a.stats->stack_overflows, (unsigned long long)__popcll(ovf));
    }
}

// Work-queue form (default, `variant_standin_forward_raster` 1), rayquery_forward_queue_kernel's schedule: a wave owns a 16x8-pixel tile, makes the
// tile's shared descent once and drains the tile's S x 128 sample rays as one queue (closest hit, PER_RAY for the depth's t, the discard
// as the walk's candidate filter).  The cut is built around the rays' common origin, the camera, and culls nothing by direction, so a
// sample ray that leaves the tile's pixel-centre frustum (up to 1/16 pixel beyond the tile border) finds every subtree it hits.  Then,
// with the whole wave: the S hits of each pixel are grouped in LDS and de-duplicated into fragments, every (pixel, triangle) fragment is
// shaded once, and the _MSAA texels, the Depth samples and the resolved texel are stored.  Decision (vi) is decided inline (!DEFER), the
// same test as traverse<>: the bits are forward_raster_kernel's.
template <uint32_t S, bool SPILL>
__global__ __launch_bounds__(kQueueBlock * 2) __attribute__((amdgpu_waves_per_eu(3, 6))) void forward_raster_queue_kernel(
    const ForwardRasterArgs a, const uint32_t stack_levels, const uint32_t refill_threshold, const uint32_t tiles_x, const uint32_t tiles_total,
    const uint32_t early_exit, const Stamps st) {
    vhr_stamp(st);
    constexpr uint32_t R = S * 128u;                     // sample rays of a tile; slot p * S + s = sample s of pixel slot p
    extern __shared__ int s_dyn[];                       // per wave: (stack_levels + 3) x 64 ints
    __shared__ uint32_t s_tri_all[2][R];                 // per slot: the visible triangle (kNoHit: none) -> at a fragment's slot, its texel
    __shared__ uint32_t s_t_all[2][R];                   // per slot: t -> the owner (the first sample of the same triangle; kNoHit: none)
    __shared__ float s_cdir_all[2][3][128];              // per pixel slot: the centre ray's direction
    __shared__ uint16_t s_frag_all[2][R];                // the tile's fragments: the slot of their first sample
    __shared__ uint8_t s_list_all[2][128];
    __shared__ float4 s_cut_all[2][kCutMax][2];
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    const uint32_t tile = blockIdx.x * 2u + wave;
    if (tile >= tiles_total) return;                     // waves of a block share nothing and never synchronise
    uint32_t (&s_tri)[R] = s_tri_all[wave];
    uint32_t (&s_t)[R] = s_t_all[wave];
    float (&s_cdir)[3][128] = s_cdir_all[wave];
    uint16_t (&s_frag)[R] = s_frag_all[wave];
    uint8_t (&s_list)[128] = s_list_all[wave];
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    const uint32_t W = a.width, H = a.height;
    const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
    auto px_of = [&](uint32_t p) { return tile_x * 16u + (p >> 6) * 8u + (p & 7u); };
    auto fy_of = [&](uint32_t p) { return tile_y * 8u + ((p & 63u) >> 3); };

    // ---- the tile's pixels: centre directions, compacted list ----
    unsigned long long in_mask[2];
    uint32_t npix = 0;
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        const uint32_t p = sub * 64u + lane, x = px_of(p), fy = fy_of(p);
        const bool in_range = x < W && fy < H;
        if (in_range) {
            const f3 c = forward_sample_dir<1>(a.pfd, cam, x, fy, 0, W, H);
            s_cdir[0][p] = c.x; s_cdir[1][p] = c.y; s_cdir[2][p] = c.z;
        }
        const unsigned long long m = __ballot(in_range);
        in_mask[sub] = m;
        if (in_range) s_list[npix + lane_rank(m)] = uint8_t(p);
        npix += uint32_t(__popcll(m));
    }
    wave_lds_sync();
    const bool traced = a.scene.node_count != 0;
    uint32_t overflow = 0;
    const uint32_t total = traced ? npix * S : 0u;
    // ---- the sample rays: closest hit among the candidates whose fragment is not discarded ----
    const uint32_t cut_n = total ? build_tile_cut_uniform(a.scene, cam, cam, s_cut_all[wave], lane) : 0u;
    const DeviceScene *sc = &a.scene;
    const auto discarded = [sc, cam, &s_cdir](uint32_t slot, uint32_t tri, float, float) {
        const uint32_t p = slot / S;
        return forward_discarded(*sc, tri, cam, f3{ s_cdir[0][p], s_cdir[1][p], s_cdir[2][p] });
    };
    wave_queue_walk<SPILL, false, false, true>(
        a.scene, stack, stack_levels, lane, total, refill_threshold, early_exit, 0.0f, 0.0f, false, overflow, s_cut_all[wave], cut_n,
        [&](uint32_t r, uint32_t &slot, f3 &ro, f3 &rd, float &tmin, float &tmax) {
            const uint32_t p = s_list[r / S], s = r % S;
            slot = p * S + s;
            ro = cam;
            rd = forward_sample_dir<S>(a.pfd, cam, px_of(p), fy_of(p), s, W, H);
            tmin = 1.0f; tmax = 3.0e38f;
        },
        [&](uint32_t slot, uint32_t tri, float u, float v, float t) {
            s_tri[slot] = tri; s_t[slot] = __float_as_uint(t);
            if (a.hits) {
                const uint32_t p = slot / S;
                forward_store_hit(a, (size_t(fy_of(p)) * W + px_of(p)) * S + slot % S, tri != kNoHit, tri, t, u, v);
            }
        },
        nullptr, NoFlag{}, discarded);
    wave_lds_sync();
    // ---- per pixel: the Depth samples, each sample's owner, the fragment list ----
    uint32_t nfrag = 0;
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        const uint32_t p = sub * 64u + lane, x = px_of(p), fy = fy_of(p);
        const bool inside = (in_mask[sub] >> lane) & 1ull;
        const size_t pix = size_t(fy) * W + x;
        uint32_t tris[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            tris[s] = inside && traced ? s_tri[p * S + s] : kNoHit;
            if (inside) {
                const bool hit = tris[s] != kNoHit;
                a.depth[pix * S + s] = hit ? forward_depth(a, cam, forward_sample_dir<S>(a.pfd, cam, x, fy, s, W, H), __uint_as_float(s_t[p * S + s])) : 0.0f;
                if (!traced && a.hits) forward_store_hit(a, pix * S + s, false, 0u, 0.0f, 0.0f, 0.0f);      // (no walk, no commit: the misses)
            }
        }
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            uint32_t owner = tris[s] != kNoHit ? s : kNoHit;
#pragma unroll
            for (uint32_t q = 0; q < s; ++q)
                if (owner == s && tris[q] == tris[s]) owner = q;
            if (inside) s_t[p * S + s] = owner;
            const bool first = owner == s;
            const unsigned long long m = __ballot(first);
            if (first) s_frag[nfrag + lane_rank(m)] = uint16_t(p * S + s);
            nfrag += uint32_t(__popcll(m));
        }
    }
    wave_lds_sync();
    // ---- default.frag once per fragment, whole wave: the texel replaces the triangle at the fragment's slot ----
    for (uint32_t f = lane; f < nfrag; f += 64u) {
        const uint32_t slot = s_frag[f], p = slot / S;
        s_tri[slot] = forward_raster_fragment(a.scene, a.pfd, s_tri[slot], cam, f3{ s_cdir[0][p], s_cdir[1][p], s_cdir[2][p] });
    }
    wave_lds_sync();
    // ---- the stores: _MSAA samples, the resolved texel, the fragment count ----
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        if (!((in_mask[sub] >> lane) & 1ull)) continue;
        const uint32_t p = sub * 64u + lane;
        const size_t pix = size_t(fy_of(p)) * W + px_of(p);
        uint32_t count = 0;
        float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t owner = s_t[p * S + s];
            const uint32_t texel = owner == kNoHit ? 0u : s_tri[p * S + owner];
            count += owner == s ? 1u : 0u;
            if (S == 1) a.out[pix] = texel;
            else { a.msaa[pix * S + s] = texel; resolve_add(acc, texel); }
        }
        if (S > 1) a.out[pix] = resolve_texel(acc);
        if (a.fragments) a.fragments[pix] = uint8_t(count);
    }
    if (a.stats && lane == 0 && overflow) atomicAdd(&a.stats->stack_overflows, 1ull);
}

int launch_forward_raster(vhr_context *ctx, const vhr_per_frame_data &pfd, Image &out, Image &depth, Image *msaa, void *sample_hits, uint8_t *fragments) {
    const uint32_t S = depth.samples;
    if (out.width != depth.width || out.height != depth.height) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: image extents differ");
    if (out.bpp != 4 || out.samples != 1)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: the output storage image must have 4-byte texels (B8G8R8A8_SRGB)");
    if (depth.format != VHR_FORMAT_D32_SFLOAT) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: \"Depth\" must be D32_SFLOAT (forward_raster_render_path.cpp:58)");
    if (S != 1 && S != kMsaaSamples) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: \"Depth\" must have 1 or 8 samples");
    if ((S == kMsaaSamples) != (msaa != nullptr)) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: msaa_image goes with an 8-sample \"Depth\"");
    if (msaa && (msaa->width != depth.width || msaa->height != depth.height || msaa->bpp != 4 || msaa->samples != kMsaaSamples))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: msaa_image must be B8G8R8A8 with 8 samples at Depth's extent");
    if (reinterpret_cast<uintptr_t>(sample_hits) % 4u) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: sample_hits must be 4-byte aligned");
    ForwardRasterArgs a;
    a.scene = ctx->device_scene();
    a.pfd = pfd;
    host_mat4_mul(pfd.camera_proj, pfd.camera_view, a.projview);
    a.out = static_cast<uint32_t *>(out.ptr);
    a.depth = static_cast<float *>(depth.ptr);
    a.msaa = msaa ? static_cast<uint32_t *>(msaa->ptr) : nullptr;
    a.hits = static_cast<uint32_t *>(sample_hits);
    a.fragments = fragments;
    a.width = depth.width;
    a.height = depth.height;
    a.stats = ctx->ray_stats_enabled ? ctx->d_ray_stats : nullptr;
    if (a.width == 0 || a.height == 0) return VHR_OK;
    if (const int rc = ray_stats_begin(ctx, a.stats != nullptr)) return rc;
    ctx->time_begin(kKernelForwardRaster);
    with_bool(S == 1, [&](auto one) {
        constexpr uint32_t SAMPLES = decltype(one)::value ? 1u : 8u;
        if (ctx->options[kOptForwardRasterVariant] == 0) {
            launch(ctx, forward_raster_kernel<SAMPLES>, dim3((a.width + 15) / 16, (a.height + 15) / 16), dim3(kTraceBlock), 0, a);
            return;
        }
        const QueueLaunch q = queue_launch(ctx, kOptLdsStackLevels, kOptEarlyExit, 2u);
        const TileGrid g = tile_grid(a.width, a.height, 16u);
        with_bool(q.spill, [&](auto sp) {
            launch(ctx, forward_raster_queue_kernel<SAMPLES, decltype(sp)::value>, g.grid, g.block, q.lds_bytes, a, q.levels, q.threshold, g.tiles_x, g.tiles_total, q.early_exit);
        });
    });
    ctx->time_end(kKernelForwardRaster);
    if (const int rc = ray_stats_end(ctx, a.stats != nullptr, "forward raster kernel launch failed")) return rc;
    ctx->raytraced_pixels = uint64_t(a.width) * a.height * S;      // ray statistics: S primary rays per pixel, nothing else
    return VHR_OK;
}

}  // namespace vhr
