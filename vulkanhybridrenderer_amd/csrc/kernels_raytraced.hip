// The raytraced render path: its "Raytracing Pass" and its composition.  (Split from kernels_trace.hip, where it followed the hybrid path's
// launches; built with the same flags.)
//
// ---------------------------------------------------------------------------------------------
// next row f4: the raytraced render path's "Raytracing Pass" (raytraced_render_path.cpp:11-47)
//   raytraced_render_path/raygen.rgen:10-23 (+ miss.rmiss:6-8, shadow_miss.rmiss:6-8, closesthit.rchit:10-58), or with the
//   alpha test for shadows switched on raygen_test_alpha.rgen:10-23 + closesthit_test_alpha.rchit:10-51 +
//   shadow_anyhit.rahit:8-27.  One pixel per lane, 8x8 pixels per wave: the primary rays of a tile and the shadow rays
//   towards the directional light are both coherent, so the per-lane walk keeps most lanes on the same nodes.
// ---------------------------------------------------------------------------------------------
#define VHR_TRACE_UNIT unit_raytraced      // this unit's copy of the sRGB decode table (trace_device.hpp)
#include "trace_queue.hpp"

namespace vhr {

// closesthit.rchit:26-57 (ALPHA: closesthit_test_alpha.rchit:26-50) once the shadow ray's answer is known
template <bool ALPHA>
__device__ f4 raytraced_hit_payload(const DeviceScene &sc, const vhr_per_frame_data &pfd, const Hit &h, bool shadowed) {
    const BvhTri &bt = sc.tris[h.tri_index];                                             // rchit:11-24
    const vhr_primitive &prim = sc.primitives[bt.prim];
    const TriAttributes at = interpolate(sc, prim, bt.tri, h.u, h.v);
    f3 albedo;
    if (!ALPHA && prim.material.base_color_texture == -1) {                              // rchit:26-32 (alpha variant: :26, unconditional)
        albedo = f3{ prim.material.base_color[0], prim.material.base_color[1], prim.material.base_color[2] };
    } else {
        const f4 t = sample_texture(sc, prim.material.base_color_texture, at.uvx, at.uvy);
        albedo = f3{ t.x, t.y, t.z };
    }
    const f3 normal = at.normal;
    f3 N = normal;                                                                       // rchit:34-41
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
    const f3 li = f3{ pfd.directional_light.intensity[0], pfd.directional_light.intensity[1], pfd.directional_light.intensity[2] };
    const f3 albedo_lighting = ALPHA ? albedo * 0.2f : albedo * VHR_PI_INVERSE;          // alpha :39 / :46
    f3 col = albedo_lighting;
    if (!shadowed) {                                                                     // rchit:52-54 / alpha :45-47
        const float nl = fmaxf(dot3(N, light_dir), 0.0f);
        f3 lit = albedo * nl;
        if (!ALPHA) lit = mul3(lit, li);                                                 // the alpha variant drops light_intensity
        lit = mul3(lit, lc);
        col = albedo_lighting + lit;
    }
    return f4{ col.x, col.y, col.z, 1.0f };
}

// the walks' candidate filter: gl_RayFlagsNoOpaqueEXT runs shadow_anyhit.rahit at every candidate (ALPHA), else none
template <bool ALPHA> __device__ __forceinline__ auto rahit_filter(const DeviceScene &sc) {
    if constexpr (ALPHA) return RahitAlpha{ &sc }; else return NoFilter{};
}

struct RaytracedArgs {
    DeviceScene scene;
    vhr_per_frame_data pfd;
    uchar4 *out;             // "RaytracedOutput", B8G8R8A8_UNORM
    uint32_t width, height;
    uint32_t row_begin, row_end;
    RayStats *stats;         // nullptr = off; covered_pixels counts the primary hits (= shadow rays)
    CostOrderArgs co;        // "raygen_cost_order" (the queue kernel)
};

// raytraced_render_path/raygen.rgen:10-23 for one pixel
template <bool ALPHA>
__device__ __forceinline__ void raytraced_pixel(const RaytracedArgs &a, const uint32_t x, const uint32_t y, int *stack, uint32_t &overflow, bool &hit_any) {
    const uint32_t W = a.width, H = a.height;
    const float ux = ((float(x) + 0.5f) / float(W)) * 2.0f - 1.0f;                   // rgen:11-13
    const float uy = ((float(y) + 0.5f) / float(H)) * 2.0f - 1.0f;
    const f4 origin = mat4_mul(a.pfd.camera_view_inverse, f4{ 0.0f, 0.0f, 0.0f, 1.0f });       // rgen:15
    const f4 target = mat4_mul(a.pfd.camera_proj_inverse, f4{ ux, uy, 1.0f, 1.0f });           // rgen:16
    const f3 tn = normalize3(f3{ target.x, target.y, target.z });
    const f4 direction = mat4_mul(a.pfd.camera_view_inverse, f4{ tn.x, tn.y, tn.z, 0.0f });    // rgen:17
    f4 payload = f4{ 0.3f, 0.8f, 0.2f, 1.0f };                                       // miss.rmiss:7
    Hit h;
    if (traverse<false>(a.scene, f3{ origin.x, origin.y, origin.z }, f3{ direction.x, direction.y, direction.z }, 0.1f, 10000.0f,
                        stack, h, overflow, rahit_filter<ALPHA>(a.scene))) {         // rgen:20
        hit_any = true;
        f3 position, unused_normal;
        hit_position_normal(a.scene, h, position, unused_normal);                    // rchit:24
        const f3 light_dir = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1], a.pfd.directional_light.direction[2] };
        Hit sh;
        // shadow ray, rchit:48-50 (alpha :41-43): shadow_payload stays true unless shadow_miss.rmiss:7 runs
        const bool shadowed = traverse<true>(a.scene, position, light_dir, 0.1f, 10000.0f, stack, sh, overflow, rahit_filter<ALPHA>(a.scene));
        payload = raytraced_hit_payload<ALPHA>(a.scene, a.pfd, h, shadowed);
    }
    a.out[size_t(y) * W + x] = make_uchar4(uint8_t(unorm8(payload.z)), uint8_t(unorm8(payload.y)), uint8_t(unorm8(payload.x)),
                                           uint8_t(unorm8(payload.w)));             // rgen:22 imageStore, B8G8R8A8
}

template <bool ALPHA>
__global__ __launch_bounds__(kTraceBlock) void raytraced_kernel(const RaytracedArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_rt_stack[kTraceStack * kTraceBlock];
    int *stack = s_rt_stack + threadIdx.x;
    uint32_t x, y;
    pixel_of_thread(x, y, a.row_begin);
    bool hit_any = false;
    uint32_t overflow = 0;
    if (x < a.width && y < a.row_end) raytraced_pixel<ALPHA>(a, x, y, stack, overflow, hit_any);
    if (a.stats) {
        const unsigned long long cov = __ballot(hit_any), ovf = __ballot(overflow != 0);
        if ((threadIdx.x & 63u) == 0) {
            if (cov) atomicAdd(&a.stats->covered_pixels, (unsigned long long)__popcll(cov));
            if (ovf) atomicAdd(&a.stats->stack_overflows, (unsigned long long)__popcll(ovf));
        }
    }
}

// Work-queue form (default, `raytraced_variant` 1): a wave owns a 16x8-pixel tile and runs wave_queue_walk twice -- the
// primary rays (closest hit), then one shadow ray per primary hit towards the light (any hit) -- with the ray setup, the
// shadow-ray origins (rchit:24) and closesthit.rchit's shading done by the whole wave in between and after.  Same rays, same
// intersection arithmetic, same shader as raytraced_kernel: bit-identical output.
template <bool SPILL, bool ALPHA>
__global__ __launch_bounds__(kQueueBlock * 2) __attribute__((amdgpu_waves_per_eu(5, 6))) void raytraced_queue_kernel(
    const RaytracedArgs a, const uint32_t stack_levels, const uint32_t refill_threshold, const uint32_t tiles_x, const uint32_t tiles_total,
    const uint32_t early_exit, const Stamps st) {
    vhr_stamp(st);
    extern __shared__ int s_dyn[];                        // per wave: (stack_levels + 3) x 64 ints
    // rows 0-2: primary direction -> primary hit record (triangle, u, v); rows 3-5: shadow-ray origin -> row 3 = its answer
    __shared__ float s_ray_all[2][6][kReflRays];
    __shared__ uint8_t s_list_all[2][kReflRays];
    __shared__ float4 s_cut_all[2][kCutMax][2];           // the tile's shared descent (build_tile_cut), once per walk
    const uint32_t lane = threadIdx.x & 63u, wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    // "raygen_cost_order" for this launch (see raygen_queue_kernel): the first block sorts the previous launch's blocks before its own tiles
    const unsigned long long t_cost0 = a.co.wave_cost ? __builtin_readcyclecounter() : 0ull;
    if (a.co.order_out && blockIdx.x == 0u) order_blocks_by_cost<2>(a.co.cost_prev, a.co.order_blocks, a.co.order_out, reinterpret_cast<uint32_t *>(s_dyn));
    const uint32_t tile = (a.co.block_order ? a.co.block_order[blockIdx.x] : blockIdx.x) * 2u + wave;
    if (tile >= tiles_total) return;                      // waves of a block share nothing and never synchronise
    float (&s_ray)[6][kReflRays] = s_ray_all[wave];
    uint8_t (&s_list)[kReflRays] = s_list_all[wave];
    int *stack = s_dyn + wave * (stack_levels + 3u) * kQueueBlock + lane;
    stack[0] = kStackSentinel;
    const uint32_t W = a.width, H = a.height;
    const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const f4 origin4 = mat4_mul(a.pfd.camera_view_inverse, f4{ 0.0f, 0.0f, 0.0f, 1.0f });           // rgen:15
    const f3 origin = f3{ origin4.x, origin4.y, origin4.z };
    const f3 light_dir = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1], a.pfd.directional_light.direction[2] };

    // ---- primary rays, whole wave (rgen:11-17) ----
    unsigned long long in_mask[2];
    uint32_t total = 0;
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        const uint32_t x = tile_x * 16u + sub * 8u + (lane & 7u), y = a.row_begin + tile_y * 8u + (lane >> 3);
        const bool in_range = x < W && y < a.row_end;
        const uint32_t p = sub * 64u + lane;
        if (in_range) {
            const float ux = ((float(x) + 0.5f) / float(W)) * 2.0f - 1.0f;
            const float uy = ((float(y) + 0.5f) / float(H)) * 2.0f - 1.0f;
            const f4 target = mat4_mul(a.pfd.camera_proj_inverse, f4{ ux, uy, 1.0f, 1.0f });
            const f3 tn = normalize3(f3{ target.x, target.y, target.z });
            const f4 direction = mat4_mul(a.pfd.camera_view_inverse, f4{ tn.x, tn.y, tn.z, 0.0f });
            s_ray[0][p] = direction.x; s_ray[1][p] = direction.y; s_ray[2][p] = direction.z;
        }
        const unsigned long long m = __ballot(in_range);
        in_mask[sub] = m;
        if (in_range) s_list[total + lane_rank(m)] = uint8_t(p);
        total += uint32_t(__popcll(m));
    }
    wave_lds_sync();
    const bool traced = a.scene.node_count != 0;
    uint32_t overflow = 0;
    // ---- walk 1: closest hit of the primary rays (rgen:20; ALPHA: gl_RayFlagsNoOpaqueEXT -> the any-hit filter) ----
    // (one origin for every ray: the shared descent follows the boxes around the camera)
    uint32_t cut_n = traced && total ? build_tile_cut_uniform(a.scene, origin, origin, s_cut_all[wave], lane) : 0u;
    wave_queue_walk<SPILL, false>(
        a.scene, stack, stack_levels, lane, traced ? total : 0u, refill_threshold, early_exit, 0.1f, 10000.0f, false, overflow, s_cut_all[wave], cut_n,
        [&](uint32_t r, uint32_t &pix, f3 &ro, f3 &rd) {
            pix = s_list[r];
            ro = origin;
            rd = f3{ s_ray[0][pix], s_ray[1][pix], s_ray[2][pix] };
        },
        [&](uint32_t pix, uint32_t tri, float u, float v) {
            s_ray[0][pix] = __uint_as_float(tri); s_ray[1][pix] = u; s_ray[2][pix] = v;
        },
        nullptr, NoFlag{}, rahit_filter<ALPHA>(a.scene));
    wave_lds_sync();
    // ---- shadow rays from the primary hits, whole wave (rchit:24,48-50) ----
    uint32_t nhit = 0;
    f3 omin = f3{ 3.0e38f, 3.0e38f, 3.0e38f }, omax = f3{ -3.0e38f, -3.0e38f, -3.0e38f };   // bounds of the shadow rays' origins
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
            s_ray[3][p] = position.x; s_ray[4][p] = position.y; s_ray[5][p] = position.z;
            omin = f3{ fminf(omin.x, position.x), fminf(omin.y, position.y), fminf(omin.z, position.z) };
            omax = f3{ fmaxf(omax.x, position.x), fmaxf(omax.y, position.y), fmaxf(omax.z, position.z) };
        }
        const unsigned long long m = __ballot(hit);
        if (hit) s_list[nhit + lane_rank(m)] = uint8_t(p);
        nhit += uint32_t(__popcll(m));
    }
    wave_lds_sync();
    // ---- walk 2: any hit towards the light; the answer (an occluder's triangle or kNoHit) lands in row 3 ----
    cut_n = nhit ? build_tile_cut_uniform(a.scene, omin, omax, s_cut_all[wave], lane) : 0u;
    wave_queue_walk<SPILL, false>(
        a.scene, stack, stack_levels, lane, nhit, refill_threshold, early_exit, 0.1f, 10000.0f, true, overflow, s_cut_all[wave], cut_n,
        [&](uint32_t r, uint32_t &pix, f3 &ro, f3 &rd) {
            pix = s_list[r];
            ro = f3{ s_ray[3][pix], s_ray[4][pix], s_ray[5][pix] };
            rd = light_dir;
        },
        [&](uint32_t pix, uint32_t tri, float, float) { s_ray[3][pix] = __uint_as_float(tri); },
        nullptr, NoFlag{}, rahit_filter<ALPHA>(a.scene));
    wave_lds_sync();
    // ---- closesthit.rchit / miss.rmiss and the image store, whole wave ----
#pragma unroll
    for (uint32_t sub = 0; sub < 2; ++sub) {
        if (!((in_mask[sub] >> lane) & 1ull)) continue;
        const uint32_t x = tile_x * 16u + sub * 8u + (lane & 7u), y = a.row_begin + tile_y * 8u + (lane >> 3);
        const uint32_t p = sub * 64u + lane;
        f4 payload = f4{ 0.3f, 0.8f, 0.2f, 1.0f };                                       // miss.rmiss:7
        const uint32_t tri = traced ? __float_as_uint(s_ray[0][p]) : kNoHit;
        if (tri != kNoHit) {
            Hit h;
            h.t = 0.0f; h.u = s_ray[1][p]; h.v = s_ray[2][p]; h.tri_index = tri; h.flat = 0;
            payload = raytraced_hit_payload<ALPHA>(a.scene, a.pfd, h, __float_as_uint(s_ray[3][p]) != kNoHit);
        }
        a.out[size_t(y) * W + x] = make_uchar4(uint8_t(unorm8(payload.z)), uint8_t(unorm8(payload.y)), uint8_t(unorm8(payload.x)),
                                               uint8_t(unorm8(payload.w)));             // rgen:22 imageStore, B8G8R8A8
    }
    if (a.stats && lane == 0) {
        if (nhit) atomicAdd(&a.stats->covered_pixels, (unsigned long long)nhit);
        if (overflow) atomicAdd(&a.stats->stack_overflows, 1ull);
    }
    if (a.co.wave_cost && lane == 0) a.co.wave_cost[tile] = uint32_t(min(__builtin_readcyclecounter() - t_cost0, 0xffffffffull));
}

int launch_raytraced(vhr_context *ctx, const vhr_per_frame_data &pfd, uint32_t width, uint32_t height, Image &out, bool alpha_test) {
    if (width != out.width || height != out.height) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "TraceRays: launch size must equal the extent of RaytracedOutput");
    if (out.bpp != 4) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "TraceRays: RaytracedOutput must be B8G8R8A8_UNORM");
    RaytracedArgs a;
    a.scene = ctx->device_scene();
    a.pfd = pfd;
    a.out = static_cast<uchar4 *>(out.ptr);
    a.width = width;
    a.height = height;
    a.row_begin = std::min(ctx->row_begin, height);          // strips: per-pixel independent, owned rows only
    a.row_end = std::min(ctx->row_end, height);
    a.stats = ctx->ray_stats_enabled ? ctx->d_ray_stats : nullptr;
    if (a.row_end <= a.row_begin) return VHR_OK;
    if (const int rc = ray_stats_begin(ctx, a.stats != nullptr)) return rc;
    ctx->time_begin(kKernelRaygen);
    with_bool(alpha_test, [&](auto al) {
        constexpr bool AL = decltype(al)::value;
        if (ctx->options[kOptRaytracedVariant] == 0) {
            launch(ctx, raytraced_kernel<AL>, dim3((width + 15) / 16, (a.row_end - a.row_begin + 15) / 16), dim3(kTraceBlock), 0, a);
            return;
        }
        const QueueLaunch q = queue_launch(ctx, kOptLdsStackLevels, kOptEarlyExit, 2u);
        const TileGrid g = tile_grid(width, a.row_end - a.row_begin, 16u);
        a.co = CostOrderArgs{};
        if (q.levels >= 5u && !a.stats)                    // "raygen_cost_order" for this path's launch (its own lifetimes and orders)
            prepare_cost_order(ctx, ctx->cost_order_raytraced, (g.tiles_total + 1u) / 2u, 2u,
                               (g.tiles_x * 2654435761u) ^ (g.tiles_total * 40503u) ^ (uint32_t(alpha_test) << 28) ^ (a.row_begin * 97u), a.co, { g.tiles_x, g.tiles_x, 1u, 16u, 8u, 0u, a.row_begin });
        with_bool(q.spill, [&](auto sp) {
            launch(ctx, raytraced_queue_kernel<decltype(sp)::value, AL>, g.grid, g.block, q.lds_bytes, a, q.levels, q.threshold, g.tiles_x, g.tiles_total, q.early_exit);
        });
    });
    ctx->time_end(kKernelRaygen);
    if (const int rc = ray_stats_end(ctx, a.stats != nullptr, "raytraced kernel launch failed")) return rc;
    ctx->raytraced_pixels = uint64_t(width) * (a.row_end - a.row_begin);
    return VHR_OK;
}

// raytraced_render_path/composition.vert:5-8 + composition.frag:11-13: "RaytracedOutput" sampled at the texel centre,
// written to the B8G8R8A8_SRGB swapchain through the flipped presentation viewport (pipeline.cpp:175-178).
__global__ __launch_bounds__(256) void raytraced_composition_kernel(const uchar4 *in, uchar4 *out, uint32_t W, uint32_t H, const Stamps st) {
    vhr_stamp(st);
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63u), j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || j >= H) return;
    const uchar4 p = in[size_t(H - 1 - j) * W + x];
    out[size_t(j) * W + x] = make_uchar4(srgb8(p.x * (1.0f / 255.0f)), srgb8(p.y * (1.0f / 255.0f)), srgb8(p.z * (1.0f / 255.0f)), p.w);
}

int launch_raytraced_composition(vhr_context *ctx, const Image &in, Image &out) {
    if (in.width != out.width || in.height != out.height) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "raytraced composition: image extents differ");
    if (in.bpp != 4 || out.bpp != 4) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "raytraced composition: 4-byte texels expected");
    launch(ctx, raytraced_composition_kernel, dim3((in.width + 63) / 64, (in.height + 3) / 4), dim3(256), 0,
                       static_cast<const uchar4 *>(in.ptr), static_cast<uchar4 *>(out.ptr), in.width, in.height);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "raytraced composition kernel launch failed");
    return VHR_OK;
}

}  // namespace vhr
