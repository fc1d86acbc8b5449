// The stand-ins for the hybrid render path's rasterised passes: the G-buffer producer (primary rays), the shadow map and the composition
// stage.  (Split from kernels_trace.hip, which held them between the raytraced path and the forward passes; built with the same flags.)
#define VHR_TRACE_UNIT unit_standin      // this unit's copy of the sRGB decode table (trace_device.hpp)
#include "trace_device.hpp"

namespace vhr {

// ---------------------------------------------------------------------------------------------
// stand-in G-buffer producer (gbuf.vert:19-28, gbuf.frag:17-59 encodings) -- primary rays
// ---------------------------------------------------------------------------------------------
struct GbufferArgs {
    DeviceScene scene;
    vhr_per_frame_data pfd;
    float projview[16], prev_projview[16];
    void *normals, *motion;
    float *depth;
    uchar4 *albedo;          // B8G8R8A8_UNORM, optional
    uint32_t width, height;
    const BvhTri *prev_tris; // "object_motion_vectors": every record's state before the last refit, slot for slot (the MOTION instantiation only)
};

constexpr int kGbufferMaxLayers = 32;      // discarded surfaces a primary ray may step through

// MOTION ("object_motion_vectors", launched only while the last refit's records differ from their previous ones): the visible point is affine in the
// hit's barycentrics, P = v0 + u e1 + v e2, so the record the slot held before the refit gives where that surface point was.  The reprojection
// goes through P + d with d = (pv0 - v0) + u (pe1 - e1) + v (pe2 - e2): the difference form is exactly 0 for a record that did not move, so
// its texel keeps the plain kernel's bits.  Nothing but motion.xy differs between the two instantiations.
template <bool MOTION>
__global__ __launch_bounds__(kTraceBlock) void gbuffer_kernel(const GbufferArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_stack[kTraceStack * kTraceBlock];
    int *stack = s_stack + threadIdx.x;
    uint32_t x, y;
    pixel_of_thread(x, y, 0);
    if (x >= a.width || y >= a.height) return;
    const uint32_t W = a.width, H = a.height;
    const float u = (float(x) + 0.5f) / float(W), v = (float(y) + 0.5f) / float(H);
    const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
    const f3 pnear = get_world_space_position(a.pfd, 1.0f, u, v);      // reverse-Z: depth 1 is the near plane
    const f3 dir = pnear - cam;
    // Row f2: gbuf.frag:27-32 discards alpha-masked / fully transparent fragments, so the surface behind shows.  A
    // primary-ray caster gets the same picture by stepping past a discarded hit (tmin = its t) and casting again.
    Hit h;
    uint32_t overflow = 0;
    bool visible = false;
    float tmin = 1.0f;
    f4 al = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
    float uvx = 0.0f, uvy = 0.0f;
    for (int layer = 0; layer < kGbufferMaxLayers; ++layer) {
        if (!traverse<false>(a.scene, cam, dir, tmin, 3.0e38f, stack, h, overflow)) break;
        const BvhTri &bt = a.scene.tris[h.tri_index];
        const vhr_primitive &prim = a.scene.primitives[bt.prim];
        const TriAttributes at = interpolate(a.scene, prim, bt.tri, h.u, h.v);
        uvx = at.uvx; uvy = at.uvy;
        al = f4{ prim.material.base_color[0], prim.material.base_color[1], prim.material.base_color[2], prim.material.base_color[3] };
        if (prim.material.base_color_texture != -1) al = sample_texture(a.scene, prim.material.base_color_texture, uvx, uvy);   // :19-26
        if ((prim.material.alpha_mask == 1 && al.w < prim.material.alpha_cutoff) || al.w == 0.0f) { tmin = h.t; continue; }    // :27-32
        visible = true;
        break;
    }
    if (!visible) {                                                                          // clears: hybrid_render_path.cpp:16-19
        store_rgba16f(a.normals, W, x, y, 0.0f, 0.0f, 0.0f, 0.0f);
        store_rgba16f(a.motion, W, x, y, 0.0f, 0.0f, -1.0f, -1.0f);
        a.depth[size_t(y) * W + x] = 0.0f;
        if (a.albedo) a.albedo[size_t(y) * W + x] = make_uchar4(0, 0, 0, 0);
        return;
    }
    const BvhTri &bt = a.scene.tris[h.tri_index];
    const vhr_primitive &prim = a.scene.primitives[bt.prim];
    const f3 P = cam + dir * h.t;
    const f4 clip = mat4_mul(a.projview, f4{ P.x, P.y, P.z, 1.0f });
    a.depth[size_t(y) * W + x] = clip.z / clip.w;
    const TriAttributes at = interpolate(a.scene, prim, bt.tri, h.u, h.v);
    const float *M = a.scene.normal_matrices + 9 * size_t(bt.prim);
    const f3 n = at.normal;
    f3 N = n;
    if (prim.material.normal_map >= 0) {                                                     // gbuf.frag:35-41
        const f4 tx = sample_texture(a.scene, prim.material.normal_map, uvx, uvy);
        const f3 tsn = normalize3(f3{ tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f });
        const f4 tg = interpolate_tangent(a.scene, prim, bt.tri, h.u, h.v);
        const f3 T = f3{ tg.x, tg.y, tg.z };
        const f3 bitangent = cross3(tsn, T) * tg.w;                  // sic: cross(tangent_space_normal, in_tangent.xyz)
        const f3 tangent = normalize3(T - n * dot3(T, n));
        N = (tangent * tsn.x + bitangent * tsn.y) + n * tsn.z;
    }
    const f3 wn = normalize3(f3{ (M[0] * N.x + M[3] * N.y) + M[6] * N.z, (M[1] * N.x + M[4] * N.y) + M[7] * N.z,
                                 (M[2] * N.x + M[5] * N.y) + M[8] * N.z });                  // gbuf.frag:43
    store_rgba16f(a.normals, W, x, y, wn.x, wn.y, wn.z, float(bt.prim));
    const float cx = (float(x) + 0.5f) * a.pfd.display_size_inverse[0];                      // gbuf.frag:46
    const float cy = (float(y) + 0.5f) * a.pfd.display_size_inverse[1];
    f3 Pp = P;
    if constexpr (MOTION) {
        const float4 *c = reinterpret_cast<const float4 *>(a.scene.tris + h.tri_index), *p = reinterpret_cast<const float4 *>(a.prev_tris + h.tri_index);
        const float4 c0 = c[0], c1 = c[1], c2 = c[2], p0 = p[0], p1 = p[1], p2 = p[2];       // (v0.xyz, e1.x) (e1.yz, e2.xy) (e2.z, ...)
        const f3 d = f3{ (p0.x - c0.x) + h.u * (p0.w - c0.w) + h.v * (p1.z - c1.z), (p0.y - c0.y) + h.u * (p1.x - c1.x) + h.v * (p1.w - c1.w),
                         (p0.z - c0.z) + h.u * (p1.y - c1.y) + h.v * (p2.x - c2.x) };
        Pp = P + d;
    }
    const f4 rp = mat4_mul(a.prev_projview, f4{ Pp.x, Pp.y, Pp.z, 1.0f });
    const float px = (rp.x / rp.w) * 0.5f + 0.5f, py = (rp.y / rp.w) * 0.5f + 0.5f;          // gbuf.frag:47
    float metallic = prim.material.metallic_factor, roughness = prim.material.roughness_factor;
    if (prim.material.metallic_roughness_texture != -1) {                                    // gbuf.frag:50-56
        const f4 mr = sample_texture(a.scene, prim.material.metallic_roughness_texture, uvx, uvy);
        metallic *= mr.y;
        roughness *= mr.z;
    }
    store_rgba16f(a.motion, W, x, y, cx - px, cy - py, metallic, roughness);                 // gbuf.frag:58
    if (a.albedo)                                                                            // gbuf.frag:33
        a.albedo[size_t(y) * W + x] = make_uchar4(uint8_t(unorm8(al.z)), uint8_t(unorm8(al.y)), uint8_t(unorm8(al.x)), uint8_t(unorm8(al.w)));
}

int launch_standin_gbuffer(vhr_context *ctx, const vhr_per_frame_data &pfd, Image &normals, Image &motion, Image &depth, Image *albedo) {
    if (albedo && (albedo->width != depth.width || albedo->height != depth.height || albedo->bpp != 4))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_gbuffer: albedo image must be B8G8R8A8 of the same extent");
    if (normals.width != depth.width || normals.height != depth.height || motion.width != depth.width || motion.height != depth.height)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_gbuffer: image extents differ");
    GbufferArgs a;
    a.scene = ctx->device_scene();
    a.pfd = pfd;
    host_mat4_mul(pfd.camera_proj, pfd.camera_view, a.projview);
    host_mat4_mul(pfd.camera_proj_prev_frame, pfd.camera_view_prev_frame, a.prev_projview);
    a.normals = normals.ptr;
    a.motion = motion.ptr;
    a.depth = static_cast<float *>(depth.ptr);
    a.albedo = albedo ? static_cast<uchar4 *>(albedo->ptr) : nullptr;
    a.width = depth.width;
    a.height = depth.height;
    // the previous records matter only while some record differs from its previous one: else the plain kernel (the "alpha_test_rays" precedent)
    const bool object_motion = ctx->object_motion_vectors && ctx->d_prev_tris && ctx->motion_differing != 0;
    a.prev_tris = object_motion ? ctx->d_prev_tris : nullptr;
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16);
    if (object_motion) { launch(ctx, gbuffer_kernel<true>, grid, dim3(kTraceBlock), 0, a); ++ctx->motion_launches; }
    else launch(ctx, gbuffer_kernel<false>, grid, dim3(kTraceBlock), 0, a);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "gbuffer kernel launch failed");
    return VHR_OK;
}

// ---------------------------------------------------------------------------------------------
// Stand-in for the rasterised "Shadow Map Pass" (hybrid_render_path.cpp:58-99, depth_prepass.vert:16-19; BASELINE configs[0]):
// the closest hit of the orthographic ray through every texel centre of directional_light.projview's frustum, from the near
// plane (NDC z = 1, reverse Z) to the far plane; depth = 1 - t, misses keep the clear value 0 (oracle decision xiv).
// ---------------------------------------------------------------------------------------------
struct ShadowMapArgs {
    DeviceScene scene;
    float inv_projview[16];
    float *out;
    uint32_t size, row_begin, row_end;
};

__global__ __launch_bounds__(kTraceBlock) void shadow_map_kernel(const ShadowMapArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_stack[kTraceStack * kTraceBlock];
    int *stack = s_stack + threadIdx.x;
    uint32_t x, y;
    pixel_of_thread(x, y, a.row_begin);
    if (x >= a.size || y >= a.row_end) return;
    const float nx = ((float(x) + 0.5f) / float(a.size)) * 2.0f - 1.0f, ny = ((float(y) + 0.5f) / float(a.size)) * 2.0f - 1.0f;
    const f4 pa = mat4_mul(a.inv_projview, f4{ nx, ny, 1.0f, 1.0f }), pb = mat4_mul(a.inv_projview, f4{ nx, ny, 0.0f, 1.0f });
    const f3 o = f3{ pa.x / pa.w, pa.y / pa.w, pa.z / pa.w }, f = f3{ pb.x / pb.w, pb.y / pb.w, pb.z / pb.w };
    Hit h;
    uint32_t overflow = 0;
    float depth = 0.0f;
    if (a.scene.node_count != 0 && traverse<false>(a.scene, o, f - o, 0.0f, 1.0f, stack, h, overflow)) depth = 1.0f - h.t;
    a.out[size_t(y) * a.size + x] = depth;
}

int launch_standin_shadow_map(vhr_context *ctx, const vhr_per_frame_data &pfd, Image &shadow_map) {
    if (shadow_map.format != VHR_FORMAT_D32_SFLOAT || shadow_map.width != shadow_map.height)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_shadow_map: a square D32_SFLOAT image is expected (4096 x 4096, hybrid_render_path.cpp:62)");
    ShadowMapArgs a;
    a.scene = ctx->device_scene();
    if (!host_mat4_inverse(pfd.directional_light.projview, a.inv_projview))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_shadow_map: directional_light.projview is singular");
    a.out = static_cast<float *>(shadow_map.ptr);
    a.size = shadow_map.width;
    a.row_begin = 0;
    a.row_end = shadow_map.height;
    launch(ctx, shadow_map_kernel, dim3((a.size + 15) / 16, (a.row_end - a.row_begin + 15) / 16), dim3(kTraceBlock), 0, a);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "shadow map kernel launch failed");
    return VHR_OK;
}

// ---------------------------------------------------------------------------------------------
// next row f3: stand-in for the composition stage (composition.vert:5-8, composition.frag:60-161)
// ---------------------------------------------------------------------------------------------
struct CompositionArgs {
    vhr_per_frame_data pfd;
    const uchar4 *albedo;        // B8G8R8A8_UNORM
    const void *normals, *motion;
    const float *depth;
    const void *shadow_ao;       // RGBA16F (denoised) or RG16F (raw)
    const void *reflections;     // RGBA16F or nullptr: "Raytraced Reflections" (mode 0) / "Screen Space Reflections" (mode 1)
    const void *ssao;            // RGBA16F or nullptr: "Screen Space Ambient Occlusion" (ambient occlusion mode 1)
    const float *shadow_map;     // D32F, shadow_size^2, or nullptr: "Shadow Map" (shadow mode 1)
    float bias_projview[16];     // SHADOW_BIAS_MATRIX * directional_light.projview (composition.frag:82, the matrix product first)
    uint32_t shadow_size;
    uchar4 *out;                 // B8G8R8A8_SRGB
    uint32_t width, height;
    int shadow_mode, ao_mode, reflection_mode, shadow_ao_is_rgba;
};

__global__ __launch_bounds__(256) void composition_kernel(const CompositionArgs a, const Stamps st) {
    vhr_stamp(st);
    const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63u), j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || j >= a.height) return;
    const uint32_t W = a.width, H = a.height, gy = H - 1 - j;         // flipped presentation viewport (pipeline.cpp:175-178)
    const float u = (float(x) + 0.5f) / float(W), v = (float(gy) + 0.5f) / float(H);
    const uchar4 ab = a.albedo[size_t(gy) * W + x];
    const f3 albedo = f3{ ab.z * (1.0f / 255.0f), ab.y * (1.0f / 255.0f), ab.x * (1.0f / 255.0f) };             // :61
    const float depth = a.depth[size_t(gy) * W + x];                                                               // :62
    const f3 P = get_world_space_position(a.pfd, depth, u, v);                                                     // :63
    const f4 nid = load_rgba16f(a.normals, W, x, gy);                                                              // :64
    const f3 N = f3{ nid.x, nid.y, nid.z };
    const f4 mm = load_rgba16f(a.motion, W, x, gy);                                                                // :65
    float rs = 1.0f, ra = 1.0f;                                                                                    // :67-70
    if (a.shadow_mode == 0 || a.ao_mode == 0) {
        if (a.shadow_ao_is_rgba) { const f4 t = load_rgba16f(a.shadow_ao, W, x, gy); rs = t.x; ra = t.y; }
        else {
            const uint32_t raw = reinterpret_cast<const uint32_t *>(a.shadow_ao)[size_t(gy) * W + x];
            rs = half_bits_to_float(uint16_t(raw & 0xffffu)); ra = half_bits_to_float(uint16_t(raw >> 16));
        }
    }
    const f3 cam = f3{ a.pfd.camera_view_inverse[12], a.pfd.camera_view_inverse[13], a.pfd.camera_view_inverse[14] };
    const f3 V = normalize3(cam - P);                                                                              // :72-75
    const f3 L = -f3{ a.pfd.directional_light.direction[0], a.pfd.directional_light.direction[1], a.pfd.directional_light.direction[2] };
    const f3 Hh = normalize3(L + V);
    float shadow = a.shadow_mode == 0 ? rs : 1.0f;                                                                 // :77-80
    if (a.shadow_mode == 1) {                                                                                      // :81-107: 16-tap PCF
        const f4 pl = mat4_mul(a.bias_projview, f4{ P.x, P.y, P.z, 1.0f });
        const float sx = pl.x / pl.w, sy = pl.y / pl.w, sz = pl.z / pl.w;
        const float scale = 1.0f / 4096.0f;
        float lit = 0.0f;
        for (int i = 0; i < 16; ++i) {
            const float ox = (float(i >> 2) - 1.5f) * scale, oy = (float(i & 3) - 1.5f) * scale;                  // offsets[i], :88-93
            const float ds = sample_depth(a.shadow_map, a.shadow_size, a.shadow_size, sx + ox, sy + oy);
            lit += (sz < ds - 1e-4f) ? 0.0f : 1.0f;
        }
        shadow = lit / 16.0f;
    }
    float ao = a.ao_mode == 0 ? ra : 1.0f;                                                                         // :114-121
    if (a.ao_mode == 1) ao = load_rgba16f(a.ssao, W, x, gy).x;                                                     // :117-119 (in_uv is the texel centre)
    const float metallic = fminf(fmaxf(mm.z, 0.0f), 1.0f), roughness = fminf(fmaxf(mm.w, 0.04f), 1.0f);            // :123-125
    const f3 li = f3{ a.pfd.directional_light.intensity[0], a.pfd.directional_light.intensity[1], a.pfd.directional_light.intensity[2] };
    const f3 lc = f3{ a.pfd.directional_light.color[0], a.pfd.directional_light.color[1], a.pfd.directional_light.color[2] };
    const f3 f0 = f3{ 0.04f * (1.0f - metallic) + albedo.x * metallic, 0.04f * (1.0f - metallic) + albedo.y * metallic,
                      0.04f * (1.0f - metallic) + albedo.z * metallic };                                           // :131-132
    const f3 F = fresnel_schlick(f0, Hh, V);
    const float ndl = fmaxf(dot3(N, L), 0.0f);                                                                     // :135
    const f3 ambient = albedo * (ao * VHR_PI_INVERSE);                                                             // :137
    const f3 dp = f3{ (1.0f - F.x) * (1.0f - metallic), (1.0f - F.y) * (1.0f - metallic), (1.0f - F.z) * (1.0f - metallic) };
    const f3 diffuse = mul3(mul3(f3{ dp.x * albedo.x / VHR_PI, dp.y * albedo.y / VHR_PI, dp.z * albedo.z / VHR_PI } * ndl, li), lc) * shadow;   // :138
    const float dg = D_GGX(roughness, N, Hh) * G_GGX(roughness, N, V, L);
    const float invd = 1.0f / fmaxf(4.0f * fmaxf(dot3(N, V), 0.0f) * fmaxf(dot3(N, L), 0.0f), 1e-6f);
    f3 spec = mul3(mul3(f3{ dg * F.x * invd, dg * F.y * invd, dg * F.z * invd } * ndl, li), lc) * shadow;          // :139
    if ((a.reflection_mode == 0 || a.reflection_mode == 1) && a.reflections) {                                     // :139-156 (the same blend for both sources)
        const f4 r = load_rgba16f(a.reflections, W, x, gy);
        const f3 refl = f3{ r.x, r.y, r.z } * shadow;
        if (metallic == 1.0f) spec = refl;
        else spec = f3{ spec.x * (1.0f - roughness) + refl.x * roughness, spec.y * (1.0f - roughness) + refl.y * roughness,
                        spec.z * (1.0f - roughness) + refl.z * roughness };
    }
    const f3 lighting = ambient + diffuse + spec;                                                                  // :160-162
    a.out[size_t(j) * W + x] = make_uchar4(srgb8(lighting.z), srgb8(lighting.y), srgb8(lighting.x), 255);
}

int launch_composition(vhr_context *ctx, const vhr_per_frame_data &pfd, const vhr_composition_desc &d, const Image &albedo, const Image &normals,
                       const Image &motion, const Image &depth, const Image &shadow_ao, const Image *reflections, const Image *ssao,
                       const Image *shadow_map, Image &out) {
    const uint32_t W = depth.width, H = depth.height;
    const Image *all[] = { &albedo, &normals, &motion, &shadow_ao, &out };
    for (const Image *im : all)
        if (im->width != W || im->height != H) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: image extents differ");
    if (reflections && (reflections->width != W || reflections->height != H)) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: image extents differ");
    if (albedo.bpp != 4 || out.bpp != 4 || normals.format != VHR_FORMAT_R16G16B16A16_SFLOAT || motion.format != VHR_FORMAT_R16G16B16A16_SFLOAT ||
        depth.format != VHR_FORMAT_D32_SFLOAT || (shadow_ao.format != VHR_FORMAT_R16G16B16A16_SFLOAT && shadow_ao.format != VHR_FORMAT_R16G16_SFLOAT))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: unexpected image format");
    if (d.shadow_mode == 1 && (!shadow_map || shadow_map->format != VHR_FORMAT_D32_SFLOAT || shadow_map->width != shadow_map->height))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: shadow_mode 1 needs the square D32 \"Shadow Map\" image");
    for (int m : { d.shadow_mode, d.ambient_occlusion_mode, d.reflection_mode })
        if (m < 0 || m > 2) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: modes are 0 (ray traced), 1 (screen space) or 2 (off)");
    if (d.ambient_occlusion_mode == 1 && (!ssao || ssao->width != W || ssao->height != H || ssao->format != VHR_FORMAT_R16G16B16A16_SFLOAT))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: ambient_occlusion_mode 1 needs the R16G16B16A16 \"Screen Space Ambient Occlusion\" image");
    CompositionArgs a;
    a.ssao = ssao ? ssao->ptr : nullptr;
    a.shadow_map = shadow_map ? static_cast<const float *>(shadow_map->ptr) : nullptr;
    a.shadow_size = shadow_map ? shadow_map->width : 0;
    static const float kShadowBias[16] = { 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.5f, 0.5f, 0.0f, 1.0f };   // common.glsl:6-11
    host_mat4_mul(kShadowBias, pfd.directional_light.projview, a.bias_projview);
    a.pfd = pfd;
    a.albedo = static_cast<const uchar4 *>(albedo.ptr);
    a.normals = normals.ptr; a.motion = motion.ptr;
    a.depth = static_cast<const float *>(depth.ptr);
    a.shadow_ao = shadow_ao.ptr;
    a.reflections = reflections ? reflections->ptr : nullptr;
    a.out = static_cast<uchar4 *>(out.ptr);
    a.width = W; a.height = H;
    a.shadow_mode = d.shadow_mode; a.ao_mode = d.ambient_occlusion_mode; a.reflection_mode = d.reflection_mode;
    a.shadow_ao_is_rgba = shadow_ao.format == VHR_FORMAT_R16G16B16A16_SFLOAT;
    launch(ctx, composition_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, a);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "composition kernel launch failed");
    return VHR_OK;
}

}  // namespace vhr
