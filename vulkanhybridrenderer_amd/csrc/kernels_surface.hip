// vhr_resolve_hits: the surface points of a batch of hits (include/vhr_amd.h).  A unit of its own: it reads the scene arrays and never the tree.
// The geometry part is surface_point.hpp's, which the host runs as well (queries.cpp, host-only contexts) and which owes it BITS, so the unit is
// built with -ffp-contract=off; the material part is the stand-in G-buffer's gbuf.frag lines (kernels_standin.hip: gbuffer_kernel) on the helpers of
// trace_device.hpp, which also gives the unit its copy of the sRGB decode table.
#define VHR_TRACE_UNIT unit_surface      // this unit's copy of the sRGB decode table (trace_device.hpp)
#include "trace_device.hpp"
#include "surface_point.hpp"

namespace vhr {

struct ResolveArgs {
    DeviceScene scene;
    const uint32_t *hits;                 // vhr_ray_hit[count] as dwords: (t, u, v, geometry_index, primitive_index, reserved); 4-byte aligned
    float4 *out;                          // vhr_surface_point[count] as five float4 each; 16-byte aligned
    SurfaceCounters *counters;            // kSurfaceCounterSlots slots
    const uint8_t *flips;                 // one byte per primitive (never null where the scene has primitives)
    uint32_t count;
};
static_assert(sizeof(vhr_ray_hit) == 6 * sizeof(uint32_t) && sizeof(vhr_surface_point) == 5 * sizeof(float4), "vhr_ray_hit / vhr_surface_point");
static_assert(sizeof(vhr_vertex) == 7 * sizeof(float2) && sizeof(vhr_primitive) == 15 * sizeof(float2), "vhr_vertex / vhr_primitive in 8-byte words");

// A vertex is 56 bytes and a primitive 120, so either starts at an 8-byte boundary of its array: 8-byte loads.  Of a vertex, words 3 and 4 are the
// tangent, which only a normal-mapped material reads (interpolate_tangent fetches it then): five loads, not seven.
__device__ __forceinline__ vhr_vertex load_vertex_no_tangent(const vhr_vertex *p) {
    const float2 *q = reinterpret_cast<const float2 *>(p);
    const float2 w0 = q[0], w1 = q[1], w2 = q[2], w5 = q[5], w6 = q[6];
    vhr_vertex v;
    v.pos[0] = w0.x; v.pos[1] = w0.y; v.pos[2] = w1.x;
    v.normal[0] = w1.y; v.normal[1] = w2.x; v.normal[2] = w2.y;
    v.tangent[0] = v.tangent[1] = v.tangent[2] = v.tangent[3] = 0.0f;
    v.uv0[0] = w5.x; v.uv0[1] = w5.y;
    v.uv1[0] = w6.x; v.uv1[1] = w6.y;
    return v;
}
__device__ __forceinline__ vhr_primitive load_primitive(const vhr_primitive *p) {
    const float2 *q = reinterpret_cast<const float2 *>(p);
    float2 w[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) w[k] = q[k];
    vhr_primitive r;
    __builtin_memcpy(&r, w, sizeof(r));
    return r;
}

// One hit per lane, no LDS, no stack.  Every check on the hit comes before the gather it guards: geometry_index against the primitive count
// before the primitive is read, primitive_index against that primitive's triangle count before its indices are (vhr_update_geometry has
// checked every index and offset of the scene arrays themselves).
template <bool MATERIAL>
__global__ __launch_bounds__(256) void resolve_hits_kernel(const ResolveArgs a, const Stamps st) {
    vhr_stamp(st);
    const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    const DeviceScene &sc = a.scene;
    uint32_t valid = 0u, discarded = 0u;
    if (i < a.count) {
        const uint32_t *h = a.hits + i * 6u;
        const float u = __uint_as_float(h[1]), v = __uint_as_float(h[2]);
        const uint32_t g = h[3], tri = h[4];
        float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o1 = o0, o2 = o0, o3 = o0, o4 = o0;
        bool ok = surface_hit_addressable(u, v, g, tri, sc.primitive_count);
        vhr_primitive prim;
        if (ok) {
            prim = load_primitive(sc.primitives + g);
            ok = tri < prim.index_count / 3u;
        }
        if (ok) {
            const uint32_t *ix = sc.indices + (size_t(prim.index_offset) + 3u * size_t(tri));
            const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
            const vhr_vertex va = load_vertex_no_tangent(sc.vertices + (size_t(prim.vertex_offset) + i0));
            const vhr_vertex vb = load_vertex_no_tangent(sc.vertices + (size_t(prim.vertex_offset) + i1));
            const vhr_vertex vc = load_vertex_no_tangent(sc.vertices + (size_t(prim.vertex_offset) + i2));
            const float *Mp = sc.normal_matrices + 9 * size_t(g);
            const float M[9] = { Mp[0], Mp[1], Mp[2], Mp[3], Mp[4], Mp[5], Mp[6], Mp[7], Mp[8] };
            SurfaceGeometry s = surface_geometry(prim.transform, a.flips[g] != 0, M, va, vb, vc, u, v);
            f4 al = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
            float metallic = 0.0f, roughness = 0.0f;
            if constexpr (MATERIAL) {
                const float uvx = s.uv0[0], uvy = s.uv0[1];
                al = f4{ prim.material.base_color[0], prim.material.base_color[1], prim.material.base_color[2], prim.material.base_color[3] };
                if (prim.material.base_color_texture != -1) al = sample_texture(sc, prim.material.base_color_texture, uvx, uvy);               // gbuf.frag:19-26
                if ((prim.material.alpha_mask == 1 && al.w < prim.material.alpha_cutoff) || al.w == 0.0f) s.flags |= VHR_SURFACE_DISCARDED;   // :27-32
                if (prim.material.normal_map >= 0) {                                                                                            // :35-41
                    const f3 n = f3{ s.normal[0], s.normal[1], s.normal[2] };
                    const f4 tx = sample_texture(sc, prim.material.normal_map, uvx, uvy);
                    const f3 tsn = normalize3(f3{ tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f });
                    const f4 tg = interpolate_tangent(sc, prim, tri, u, v);
                    const f3 T = f3{ tg.x, tg.y, tg.z };
                    const f3 bitangent = cross3(tsn, T) * tg.w;                  // sic: cross(tangent_space_normal, in_tangent.xyz)
                    const f3 tangent = normalize3(T - n * dot3(T, n));
                    const f3 N = (tangent * tsn.x + bitangent * tsn.y) + n * tsn.z;
                    const float Nv[3] = { N.x, N.y, N.z };
                    s.flags = (s.flags & ~uint32_t(VHR_SURFACE_NO_SHADING_NORMAL)) | VHR_SURFACE_NORMAL_MAPPED;
                    if (!surface_world_normal(M, Nv, s.shading_normal)) s.flags |= VHR_SURFACE_NO_SHADING_NORMAL;                             // :43
                }
                metallic = prim.material.metallic_factor; roughness = prim.material.roughness_factor;
                if (prim.material.metallic_roughness_texture != -1) {                                                                           // :50-56
                    const f4 mr = sample_texture(sc, prim.material.metallic_roughness_texture, uvx, uvy);
                    metallic *= mr.y;
                    roughness *= mr.z;
                }
            }
            valid = 1u;
            discarded = (s.flags & VHR_SURFACE_DISCARDED) ? 1u : 0u;
            o0 = make_float4(s.position[0], s.position[1], s.position[2], __uint_as_float(s.flags));
            o1 = make_float4(s.geometric_normal[0], s.geometric_normal[1], s.geometric_normal[2], metallic);
            o2 = make_float4(s.shading_normal[0], s.shading_normal[1], s.shading_normal[2], roughness);
            o3 = make_float4(al.x, al.y, al.z, al.w);
            o4 = make_float4(s.uv0[0], s.uv0[1], s.uv1[0], s.uv1[1]);
        }
        float4 *const o = a.out + i * 5u;
        o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3; o[4] = o4;
    }
    // the wave's sums, one vector atomic each from its first lane (every lane of the wave arrives here), into the slot of the block's index
    for (int off = 32; off > 0; off >>= 1) { valid += uint32_t(__shfl_xor(int(valid), off)); discarded += uint32_t(__shfl_xor(int(discarded), off)); }
    if ((threadIdx.x & 63u) == 0u) {
        SurfaceCounters *const c = a.counters + (blockIdx.x & (kSurfaceCounterSlots - 1u));
        if (valid) atomicAdd(&c->valid, (unsigned long long)valid);
        if (discarded) atomicAdd(&c->discarded, (unsigned long long)discarded);
    }
}

int launch_resolve_hits(vhr_context *ctx, const vhr_ray_hit *hits, uint32_t count, bool material, vhr_surface_point *out) {
    if (count == 0) return VHR_OK;
    const QueryScratch *const s = stream_scratch(ctx, ctx->sp_scratch, sizeof(SurfaceCounters) * kSurfaceCounterSlots, "vhr_resolve_hits");        // this stream's counters
    if (!s) return VHR_ERROR_DEVICE;
    ResolveArgs a;
    a.scene = ctx->device_scene();
    a.hits = reinterpret_cast<const uint32_t *>(hits);
    a.out = reinterpret_cast<float4 *>(out);
    ctx->sp_last_counters = a.counters = static_cast<SurfaceCounters *>(s->counters);
    a.flips = nullptr;
    a.count = count;
    if (ctx->primitive_count != 0) {
        if (const int rc = ensure_device_prim_flips(ctx)) return rc;
        a.flips = ctx->d_prim_flips;
    }
    const dim3 grid(uint32_t((uint64_t(count) + 255u) / 256u));
    if (material) launch(ctx, resolve_hits_kernel<true>, grid, dim3(256), 0, a);
    else launch(ctx, resolve_hits_kernel<false>, grid, dim3(256), 0, a);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "vhr_resolve_hits: kernel launch failed");
    return VHR_OK;
}

}  // namespace vhr
