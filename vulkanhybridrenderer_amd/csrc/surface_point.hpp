// The geometry part of vhr_resolve_hits: ONE definition for the device (kernels_surface.hip: resolve_hits_kernel) and for the host (queries.cpp:
// the loop a host-only context runs).  The two owe each other BITS (tests/test_gpu_surface.py), so the rules are those closest_point.hpp states
// for itself: plain fp32, every operation rounded once in the order written (both files are built with -ffp-contract=off), every quotient an
// IEEE division, the square roots IEEE's, every selection a comparison -- no fminf / fmaxf -- and no intrinsic.
//
// surface_geometry(transform, flip, normal matrix, the triangle's three vertices, u, v) -> position, geometric normal, uv0, uv1, the un-mapped
// shading normal and the result bits that belong to them:
//   - (v0, e1, e2) = bvh_math::world_record(transform, pos0, pos1, pos2): the function the builders and the refits use, so these are the bits of
//     the leaf record the walkers tested, whichever tree holds it (there is no slot lookup, the tree is never read);
//   - position = (v0 + u e1) + v e2 per component: the point the closest-point query measured to, the P of the object-motion contract;
//   - geometric normal = cross(e1, e2), negated where the primitive's flip byte is 1, over sqrtf(n . n); n . n not in (0, inf) -- a triangle without
//     area, products that underflow to 0, or that overflow -- gives the zero vector and VHR_SURFACE_DEGENERATE;
//   - uv0, uv1 and the object-space normal with barycentrics (1 - u - v, u, v), the products summed left to right (trace_device.hpp: interpolate);
//   - shading normal = surface_world_normal(normal matrix, object-space normal), the stand-in G-buffer's gbuf.frag:43 operation for operation.
// The material half (textures, the normal map's perturbation) lives in kernels_surface.hip; it ends in surface_world_normal as well.
#pragma once

#include <hip/hip_runtime.h>

#include "bvh_math.hpp"

namespace vhr {

struct SurfaceGeometry {
    float position[3];
    float geometric_normal[3];
    float normal[3];              // object space, interpolated, not normalised (what the normal map perturbs)
    float shading_normal[3];      // surface_world_normal of `normal`
    float uv0[2], uv1[2];
    uint32_t flags;               // VHR_SURFACE_VALID | DEGENERATE | NO_SHADING_NORMAL
};

// the checks that come before any gather: a miss, a primitive the scene does not have, barycentrics that are no numbers
__host__ __device__ inline bool surface_hit_addressable(float u, float v, uint32_t geometry_index, uint32_t primitive_index, uint32_t primitive_count) {
    return geometry_index != 0xFFFFFFFFu && primitive_index != 0xFFFFFFFFu && geometry_index < primitive_count && __builtin_isfinite(u) && __builtin_isfinite(v);
}

// normalize(M N) as kernels_standin.hip:86-87 writes it: M column-major 3 x 3, the row sums left to right, then a * (1 / sqrtf(a . a)).
// false (and out = 0) where a . a is not a positive finite number
__host__ __device__ inline bool surface_world_normal(const float M[9], const float N[3], float out[3]) {
    const float x = (M[0] * N[0] + M[3] * N[1]) + M[6] * N[2], y = (M[1] * N[0] + M[4] * N[1]) + M[7] * N[2], z = (M[2] * N[0] + M[5] * N[1]) + M[8] * N[2];
    const float d = (x * x + y * y) + z * z;
    if (!(d > 0.0f && d < __builtin_inff())) { out[0] = out[1] = out[2] = 0.0f; return false; }
    const float inv = 1.0f / sqrtf(d);
    out[0] = x * inv; out[1] = y * inv; out[2] = z * inv;
    return true;
}

__host__ __device__ inline SurfaceGeometry surface_geometry(const float transform[16], bool flip, const float M[9], const vhr_vertex &a, const vhr_vertex &b,
                                                            const vhr_vertex &c, float u, float v) {
    SurfaceGeometry r;
    r.flags = VHR_SURFACE_VALID;
    float v0[3], e1[3], e2[3];
    (void)bvh_math::world_record(transform, a.pos, b.pos, c.pos, v0, e1, e2);
    for (int k = 0; k < 3; ++k) r.position[k] = (v0[k] + u * e1[k]) + v * e2[k];
    float n[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
    if (flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (nn > 0.0f && nn < __builtin_inff()) {
        const float len = sqrtf(nn);
        for (int k = 0; k < 3; ++k) r.geometric_normal[k] = n[k] / len;
    } else {
        r.geometric_normal[0] = r.geometric_normal[1] = r.geometric_normal[2] = 0.0f;
        r.flags |= VHR_SURFACE_DEGENERATE;
    }
    const float bx = 1.0f - u - v, by = u, bz = v;
    for (int k = 0; k < 2; ++k) {
        r.uv0[k] = a.uv0[k] * bx + b.uv0[k] * by + c.uv0[k] * bz;
        r.uv1[k] = a.uv1[k] * bx + b.uv1[k] * by + c.uv1[k] * bz;
    }
    for (int k = 0; k < 3; ++k) r.normal[k] = a.normal[k] * bx + b.normal[k] * by + c.normal[k] * bz;
    if (!surface_world_normal(M, r.normal, r.shading_normal)) r.flags |= VHR_SURFACE_NO_SHADING_NORMAL;
    return r;
}

}  // namespace vhr
