// Which side of a triangle a ray meets (vhr_ray_query_faces: face culling and the hit kind): ONE definition for the device (kernels_ray_query.hip:
// the face filter of both walkers, the hit kind at the commit and the pairs kernel of vhr_debug_ray_facing) and for the host (queries.cpp:
// vhr_debug_ray_facing on a host-only context, and the primitives' flip bytes).  The counterpart of closest_point.hpp; every unit that includes
// it is built with -ffp-contract=off.
//
// Facing is the sign of Moeller-Trumbore's determinant det = e1 . (d x e2) = -d . (e1 x e2): det > 0 = the vertices v0, v0 + e1, v0 + e2 appear
// counter-clockwise from the ray's origin = FRONT (glTF's winding, VK_FRONT_FACE_COUNTER_CLOCKWISE, an instance with
// VK_GEOMETRY_INSTANCE_TRIANGLE_FRONT_COUNTERCLOCKWISE_BIT_KHR).  At grazing incidence the fp32 determinant is rounding noise -- exactly where
// decision (vi) hands the candidate to binary64 -- so the sign is taken from the binary64 determinant, operation for operation mt_binary64's
// (trace_device.hpp): the fp32 operands and every product of two of them are exact in binary64, every other operation rounds once in the order
// written.  tests/test_face_cull_host.py holds it against exact rational arithmetic (DESIGN.md 4e has the count of pairs the fp32 sign gets wrong).
//
// Everything that is not > 0 is BACK: det == 0, and the NaN of a NaN direction (such a pair is a candidate through noise only), so the two
// cull modes partition every ray's candidates.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace vhr {

constexpr uint32_t kFaceCullNone = 0u, kFaceCullBack = 1u, kFaceCullFront = 2u;        // VHR_FACE_CULL_*
constexpr uint32_t kHitKindFront = 0xFEu, kHitKindBack = 0xFFu;                        // VHR_HIT_KIND_*

// true = the triangle (e1, e2) is front-facing for a ray of direction d.  `flip`: the primitive's transform mirrors (facing_flip below): the
// records' e1, e2 are world space with the transform baked in, facing is decided in object space.
// The determinant in its two steps, p = d x e2 and det = e1 . p (a caller short of registers may fetch e1 between them: RayFaceReject).
struct FacingPvec { double x, y, z; };
__host__ __device__ inline FacingPvec facing_pvec(float dx, float dy, float dz, float e2x, float e2y, float e2z) {
    FacingPvec p;
    p.x = double(dy) * double(e2z) - double(dz) * double(e2y);
    p.y = double(dz) * double(e2x) - double(dx) * double(e2z);
    p.z = double(dx) * double(e2y) - double(dy) * double(e2x);
    return p;
}
__host__ __device__ inline bool facing_front(const FacingPvec &p, float e1x, float e1y, float e1z, bool flip) {
    const double det = (double(e1x) * p.x + double(e1y) * p.y) + double(e1z) * p.z;
    return (det > 0.0) != flip;
}
__host__ __device__ inline bool ray_front_facing(float dx, float dy, float dz, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, bool flip) {
    return facing_front(facing_pvec(dx, dy, dz, e2x, e2y, e2z), e1x, e1y, e1z, flip);
}
__host__ __device__ inline uint32_t ray_hit_kind(float dx, float dy, float dz, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, bool flip) {
    return ray_front_facing(dx, dy, dz, e1x, e1y, e1z, e2x, e2y, e2z, flip) ? kHitKindFront : kHitKindBack;
}
// does a ray of this cull mode not see the triangle?  (mode: wave-uniform; kFaceCullNone culls nothing)
__host__ __device__ inline bool ray_face_culled(uint32_t mode, bool front) { return mode == kFaceCullBack ? !front : (mode == kFaceCullFront ? front : false); }

// 1 = the primitive's transform reverses the winding ("a negative determinant of the global transform reverses the winding", glTF 2.0 3.7.4;
// Vulkan decides facing in object space likewise): the determinant of the upper 3 x 3 of the column-major 4 x 4 `m` in binary64, expanded by
// cofactors along the first row -- (m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20)) + m02 (m10 m21 - m11 m20), m_rc = m[c * 4 + r] -- every
// product of two fp32 values exact, every other operation rounded once in the order written.  < 0 gives 1; zero and NaN give 0.
inline uint8_t facing_flip(const float m[16]) {
    const double m00 = m[0], m10 = m[1], m20 = m[2], m01 = m[4], m11 = m[5], m21 = m[6], m02 = m[8], m12 = m[9], m22 = m[10];
    const double c0 = m11 * m22 - m12 * m21, c1 = m10 * m22 - m12 * m20, c2 = m10 * m21 - m11 * m20;
    const double det = (m00 * c0 - m01 * c1) + m02 * c2;
    return det < 0.0 ? uint8_t(1) : uint8_t(0);
}

}  // namespace vhr
