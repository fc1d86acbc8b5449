// The point / triangle distance of vhr_closest_point_query: ONE definition for the device (kernels_point_query.hip: the walker's leaf test and the
// pairs kernel of vhr_debug_point_triangle) and for the host (queries.cpp: vhr_debug_point_triangle on a host-only context).  The two owe each
// other BITS (tests/test_gpu_point_query.py), so everything here is plain fp32, every operation rounded once in the order written (both files
// are built with -ffp-contract=off), every quotient an IEEE division, every selection a comparison -- no fminf / fmaxf, whose answer for (-0, +0)
// is the implementation's choice -- and no intrinsic.
//
// point_triangle(p, v0, e1, e2) -> (d2, u, v): the squared distance from p to the closed triangle v0 + u e1 + v e2 (u, v >= 0, u + v <= 1) of a
// leaf record, and the barycentrics of the nearest point.  An equivalent of the region classification of Ericson, Real-Time Collision
// Detection 5.1.5, made of the same seven regions but decided by DISTANCE, not by the signs of 2 x 2 determinants of dot products:
//   - four candidates, each a point OF the triangle: the foot of p's perpendicular on the plane if its barycentrics fall inside (the face
//     region), and the nearest point of each of the three edges as segments (a clamped parameter: the edge and vertex regions);
//   - every candidate's d2 = |(ap - u e1) - v e2|^2 from its own (u, v) by the same three lines; the smallest wins (face, AB, AC, BC: the earlier
//     one on a tie).
// Why: a record may have no area (a segment or a point: the fuzz scenes hold such records) or next to none, and then the determinants the
// classification tests are rounding noise -- it may call the face region with barycentrics anywhere on the record.  Here a wrong or missing face
// candidate costs nothing: every candidate is a point of the record, so no d2 is below the truth by more than its own evaluation error, and the
// nearest boundary point is never farther from the true nearest point than the inradius.  The error bound that follows is derived in DESIGN.md 4d
// and held against a binary64 truth by tests/test_point_query_host.py.
//   - A zero denominator (an edge of length 0, a normal of length 0) selects the vertex or drops the face candidate; it is never divided by.
//   - (u, v) is always finite and inside the closed unit triangle IN EXACT ARITHMETIC: u + v of an edge-BC point is exactly 1 (one of 1 - w and
//     1 - (1 - w) is exact by Sterbenz' lemma), and the face candidate's u + v <= 1 is tested without rounding the same way.
//   - A non-finite p gives d2 = +inf, (u, v) = (0, 0): no candidate.  A record with non-finite numbers gives +inf too unless some candidate's d2
//     is a number.
#pragma once

#include <hip/hip_runtime.h>

namespace vhr {

struct PointTriangle { float d2, u, v; };

// |(ap - u e1) - v e2|^2, the one evaluation every candidate goes through
__host__ __device__ inline float point_triangle_d2(const float ap[3], const float e1[3], const float e2[3], float u, float v) {
    const float rx = (ap[0] - u * e1[0]) - v * e2[0], ry = (ap[1] - u * e1[1]) - v * e2[1], rz = (ap[2] - u * e1[2]) - v * e2[2];
    return (rx * rx + ry * ry) + rz * rz;
}

// num / den clamped to [0, 1]; den == 0 (or not a number, or negative: it is a squared length) selects 0, as does a quotient that is not a number
__host__ __device__ inline float clamped_quotient(float num, float den) {
    if (!(den > 0.0f)) return 0.0f;
    const float t = num / den;
    return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;
}

__host__ __device__ inline PointTriangle point_triangle(const float p[3], const float v0[3], const float e1[3], const float e2[3]) {
    PointTriangle best{ __builtin_inff(), 0.0f, 0.0f };
    if (!(__builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]))) return best;
    const float ap[3] = { p[0] - v0[0], p[1] - v0[1], p[2] - v0[2] };
    // the face region: n = e1 x e2, u = ((ap x e2) . n) / (n . n), v = ((e1 x ap) . n) / (n . n)
    const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    const float nn = (nx * nx + ny * ny) + nz * nz;
    if (nn > 0.0f) {
        const float ax = ap[1] * e2[2] - ap[2] * e2[1], ay = ap[2] * e2[0] - ap[0] * e2[2], az = ap[0] * e2[1] - ap[1] * e2[0];
        const float bx = e1[1] * ap[2] - e1[2] * ap[1], by = e1[2] * ap[0] - e1[0] * ap[2], bz = e1[0] * ap[1] - e1[1] * ap[0];
        const float u = ((ax * nx + ay * ny) + az * nz) / nn, v = ((bx * nx + by * ny) + bz * nz) / nn;
        // u + v <= 1 without rounding: 1 - x is exact for x in [0.5, 1], and two numbers below 0.5 sum to less than 1
        bool inside = u >= 0.0f && v >= 0.0f && u <= 1.0f && v <= 1.0f;
        if (inside && u >= 0.5f) inside = v <= 1.0f - u;
        else if (inside && v >= 0.5f) inside = u <= 1.0f - v;
        if (inside) {
            const float d2 = point_triangle_d2(ap, e1, e2, u, v);
            if (d2 < best.d2) best = PointTriangle{ d2, u, v };
        }
    }
    {   // edge AB (and the vertex regions at its ends): v0 + t e1
        const float t = clamped_quotient((ap[0] * e1[0] + ap[1] * e1[1]) + ap[2] * e1[2], (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);
        const float d2 = point_triangle_d2(ap, e1, e2, t, 0.0f);
        if (d2 < best.d2) best = PointTriangle{ d2, t, 0.0f };
    }
    {   // edge AC: v0 + t e2
        const float t = clamped_quotient((ap[0] * e2[0] + ap[1] * e2[1]) + ap[2] * e2[2], (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]);
        const float d2 = point_triangle_d2(ap, e1, e2, 0.0f, t);
        if (d2 < best.d2) best = PointTriangle{ d2, 0.0f, t };
    }
    {   // edge BC: (v0 + e1) + w (e2 - e1) = v0 + (1 - w) e1 + w e2
        const float ex = e2[0] - e1[0], ey = e2[1] - e1[1], ez = e2[2] - e1[2];
        const float bpx = ap[0] - e1[0], bpy = ap[1] - e1[1], bpz = ap[2] - e1[2];
        const float w = clamped_quotient((bpx * ex + bpy * ey) + bpz * ez, (ex * ex + ey * ey) + ez * ez);
        float u, v;
        if (w < 0.5f) { u = 1.0f - w; v = 1.0f - u; }      // u >= 0.5 (rounded once), so 1 - u is exact: u + v == 1
        else { v = w; u = 1.0f - w; }                      // w in [0.5, 1]: 1 - w is exact
        const float d2 = point_triangle_d2(ap, e1, e2, u, v);
        if (d2 < best.d2) best = PointTriangle{ d2, u, v };
    }
    return best;
}

}  // namespace vhr
