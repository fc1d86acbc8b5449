// What every ray-tracing unit (kernels_trace.hip, kernels_raytraced.hip, kernels_forward.hip, kernels_standin.hip, kernels_ray_query.hip)
// shares on the device: the triangle test of decision (vi), the candidate-filter protocol and its filters, the per-lane walker traverse<>,
// the image and texture helpers and the mirror ray's hit shader.  Device and host helpers only: no kernel and no launcher lives here.  (Until the ray-tracing unit was split
// by render path this was the head of kernels_trace.hip.)
//
// Replaces the driver's acceleration-structure traversal (traceRayEXT) by traverse<>(), and
//   data/shaders/hybrid_render_path/reflection_hit.rchit:10-72 -> shade_reflection_hit
//   data/shaders/raytraced_render_path/shadow_anyhit.rahit:8-27 -> alpha_ignored (the filter RahitAlpha)
//
// Every unit that includes this is compiled with -ffp-contract=off: ray setup and Moeller-Trumbore follow the exact-arithmetic contract of
// device_math.hpp so visibility results are bit-reproducible.
#pragma once

#include <type_traits>

#include "device_math.hpp"
#include "ray_facing.hpp"
#include "vhr_internal.hpp"

#ifndef VHR_TRACE_UNIT
#error "define VHR_TRACE_UNIT, a name of this unit's own, before including trace_device.hpp: it names the unit's copy of the sRGB decode table"
#endif

namespace vhr {

// The sRGB decode table fetch_texel() reads.  The library is built without relocatable device code, so every unit that includes this header
// has a table of its own, and `s_srgb_lut_copy` links that copy into the list upload_srgb_lut() fills (vhr_internal.hpp): a unit is registered
// by including this.  The table keeps external linkage -- a file-local one is reached through the code object's offset table, one more scalar
// load in every kernel that samples a texture -- so the copies differ by name: each lives in an inline namespace of its unit's, VHR_TRACE_UNIT.
// A unit that does not name itself does not compile, and two units with one name do not link.
inline namespace VHR_TRACE_UNIT {
__constant__ float c_srgb_lut[256];
}
static SrgbLutCopy s_srgb_lut_copy([](const float *lut) { return hipMemcpyToSymbol(HIP_SYMBOL(c_srgb_lut), lut, 256 * sizeof(float)) == hipSuccess ? 0 : -1; });

constexpr int kTraceBlock = 256;          // 4 waves; each wave owns an 8x8 pixel tile of a 16x16 block tile

struct Hit {
    float t, u, v;
    uint32_t tri_index;    // index into DeviceScene::tris
    uint32_t flat;
};

// Decision (vi), second half.  A candidate of fp32 Moeller-Trumbore whose solution is CONSISTENT -- the ray's point
// o + t d and the triangle's point v0 + u e1 + v e2 agree per axis to within 5e-4 + 5e-6 |coordinate|, half the padding of any box around the
// triangle -- is accepted as it is: whatever it is, it lies inside every box that leads to the triangle, in any frame.  For a ray within rounding
// of the triangle's plane the determinant is rounding noise and (t, u, v) contradict themselves: round 5 rejected such a candidate, which removed
// the hits that are not there (a point centimetres beside the triangle) and, at grazing incidence on large triangles, true ones with them
// (profiles/r6_decision_vi.txt: 21 059 of 387 896 exact hits on the raytraced path's terminator rays).  Since round 6 it is DECIDED AGAIN IN
// BINARY64 (mt_binary64 below): the audit against exact arithmetic counts no lost and no invented hit among them.
// Individually rounded operations in the oracle's order; a NaN is inconsistent.
__device__ __forceinline__ bool solution_consistent(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float t, float u, float v) {
    const float px = o.x + d.x * t, py = o.y + d.y * t, pz = o.z + d.z * t;
    const float qx = (v0.x + e1.x * u) + e2.x * v, qy = (v0.y + e1.y * u) + e2.y * v, qz = (v0.z + e1.z * u) + e2.z * v;
    return fabsf(px - qx) <= 5e-4f + 5e-6f * fabsf(qx) && fabsf(py - qy) <= 5e-4f + 5e-6f * fabsf(qy) && fabsf(pz - qz) <= 5e-4f + 5e-6f * fabsf(qz);
}

// Moeller-Trumbore in binary64 (the oracle's mt_binary64, operation for operation): the fp32 operands and every product of two of them are exact,
// every other operation rounds once in the order written (this unit is built with -ffp-contract=off), the quotients are IEEE divisions; the comparisons
// are ray_triangle()'s and (t, u, v) come back rounded to fp32.  Written for few live registers -- operands are widened where they are used, pvec and
// tvec are the only vectors kept.  It sits inside the leaf tests of the per-pixel walkers (traverse<>) and of the raytraced path's queue kernel; the two
// queue kernels of the hybrid path keep it OUT of their loops: a self-contradicting candidate marks the pixel, and the tile's epilogue computes the pixel
// again through traverse<> behind one call (redo_pixel_visibility / redo_pixel_reflection).  Inside the any-hit queue kernel's leaf test it cost 13
// registers = a wave per SIMD = 1.5 % of the frame, inside the two-bounce mirror kernel's 45 spilled registers = 13 % of the launch; the forms measured on
// the way (a call from the leaf test, a second launch, a list per ray decided at the ray's commit) are in profiles/r6_decision_vi_cost.txt.
__device__ __forceinline__ bool mt_binary64(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float tmin, float tmax, float &t, float &u, float &v) {
    const double px = double(d.y) * double(e2.z) - double(d.z) * double(e2.y);
    const double py = double(d.z) * double(e2.x) - double(d.x) * double(e2.z);
    const double pz = double(d.x) * double(e2.y) - double(d.y) * double(e2.x);
    const double det = (double(e1.x) * px + double(e1.y) * py) + double(e1.z) * pz;
    if (det == 0.0) return false;
    const double tx = double(o.x) - double(v0.x), ty = double(o.y) - double(v0.y), tz = double(o.z) - double(v0.z);
    const double uu = ((tx * px + ty * py) + tz * pz) / det;
    if (!(uu >= 0.0) || uu > 1.0) return false;
    const double qx = ty * double(e1.z) - tz * double(e1.y), qy = tz * double(e1.x) - tx * double(e1.z), qz = tx * double(e1.y) - ty * double(e1.x);
    const double vv = ((double(d.x) * qx + double(d.y) * qy) + double(d.z) * qz) / det;
    if (!(vv >= 0.0) || uu + vv > 1.0) return false;
    const double tt = ((double(e2.x) * qx + double(e2.y) * qy) + double(e2.z) * qz) / det;
    if (!(tt > double(tmin) && tt < double(tmax))) return false;
    t = float(tt); u = float(uu); v = float(vv);
    return true;
}

// Moeller-Trumbore, two-sided, det == 0 -> miss, accept iff tmin < t < tmax; a candidate whose solution contradicts itself is decided again in
// binary64 (decision vi in DESIGN.md).
__device__ __forceinline__ bool ray_triangle(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float tmin, float tmax,
                                             float &t, float &u, float &v) {
    f3 pvec = cross3(d, e2);
    float det = dot3(e1, pvec);
    if (det == 0.0f) return false;
    float inv = 1.0f / det;
    f3 tvec = o - v0;
    float uu = dot3(tvec, pvec) * inv;
    if (!(uu >= 0.0f) || uu > 1.0f) return false;
    f3 qvec = cross3(tvec, e1);
    float vv = dot3(d, qvec) * inv;
    if (!(vv >= 0.0f) || uu + vv > 1.0f) return false;
    float tt = dot3(e2, qvec) * inv;
    if (!(tt > tmin && tt < tmax)) return false;
    t = tt; u = uu; v = vv;
    if (solution_consistent(o, d, v0, e1, e2, tt, uu, vv)) return true;
    return mt_binary64(o, d, v0, e1, e2, tmin, tmax, t, u, v);
}

// Moeller-Trumbore's comparisons without ray_triangle()'s early returns: the same operations in the same order on the same operands (a lane the
// branching form would have sent home early computes on and fails the same comparison at the end; det == 0 gives inf / NaN quotients, which fail
// every comparison, and is tested explicitly as well).  Used by the queue kernels' leaf stage, where the early returns buy nothing (some lane of
// the wave always goes on) and cost a second memory round trip: the compiler sinks the load of v0 behind the `det == 0` return, so every triangle
// test waited for memory twice.  true = a CANDIDATE; the caller accepts it if solution_consistent() and decides it again with mt_binary64() if not.
__device__ __forceinline__ bool mt_candidate(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float tmin, float tmax, float &t, float &u, float &v) {
    const f3 pvec = cross3(d, e2);
    const float det = dot3(e1, pvec);
    const float inv = 1.0f / det;
    const f3 tvec = o - v0;
    const float uu = dot3(tvec, pvec) * inv;
    const f3 qvec = cross3(tvec, e1);
    const float vv = dot3(d, qvec) * inv;
    const float tt = dot3(e2, qvec) * inv;
    t = tt; u = uu; v = vv;
    return det != 0.0f && uu >= 0.0f && !(uu > 1.0f) && vv >= 0.0f && !(uu + vv > 1.0f) && tt > tmin && tt < tmax;
}

// Slab test of one child box against [tmin, tlimit]; NaNs from 0 * inf drop out of fminf/fmaxf
// (IEEE minNum/maxNum), which can only enlarge the interval, i.e. stays conservative.
__device__ __forceinline__ bool box_test(float lox, float loy, float loz, float hix, float hiy, float hiz, f3 o, f3 inv,
                                         float tmin, float tlimit, float &tnear) {
    float t0 = (lox - o.x) * inv.x, t1 = (hix - o.x) * inv.x;
    float tn = fmaxf(tmin, fminf(t0, t1)), tf = fminf(tlimit, fmaxf(t0, t1));
    t0 = (loy - o.y) * inv.y; t1 = (hiy - o.y) * inv.y;
    tn = fmaxf(tn, fminf(t0, t1)); tf = fminf(tf, fmaxf(t0, t1));
    t0 = (loz - o.z) * inv.z; t1 = (hiz - o.z) * inv.z;
    tn = fmaxf(tn, fminf(t0, t1)); tf = fminf(tf, fmaxf(t0, t1));
    tnear = tn;
    return tn <= tf;
}

// "bvh_frame": what the slab tests see of a ray.  The boxes of all node forms live in the frame DeviceScene::frame (row i = axis i in world
// coordinates); a walker rotates origin and direction once per ray for them and intersects triangles in world space as ever (boxes only cull:
// the rotation's five roundings per coordinate, each 2^-24 of the WORLD magnitude, are what the frame's share of the boxes' padding -- 2^-18 of
// the tree's world magnitude, bvh_math.hpp -- is sized for).  frame_on is uniform: a scalar branch around 18 FMAs.
__device__ __forceinline__ f3 frame_rotate(const float *R, f3 p) {
    return f3{ (R[0] * p.x + R[1] * p.y) + R[2] * p.z, (R[3] * p.x + R[4] * p.y) + R[5] * p.z, (R[6] * p.x + R[7] * p.y) + R[8] * p.z };
}
__device__ __forceinline__ void box_ray(const DeviceScene &sc, f3 ro, f3 rd, f3 &bo, f3 &bd) {
    bo = ro; bd = rd;
    if (sc.frame_on) { bo = frame_rotate(sc.frame, ro); bd = frame_rotate(sc.frame, rd); }
}
// the bounds of a tile's ray origins in the frame: the box of the rotated box (centre R c, half extent |R| h -- a superset of the rotated origins)
__device__ __forceinline__ void box_bounds(const DeviceScene &sc, f3 &omin, f3 &omax) {
    if (!sc.frame_on || !(omin.x <= omax.x)) return;
    const float *R = sc.frame;
    const f3 c = f3{ 0.5f * omin.x + 0.5f * omax.x, 0.5f * omin.y + 0.5f * omax.y, 0.5f * omin.z + 0.5f * omax.z };
    const f3 h = f3{ (omax.x - c.x) * 1.000001f + 1e-6f, (omax.y - c.y) * 1.000001f + 1e-6f, (omax.z - c.z) * 1.000001f + 1e-6f };
    const f3 rc = frame_rotate(R, c);
    const f3 rh = f3{ (fabsf(R[0]) * h.x + fabsf(R[1]) * h.y) + fabsf(R[2]) * h.z, (fabsf(R[3]) * h.x + fabsf(R[4]) * h.y) + fabsf(R[5]) * h.z,
                      (fabsf(R[6]) * h.x + fabsf(R[7]) * h.y) + fabsf(R[8]) * h.z };
    omin = f3{ rc.x - rh.x, rc.y - rh.y, rc.z - rh.z };
    omax = f3{ rc.x + rh.x, rc.y + rh.y, rc.z + rh.z };
}

__device__ __forceinline__ void pixel_of_thread(uint32_t &x, uint32_t &y, uint32_t row_begin) {
    // 16x16 pixel tile per block; wave w covers the 8x8 sub-tile (w & 1, w >> 1)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
    y = row_begin + blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
}

// ---------------------------------------------------------------------------------------------
// image helpers (linear, row-major, tightly packed)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f4 load_rgba16f(const void *img, uint32_t W, uint32_t x, uint32_t y) {
    const uint2 raw = reinterpret_cast<const uint2 *>(img)[size_t(y) * W + x];
    return f4{ half_bits_to_float(uint16_t(raw.x & 0xffffu)), half_bits_to_float(uint16_t(raw.x >> 16)),
               half_bits_to_float(uint16_t(raw.y & 0xffffu)), half_bits_to_float(uint16_t(raw.y >> 16)) };
}
__device__ __forceinline__ void store_rgba16f(void *img, uint32_t W, uint32_t x, uint32_t y, float a, float b, float c, float d) {
    uint2 raw;
    raw.x = uint32_t(float_to_half_bits(a)) | (uint32_t(float_to_half_bits(b)) << 16);
    raw.y = uint32_t(float_to_half_bits(c)) | (uint32_t(float_to_half_bits(d)) << 16);
    reinterpret_cast<uint2 *>(img)[size_t(y) * W + x] = raw;
}
__device__ __forceinline__ void store_rg16f(void *img, uint32_t W, uint32_t x, uint32_t y, float a, float b) {
    reinterpret_cast<uint32_t *>(img)[size_t(y) * W + x] =
        uint32_t(float_to_half_bits(a)) | (uint32_t(float_to_half_bits(b)) << 16);
}
__device__ __forceinline__ uint32_t unorm8(float f) { return uint32_t(fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f + 0.5f); }
__device__ __forceinline__ uint8_t srgb8(float c) {       // sRGB attachment store: NaN -> 0, clamp, encode, round
    if (!(c > 0.0f)) return 0;
    if (c >= 1.0f) return 255;
    const float e = c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f;
    return uint8_t(e * 255.0f + 0.5f);
}

// glsl_common.h:118-122
__device__ __forceinline__ f3 get_world_space_position(const vhr_per_frame_data &pfd, float depth, float u, float v) {
    const f4 r = mat4_mul(pfd.camera_viewproj_inverse, f4{ u * 2.0f - 1.0f, v * 2.0f - 1.0f, depth, 1.0f });
    return f3{ r.x / r.w, r.y / r.w, r.z / r.w };
}

// ---------------------------------------------------------------------------------------------
// texture(): LOD 0, per-texture sampler, software bilinear (float tolerance, not bit-exact)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int wrap_coord(int i, int n, int mode) {
    if (mode == 2) return min(max(i, 0), n - 1);
    if (mode == 1) {
        const int p = 2 * n;
        int m = i % p;
        if (m < 0) m += p;
        return m < n ? m : p - 1 - m;
    }
    int m = i % n;
    if (m < 0) m += n;
    return m;
}
__device__ __forceinline__ f4 fetch_texel(const DeviceTexture &t, int x, int y) {
    const uchar4 p = reinterpret_cast<const uchar4 *>(t.texels)[size_t(y) * t.width + x];
    f4 r;
    if (t.format == VHR_FORMAT_R8G8B8A8_SRGB) { r.x = c_srgb_lut[p.x]; r.y = c_srgb_lut[p.y]; r.z = c_srgb_lut[p.z]; }
    else { r.x = p.x * (1.0f / 255.0f); r.y = p.y * (1.0f / 255.0f); r.z = p.z * (1.0f / 255.0f); }
    r.w = p.w * (1.0f / 255.0f);
    return r;
}
__device__ f4 sample_texture(const DeviceScene &sc, int idx, float u, float v) {
    if (idx < 0 || uint32_t(idx) >= sc.texture_count) return f4{ 0, 0, 0, 0 };
    const DeviceTexture t = sc.textures[idx];
    float x = u * float(t.width), y = v * float(t.height);
    if (t.mag_filter == 0)
        return fetch_texel(t, wrap_coord(int(floorf(x)), int(t.width), t.address_u), wrap_coord(int(floorf(y)), int(t.height), t.address_v));
    x -= 0.5f; y -= 0.5f;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float fx = x - fx0, fy = y - fy0;
    const int x0 = wrap_coord(int(fx0), int(t.width), t.address_u), x1 = wrap_coord(int(fx0) + 1, int(t.width), t.address_u);
    const int y0 = wrap_coord(int(fy0), int(t.height), t.address_v), y1 = wrap_coord(int(fy0) + 1, int(t.height), t.address_v);
    const f4 a = fetch_texel(t, x0, y0), b = fetch_texel(t, x1, y0), c = fetch_texel(t, x0, y1), d = fetch_texel(t, x1, y1);
    f4 r;
    r.x = (a.x * (1.0f - fx) + b.x * fx) * (1.0f - fy) + (c.x * (1.0f - fx) + d.x * fx) * fy;
    r.y = (a.y * (1.0f - fx) + b.y * fx) * (1.0f - fy) + (c.y * (1.0f - fx) + d.y * fx) * fy;
    r.z = (a.z * (1.0f - fx) + b.z * fx) * (1.0f - fy) + (c.z * (1.0f - fx) + d.z * fx) * fy;
    r.w = (a.w * (1.0f - fx) + b.w * fx) * (1.0f - fy) + (c.w * (1.0f - fx) + d.w * fx) * fy;
    return r;
}

// vertex K of triangle `tri` of a primitive, and a hit's uv0 as the shaders interpolate it (shadow_anyhit.rahit:19-20,
// reflection_hit.rchit:21-22): barycentrics (1 - u - v, u, v), the products summed left to right
template <int K> __device__ __forceinline__ const vhr_vertex &tri_vertex(const DeviceScene &sc, const vhr_primitive &prim, uint32_t tri) {
    return sc.vertices[prim.vertex_offset + sc.indices[prim.index_offset + 3 * tri + K]];
}
struct Uv0 { float x, y; };
__device__ __forceinline__ Uv0 interpolate_uv0(const DeviceScene &sc, const vhr_primitive &prim, uint32_t tri, float u, float v) {
    const vhr_vertex &a = tri_vertex<0>(sc, prim, tri), &b = tri_vertex<1>(sc, prim, tri), &c = tri_vertex<2>(sc, prim, tri);
    const float bx = 1.0f - u - v, by = u, bz = v;
    return Uv0{ a.uv0[0] * bx + b.uv0[0] * by + c.uv0[0] * bz, a.uv0[1] * bx + b.uv0[1] * by + c.uv0[1] * bz };
}

// shadow_anyhit.rahit:8-27: true = ignoreIntersectionEXT.  textures[-1] (no base colour texture) reads (0, 0, 0, 0)
// (decision ix of the oracle; out of bounds in the reference).
__device__ bool alpha_ignored(const DeviceScene &sc, uint32_t tri_index, float u, float v) {
    const BvhTri &bt = sc.tris[tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];                                  // rahit:9
    if (prim.material.alpha_mask != 1) return false;                                     // rahit:24 (the texture fetch has no other effect)
    const Uv0 uv = interpolate_uv0(sc, prim, bt.tri, u, v);                              // rahit:19-20
    const f4 albedo = sample_texture(sc, prim.material.base_color_texture, uv.x, uv.y);  // rahit:23
    return albedo.w < prim.material.alpha_cutoff;                                        // rahit:24-26
}

// gbuf.frag:20-32 evaluated at a candidate hit: true = the G-buffer pass would discard the fragment, so the surface has a hole there and the
// candidate does not exist for a ray that is to see what the raster pass drew ("alpha_test_rays", VHR_RAY_QUERY_ALPHA_TEST).  uv0 is
// interpolated as shadow_anyhit.rahit:19-20 does; an untextured primitive's albedo is its base colour (the rahit reads textures[-1] there and
// has no `a == 0` clause: alpha_ignored above keeps that rule for the raytraced path).  A pure function of (triangle, u, v).
__device__ bool gbuf_discarded(const DeviceScene &sc, uint32_t tri_index, float u, float v) {
    const BvhTri &bt = sc.tris[tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];
    float alpha = prim.material.base_color[3];                                           // gbuf.frag:19-26
    if (prim.material.base_color_texture != -1) {
        // interpolate_uv0, spelled out: through the helper the compiler orders this block differently in every kernel that inlines it, and two
        // queue kernels' statistics builds spill differently (profiles/filter_protocol_resources.txt)
        const vhr_vertex &a = sc.vertices[prim.vertex_offset + sc.indices[prim.index_offset + 3 * bt.tri + 0]];
        const vhr_vertex &b = sc.vertices[prim.vertex_offset + sc.indices[prim.index_offset + 3 * bt.tri + 1]];
        const vhr_vertex &c = sc.vertices[prim.vertex_offset + sc.indices[prim.index_offset + 3 * bt.tri + 2]];
        const float bx = 1.0f - u - v, by = u, bz = v;                                   // rahit:19
        const float uvx = a.uv0[0] * bx + b.uv0[0] * by + c.uv0[0] * bz;                 // rahit:20
        const float uvy = a.uv0[1] * bx + b.uv0[1] * by + c.uv0[1] * bz;
        alpha = sample_texture(sc, prim.material.base_color_texture, uvx, uvy).w;
    }
    return (prim.material.alpha_mask == 1 && alpha < prim.material.alpha_cutoff) || alpha == 0.0f;   // gbuf.frag:27-32
}

// ---------------------------------------------------------------------------------------------
// Candidate filters.  Both walkers (traverse<> below, wave_queue_walk<> in trace_queue.hpp) decide a leaf's triangle in three steps: the
// triangle test with decision (vi) says whether the ray has a candidate at (t, u, v); the ray's filter says whether that candidate exists
// for this ray; what is left is committed (any hit: the ray ends; closest hit: min t, then the smaller flat index).  A filter is a trivially
// copyable callable with one call shape,
//     bool operator()(uint32_t ray, uint32_t tri, float u, float v) const      // true: the candidate does not exist for this ray
// `ray` is what the walk's fetch gave for the lane's ray (wave_queue_walk: pix; traverse<>: its trailing argument, 0 unless the caller says
// otherwise), `tri` the triangle's index in sc.tris, (u, v) the candidate's barycentrics.  The one thing a walker asks of the type is whether it is
// NoFilter, which costs no code.  (The features that brought the filters: DESIGN.md 4b, 4c.)
// ---------------------------------------------------------------------------------------------
struct NoFilter { __device__ __forceinline__ bool operator()(uint32_t, uint32_t, float, float) const { return false; } };
// the raytraced path's gl_RayFlagsNoOpaqueEXT rays (raygen_test_alpha.rgen:20, closesthit_test_alpha.rchit:42): shadow_anyhit.rahit
struct RahitAlpha {
    const DeviceScene *sc;
    __device__ __forceinline__ bool operator()(uint32_t, uint32_t tri, float u, float v) const { return alpha_ignored(*sc, tri, u, v); }
};
// the hybrid path's rays and the ray query with their alpha test on: what the G-buffer pass discards
struct GbufDiscard {
    const DeviceScene *sc;
    __device__ __forceinline__ bool operator()(uint32_t, uint32_t tri, float u, float v) const { return gbuf_discarded(*sc, tri, u, v); }
};

// Ray cull masks (vhr_set_primitive_masks, vhr_ray_query_masked, the "*_ray_mask" options): a candidate on primitive p does not exist for a
// ray of mask m iff (masks[p] & m) == 0 -- VkAccelerationStructureInstanceKHR::mask against traceRayEXT's cullMask, per geometry.  The kernels
// that filter carry this in their launch arguments (RaygenArgs, RayQueryArgs), never in DeviceScene.
struct RayMaskArgs {
    const uint8_t *prim_masks;            // one byte per primitive (never null in a launch that filters)
    uint32_t shadow, ao, reflection;      // the hybrid path's class masks; the ray query: `shadow` = its cull_mask
    uint32_t alpha;                       // wave-uniform: the alpha rule (gbuf_discarded) applies as well, behind the mask test
};
// the mask test, then (by the runtime bit) the alpha rule.  Where the launch has per-ray masks (the batched query: ray_masks != nullptr)
// the ray id picks the ray's own, read at the candidate.
struct RayMaskReject {
    const DeviceScene *sc;
    const uint8_t *prim_masks, *ray_masks;
    uint32_t mask, alpha;
    __device__ __forceinline__ bool operator()(uint32_t ray, uint32_t tri, float u, float v) const {
        const uint32_t m = ray_masks ? uint32_t(ray_masks[ray]) & mask : mask;
        if ((uint32_t(prim_masks[sc->tris[tri].prim]) & m) == 0u) return true;
        return alpha != 0u && gbuf_discarded(*sc, tri, u, v);
    }
};
// Ray face culling (vhr_ray_query_faces; gl_RayFlagsCullBackFacingTrianglesEXT / CullFrontFacing): a candidate on a triangle that faces away from
// (VHR_FACE_CULL_BACK) or towards (VHR_FACE_CULL_FRONT) the ray does not exist for it.  What RayMaskReject carries, plus the primitives' flip
// bytes, the cull mode (wave-uniform) and the rays array: the ray id picks the ray's direction, read at the candidate as its mask is, and the
// record's edges are read again by the triangle's index -- nothing of the face rule is alive in the walk's box loop.  The mask test (runtime:
// only where the mask acts, prim_masks != nullptr), then the face test (ray_facing.hpp: the binary64 determinant's sign), then the alpha rule
// (runtime bit): one instantiation serves face + mask + alpha.  The ray query's kernels only (kFilterFace); no render path culls faces.
struct RayFaceReject {
    const DeviceScene *sc;
    const uint8_t *prim_masks, *ray_masks, *flips;
    const float4 *rays;                   // 2 x float4 per ray, as RayQueryArgs::rays
    uint32_t mask, alpha, cull;
    __device__ __forceinline__ bool operator()(uint32_t ray, uint32_t tri, float u, float v) const {
        const BvhTri &bt = sc->tris[tri];
        if (prim_masks) {
            const uint32_t m = ray_masks ? uint32_t(ray_masks[ray]) & mask : mask;
            if ((uint32_t(prim_masks[bt.prim]) & m) == 0u) return true;
        }
        if (cull != kFaceCullNone) {
            const float4 q = rays[size_t(ray) * 2u + 1u];
            const FacingPvec p = facing_pvec(q.x, q.y, q.z, bt.e2[0], bt.e2[1], bt.e2[2]);
            asm volatile("" ::: "memory");            // e1 and the flip byte are fetched behind the cross product, not held through it
            const bool front = facing_front(p, bt.e1[0], bt.e1[1], bt.e1[2], flips[bt.prim] != 0);
            if (ray_face_culled(cull, front)) return true;
        }
        return alpha != 0u && gbuf_discarded(*sc, tri, u, v);
    }
};
// the hybrid path's and the ray query's kernels name their filter by a launch-side constant: none, the alpha rule, or the mask (with the
// alpha rule as a runtime bit); the ray query alone has a fourth, the face rule (with the mask and the alpha rule as runtime bits), which it
// constructs itself (kernels_ray_query.hip): ray_filter<> and with_filter() below know the first three
constexpr int kFilterNone = 0, kFilterAlpha = 1, kFilterMask = 2, kFilterFace = 3;
template <int FILTER> using RayFilter = std::conditional_t<FILTER == kFilterMask, RayMaskReject, std::conditional_t<FILTER == kFilterAlpha, GbufDiscard, NoFilter>>;
template <int FILTER> __device__ __forceinline__ RayFilter<FILTER> ray_filter(const DeviceScene &sc, const RayMaskArgs &m, uint32_t ray_mask,
                                                                             const uint8_t *ray_masks = nullptr) {
    if constexpr (FILTER == kFilterMask) return RayMaskReject{ &sc, m.prim_masks, ray_masks, ray_mask, m.alpha };
    else if constexpr (FILTER == kFilterAlpha) return GbufDiscard{ &sc };
    else return NoFilter{};
}

// Per-lane BVH2 walk with the traversal stack in LDS (stack[level * kTraceBlock + thread]: conflict free; STRIDE 1: a private array).
// ANY_HIT: gl_RayFlagsTerminateOnFirstHitEXT | SkipClosestHitShader (raygen.rgen:39,51) -- returns at the
// first accepted triangle; the boolean result does not depend on the visiting order.
// !ANY_HIT: closest hit = min t, ties broken by the smaller flat triangle index; subtrees are pruned with
// tnear > best t only (strict), so equal-t candidates are always examined.
// Leaf: ray_triangle (the triangle test with decision (vi) inline), then filter(ray, triangle, u, v), then the commit.
template <bool ANY_HIT, int STRIDE = kTraceBlock, typename Filter = NoFilter>
__device__ __forceinline__ bool traverse(const DeviceScene &sc, f3 o, f3 d, float tmin, float tmax, int *stack, Hit &best,
                                         uint32_t &overflow, Filter filter = Filter{}, uint32_t ray = 0) {
    if (sc.node_count == 0) return false;
    f3 bo, bd;
    box_ray(sc, o, d, bo, bd);                                  // "bvh_frame": the slab tests' ray; the triangle tests below keep (o, d)
    const f3 inv = f3{ 1.0f / bd.x, 1.0f / bd.y, 1.0f / bd.z };
    bool found = false;
    float tbest = tmax;
    int sp = 0;
    int cur = 0;
    for (;;) {
        if (cur >= 0) {
            const float4 *np = reinterpret_cast<const float4 *>(sc.nodes + cur);
            const float4 q0 = np[0], q1 = np[1], q2 = np[2];
            const int4 q3 = reinterpret_cast<const int4 *>(np)[3];
            float tn0, tn1;
            const bool h0 = box_test(q0.x, q0.z, q1.x, q0.y, q0.w, q1.y, bo, inv, tmin, tbest, tn0);
            const bool h1 = box_test(q1.z, q2.x, q2.z, q1.w, q2.y, q2.w, bo, inv, tmin, tbest, tn1);
            if (h0 && h1) {
                const bool first0 = tn0 <= tn1;
                const int nearc = first0 ? q3.x : q3.y, farc = first0 ? q3.y : q3.x;
                if (sp < kTraceStack) { stack[sp * STRIDE] = farc; ++sp; } else { overflow = 1; }
                cur = nearc;
                continue;
            }
            if (h0) { cur = q3.x; continue; }
            if (h1) { cur = q3.y; continue; }
        } else {
            const uint32_t v = ~uint32_t(cur);
            const uint32_t first = v >> 2, count = (v & 3u) + 1u;
            for (uint32_t i = 0; i < count; ++i) {
                const float4 *tp = reinterpret_cast<const float4 *>(sc.tris + first + i);
                const float4 a = tp[0], b = tp[1];
                const float4 c = tp[2];
                float t, u, w;
                if (ray_triangle(o, d, f3{ a.x, a.y, a.z }, f3{ a.w, b.x, b.y }, f3{ b.z, b.w, c.x }, tmin, tmax, t, u, w)) {
                    if constexpr (!std::is_same_v<Filter, NoFilter>) { if (filter(ray, first + i, u, w)) continue; }
                    if (ANY_HIT) return true;
                    const uint32_t flat = __float_as_uint(c.w);
                    if (!found || t < best.t || (t == best.t && flat < best.flat)) {
                        found = true;
                        best.t = t; best.u = u; best.v = w; best.tri_index = first + i; best.flat = flat;
                        tbest = t;
                    }
                }
            }
        }
        if (sp == 0) break;
        --sp;
        cur = stack[sp * STRIDE];
    }
    return found;
}

// ---------------------------------------------------------------------------------------------
// K2: reflection_hit.rchit:10-72
// ---------------------------------------------------------------------------------------------
struct TriAttributes { float uvx, uvy; f3 normal; f3 object_pos; };

__device__ __forceinline__ TriAttributes interpolate(const DeviceScene &sc, const vhr_primitive &prim, uint32_t tri, float u, float v) {
    const uint32_t i0 = sc.indices[prim.index_offset + 3 * tri + 0];
    const uint32_t i1 = sc.indices[prim.index_offset + 3 * tri + 1];
    const uint32_t i2 = sc.indices[prim.index_offset + 3 * tri + 2];
    const vhr_vertex &a = sc.vertices[prim.vertex_offset + i0];
    const vhr_vertex &b = sc.vertices[prim.vertex_offset + i1];
    const vhr_vertex &c = sc.vertices[prim.vertex_offset + i2];
    const float bx = 1.0f - u - v, by = u, bz = v;                                     // rchit:21
    TriAttributes r;
    r.uvx = a.uv0[0] * bx + b.uv0[0] * by + c.uv0[0] * bz;                             // rchit:22
    r.uvy = a.uv0[1] * bx + b.uv0[1] * by + c.uv0[1] * bz;
    r.normal = f3{ a.normal[0] * bx + b.normal[0] * by + c.normal[0] * bz,            // rchit:23 (object space)
                   a.normal[1] * bx + b.normal[1] * by + c.normal[1] * bz,
                   a.normal[2] * bx + b.normal[2] * by + c.normal[2] * bz };
    r.object_pos = f3{ a.pos[0] * bx + b.pos[0] * by + c.pos[0] * bz, a.pos[1] * bx + b.pos[1] * by + c.pos[1] * bz,
                       a.pos[2] * bx + b.pos[2] * by + c.pos[2] * bz };
    return r;
}

// gbuf.vert:21 passes the vertex tangent through; the rasteriser interpolates it like the normal
__device__ __forceinline__ f4 interpolate_tangent(const DeviceScene &sc, const vhr_primitive &prim, uint32_t tri, float u, float v) {
    const vhr_vertex &a = tri_vertex<0>(sc, prim, tri), &b = tri_vertex<1>(sc, prim, tri), &c = tri_vertex<2>(sc, prim, tri);
    const float bx = 1.0f - u - v, by = u, bz = v;
    return f4{ a.tangent[0] * bx + b.tangent[0] * by + c.tangent[0] * bz, a.tangent[1] * bx + b.tangent[1] * by + c.tangent[1] * bz,
               a.tangent[2] * bx + b.tangent[2] * by + c.tangent[2] * bz, a.tangent[3] * bx + b.tangent[3] * by + c.tangent[3] * bz };
}

// second_bounce (may be nullptr): the documented 2-bounce extension (BASELINE config 5; the reference traces one bounce and
// declares recursion depth 2, pipeline.cpp:285): the payload of a mirror ray traced from this hit replaces / blends into the
// specular term exactly like composition.frag:141-149 blends the first bounce at the primary hit.  hit_position / hit_normal
// (optional) return the world-space hit point and the shader's N for the caller to build that ray.
__device__ f4 shade_reflection_hit(const DeviceScene &sc, const vhr_per_frame_data &pfd, const Hit &h, const f4 *second_bounce = nullptr,
                                   f3 *hit_position = nullptr, f3 *hit_normal = nullptr) {
    const BvhTri &bt = sc.tris[h.tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];                                 // rchit:11
    const TriAttributes at = interpolate(sc, prim, bt.tri, h.u, h.v);
    const f3 position = mat4_mul_point(prim.transform, at.object_pos);                  // rchit:24
    f3 albedo;
    if (prim.material.base_color_texture == -1) {                                       // rchit:27-32
        albedo = f3{ prim.material.base_color[0], prim.material.base_color[1], prim.material.base_color[2] };
    } else {
        const f4 t = sample_texture(sc, prim.material.base_color_texture, at.uvx, at.uvy);
        albedo = f3{ t.x, t.y, t.z };
    }
    float metallic = prim.material.metallic_factor, roughness = prim.material.roughness_factor;
    if (prim.material.metallic_roughness_texture != -1) {                               // rchit:35-39
        const f4 mr = sample_texture(sc, prim.material.metallic_roughness_texture, at.uvx, at.uvy);
        metallic *= mr.y;
        roughness *= mr.z;
    }
    const f3 cam = f3{ pfd.camera_view_inverse[12], pfd.camera_view_inverse[13], pfd.camera_view_inverse[14] };
    const f3 V = normalize3(cam - position);                                            // rchit:42
    const f3 L = -f3{ pfd.directional_light.direction[0], pfd.directional_light.direction[1], pfd.directional_light.direction[2] };
    const f3 N = at.normal;                                                             // rchit:44 (not normalised)
    const f3 H = normalize3(L + V);
    roughness = fminf(fmaxf(roughness, 0.04f), 1.0f);                                   // rchit:53-55
    metallic = fminf(fmaxf(metallic, 0.0f), 1.0f);
    const float ambient_factor = VHR_PI_INVERSE * 0.2f;                                 // rchit:59
    const f3 li = f3{ pfd.directional_light.intensity[0], pfd.directional_light.intensity[1], pfd.directional_light.intensity[2] };
    const f3 lc = f3{ pfd.directional_light.color[0], pfd.directional_light.color[1], pfd.directional_light.color[2] };
    const f3 f0 = f3{ 0.04f * (1.0f - metallic) + albedo.x * metallic, 0.04f * (1.0f - metallic) + albedo.y * metallic,
                      0.04f * (1.0f - metallic) + albedo.z * metallic };                // rchit:63-64
    const f3 F = fresnel_schlick(f0, H, V);
    const f3 ambient = albedo * ambient_factor;                                         // rchit:67
    const f3 dp = f3{ (1.0f - F.x) * (1.0f - metallic), (1.0f - F.y) * (1.0f - metallic), (1.0f - F.z) * (1.0f - metallic) };
    const f3 diffuse = f3{ dp.x * albedo.x / VHR_PI, dp.y * albedo.y / VHR_PI, dp.z * albedo.z / VHR_PI };
    const float dg = D_GGX(roughness, N, H) * G_GGX(roughness, N, V, L);
    const float denom = 4.0f * fmaxf(dot3(N, V), 0.0f) * fmaxf(dot3(N, L), 0.0f);
    const float invd = 1.0f / fmaxf(denom, 1e-6f);
    const f3 specular = f3{ dg * F.x * invd, dg * F.y * invd, dg * F.z * invd };
    const float nl = fmaxf(dot3(N, L), 0.0f);
    if (hit_position) *hit_position = position;
    if (hit_normal) *hit_normal = N;
    if (second_bounce) {
        const f3 dl = mul3(mul3(diffuse * nl, li), lc);                                 // composition.frag:138 without the shadow factor
        f3 sl = mul3(mul3(specular * nl, li), lc);                                      // :139
        const f3 refl = f3{ second_bounce->x, second_bounce->y, second_bounce->z };
        if (metallic == 1.0f) sl = refl;                                                // :141-149
        else sl = f3{ sl.x * (1.0f - roughness) + refl.x * roughness, sl.y * (1.0f - roughness) + refl.y * roughness,
                      sl.z * (1.0f - roughness) + refl.z * roughness };
        const f3 lighting2 = (ambient + dl) + sl;                                       // :160
        return f4{ lighting2.x, lighting2.y, lighting2.z, 1.0f };
    }
    const f3 lit = mul3(mul3((diffuse + specular) * nl, li), lc);                       // rchit:70
    const f3 lighting = ambient + lit;
    return f4{ lighting.x, lighting.y, lighting.z, 1.0f };
}

// world-space hit point and the shader's N of reflection_hit.rchit:11-24,44 (what shade_reflection_hit returns through
// hit_position / hit_normal, without the shading)
__device__ __forceinline__ void hit_position_normal(const DeviceScene &sc, const Hit &h, f3 &position, f3 &normal) {
    const BvhTri &bt = sc.tris[h.tri_index];
    const vhr_primitive &prim = sc.primitives[bt.prim];
    const TriAttributes at = interpolate(sc, prim, bt.tri, h.u, h.v);
    position = mat4_mul_point(prim.transform, at.object_pos);
    normal = at.normal;
}

// The mirror ray of raygen.rgen:59-65 with the optional second bounce: a mirror ray from the first hit about the shader's N
// (normalised, facing the incoming ray), origin biased like raygen.rgen:29, shaded by reflection_hit.rchit without recursion.
// `filter` ("alpha_test_rays": GbufDiscard; "reflection_ray_mask": RayMaskReject): both bounces skip the candidates it names.
template <int STRIDE = kTraceBlock, typename Filter = NoFilter>
__device__ __forceinline__ f4 trace_reflection(const DeviceScene &sc, const vhr_per_frame_data &pfd, const vhr_trace_params &tp, f3 origin,
                                               f3 rdir, int *stack, uint32_t &overflow, bool &second_ray, Filter filter = Filter{}) {
    Hit hit;
    second_ray = false;
    if (!traverse<false, STRIDE>(sc, origin, rdir, tp.tmin, tp.tmax, stack, hit, overflow, filter)) return f4{ 0.0f, 0.0f, 0.0f, 0.0f };   // reflection_miss.rmiss:7
    if (tp.reflections < 2) return shade_reflection_hit(sc, pfd, hit);
    f3 hp, hn;
    (void)shade_reflection_hit(sc, pfd, hit, nullptr, &hp, &hn);
    const f3 nn = normalize3(hn);
    const float ni = dot3(nn, rdir);
    const f3 nf = ni < 0.0f ? nn : -nn;
    const f3 d2 = rdir - nn * (2.0f * ni);
    const f3 o2 = hp + nf * tp.normal_bias;
    second_ray = true;
    Hit hit2;
    f4 second = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
    if (traverse<false, STRIDE>(sc, o2, d2, tp.tmin, tp.tmax, stack, hit2, overflow, filter)) second = shade_reflection_hit(sc, pfd, hit2);
    return shade_reflection_hit(sc, pfd, hit, &second);
}

// ---------------------------------------------------------------------------------------------
// host: 4x4 matrices as the launchers need them (column major, like PerFrameData)
// ---------------------------------------------------------------------------------------------
static void host_mat4_mul(const float *a, const float *b, float *out) {
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < 4; ++i)
            out[c * 4 + i] = ((a[0 * 4 + i] * b[c * 4 + 0] + a[1 * 4 + i] * b[c * 4 + 1]) + a[2 * 4 + i] * b[c * 4 + 2]) + a[3 * 4 + i] * b[c * 4 + 3];
}

// general 4x4 inverse by cofactors in double, rounded once (the light's projview has no inverse in PerFrameData)
static bool host_mat4_inverse(const float *m, float *out) {
    double a[16], inv[16];
    for (int i = 0; i < 16; ++i) a[i] = double(m[i]);
    inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
    inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
    inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
    inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
    inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
    inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
    inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
    inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
    inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
    inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
    inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
    inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
    inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
    inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
    inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
    inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
    const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
    if (det == 0.0) return false;
    for (int i = 0; i < 16; ++i) out[i] = float(inv[i] / det);
    return true;
}

}  // namespace vhr
