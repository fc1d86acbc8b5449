// K0: the arithmetic both builders share -- the one definition of a leaf record, its box, a padded slot, a leaf link, the three derived
// node forms, their containment checks, the refit's own check, the scene centre and the surface-area term.
//
// The host builder (bvh_build.cpp) and the device builder (kernels_bvh.hip, with its refits in kernels_bvh_refit.hip) owe each other BITS: the
// same records, the same child boxes, the same tree fingerprint, the same derived forms.  Every function here is `__host__ __device__ inline`
// over plain arrays and the structs of vhr_internal.hpp, both sides are compiled without FMA contraction, and neither keeps a copy of any of it.  The one place the two
// sides have different bodies is the float -> half conversion (half_nearest / half_upward): the device uses the hardware's, the host a
// software one with the same rounding -- nearest-even, ties included ("one definition of the BVH arithmetic").
#pragma once

#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "vhr_internal.hpp"
#include "bvh_frame.hpp"

namespace vhr {
namespace bvh_math {

#define VHR_BM __host__ __device__ inline

// ---- leaf links: child < 0 is a leaf, ~child = (first record << 2) | (records - 1) ----
VHR_BM int32_t leaf_link(uint32_t first, uint32_t count) { return ~int32_t((first << 2) | (count - 1u)); }
VHR_BM uint32_t leaf_first(int32_t link) { return ~uint32_t(link) >> 2; }
VHR_BM uint32_t leaf_count(int32_t link) { return (~uint32_t(link) & 3u) + 1u; }
// an inner link of the 48- and 32-byte forms is a BYTE offset (index * sizeof(Node)): the walkers add it to the base address as it is
template <typename Node>
VHR_BM int32_t link_as_offset(int32_t link) { return link >= 0 ? link * int32_t(sizeof(Node)) : link; }
// a one-leaf scene: child 1 is a copy of child 0 behind an inverted box, and nothing ever enters or refits it
VHR_BM bool absent_child1(const BvhNode &nd, bool single) { return single && nd.child1 == nd.child0; }

// ---- records ----
// One world-space Moeller-Trumbore record from its primitive's transform and its three corners: transform * vec4(pos, 1), columns
// accumulated left to right, every product and sum rounded on its own; e1 = w1 - w0, e2 = w2 - w0.  Part of the bit-exact visibility
// contract ("exact arithmetic").  Returns the number of non-finite coordinates in the record.
VHR_BM uint32_t world_record(const float m[16], const float *p0, const float *p1, const float *p2, float v0[3], float e1[3], float e2[3]) {
    const float *p[3] = { p0, p1, p2 };
    float w[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *v = p[c];
        w[c][0] = ((m[0] * v[0] + m[4] * v[1]) + m[8] * v[2]) + m[12];
        w[c][1] = ((m[1] * v[0] + m[5] * v[1]) + m[9] * v[2]) + m[13];
        w[c][2] = ((m[2] * v[0] + m[6] * v[1]) + m[10] * v[2]) + m[14];
    }
    uint32_t bad = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v0[a] = w[0][a];
        e1[a] = w[1][a] - w[0][a];
        e2[a] = w[2][a] - w[0][a];
        bad += uint32_t(!__builtin_isfinite(v0[a])) + uint32_t(!__builtin_isfinite(e1[a])) + uint32_t(!__builtin_isfinite(e2[a]));
    }
    return bad;
}

// ---- boxes ----
VHR_BM void grow(float lo[3], float hi[3], const float olo[3], const float ohi[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], olo[a]); hi[a] = fmaxf(hi[a], ohi[a]); }
}
// the unpadded box of what the walkers intersect -- the corners v0, v0 + e1, v0 + e2 -- on the world axes or in the tree's frame
VHR_BM void record_box(const BvhTri &t, const float frame[9], bool frame_on, float lo[3], float hi[3]) {
    if (frame_on) {
        bvh_frame::box_in_frame(frame, t, lo, hi);
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p1 = t.v0[a] + t.e1[a], p2 = t.v0[a] + t.e2[a];
        lo[a] = fminf(fminf(t.v0[a], p1), p2);
        hi[a] = fmaxf(fmaxf(t.v0[a], p1), p2);
    }
}
// the unpadded box of a leaf: the union of its records' boxes
VHR_BM void leaf_box(int32_t link, const BvhTri *tris, const float frame[9], bool frame_on, float lo[3], float hi[3]) {
    const uint32_t first = leaf_first(link), count = leaf_count(link);
    record_box(tris[first], frame, frame_on, lo, hi);
    for (uint32_t i = 1; i < count; ++i) {
        float olo[3], ohi[3];
        record_box(tris[first + i], frame, frame_on, olo, ohi);
        grow(lo, hi, olo, ohi);
    }
}
// A child box as its parent stores it, (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z), with the conservative padding: box culling must never change
// which triangles are accepted.  frame_pad: frame_pad_of(the tree's world magnitude) in a frame, 0 on the world axes (x + 0 = x: the
// world-axes slots keep their bits).
VHR_BM void pad_slot(const float lo[3], const float hi[3], float frame_pad, float slot[6]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pad = (1e-3f + 1e-5f * fmaxf(fabsf(lo[a]), fabsf(hi[a]))) + frame_pad;
        slot[2 * a] = lo[a] - pad;
        slot[2 * a + 1] = hi[a] + pad;
    }
}
// ---- the frame's padding ----
// In a frame a box coordinate near 0 can come from world coordinates of any size, and the roundings of bvh_frame::rotate() -- the builder's on
// the corners, the walker's on the ray (box_ray) -- are relative to the WORLD magnitude W, not to the frame coordinate 1e-5 |x| pads by.  With
// every |world coordinate| <= W: the builder's corner sum and rotation 6 sqrt(3) 2^-24 W, the walker's origin 5 sqrt(3) 2^-24 W, its direction
// over t <= 2 sqrt(3) W inside the scene 30 * 2^-24 W, the slab products 3 * 2^-24 |face - origin| <= 6 sqrt(3) 2^-24 W: together below
// 60 * 2^-24 W, which 2^-18 W covers.  W is fixed when the tree is built -- the power of two at or above twice the largest |coordinate| of the
// records' corners -- so that a refit of either kind pads as the build did; a refit whose records leave W fails like one that meets a
// non-finite coordinate (coordinates_beyond), and the caller rebuilds.
constexpr float kFramePadFactor = 1.0f / 262144.0f;          // 2^-18
VHR_BM float frame_pad_of(float magnitude) { return magnitude * kFramePadFactor; }
// the largest |coordinate| of a record's three corners as record_box meets them (0 for a non-finite one: world_record has counted it)
VHR_BM float record_magnitude(const BvhTri &t) {
    float m = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float c[3] = { t.v0[a], t.v0[a] + t.e1[a], t.v0[a] + t.e2[a] };
#pragma unroll
        for (int k = 0; k < 3; ++k) if (__builtin_isfinite(c[k])) m = fmaxf(m, fabsf(c[k]));
    }
    return m;
}
// W from the largest |coordinate| of all records: the power of two >= 2 * largest (0 for an empty or all-zero scene; at most 2^127)
VHR_BM float frame_magnitude_of(float largest) {
    if (!(largest > 0.0f)) return 0.0f;
    uint32_t bits;
    memcpy(&bits, &largest, 4);
    uint32_t e = (bits >> 23) + ((bits & 0x7fffffu) ? 2u : 1u);          // exponent field of the power of two >= 2 * largest
    if (e < 1u) e = 1u;
    if (e > 254u) e = 254u;
    bits = e << 23;
    float w;
    memcpy(&w, &bits, 4);
    return w;
}
// finite corner coordinates of a record beyond the tree's world magnitude (a tree on the world axes has none: its padding does not depend on W)
VHR_BM uint32_t coordinates_beyond(const float v0[3], const float e1[3], const float e2[3], float magnitude, bool frame_on) {
    if (!frame_on) return 0u;
    uint32_t n = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float c[3] = { v0[a], v0[a] + e1[a], v0[a] + e2[a] };
#pragma unroll
        for (int k = 0; k < 3; ++k) n += uint32_t(__builtin_isfinite(c[k]) && fabsf(c[k]) > magnitude);
    }
    return n;
}
// One node of a refit: its children's unpadded boxes (a leaf's from its records, an inner child's from `self_box`, six floats per node, lo
// then hi, filled for every node below this one) padded into its two slots (frame_pad: pad_slot's); mine = its own unpadded box, for its
// parent.  Links are read, never written.
VHR_BM void refit_slots(BvhNode &nd, bool single, const BvhTri *tris, const float *self_box, const float frame[9], bool frame_on, float frame_pad, float mine_lo[3], float mine_hi[3]) {
    auto child_box = [&](int32_t link, float lo[3], float hi[3]) {
        if (link < 0) { leaf_box(link, tris, frame, frame_on, lo, hi); return; }
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = self_box[6 * size_t(link) + a]; hi[a] = self_box[6 * size_t(link) + 3 + a]; }
    };
    child_box(nd.child0, mine_lo, mine_hi);
    pad_slot(mine_lo, mine_hi, frame_pad, nd.box0);
    if (absent_child1(nd, single)) return;
    float lo[3], hi[3];
    child_box(nd.child1, lo, hi);
    pad_slot(lo, hi, frame_pad, nd.box1);
    grow(mine_lo, mine_hi, lo, hi);
}

// ---- the scene centre: the origin of the 32-byte form's halves ----
VHR_BM void no_bounds(float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
}
// grows (lo, hi) by the node's child boxes that exist
VHR_BM void bounds_of_node(const BvhNode &nd, float lo[3], float hi[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (nd.box0[2 * a] <= nd.box0[2 * a + 1]) { lo[a] = fminf(lo[a], nd.box0[2 * a]); hi[a] = fmaxf(hi[a], nd.box0[2 * a + 1]); }
        if (nd.box1[2 * a] <= nd.box1[2 * a + 1]) { lo[a] = fminf(lo[a], nd.box1[2 * a]); hi[a] = fmaxf(hi[a], nd.box1[2 * a + 1]); }
    }
}
VHR_BM void centre_of(const float lo[3], const float hi[3], float centre[3]) {
    for (int a = 0; a < 3; ++a) centre[a] = lo[a] <= hi[a] ? 0.5f * (lo[a] + hi[a]) : 0.0f;
}
// The centre from the root alone.  Every other slot lies inside the root's two (the containment refit_check counts violations of, which
// the padding guarantees for finite coordinates), so this is the reduction over all nodes, bit for bit.
VHR_BM void centre_of_root(const BvhNode &root, float centre[3]) {
    float lo[3], hi[3];
    no_bounds(lo, hi);
    bounds_of_node(root, lo, hi);
    centre_of(lo, hi, centre);
}

// ---- halves ----
// the exact value of a half bit pattern (halves travel as 32-bit words here: 16-bit parameters cost k0_check_forms_kernel ten registers)
VHR_BM double half_value(uint32_t h) {
    const int e = (h >> 10) & 31, m = h & 1023;
    const double v = e == 0 ? ldexp(double(m), -24) : (e == 31 ? (m ? __builtin_nan("") : __builtin_inf()) : ldexp(double(1024 + m), e - 25));
    return (h & 0x8000) ? -v : v;
}
// float -> half bits: to nearest, ties to even (half_nearest), and toward +inf (half_upward).  Beyond the half range both give +-inf.
#if defined(__HIP_DEVICE_COMPILE__)
VHR_BM uint16_t half_nearest(float x) { return __half_as_ushort(__float2half_rn(x)); }
VHR_BM uint16_t half_upward(float x) { return __half_as_ushort(__float2half_ru(x)); }
#else
inline uint16_t half_nearest(float x) {
    if (std::isnan(x)) return 0x7e00;
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const float ax = std::fabs(x);
    if (ax >= 65520.0f) return uint16_t(sign | 0x7c00u);              // (65520 is the tie between the largest half and 2^16: to even = inf)
    if (ax < 5.9604645e-8f * 0.5f) return uint16_t(sign);
    int e;
    const float m = std::frexp(ax, &e);                                 // ax = m * 2^e, m in [0.5, 1)
    int he = e + 14;                                                    // half exponent field for normals
    if (he <= 0) return uint16_t(sign | uint32_t(std::nearbyint(std::ldexp(ax, 24))));      // subnormal half: units of 2^-24
    uint32_t q = uint32_t(std::nearbyint(std::ldexp(m, 11)));           // 11-bit significand incl. the implicit bit (nearbyint: ties to even)
    if (q == 2048u) { q = 1024u; ++he; }
    return he >= 31 ? uint16_t(sign | 0x7c00u) : uint16_t(sign | (uint32_t(he) << 10) | (q & 0x3ffu));
}
inline uint16_t half_upward(float x) {
    uint16_t h = half_nearest(x);
    if (half_value(h) < double(x)) {                                    // landed below: the next half toward +inf
        if ((h & 0x7fffu) == 0) h = 0x0001;
        else h = (h & 0x8000u) ? uint16_t(h - 1) : uint16_t(h + 1);
    }
    return h;
}
#endif
// what the 32-byte form's walker can read: no inf / NaN / subnormal half (a centre may be zero)
VHR_BM bool half_pair_in_range(uint32_t c, uint32_t h) {
    const uint32_t ec = (c >> 10) & 31u, eh = (h >> 10) & 31u;
    return !(ec == 31u || (ec == 0u && c != 0) || eh == 31u || eh == 0u);
}
VHR_BM bool half16_in_range(const BvhNode16 &n) {
    bool in = true;
    for (int i = 0; i < 6; ++i) in = in && half_pair_in_range(n.c[i], n.h[i]);
    return in;
}

// ---- the derived forms of one (lo, hi) node ----
// the upper half of an fp32 half extent, rounded up (the -1 of an absent child is exact; an overflow would give +inf: no finite h gets there)
VHR_BM uint32_t upper16(float h) {
    uint32_t bits;
    memcpy(&bits, &h, 4);
    if (h > 0.0f && (bits & 0xffffu)) bits += 0x10000u;
    return bits >> 16;
}
VHR_BM double from_upper16(uint32_t w16) {
    const uint32_t bits = w16 << 16;
    float f;
    memcpy(&f, &bits, 4);
    return double(f);
}
// All three forms of `nd`; `centre` is the scene centre.
//   BvhNodeCH: c +- h contains [lo, hi] in exact arithmetic (h is widened until it does, plus 4 ulp of the magnitudes involved).
//   BvhNode48: the same centres, the half extents as upper16.
//   BvhNode16: centre + c +- h contains [lo, hi] in exact arithmetic with a few fp32 ulp to spare (the walker rounds o - centre and its
//   FMAs); c is the half nearest to the box's middle, flushed to 0 if subnormal, h the smallest normal half that reaches.  Both halves are
//   always computed: a scene beyond the half range leaves inf in them, which half16_in_range finds afterwards (the walkers then stay on the
//   48-byte form).
// An absent child (lo > hi) has c = 0, h = -1 in every form: never entered.
VHR_BM void forms_of(const BvhNode &nd, const float centre[3], BvhNodeCH &c, BvhNode48 &n48, BvhNode16 &h16) {
    c = BvhNodeCH{};
    n48 = BvhNode48{};
    h16 = BvhNode16{};
    const float inf = __builtin_inff();
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const float *box = which == 0 ? nd.box0 : nd.box1;
        float *hdst = which == 0 ? c.h0 : c.h1;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = box[2 * a], hi = box[2 * a + 1];
            float cc = 0.0f, hh = -1.0f;
            uint16_t cb = 0, hb = 0xbc00;
            if (lo <= hi) {
                cc = 0.5f * lo + 0.5f * hi;
                hh = fmaxf(hi - cc, cc - lo);
                hh += (fabsf(cc) + hh) * 2.4e-7f;
                while (double(cc) - double(hh) > double(lo) || double(cc) + double(hh) < double(hi)) hh = nextafterf(hh, inf);
                const double mid = 0.5 * double(lo) + 0.5 * double(hi) - double(centre[a]);
                cb = half_nearest(float(mid));
                if (((cb >> 10) & 31) == 0) cb = 0;
                const double cv = double(centre[a]) + half_value(cb);
                double need = fmax(double(hi) - cv, cv - double(lo));
                need += (fabs(double(centre[a])) + fabs(cv - double(centre[a])) + need) * 4.8e-7 + 1e-30;
                float nf = float(need);
                if (double(nf) < need) nf = nextafterf(nf, inf);
                hb = half_upward(nf);
                if (((hb >> 10) & 31) == 0) hb = 0x0400;          // the smallest normal half
            }
            (a == 0 ? c.cx : a == 1 ? c.cy : c.cz)[which] = cc;
            hdst[a] = hh;
            h16.c[2 * a + which] = cb;
            h16.h[2 * a + which] = hb;
        }
    }
    c.child0 = nd.child0; c.child1 = nd.child1;
    h16.child0 = link_as_offset<BvhNode16>(nd.child0);
    h16.child1 = link_as_offset<BvhNode16>(nd.child1);
    n48.cx[0] = c.cx[0]; n48.cx[1] = c.cx[1]; n48.cy[0] = c.cy[0]; n48.cy[1] = c.cy[1]; n48.cz[0] = c.cz[0]; n48.cz[1] = c.cz[1];
    n48.hp[0] = (upper16(c.h0[0]) << 16) | upper16(c.h0[1]);
    n48.hp[1] = (upper16(c.h0[2]) << 16) | upper16(c.h1[0]);
    n48.hp[2] = (upper16(c.h1[1]) << 16) | upper16(c.h1[2]);
    n48.child0 = link_as_offset<BvhNode48>(c.child0);
    n48.child1 = link_as_offset<BvhNode48>(c.child1);
}

// Every derived form must CONTAIN the (lo, hi) boxes of the node in exact arithmetic (doubles hold every value involved exactly) -- that is
// all the walkers' bit-identity rests on (boxes only cull).  Adds to bad[0] the boxes checked, bad[1] centre / half-extent boxes that do not
// contain theirs, bad[2] 48-byte boxes that do not contain the centre / half-extent box (or links that differ), bad[3] 32-byte boxes that do
// not contain theirs (or links that differ), bad[4] half pairs of the 32-byte form outside the range its walker reads.  bad[3] means
// something only where the 32-byte form is in use: a caller keeps it only if bad[4] stays 0 over the whole tree.
VHR_BM void check_forms(const BvhNode &nd, const BvhNodeCH &ch, const BvhNode48 &n48, const BvhNode16 &n16, const float centre[3], uint32_t bad[5]) {
    const double h48[6] = { from_upper16(n48.hp[0] >> 16), from_upper16(n48.hp[0] & 0xffffu), from_upper16(n48.hp[1] >> 16),
                            from_upper16(n48.hp[1] & 0xffffu), from_upper16(n48.hp[2] >> 16), from_upper16(n48.hp[2] & 0xffffu) };
    for (int i = 0; i < 6; ++i)
        if (!half_pair_in_range(n16.c[i], n16.h[i])) ++bad[4];
    for (int which = 0; which < 2; ++which) {
        const float *box = which == 0 ? nd.box0 : nd.box1;
        const float *hh = which == 0 ? ch.h0 : ch.h1;
        ++bad[0];
        for (int a = 0; a < 3; ++a) {
            const double lo = box[2 * a], hi = box[2 * a + 1];
            const double c = (a == 0 ? ch.cx : a == 1 ? ch.cy : ch.cz)[which], h = hh[a];
            const double c48 = (a == 0 ? n48.cx : a == 1 ? n48.cy : n48.cz)[which], hw = h48[3 * which + a];
            const uint32_t cb = n16.c[2 * a + which], hb = n16.h[2 * a + which];
            const double c16 = double(centre[a]) + half_value(cb), h16 = half_value(hb);
            if (!(lo <= hi)) {                           // an absent child: never entered in any form
                if (!(h < 0.0)) ++bad[1];
                if (!(hw < 0.0)) ++bad[2];
                if (!(h16 < 0.0)) ++bad[3];
                continue;
            }
            if (c - h > lo || c + h < hi) ++bad[1];
            if (c48 != c || hw < h) ++bad[2];
            if (!half_pair_in_range(cb, hb) || !(c16 - h16 <= lo) || !(c16 + h16 >= hi)) ++bad[3];
        }
    }
    if (n48.child0 != link_as_offset<BvhNode48>(nd.child0) || n48.child1 != link_as_offset<BvhNode48>(nd.child1) || ch.child0 != nd.child0 || ch.child1 != nd.child1) ++bad[2];
    if (n16.child0 != link_as_offset<BvhNode16>(nd.child0) || n16.child1 != link_as_offset<BvhNode16>(nd.child1)) ++bad[3];
}

// ---- the refit's own check: what the walkers will meet, in exact comparisons ----
VHR_BM bool inside(const float lo[3], const float hi[3], const float slot[6]) {
    bool in = true;
    for (int a = 0; a < 3; ++a) in = in && lo[a] >= slot[2 * a] && hi[a] <= slot[2 * a + 1];
    return in;
}
// one node: adds its leaf records whose corners lie outside the slot it holds for them, and its inner children's slots outside theirs
VHR_BM void refit_check(const BvhNode &nd, bool single, const BvhNode *nodes, const BvhTri *tris, const float frame[9], bool frame_on, int &records_outside,
                        int &children_outside) {
    for (int which = 0; which < 2; ++which) {
        if (which == 1 && absent_child1(nd, single)) continue;
        const float *slot = which == 0 ? nd.box0 : nd.box1;
        const int32_t link = which == 0 ? nd.child0 : nd.child1;
        if (link >= 0) {
            const BvhNode c = nodes[link];
            for (int w = 0; w < 2; ++w) {
                const float *cb = w == 0 ? c.box0 : c.box1;
                const float lo[3] = { cb[0], cb[2], cb[4] }, hi[3] = { cb[1], cb[3], cb[5] };
                if (!inside(lo, hi, slot)) ++children_outside;
            }
        } else {
            const uint32_t first = leaf_first(link), n = leaf_count(link);
            for (uint32_t i = 0; i < n; ++i) {
                float lo[3], hi[3];
                record_box(tris[first + i], frame, frame_on, lo, hi);
                if (!inside(lo, hi, slot)) ++records_outside;
            }
        }
    }
}

// ---- surface-area cost ----
VHR_BM double half_area_of_slot(const float b[6]) {
    const double dx = double(b[1]) - double(b[0]), dy = double(b[3]) - double(b[2]), dz = double(b[5]) - double(b[4]);
    return dx * dy + dy * dz + dz * dx;
}
// a child's term: its slot's half area x (1 for an inner child, the number of records for a leaf)
VHR_BM double sah_term(const float box[6], int32_t link) { return half_area_of_slot(box) * (link >= 0 ? 1.0 : double(leaf_count(link))); }
// the sum of every child's term over the half area of the root's two slots together
VHR_BM double sah_cost(double sum, const BvhNode &root, bool single) {
    float box[6];
    for (int i = 0; i < 6; ++i) box[i] = root.box0[i];
    if (!absent_child1(root, single))
        for (int a = 0; a < 3; ++a) { box[2 * a] = fminf(box[2 * a], root.box1[2 * a]); box[2 * a + 1] = fmaxf(box[2 * a + 1], root.box1[2 * a + 1]); }
    const double area = half_area_of_slot(box);
    return area > 0.0 ? sum / area : 0.0;
}

#undef VHR_BM

}  // namespace bvh_math
}  // namespace vhr
