// The batched closest-point query (vhr_closest_point_query), the k-nearest query on the same walk (vhr_nearest_points_query) and the debug kernel
// that runs their point / triangle distance on explicit pairs (vhr_debug_point_triangle).  A unit of its own: it reads DeviceScene and shares no code with the ray walkers (no trace_device.hpp, so no
// sRGB table either).  Built with -ffp-contract=off: point_triangle (closest_point.hpp) owes the host its bits.
#include "closest_point.hpp"
#include "vhr_internal.hpp"

namespace vhr {

// ---------------------------------------------------------------------------------------------
// vhr_debug_point_triangle on a device context: 12 floats per pair (p, v0, e1, e2) -> 3 floats (d2, u, v).  One pair per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void point_triangle_pairs_kernel(const float *pairs, const uint32_t n, float *out, const Stamps st) {
    vhr_stamp(st);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *s = pairs + size_t(i) * 12u;
    const float p[3] = { s[0], s[1], s[2] }, v0[3] = { s[3], s[4], s[5] }, e1[3] = { s[6], s[7], s[8] }, e2[3] = { s[9], s[10], s[11] };
    const PointTriangle r = point_triangle(p, v0, e1, e2);
    out[size_t(i) * 3u] = r.d2; out[size_t(i) * 3u + 1u] = r.u; out[size_t(i) * 3u + 2u] = r.v;
}

int launch_point_triangle_pairs(vhr_context *ctx, const float *pairs, uint32_t n, float *out) {
    PairArray a[2] = { { pairs, nullptr, size_t(n) * 12u * sizeof(float) }, { nullptr, out, size_t(n) * 3u * sizeof(float) } };
    return run_pairs(ctx, "vhr_debug_point_triangle", a, [&] {
        launch(ctx, point_triangle_pairs_kernel, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<const float *>(a[0].d), n, static_cast<float *>(a[1].d));
    });
}

// ---------------------------------------------------------------------------------------------
// vhr_closest_point_query.  One query per lane; a per-lane walk of the fp32 (lo, hi) nodes with the traversal stack in LDS, laid out as
// traverse<> lays its own out (entry `level` of thread t at [level * block + t]: conflict free), kTraceStack levels = the depth bound of any tree
// the walkers are given.  Beside every link sits the lower bound its box had when it was pushed: a popped entry is tested against the best d2
// of NOW before it is opened.  At an inner node both children's bounds are computed, the nearer child is entered first and the farther one is
// pushed only if it can still hold the winner.
//
// What a box may be skipped on (DESIGN.md 4d has the argument in full).  A query returns, bit for bit, the winner of the brute-force loop of
// point_triangle over all records -- so a box is skipped only if NO record below it can have a computed d2 <= the best computed d2.  The bound
// of a box is, per axis of the tree's frame, the gap g = max(lo - x, x - hi, 0) between the (rotated) point and the PADDED slot, less a slack
//     eps = 2^-18 (M + |p.x| + |p.y| + |p.z|),        M = the largest |coordinate| of the root's two slots,
// clamped at 0, squared and summed, times 1 - 2^-18.  The slack pays for every ABSOLUTE rounding error between what the builder boxed and what
// point_triangle computes -- the record's corners v0 + e1, v0 + e2 rounded, the frame's rotation of corners and of the point, ap = p - v0 and
// the three lines of point_triangle_d2 -- each a small multiple of 2^-24 times a coordinate's magnitude, 51 2^-24 M + 8.2 2^-24 |p|_1 in all;
// the factor pays for the relative ones (the bound's own squares and sums, d2's, the frame's rows not being exactly orthonormal: 15 2^-24).
// The slots' own padding (1e-3 + 1e-5 |x|: bvh_math::pad_slot) is NOT spent by the argument; it is why no product in it underflows (a point with a
// positive gap is at least 1e-3 away from every record of the box).  A box is skipped iff bound > best: an equal bound is opened (a record at the
// same d2 with a smaller flat index wins), and so is a bound that is not a number.
// ---------------------------------------------------------------------------------------------
constexpr int kPointBlock = 128;          // 2 waves; 2 x 4 B x kTraceStack x 128 = 40 KB of LDS per workgroup
constexpr float kBoundSlack = 0x1p-18f, kBoundShrink = 1.0f - 0x1p-18f;

struct PointQueryArgs {
    DeviceScene scene;
    const float4 *points;                 // (point, max_distance) per query
    void *results;                        // vhr_ray_hit[count] or uint8_t[count] (ANY_WITHIN)
    PointQueryCounters *counters;
    const uint8_t *prim_masks;            // one byte per primitive (the MASK instantiations; never null there)
    uint32_t count, cull_mask;
};
static_assert(sizeof(vhr_point_query) == sizeof(float4), "vhr_point_query is one float4");

// the bound of one slot (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z as the node stores them); false: an absent child (an inverted box), never entered
__device__ __forceinline__ bool slot_bound(float lox, float hix, float loy, float hiy, float loz, float hiz, float x, float y, float z, float eps, float &bound) {
    const float gx = fmaxf(fmaxf(fmaxf(lox - x, x - hix), 0.0f) - eps, 0.0f);
    const float gy = fmaxf(fmaxf(fmaxf(loy - y, y - hiy), 0.0f) - eps, 0.0f);
    const float gz = fmaxf(fmaxf(fmaxf(loz - z, z - hiz), 0.0f) - eps, 0.0f);
    bound = ((gx * gx + gy * gy) + gz * gz) * kBoundShrink;
    return lox <= hix;
}

// what a walk starts from: the point in the boxes' frame ("bvh_frame"; the records stay in world space) and the slack eps of every bound
__device__ __forceinline__ float walk_start(const DeviceScene &sc, const float p[3], float &x, float &y, float &z) {
    x = p[0]; y = p[1]; z = p[2];
    if (sc.frame_on) {
        const float *R = sc.frame;
        x = (R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]; y = (R[3] * p[0] + R[4] * p[1]) + R[5] * p[2]; z = (R[6] * p[0] + R[7] * p[1]) + R[8] * p[2];
    }
    // M from the root (every other slot lies inside the root's two); an absent child's inverted box does not count
    const float4 *np = reinterpret_cast<const float4 *>(sc.nodes);
    const float4 r0 = np[0], r1 = np[1], r2 = np[2];
    float m = fmaxf(fmaxf(fmaxf(fabsf(r0.x), fabsf(r0.y)), fmaxf(fabsf(r0.z), fabsf(r0.w))), fmaxf(fabsf(r1.x), fabsf(r1.y)));
    if (r1.z <= r1.w) m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(r1.z), fabsf(r1.w)), fmaxf(fabsf(r2.x), fabsf(r2.y))), fmaxf(fabsf(r2.z), fabsf(r2.w))));
    return kBoundSlack * (m + ((fabsf(p[0]) + fabsf(p[1])) + fabsf(p[2])));
}

template <bool ANY_WITHIN, bool MASK>
__global__ __launch_bounds__(kPointBlock) void point_query_kernel(const PointQueryArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_link[kTraceStack * kPointBlock];
    __shared__ float s_bound[kTraceStack * kPointBlock];
    const uint64_t q64 = uint64_t(blockIdx.x) * kPointBlock + threadIdx.x;
    const bool live = q64 < a.count;
    const uint32_t q = uint32_t(q64);
    const DeviceScene &sc = a.scene;
    uint32_t evals = 0, overflow = 0;
    bool found = false;
    float best = 0.0f, bu = 0.0f, bv = 0.0f;
    uint32_t best_flat = 0xffffffffu, best_index = 0u;
    if (live) {
        const float4 pq = a.points[q];
        const float p[3] = { pq.x, pq.y, pq.z };
        // a negative or NaN max_distance and a non-finite point find nothing; max_distance = +inf bounds nothing
        const bool valid = pq.w >= 0.0f && __builtin_isfinite(pq.x) && __builtin_isfinite(pq.y) && __builtin_isfinite(pq.z);
        best = pq.w * pq.w;                                             // fl(max_distance^2): a candidate has d2 <= it
        if (valid && sc.node_count != 0) {
            float x, y, z;
            const float eps = walk_start(sc, p, x, y, z);
            int *const link = s_link + threadIdx.x;
            float *const bound = s_bound + threadIdx.x;
            int sp = 0, cur = 0;
            for (;;) {
                if (cur >= 0) {
                    const float4 *np = reinterpret_cast<const float4 *>(sc.nodes + cur);
                    const float4 q0 = np[0], q1 = np[1], q2 = np[2];
                    const int4 q3 = reinterpret_cast<const int4 *>(np)[3];
                    float b0, b1;
                    bool h0 = slot_bound(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, x, y, z, eps, b0);
                    bool h1 = slot_bound(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, x, y, z, eps, b1);
                    h0 = h0 && !(b0 > best);
                    h1 = h1 && !(b1 > best);
                    if (h0 && h1) {
                        const bool first0 = b0 <= b1;
                        if (sp < kTraceStack) {
                            link[sp * kPointBlock] = first0 ? q3.y : q3.x;
                            bound[sp * kPointBlock] = first0 ? b1 : b0;
                            ++sp;
                        } else {
                            overflow = 1;
                        }
                        cur = first0 ? q3.x : q3.y;
                        continue;
                    }
                    if (h0) { cur = q3.x; continue; }
                    if (h1) { cur = q3.y; continue; }
                } else {
                    const uint32_t w = ~uint32_t(cur);
                    const uint32_t first = w >> 2, n = (w & 3u) + 1u;
                    bool done = false;
                    for (uint32_t i = 0; i < n; ++i) {
                        const float4 *tp = reinterpret_cast<const float4 *>(sc.tris + first + i);
                        const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                        if constexpr (MASK) { if ((uint32_t(a.prim_masks[__float_as_uint(tc.y)]) & a.cull_mask) == 0u) continue; }      // (tc = e2.z, prim, tri, flat)
                        const float v0[3] = { ta.x, ta.y, ta.z }, e1[3] = { ta.w, tb.x, tb.y }, e2[3] = { tb.z, tb.w, tc.x };
                        const PointTriangle r = point_triangle(p, v0, e1, e2);
                        ++evals;
                        if constexpr (ANY_WITHIN) {
                            if (r.d2 <= best) { found = true; done = true; break; }
                        } else {
                            const uint32_t flat = __float_as_uint(tc.w);
                            if (found ? (r.d2 < best || (r.d2 == best && flat < best_flat)) : r.d2 <= best) {
                                found = true;
                                best = r.d2; bu = r.u; bv = r.v; best_flat = flat; best_index = first + i;
                            }
                        }
                    }
                    if (done) break;
                }
                bool open = false;
                while (sp > 0 && !open) {                               // the next entry that can still hold the winner
                    --sp;
                    cur = link[sp * kPointBlock];
                    open = !(bound[sp * kPointBlock] > best);
                }
                if (!open) break;
            }
        }
        if constexpr (ANY_WITHIN) {
            static_cast<uint8_t *>(a.results)[q] = found ? 1u : 0u;
        } else {
            uint32_t *const r = static_cast<uint32_t *>(a.results) + size_t(q) * 6u;        // vhr_ray_hit (results is 4-byte aligned)
            const uint32_t none = 0xffffffffu;
            r[0] = found ? __float_as_uint(sqrtf(best)) : 0u; r[1] = found ? __float_as_uint(bu) : 0u; r[2] = found ? __float_as_uint(bv) : 0u;
            r[3] = found ? sc.tris[best_index].prim : none; r[4] = found ? sc.tris[best_index].tri : none; r[5] = 0u;
        }
    }
    // the wave's sums, one vector atomic each from its first lane (every lane of the wave arrives here)
    uint32_t hits = found ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) { hits += uint32_t(__shfl_xor(int(hits), off)); evals += uint32_t(__shfl_xor(int(evals), off)); }
    const bool wave_overflow = __any(overflow != 0u);
    if ((threadIdx.x & 63u) == 0u) {
        if (hits) atomicAdd(&a.counters->found, (unsigned long long)hits);
        if (evals) atomicAdd(&a.counters->evaluations, (unsigned long long)evals);
        if (wave_overflow) atomicAdd(&a.counters->overflows, 1u);
    }
}

int launch_point_query(vhr_context *ctx, const vhr_point_query *points, uint32_t count, bool any_within, uint32_t cull_mask, void *results) {
    if (count == 0) return VHR_OK;
    const QueryScratch *const s = stream_scratch(ctx, ctx->pq_scratch, sizeof(PointQueryCounters), "vhr_closest_point_query");      // this stream's counters
    if (!s) return VHR_ERROR_DEVICE;
    PointQueryArgs a;
    a.scene = ctx->device_scene();
    a.points = reinterpret_cast<const float4 *>(points);
    a.results = results;
    ctx->pq_last_counters = a.counters = static_cast<PointQueryCounters *>(s->counters);
    a.prim_masks = nullptr;
    a.count = count;
    a.cull_mask = cull_mask;
    // the mask instantiations only where the cull mask acts on the masks the primitives carry: the defaults launch the plain ones
    const bool mask_acts = ctx->ray_mask_acts(cull_mask);
    if (mask_acts) {
        if (const int rc = ensure_device_prim_masks(ctx)) return rc;
        a.prim_masks = ctx->d_prim_masks;
    }
    const dim3 grid(uint32_t((uint64_t(count) + kPointBlock - 1u) / kPointBlock));
    if (any_within) {
        if (mask_acts) launch(ctx, point_query_kernel<true, true>, grid, dim3(kPointBlock), 0, a);
        else launch(ctx, point_query_kernel<true, false>, grid, dim3(kPointBlock), 0, a);
    } else {
        if (mask_acts) launch(ctx, point_query_kernel<false, true>, grid, dim3(kPointBlock), 0, a);
        else launch(ctx, point_query_kernel<false, false>, grid, dim3(kPointBlock), 0, a);
    }
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "vhr_closest_point_query: kernel launch failed");
    return VHR_OK;
}

// ---------------------------------------------------------------------------------------------
// vhr_nearest_points_query: the k nearest triangles of every query, ordered by (d2, flat).  point_query_kernel's walk -- the same stack, the same
// bounds, the same near / far order -- with the scalar `best` replaced by `limit`: fl(max_distance^2) until the lane's list holds k entries, the
// k-th entry's d2 from then on.  A box is skipped iff bound > limit (an equal bound is opened: an equal d2 with a smaller flat index displaces
// the k-th; a bound that is not a number is opened).  The limit only falls, and a record with d2 > limit has k candidates ahead of it, so 4d's
// argument holds as it stands.
//
// The list is sorted and lives in dynamic LDS, sized by the call's k: d2 of entry j of lane t at [j * block + t], its record index at
// [(k + j) * block + t] (8 B per entry; conflict free like the stack).  A record's flat index is read from the record itself, and only where two
// d2 are equal: the order needs it for nothing else, and a second reference to a listed triangle ("bvh_presplit": identical records, one flat
// index) has the listed one's d2, bit for bit, so that is also where the scan meets it and drops it.  (u, v) are not kept (16 B per entry would
// not fit beside the stack at k = 16): the k kept records are evaluated once more at the end, by the same function on the same record.
// ---------------------------------------------------------------------------------------------
struct NearestQueryArgs {
    DeviceScene scene;
    const float4 *points;                 // (point, max_distance) per query
    uint32_t *results;                    // vhr_ray_hit[count * k]
    NearestQueryCounters *counters;
    const uint8_t *prim_masks;            // one byte per primitive (the MASK instantiation; never null there)
    uint32_t count, k, cull_mask;
};

template <bool MASK>
__global__ __launch_bounds__(kPointBlock) void nearest_points_kernel(const NearestQueryArgs a, const Stamps st) {
    vhr_stamp(st);
    __shared__ int s_link[kTraceStack * kPointBlock];
    __shared__ float s_bound[kTraceStack * kPointBlock];
    extern __shared__ uint32_t s_list[];                                // 2 * k * kPointBlock words
    const uint64_t q64 = uint64_t(blockIdx.x) * kPointBlock + threadIdx.x;
    const bool live = q64 < a.count;
    const DeviceScene &sc = a.scene;
    const uint32_t k = a.k;
    float *const l_d2 = reinterpret_cast<float *>(s_list) + threadIdx.x;
    uint32_t *const l_rec = s_list + k * kPointBlock + threadIdx.x;
    uint32_t evals = 0, overflow = 0, n = 0;                            // n: entries in the list
    if (live) {
        const float4 pq = a.points[q64];
        const float p[3] = { pq.x, pq.y, pq.z };
        // a negative or NaN max_distance and a non-finite point find nothing; max_distance = +inf bounds nothing
        const bool valid = pq.w >= 0.0f && __builtin_isfinite(pq.x) && __builtin_isfinite(pq.y) && __builtin_isfinite(pq.z);
        float limit = pq.w * pq.w;                                      // fl(max_distance^2) while n < k, then the k-th entry's d2
        if (valid && sc.node_count != 0) {
            float x, y, z;
            const float eps = walk_start(sc, p, x, y, z);
            int *const link = s_link + threadIdx.x;
            float *const bound = s_bound + threadIdx.x;
            int sp = 0, cur = 0;
            for (;;) {
                if (cur >= 0) {
                    const float4 *np = reinterpret_cast<const float4 *>(sc.nodes + cur);
                    const float4 q0 = np[0], q1 = np[1], q2 = np[2];
                    const int4 q3 = reinterpret_cast<const int4 *>(np)[3];
                    float b0, b1;
                    bool h0 = slot_bound(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, x, y, z, eps, b0);
                    bool h1 = slot_bound(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, x, y, z, eps, b1);
                    h0 = h0 && !(b0 > limit);
                    h1 = h1 && !(b1 > limit);
                    if (h0 && h1) {
                        const bool first0 = b0 <= b1;
                        if (sp < kTraceStack) {
                            link[sp * kPointBlock] = first0 ? q3.y : q3.x;
                            bound[sp * kPointBlock] = first0 ? b1 : b0;
                            ++sp;
                        } else {
                            overflow = 1;
                        }
                        cur = first0 ? q3.x : q3.y;
                        continue;
                    }
                    if (h0) { cur = q3.x; continue; }
                    if (h1) { cur = q3.y; continue; }
                } else {
                    const uint32_t w = ~uint32_t(cur);
                    const uint32_t first = w >> 2, cnt = (w & 3u) + 1u;
                    for (uint32_t i = 0; i < cnt; ++i) {
                        const float4 *tp = reinterpret_cast<const float4 *>(sc.tris + first + i);
                        const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                        if constexpr (MASK) { if ((uint32_t(a.prim_masks[__float_as_uint(tc.y)]) & a.cull_mask) == 0u) continue; }      // (tc = e2.z, prim, tri, flat)
                        const float v0[3] = { ta.x, ta.y, ta.z }, e1[3] = { ta.w, tb.x, tb.y }, e2[3] = { tb.z, tb.w, tc.x };
                        const float d2 = point_triangle(p, v0, e1, e2).d2;
                        ++evals;
                        if (!(d2 <= limit)) continue;                   // beyond max_distance, or behind the k-th
                        const uint32_t flat = __float_as_uint(tc.w);
                        // the entries behind the newcomer in (d2, flat): [at, n).  A listed entry with the newcomer's d2 AND flat index is
                        // another reference to the same triangle: the newcomer is dropped
                        uint32_t at = n;
                        bool listed = false;
                        while (at > 0) {
                            const float e = l_d2[(at - 1u) * kPointBlock];
                            if (e < d2) break;
                            if (e == d2) {
                                const uint32_t e_flat = sc.tris[l_rec[(at - 1u) * kPointBlock]].flat;
                                if (e_flat == flat) { listed = true; break; }
                                if (e_flat < flat) break;
                            }
                            --at;
                        }
                        if (listed || at == k) continue;                // (at == k: a full list whose k-th ties on d2 with a smaller flat index)
                        for (uint32_t j = n < k ? n : k - 1u; j > at; --j) {     // a full list loses its last entry
                            l_d2[j * kPointBlock] = l_d2[(j - 1u) * kPointBlock];
                            l_rec[j * kPointBlock] = l_rec[(j - 1u) * kPointBlock];
                        }
                        l_d2[at * kPointBlock] = d2;
                        l_rec[at * kPointBlock] = first + i;
                        if (n < k) ++n;
                        if (n == k) limit = l_d2[(k - 1u) * kPointBlock];
                    }
                }
                bool open = false;
                while (sp > 0 && !open) {                               // the next entry that can still hold one of the k: the limit of NOW
                    --sp;
                    cur = link[sp * kPointBlock];
                    open = !(bound[sp * kPointBlock] > limit);
                }
                if (!open) break;
            }
        }
        // entry j of query q at results[q * k + j]: the kept records once more for (u, v), then miss records
        uint32_t *r = a.results + q64 * k * 6u;                          // vhr_ray_hit (results is 4-byte aligned)
        for (uint32_t j = 0; j < k; ++j, r += 6) {
            if (j < n) {
                const uint32_t rec = l_rec[j * kPointBlock];
                const float4 *tp = reinterpret_cast<const float4 *>(sc.tris + rec);
                const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                const float v0[3] = { ta.x, ta.y, ta.z }, e1[3] = { ta.w, tb.x, tb.y }, e2[3] = { tb.z, tb.w, tc.x };
                const PointTriangle pt = point_triangle(p, v0, e1, e2);
                r[0] = __float_as_uint(sqrtf(pt.d2)); r[1] = __float_as_uint(pt.u); r[2] = __float_as_uint(pt.v);
                r[3] = __float_as_uint(tc.y); r[4] = __float_as_uint(tc.z); r[5] = 0u;
            } else {
                r[0] = 0u; r[1] = 0u; r[2] = 0u; r[3] = 0xffffffffu; r[4] = 0xffffffffu; r[5] = 0u;
            }
        }
    }
    // the wave's sums, one vector atomic each from its first lane (every lane of the wave arrives here)
    uint32_t entries = n;
    for (int off = 32; off > 0; off >>= 1) { entries += uint32_t(__shfl_xor(int(entries), off)); evals += uint32_t(__shfl_xor(int(evals), off)); }
    const bool wave_overflow = __any(overflow != 0u);
    if ((threadIdx.x & 63u) == 0u) {
        if (entries) atomicAdd(&a.counters->entries, (unsigned long long)entries);
        if (evals) atomicAdd(&a.counters->evaluations, (unsigned long long)evals);
        if (wave_overflow) atomicAdd(&a.counters->overflows, 1u);
    }
}

int launch_nearest_query(vhr_context *ctx, const vhr_point_query *points, uint32_t count, uint32_t k, uint32_t cull_mask, vhr_ray_hit *results) {
    if (count == 0) return VHR_OK;
    const QueryScratch *const s = stream_scratch(ctx, ctx->nq_scratch, sizeof(NearestQueryCounters), "vhr_nearest_points_query");      // this stream's counters
    if (!s) return VHR_ERROR_DEVICE;
    NearestQueryArgs a;
    a.scene = ctx->device_scene();
    a.points = reinterpret_cast<const float4 *>(points);
    a.results = reinterpret_cast<uint32_t *>(results);
    ctx->nq_last_counters = a.counters = static_cast<NearestQueryCounters *>(s->counters);
    a.prim_masks = nullptr;
    a.count = count;
    a.k = k;
    a.cull_mask = cull_mask;
    // the mask instantiation only where the cull mask acts on the masks the primitives carry, as in launch_point_query
    const bool mask_acts = ctx->ray_mask_acts(cull_mask);
    if (mask_acts) {
        if (const int rc = ensure_device_prim_masks(ctx)) return rc;
        a.prim_masks = ctx->d_prim_masks;
    }
    const dim3 grid(uint32_t((uint64_t(count) + kPointBlock - 1u) / kPointBlock));
    const size_t list_bytes = size_t(k) * 2u * sizeof(uint32_t) * kPointBlock;        // k <= VHR_NEAREST_MAX_K: at most 16 KB beside the stack's 40 KB
    if (mask_acts) launch(ctx, nearest_points_kernel<true>, grid, dim3(kPointBlock), list_bytes, a);
    else launch(ctx, nearest_points_kernel<false>, grid, dim3(kPointBlock), list_bytes, a);
    if (hipGetLastError() != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "vhr_nearest_points_query: kernel launch failed");
    return VHR_OK;
}

}  // namespace vhr
