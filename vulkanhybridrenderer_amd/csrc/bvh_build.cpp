// K0: acceleration-structure build.  Replaces ResourceManager::UpdateBLAS / UpdateTLAS
// (/root/reference/src/rendering_backend/resource_manager.cpp:593-801): one geometry per Primitive with
// its transform baked in (:608-617), all opaque (:633), triangle count index_count / 3 (:637), indices
// offset by index_offset and vertices by vertex_offset (:638-639), one identity instance with face
// culling disabled (:704-718)  ==>  a world-space, two-sided triangle soup.
//
// Output: a binned-SAH BVH2 laid out for the CDNA4 traversal kernel -- 64-byte nodes holding BOTH child
// boxes (one node fetch = 4 dwordx4 loads decides both children), emitted in breadth-first order so the
// first K nodes are the top of the tree (the part the traversal kernel stages in LDS), leaves of <= 4
// triangles stored contiguously as 48-byte Moeller-Trumbore records.  Depth is bounded by kMaxBvhDepth,
// which is also the capacity of the traversal stack.
//
// Built with -ffp-contract=off: the world-space vertex transform and the edge subtraction below are part
// of the bit-exact visibility contract ("exact arithmetic").
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <atomic>
#include <limits>
#include <queue>
#include <thread>
#include <mutex>
#include <system_error>

#include "vhr_internal.hpp"
#include "presplit.hpp"
#include "bvh_frame.hpp"
#include "bvh_math.hpp"

namespace vhr {
namespace {

struct Box {
    float lo[3], hi[3];
    void reset() {
        for (int a = 0; a < 3; ++a) { lo[a] = std::numeric_limits<float>::infinity(); hi[a] = -std::numeric_limits<float>::infinity(); }
    }
    void grow(const Box &b) {
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); }
    }
    void grow(const float p[3]) {
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
    }
    float half_area() const {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx < 0 || dy < 0 || dz < 0) return 0.0f;
        return dx * dy + dy * dz + dz * dx;
    }
};

struct TmpNode {
    Box box;
    int32_t left = -1, right = -1;
    uint32_t first = 0, count = 0;     // leaf range in `order`
    uint32_t depth = 0;
};

// [0, n) cut into one contiguous range per thread (the per-node / per-triangle loops around the tree build: independent items)
template <typename F>
void parallel_for(size_t n, unsigned threads, F &&fn) {
    if (threads <= 1 || n < 16384) { fn(size_t(0), n); return; }
    std::vector<std::thread> pool;
    const size_t chunk = (n + threads - 1) / threads;
    for (unsigned t = 1; t < threads; ++t) {
        const size_t b = std::min(n, size_t(t) * chunk), e = std::min(n, b + chunk);
        if (b >= e) continue;
        // a thread that cannot be created (std::system_error) must not escape through the C boundary: its range runs here instead
        try { pool.emplace_back([&fn, b, e]() { fn(b, e); }); } catch (const std::system_error &) { fn(b, e); }
    }
    fn(size_t(0), std::min(n, chunk));
    for (auto &th : pool) th.join();
}
unsigned host_threads(int threads) { return threads > 0 ? unsigned(std::min(threads, 64)) : std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

struct Builder {
    std::vector<BvhTri> tris;          // flat order
    std::vector<Box> tri_box;
    std::vector<float> centroid;       // 3 per tri
    std::vector<uint32_t> order;
    std::vector<TmpNode> nodes;
    uint32_t max_depth = 0;
    int leaf_tris = kMaxLeafTris;      // per build (vhr_set_option "bvh_leaf_triangles" of the context that builds)
    unsigned top_threads = 1;          // > 1 while the one thread that builds the top of the tree may spread a big node's passes over triangles

    uint32_t levels_needed(uint32_t count) const {
        uint32_t leaves = (count + leaf_tris - 1) / leaf_tris;
        uint32_t l = 0;
        while ((1u << l) < leaves) ++l;
        return l;
    }

    // Subtrees of at most `defer_below` triangles are not built here but recorded in `tasks` (their link is the code
    // kDeferred - task index): the top of the tree is built by one thread, the subtrees below it by a pool, each into a node
    // vector of its own, and spliced in afterwards (build_parallel).  `order` is partitioned in place on disjoint ranges, so the
    // workers share it without locks; the result is the tree the one-thread build makes (same splits: nothing depends on node ids).
    struct Task { uint32_t first, count, depth; };
    static constexpr int32_t kDeferred = -1000000000;

    int32_t build(std::vector<TmpNode> &nodes, uint32_t &max_depth, uint32_t first, uint32_t count, uint32_t depth, uint32_t defer_below = 0,
                  std::vector<Task> *tasks = nullptr) {
        if (tasks && count <= defer_below && count > uint32_t(leaf_tris)) {
            tasks->push_back(Task{ first, count, depth });
            return kDeferred - int32_t(tasks->size() - 1);
        }
        int32_t id = int32_t(nodes.size());
        nodes.emplace_back();
        TmpNode n;
        n.box.reset();
        Box cb;
        cb.reset();
        const bool wide = top_threads > 1 && count >= 131072u;      // min / max and counts: the same values in any order
        if (wide) {
            std::mutex m;
            parallel_for(count, top_threads, [&](size_t i0, size_t i1) {
                Box pb, pc;
                pb.reset(); pc.reset();
                for (size_t i = first + i0; i < first + i1; ++i) { pb.grow(tri_box[order[i]]); pc.grow(&centroid[size_t(order[i]) * 3]); }
                std::lock_guard<std::mutex> g(m);
                n.box.grow(pb); cb.grow(pc);
            });
        } else {
            for (uint32_t i = first; i < first + count; ++i) {
                n.box.grow(tri_box[order[i]]);
                cb.grow(&centroid[size_t(order[i]) * 3]);
            }
        }
        n.first = first;
        n.count = count;
        n.depth = depth;
        max_depth = std::max(max_depth, depth);
        if (count <= uint32_t(leaf_tris)) {
            nodes[id] = n;
            return id;
        }
        uint32_t mid = 0;
        bool force_median = depth + levels_needed(count) + 1 >= uint32_t(kMaxBvhDepth);
        if (!force_median) {
            constexpr int kBins = 16;
            float best_cost = std::numeric_limits<float>::infinity();
            int best_axis = -1, best_bin = -1;
            for (int axis = 0; axis < 3; ++axis) {
                float ext = cb.hi[axis] - cb.lo[axis];
                if (!(ext > 0.0f)) continue;
                Box bin_box[kBins];
                uint32_t bin_count[kBins] = {};
                for (auto &b : bin_box) b.reset();
                float scale = float(kBins) / ext;
                auto bin_range = [&](size_t i0, size_t i1, Box *bb, uint32_t *bc) {
                    for (size_t i = first + i0; i < first + i1; ++i) {
                        uint32_t t = order[i];
                        int b = std::min(kBins - 1, std::max(0, int((centroid[size_t(t) * 3 + axis] - cb.lo[axis]) * scale)));
                        bb[b].grow(tri_box[t]);
                        ++bc[b];
                    }
                };
                if (wide) {
                    std::mutex m;
                    parallel_for(count, top_threads, [&](size_t i0, size_t i1) {
                        Box bb[kBins];
                        uint32_t bc[kBins] = {};
                        for (auto &b : bb) b.reset();
                        bin_range(i0, i1, bb, bc);
                        std::lock_guard<std::mutex> g(m);
                        for (int b = 0; b < kBins; ++b) { bin_box[b].grow(bb[b]); bin_count[b] += bc[b]; }
                    });
                } else {
                    bin_range(0, count, bin_box, bin_count);
                }
                float right_area[kBins];
                uint32_t right_count[kBins];
                Box acc;
                acc.reset();
                uint32_t c = 0;
                for (int b = kBins - 1; b > 0; --b) {
                    acc.grow(bin_box[b]);
                    c += bin_count[b];
                    right_area[b] = acc.half_area();
                    right_count[b] = c;
                }
                acc.reset();
                c = 0;
                for (int b = 0; b < kBins - 1; ++b) {
                    acc.grow(bin_box[b]);
                    c += bin_count[b];
                    if (c == 0 || right_count[b + 1] == 0) continue;
                    float cost = acc.half_area() * float(c) + right_area[b + 1] * float(right_count[b + 1]);
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = b; }
                }
            }
            if (best_axis >= 0) {
                float ext = cb.hi[best_axis] - cb.lo[best_axis];
                float scale = 16.0f / ext;
                auto it = std::partition(order.begin() + first, order.begin() + first + count, [&](uint32_t t) {
                    int b = std::min(15, std::max(0, int((centroid[size_t(t) * 3 + best_axis] - cb.lo[best_axis]) * scale)));
                    return b <= best_bin;
                });
                mid = uint32_t(it - order.begin());
            }
        }
        if (mid <= first || mid >= first + count) {      // forced or degenerate: split by count along the widest axis
            int axis = 0;
            float ext = cb.hi[0] - cb.lo[0];
            if (cb.hi[1] - cb.lo[1] > ext) { axis = 1; ext = cb.hi[1] - cb.lo[1]; }
            if (cb.hi[2] - cb.lo[2] > ext) { axis = 2; }
            mid = first + count / 2;
            std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count,
                             [&](uint32_t a, uint32_t b) {
                                 float ca = centroid[size_t(a) * 3 + axis], cb2 = centroid[size_t(b) * 3 + axis];
                                 return ca < cb2 || (!(cb2 < ca) && a < b);      // a strict weak order whatever the values (inputs are validated finite)
                             });
        }
        n.count = 0;
        nodes[id] = n;
        int32_t l = build(nodes, max_depth, first, mid - first, depth + 1, defer_below, tasks);
        int32_t r = build(nodes, max_depth, mid, first + count - mid, depth + 1, defer_below, tasks);
        nodes[id].left = l;
        nodes[id].right = r;
        return id;
    }

    // splice: a subtree's nodes keep their relative links, its root (its first node) replaces the deferred code in dst[0 .. top)
    static void splice(std::vector<TmpNode> &dst, std::vector<std::vector<TmpNode>> &subs) {
        const size_t top = dst.size();
        std::vector<int32_t> root_of(subs.size());
        size_t total = top;
        for (const auto &v : subs) total += v.size();
        dst.reserve(total);
        for (size_t k = 0; k < subs.size(); ++k) {
            const int32_t offset = int32_t(dst.size());
            root_of[k] = offset;
            for (TmpNode t : subs[k]) {
                if (t.left >= 0) { t.left += offset; t.right += offset; }
                dst.push_back(t);
            }
            std::vector<TmpNode>().swap(subs[k]);
        }
        for (size_t i = 0; i < top; ++i) {
            TmpNode &t = dst[i];
            if (t.left <= kDeferred) t.left = root_of[size_t(kDeferred - t.left)];
            if (t.right <= kDeferred) t.right = root_of[size_t(kDeferred - t.right)];
        }
    }
    template <typename F>
    static void run_pool(unsigned threads, size_t n, F &&fn) {
        std::atomic<size_t> next{ 0 };
        auto worker = [&]() { for (size_t k = next.fetch_add(1); k < n; k = next.fetch_add(1)) fn(k); };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < threads && t < n; ++t) {
            try { pool.emplace_back(worker); } catch (const std::system_error &) { break; }      // fewer workers: the queue is drained all the same
        }
        worker();
        for (auto &t : pool) t.join();
    }

    // Three phases.  A: one thread splits the top of the tree down to regions of <= n / 8 triangles (the passes over a big node's
    // triangles spread over the threads).  B: the regions' own tops, one region per thread, down to subtrees of a few thousand
    // triangles.  C: those subtrees, from one queue.  Every piece is built into a node vector of its own and spliced in afterwards;
    // `order` is partitioned in place on disjoint ranges, so nothing is shared, and the tree is the one thread's tree.
    void build_parallel(uint32_t n, int threads) {
        const unsigned hw = host_threads(threads);
        if (hw == 1 || n < 32768u) {                     // small scenes: one thread
            build(nodes, max_depth, 0, n, 0);
            return;
        }
        const uint32_t region = std::max<uint32_t>(16384u, n / 8u), small = std::max<uint32_t>(4096u, n / (8u * hw));
        std::vector<Task> regions;
        top_threads = hw;
        build(nodes, max_depth, 0, n, 0, region, &regions);
        top_threads = 1;
        std::vector<std::vector<TmpNode>> mid(regions.size());
        std::vector<std::vector<Task>> tasks(regions.size());
        std::vector<uint32_t> mid_depth(regions.size(), 0);
        run_pool(hw, regions.size(), [&](size_t k) {
            const Task &r = regions[k];
            build(mid[k], mid_depth[k], r.first, r.count, r.depth, small, r.count > small ? &tasks[k] : nullptr);
        });
        struct Ref { uint32_t region, task; };
        std::vector<Ref> flat;
        for (size_t k = 0; k < regions.size(); ++k)
            for (size_t j = 0; j < tasks[k].size(); ++j) flat.push_back(Ref{ uint32_t(k), uint32_t(j) });
        std::vector<std::vector<std::vector<TmpNode>>> sub(regions.size());
        for (size_t k = 0; k < regions.size(); ++k) sub[k].resize(tasks[k].size());
        std::vector<uint32_t> sub_depth(flat.size(), 0);
        run_pool(hw, flat.size(), [&](size_t f) {
            const Task &t = tasks[flat[f].region][flat[f].task];
            auto &v = sub[flat[f].region][flat[f].task];
            v.reserve(size_t(t.count));
            build(v, sub_depth[f], t.first, t.count, t.depth);
        });
        for (size_t k = 0; k < regions.size(); ++k) splice(mid[k], sub[k]);
        splice(nodes, mid);
        for (uint32_t d : mid_depth) max_depth = std::max(max_depth, d);
        for (uint32_t d : sub_depth) max_depth = std::max(max_depth, d);
    }
};

}  // namespace

void build_bvh(const vhr_vertex *vertices, const uint32_t *indices, const vhr_primitive *primitives,
               uint32_t primitive_count, HostBvh &out, int leaf_tris, int threads, int presplit_percent, int frame_mode) {
    const bool k0trace = std::getenv("VHR_K0_TRACE") != nullptr; auto k0t = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (k0trace) { auto t = std::chrono::steady_clock::now(); std::fprintf(stderr, "K0 %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(t - k0t).count()); k0t = t; } };
    Builder b;
    b.leaf_tris = std::max(1, std::min(kMaxLeafTris, leaf_tris));
    size_t total = 0;
    for (uint32_t p = 0; p < primitive_count; ++p) total += primitives[p].index_count / 3;
    b.tris.reserve(total);
    for (uint32_t p = 0; p < primitive_count; ++p) {
        const vhr_primitive &pr = primitives[p];
        for (uint32_t t = 0; t < pr.index_count / 3; ++t) {
            const uint32_t *vi = indices + pr.index_offset + 3 * t;
            BvhTri tri;
            bvh_math::world_record(pr.transform, vertices[pr.vertex_offset + vi[0]].pos, vertices[pr.vertex_offset + vi[1]].pos, vertices[pr.vertex_offset + vi[2]].pos, tri.v0,
                                   tri.e1, tri.e2);
            tri.prim = p;
            tri.tri = t;
            tri.flat = uint32_t(b.tris.size());
            b.tris.push_back(tri);
        }
    }
    uint32_t n = uint32_t(b.tris.size());
    out.nodes.clear();
    out.nodes16.clear();
    out.nodes_ch.clear();
    out.nodes48.clear();
    out.tris.clear();
    out.max_depth = 0;
    if (n == 0) return;

    b.tri_box.resize(n);
    b.centroid.resize(size_t(n) * 3);
    b.order.resize(n);
    const unsigned hw = host_threads(threads);
    // "bvh_frame" 1: the frame the boxes are built in (bvh_frame.hpp; the device builder runs the same search with a kernel as the pass)
    out.frame_on = false;
    { const float identity[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }; std::memcpy(out.frame, identity, sizeof(identity)); }
    if (frame_mode == 1 && n >= 2u) {
        float frame[9];
        const bool found = bvh_frame::choose([&](const bvh_frame::Candidates &c, uint64_t *sums) {
            for (int k = 0; k < c.n; ++k) sums[k] = 0;
            std::mutex m;
            const size_t stride = bvh_frame::sample_stride(n), samples = (size_t(n) + stride - 1) / stride;
            parallel_for(samples, hw, [&](size_t i0, size_t i1) {
                uint64_t part[bvh_frame::kMaxCandidates] = {};
                for (size_t i = i0; i < i1; ++i)
                    for (int k = 0; k < c.n; ++k) part[k] += bvh_frame::cost_term(c.r[k], b.tris[i * stride]);
                std::lock_guard<std::mutex> lock(m);
                for (int k = 0; k < c.n; ++k) sums[k] += part[k];
            });
        }, frame);
        if (found) { std::memcpy(out.frame, frame, sizeof(frame)); out.frame_on = true; }
        lap("frame search");
    }
    const bool framed = out.frame_on;
    // the world magnitude the frame's padding is built with (bvh_math.hpp, "the frame's padding"; the device builder: k0_frame_boxes_kernel)
    out.frame_magnitude = 0.0f;
    if (framed) {
        float largest = 0.0f;
        for (const BvhTri &t : b.tris) largest = std::max(largest, bvh_math::record_magnitude(t));
        out.frame_magnitude = bvh_math::frame_magnitude_of(largest);
    }
    const float frame_pad = bvh_math::frame_pad_of(out.frame_magnitude);
    parallel_for(n, hw, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
        const BvhTri &t = b.tris[i];
        Box bx;
        bvh_math::record_box(t, out.frame, framed, bx.lo, bx.hi);
        b.tri_box[i] = bx;
        for (int a = 0; a < 3; ++a) b.centroid[size_t(i) * 3 + a] = 0.5f * (bx.lo[a] + bx.hi[a]);
        b.order[i] = uint32_t(i);
    }
    });
    lap("triangles + boxes");
    out.presplit_level = -1;
    if (presplit_percent > 0 && n >= 2u && !framed) {           // (a rotated frame takes the place of splitting: the option is not combined with it)
        // fat triangles entered once per grid cell they pass through (presplit.hpp; the device builder's k0_presplit_* kernels do the same)
        float clo[3] = { b.centroid[0], b.centroid[1], b.centroid[2] }, chi[3] = { b.centroid[0], b.centroid[1], b.centroid[2] };
        for (size_t i = 1; i < n; ++i)
            for (int a = 0; a < 3; ++a) { clo[a] = std::min(clo[a], b.centroid[i * 3 + a]); chi[a] = std::max(chi[a], b.centroid[i * 3 + a]); }
        uint64_t estimates[presplit::kLevels] = {};
        for (int k = 0; k < presplit::kLevels; ++k) {
            const presplit::Grid g = presplit::make_grid(clo, chi, k);
            std::mutex m;
            parallel_for(n, hw, [&](size_t i0, size_t i1) {
                uint64_t sum = 0;
                for (size_t i = i0; i < i1; ++i) sum += presplit::estimate(g, b.tris[i], b.tri_box[i].lo, b.tri_box[i].hi);
                std::lock_guard<std::mutex> lock(m);
                estimates[k] += sum;
            });
        }
        int level = presplit::choose_level(estimates, n, uint32_t(presplit_percent), clo, chi);
        const uint64_t hard_limit = uint64_t(n) + 2ull * uint64_t(n) * uint64_t(presplit_percent) / 100ull;
        std::vector<uint32_t> refs(n);
        uint64_t total = n;
        for (; level >= 0; --level) {                 // the exact count; an estimate that was too low by more than 2x goes one level up
            const presplit::Grid g = presplit::make_grid(clo, chi, level);
            parallel_for(n, hw, [&](size_t i0, size_t i1) {
                for (size_t i = i0; i < i1; ++i) refs[i] = presplit::references(g, b.tris[i], b.tri_box[i].lo, b.tri_box[i].hi, [](const float *, const float *) {});
            });
            total = 0;
            for (uint32_t r : refs) total += r;
            if (total <= hard_limit && total < (1ull << 31)) break;
        }
        if (level >= 0 && total > n) {
            const presplit::Grid g = presplit::make_grid(clo, chi, level);
            std::vector<uint64_t> start(size_t(n) + 1, 0);
            for (size_t i = 0; i < n; ++i) start[i + 1] = start[i] + refs[i];
            std::vector<BvhTri> tris2(total);
            std::vector<Box> box2(total);
            parallel_for(n, hw, [&](size_t i0, size_t i1) {
                for (size_t i = i0; i < i1; ++i) {
                    uint64_t at = start[i];
                    presplit::references(g, b.tris[i], b.tri_box[i].lo, b.tri_box[i].hi, [&](const float *lo, const float *hi) {
                        tris2[at] = b.tris[i];
                        for (int a = 0; a < 3; ++a) { box2[at].lo[a] = lo[a]; box2[at].hi[a] = hi[a]; }
                        ++at;
                    });
                }
            });
            b.tris.swap(tris2);
            b.tri_box.swap(box2);
            n = uint32_t(total);
            b.centroid.resize(size_t(n) * 3);
            b.order.resize(n);
            for (size_t i = 0; i < n; ++i) {
                for (int a = 0; a < 3; ++a) b.centroid[i * 3 + a] = 0.5f * (b.tri_box[i].lo[a] + b.tri_box[i].hi[a]);
                b.order[i] = uint32_t(i);
            }
            out.presplit_level = level;
        }
        if (k0trace) std::fprintf(stderr, "K0 presplit: level %d, %zu triangles -> %u references\n", level, refs.size(), n);
        lap("presplit");
    }
    b.nodes.reserve(size_t(n));
    b.build_parallel(n, threads);
    lap("tree");
    out.max_depth = b.max_depth;

    // Triangle order: by TREELETS.  Breadth first over groups of up to four subtrees -- an inner node with its two children, of which the
    // inner one with the largest box is opened (replaced by its two children, in place) until there are four or only leaves are left --
    // and the leaves of one group are neighbours in `tris`: the two to four leaves a ray reaches within two steps of each other share
    // cache lines (against the plain breadth-first order of the binary tree's leaves, r4: equal on sponza_proc, the any-hit launch -3 % on
    // bistro_proc).
    std::vector<uint32_t> leaf_pos(b.nodes.size(), 0u);
    if (b.nodes[0].left >= 0) {
        uint32_t pos = 0;
        std::vector<int32_t> queue{ 0 };
        for (size_t head = 0; head < queue.size(); ++head) {
            const int32_t id = queue[head];
            int32_t child[4] = { b.nodes[id].left, b.nodes[id].right, -1, -1 };
            int nc = 2;
            while (nc < 4) {
                int best = -1;
                float best_area = -1.0f;
                for (int c = 0; c < nc; ++c) {
                    const TmpNode &t = b.nodes[child[c]];
                    if (t.left < 0) continue;
                    const float area = t.box.half_area();
                    if (area > best_area) { best_area = area; best = c; }
                }
                if (best < 0) break;
                const TmpNode &t = b.nodes[child[best]];
                for (int c = nc; c > best + 1; --c) child[c] = child[c - 1];
                child[best] = t.left;
                child[best + 1] = t.right;
                ++nc;
            }
            for (int c = 0; c < nc; ++c) {
                if (b.nodes[child[c]].left >= 0) queue.push_back(child[c]);
                else { leaf_pos[child[c]] = pos; pos += b.nodes[child[c]].count; }
            }
        }
    }
    out.tris.resize(n);
    parallel_for(b.nodes.size(), hw, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const TmpNode &t = b.nodes[i];
            if (t.left >= 0) continue;
            for (uint32_t j = 0; j < t.count; ++j) out.tris[leaf_pos[i] + j] = b.tris[b.order[t.first + j]];
        }
    });
    lap("triangle order");

    const float inf = std::numeric_limits<float>::infinity();
    auto set_child = [&](BvhNode &node, int which, const TmpNode &child, int32_t link) {
        bvh_math::pad_slot(child.box.lo, child.box.hi, frame_pad, which == 0 ? node.box0 : node.box1);
        (which == 0 ? node.child0 : node.child1) = link;
    };

    const TmpNode &root = b.nodes[0];
    if (root.left < 0) {                       // whole scene fits one leaf
        BvhNode node{};
        set_child(node, 0, root, bvh_math::leaf_link(leaf_pos[0], root.count));
        for (int a = 0; a < 3; ++a) { node.box1[2 * a] = inf; node.box1[2 * a + 1] = -inf; }
        node.child1 = node.child0;
        out.nodes.push_back(node);
        derive_node_forms(out, threads);
        return;
    }
    // breadth-first numbering of the inner nodes
    std::vector<int32_t> bfs_index(b.nodes.size(), -1);
    std::vector<int32_t> bfs_order;
    std::queue<int32_t> q;
    q.push(0);
    while (!q.empty()) {
        int32_t id = q.front();
        q.pop();
        bfs_index[id] = int32_t(bfs_order.size());
        bfs_order.push_back(id);
        const TmpNode &t = b.nodes[id];
        if (b.nodes[t.left].left >= 0) q.push(t.left);
        if (b.nodes[t.right].left >= 0) q.push(t.right);
    }
    out.nodes.resize(bfs_order.size());
    parallel_for(bfs_order.size(), hw, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; ++k) {
        const TmpNode &t = b.nodes[bfs_order[k]];
        BvhNode node{};
        const TmpNode &l = b.nodes[t.left], &r = b.nodes[t.right];
        set_child(node, 0, l, l.left >= 0 ? bfs_index[t.left] : bvh_math::leaf_link(leaf_pos[t.left], l.count));
        set_child(node, 1, r, r.left >= 0 ? bfs_index[t.right] : bvh_math::leaf_link(leaf_pos[t.right], r.count));
        out.nodes[k] = node;
    }
    });
    lap("numbering + (lo, hi) nodes");
    derive_node_forms(out, threads);
    lap("derived node forms");
}

// The scene centre and the derived node forms of out.nodes (centre / half extent, 48-byte, half precision; bvh_math::forms_of): the last stage of a
// build and of a refit.  `only` (a partial refit whose scene centre kept its bits): the forms of the flagged nodes with out.centre as it stands
void derive_node_forms(HostBvh &out, int threads, const std::vector<uint8_t> *only) {
    const unsigned hw = host_threads(threads);
    const size_t n = out.nodes.size();
    if (!only) {
        float lo[3], hi[3];
        bvh_math::no_bounds(lo, hi);
        for (const BvhNode &nd : out.nodes) bvh_math::bounds_of_node(nd, lo, hi);
        bvh_math::centre_of(lo, hi, out.centre);
    }
    out.nodes_ch.resize(n);
    out.nodes48.resize(n);
    out.nodes16.resize(n);
    parallel_for(n, hw, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k)
            if (!only || (*only)[k]) bvh_math::forms_of(out.nodes[k], out.centre, out.nodes_ch[k], out.nodes48[k], out.nodes16[k]);
    });
    // (`only`: the nodes left alone count too -- an overflow leaves a centre or a half extent with the exponent of inf, which is what
    // nodes16_in_range looks for; nothing else forms_of writes is out of the walkers' range)
    out.nodes16_valid = nodes16_in_range(out);
}

// A 64-bit multiplicative hash over the (lo, hi) nodes and the leaf triangles in their final order, eight bytes at a time: the
// identity of a build (tests: the tree must not depend on the number of build threads)
namespace {
struct WordHash {
    uint64_t h = 1469598103934665603ull;
    template <typename T>
    void eat(const T *p, size_t count) {
        static_assert(sizeof(T) % 8 == 0, "whole words");
        const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
        for (size_t i = 0; i + 8 <= count * sizeof(T); i += 8) { uint64_t w; std::memcpy(&w, b + i, 8); h = (h ^ w) * 1099511628211ull; h ^= h >> 29; }
    }
};
}  // namespace
uint64_t bvh_fingerprint(const HostBvh &bvh) {
    WordHash hash;
    hash.eat(bvh.nodes.data(), bvh.nodes.size());
    hash.eat(bvh.tris.data(), bvh.tris.size());
    return hash.h;
}
// ... and the same hash over what the walkers read instead: the scene centre and the three derived forms, the 32-byte form whether it is in
// range or not (a scene beyond the half range leaves the same inf in it with either builder)
uint64_t bvh_forms_fingerprint(const HostBvh &bvh) {
    WordHash hash;
    const struct { float c[4]; } centre = { { bvh.centre[0], bvh.centre[1], bvh.centre[2], 0.0f } };
    hash.eat(&centre, 1);
    hash.eat(bvh.nodes_ch.data(), bvh.nodes_ch.size());
    hash.eat(bvh.nodes48.data(), bvh.nodes48.size());
    hash.eat(bvh.nodes16.data(), bvh.nodes16.size());
    return hash.h;
}

// A hash of the TREE rather than of its arrays: per inner node the bits of its two child boxes and its children's hashes (left, right),
// per leaf the flat ids of its triangles in ascending order -- whatever the numbering of the nodes, the order of the leaves in memory and
// the order of the triangles inside a leaf.  Two builders that make the same tree agree on it (the host's and the device's: tests).
// Needs parents before children in `nodes` (both builders number breadth first).
uint64_t bvh_tree_fingerprint(const HostBvh &bvh) {
    auto mix = [](uint64_t h, uint64_t w) { h = (h ^ w) * 1099511628211ull; return h ^ (h >> 29); };
    auto leaf_hash = [&](int32_t link) {
        const uint32_t first = bvh_math::leaf_first(link), count = bvh_math::leaf_count(link);
        uint32_t ids[4] = { 0, 0, 0, 0 };
        for (uint32_t i = 0; i < count; ++i) ids[i] = bvh.tris[first + i].flat;
        std::sort(ids, ids + count);
        uint64_t h = mix(14695981039346656037ull, count);
        for (uint32_t i = 0; i < count; ++i) h = mix(h, ids[i]);
        return h;
    };
    std::vector<uint64_t> sig(bvh.nodes.size(), 0);
    for (size_t k = bvh.nodes.size(); k-- > 0;) {
        const BvhNode &nd = bvh.nodes[k];
        uint64_t h = 1469598103934665603ull;
        for (int i = 0; i < 6; ++i) { uint32_t b0, b1; std::memcpy(&b0, &nd.box0[i], 4); std::memcpy(&b1, &nd.box1[i], 4); h = mix(h, (uint64_t(b0) << 32) | b1); }
        const bool absent1 = !(nd.box1[0] <= nd.box1[1]);                   // (a one-leaf scene: child 1 is a copy of child 0 behind an empty box)
        h = mix(h, nd.child0 >= 0 ? sig[size_t(nd.child0)] : leaf_hash(nd.child0));
        h = mix(h, absent1 ? 0ull : (nd.child1 >= 0 ? sig[size_t(nd.child1)] : leaf_hash(nd.child1)));
        sig[k] = h;
    }
    return sig.empty() ? 0ull : sig[0];
}

// Every derived node form must CONTAIN the (lo, hi) boxes of `nodes` in exact arithmetic -- that is all the walkers' bit-identity
// rests on (boxes only cull).  out: boxes checked, centre / half-extent boxes that do not contain theirs, 48-byte boxes that do not
// contain the centre / half-extent box, half-precision 32-byte (compact) boxes that do not contain theirs.  (vhr_get_bvh_form_checks)
void check_node_forms(const HostBvh &bvh, uint64_t out[4], int threads) {
    std::atomic<uint64_t> total[4];
    for (auto &t : total) t = 0;
    parallel_for(bvh.nodes.size(), host_threads(threads), [&](size_t k0, size_t k1) {
        uint64_t mine[4] = { 0, 0, 0, 0 };                 // this thread's counts
        for (size_t k = k0; k < k1; ++k) {
            uint32_t bad[5] = { 0, 0, 0, 0, 0 };
            bvh_math::check_forms(bvh.nodes[k], bvh.nodes_ch[k], bvh.nodes48[k], bvh.nodes16[k], bvh.centre, bad);
            for (int i = 0; i < 3; ++i) mine[i] += bad[i];
            if (bvh.nodes16_valid) mine[3] += bad[3];      // (the 32-byte form is checked only where it is in use)
        }
        for (int i = 0; i < 4; ++i) total[i] += mine[i];
    });
    for (int i = 0; i < 4; ++i) out[i] = total[i];
}

bool nodes16_in_range(const HostBvh &bvh) {
    if (bvh.nodes16.size() != bvh.nodes.size() || bvh.nodes16.size() * sizeof(BvhNode16) >= (size_t(1) << 31)) return false;
    for (const BvhNode16 &n : bvh.nodes16)
        if (!bvh_math::half16_in_range(n)) return false;
    return true;
}

// ---- refit: the host side of csrc/kernels_bvh_refit.hip's k0_refit_* kernels (the arithmetic of both: bvh_math.hpp) ----
namespace {
// the walk of both refits relies on this and on nothing else: links in range, children numbered after their parents, records of this scene
bool refit_can_walk(const HostBvh &bvh, const vhr_primitive *primitives, uint32_t primitive_count, bool links) {
    const size_t n_nodes = bvh.nodes.size(), n_tris = bvh.tris.size();
    for (size_t k = 0; links && k < n_nodes; ++k) {
        const int32_t both[2] = { bvh.nodes[k].child0, bvh.nodes[k].child1 };
        for (int32_t link : both) {
            if (link >= 0) { if (size_t(link) <= k || size_t(link) >= n_nodes) return false; continue; }
            if (size_t(bvh_math::leaf_first(link)) + bvh_math::leaf_count(link) > n_tris) return false;
        }
    }
    for (const BvhTri &t : bvh.tris)
        if (t.prim >= primitive_count || t.tri >= primitives[t.prim].index_count / 3) return false;
    return true;
}
// record `tri` re-derived in its slot from (prim, tri); returns the coordinates met that the tree cannot hold: non-finite ones and, in a frame,
// those beyond the world magnitude its padding was built with
// (`beyond` grows by the latter alone: the two want different remedies, and the refit's message says which it met)
uint32_t refit_record(BvhTri &tri, const vhr_vertex *vertices, const uint32_t vi[3], const vhr_primitive &pr, const HostBvh &bvh, uint64_t &beyond) {
    const uint32_t bad = bvh_math::world_record(pr.transform, vertices[vi[0]].pos, vertices[vi[1]].pos, vertices[vi[2]].pos, tri.v0, tri.e1, tri.e2);
    const uint32_t far = bvh_math::coordinates_beyond(tri.v0, tri.e1, tri.e2, bvh.frame_magnitude, bvh.frame_on);
    beyond += far;
    return bad + far;
}
void record_corners(const BvhTri &tri, const uint32_t *indices, const vhr_primitive &pr, uint32_t vi[3]) {
    for (int c = 0; c < 3; ++c) vi[c] = pr.vertex_offset + indices[pr.index_offset + 3 * tri.tri + c];
}
// "object_motion_vectors", the bookkeeping of k0_refit_records_kernel<true> / k0_refit_mark_kernel<true> (vhr_context::d_prev_saved has the rules):
// before record i is rewritten by refit `epoch` ...
void motion_save(HostBvh &bvh, size_t i, uint32_t epoch) {
    if (bvh.prev_saved[i] == epoch) return;              // saved by a failed attempt of this refit: the record holds that attempt's values
    bvh.prev_tris[i] = bvh.tris[i];
    bvh.prev_saved[i] = epoch;
}
// ... a record the refit leaves as it is ...
void motion_settle(HostBvh &bvh, size_t i, uint32_t epoch) {
    if (bvh.prev_saved[i] == epoch - 1u) bvh.prev_tris[i] = bvh.tris[i];
}
// ... and whether the two differ in any of the nine words afterwards
uint64_t motion_differs(const HostBvh &bvh, size_t i) {
    const BvhTri &p = bvh.prev_tris[i], &c = bvh.tris[i];
    return (std::memcmp(p.v0, c.v0, sizeof(c.v0)) || std::memcmp(p.e1, c.e1, sizeof(c.e1)) || std::memcmp(p.e2, c.e2, sizeof(c.e2))) ? 1u : 0u;
}
}  // namespace

void refit_check_pass(const HostBvh &bvh, uint64_t counts[3], unsigned hw);

bool refit_bvh(const vhr_vertex *vertices, const uint32_t *indices, const vhr_primitive *primitives, uint32_t primitive_count, HostBvh &bvh, uint64_t counts[3], int threads,
               uint32_t motion_epoch) {
    counts[0] = counts[1] = counts[2] = 0;
    const size_t n_nodes = bvh.nodes.size(), n_tris = bvh.tris.size();
    if (!n_nodes || !n_tris || !refit_can_walk(bvh, primitives, primitive_count, true)) return false;
    const bool motion = motion_epoch != 0 && bvh.prev_tris.size() == n_tris && bvh.prev_saved.size() == n_tris;
    const unsigned hw = host_threads(threads);
    // 1. the records, each in its slot
    std::atomic<uint64_t> non_finite{ 0 }, differing{ 0 }, beyond{ 0 };
    parallel_for(n_tris, hw, [&](size_t i0, size_t i1) {
        uint64_t bad = 0, differs = 0, far = 0;
        for (size_t i = i0; i < i1; ++i) {
            const vhr_primitive &pr = primitives[bvh.tris[i].prim];
            uint32_t vi[3];
            record_corners(bvh.tris[i], indices, pr, vi);
            if (motion) motion_save(bvh, i, motion_epoch);
            bad += refit_record(bvh.tris[i], vertices, vi, pr, bvh, far);
            if (motion) differs += motion_differs(bvh, i);
        }
        non_finite += bad;
        differing += differs;
        beyond += far;
    });
    counts[2] = non_finite;
    bvh.refit_beyond = beyond;
    bvh.prev_differing = differing;
    // 2. + 3. the boxes bottom-up (children have larger indices than their parents), padded into the parents' slots; and what a partial refit
    // starts from: the unpadded boxes, every node's parent, every record's leaf node
    bvh.self_box.resize(n_nodes * 6);
    bvh.parent.assign(n_nodes, 0xffffffffu);
    bvh.owner.assign(n_tris, 0u);
    for (size_t k = n_nodes; k-- > 0;) {
        BvhNode &nd = bvh.nodes[k];
        bvh_math::refit_slots(nd, n_nodes == 1, bvh.tris.data(), bvh.self_box.data(), bvh.frame, bvh.frame_on, bvh_math::frame_pad_of(bvh.frame_magnitude), &bvh.self_box[6 * k], &bvh.self_box[6 * k + 3]);
        const int32_t both[2] = { nd.child0, nd.child1 };
        for (int32_t link : both) {
            if (link >= 0) { bvh.parent[size_t(link)] = uint32_t(k); continue; }
            for (uint32_t i = 0; i < bvh_math::leaf_count(link); ++i) bvh.owner[bvh_math::leaf_first(link) + i] = uint32_t(k);
        }
    }
    // 4. the scene centre and the derived forms
    derive_node_forms(bvh, threads);
    refit_check_pass(bvh, counts, hw);
    return true;
}

// the check pass: exact comparisons of what the walkers will meet
void refit_check_pass(const HostBvh &bvh, uint64_t counts[3], unsigned hw) {
    const size_t n_nodes = bvh.nodes.size();
    std::atomic<uint64_t> records_outside{ 0 }, children_outside{ 0 };
    parallel_for(n_nodes, hw, [&](size_t k0, size_t k1) {
        int bad_records = 0, bad_children = 0;
        for (size_t k = k0; k < k1; ++k)
            bvh_math::refit_check(bvh.nodes[k], n_nodes == 1, bvh.nodes.data(), bvh.tris.data(), bvh.frame, bvh.frame_on, bad_records, bad_children);
        records_outside += uint64_t(bad_records);
        children_outside += uint64_t(bad_children);
    });
    counts[0] = records_outside;
    counts[1] = children_outside;
}

// the partial refit's host twin (k0_refit_mark_kernel, the level kernels with their one-bit test, the forms restricted to the dirty nodes).  The
// two check passes stay whole-tree here: the host is not the hot path, and their totals are what a dirty pass has to reproduce anyway.
bool refit_bvh_partial(const vhr_vertex *vertices, const uint32_t *indices, const vhr_primitive *primitives, uint32_t primitive_count, HostBvh &bvh,
                       const RefitDirty &dirty, uint64_t counts[3], uint64_t out[4], int threads, uint32_t motion_epoch) {
    counts[0] = counts[1] = counts[2] = 0;
    out[0] = out[1] = out[2] = out[3] = 0;
    const size_t n_nodes = bvh.nodes.size(), n_tris = bvh.tris.size();
    if (!n_nodes || !n_tris || bvh.self_box.size() != n_nodes * 6 || bvh.parent.size() != n_nodes || bvh.owner.size() != n_tris) return false;
    if (!refit_can_walk(bvh, primitives, primitive_count, false)) return false;
    const bool motion = motion_epoch != 0 && bvh.prev_tris.size() == n_tris && bvh.prev_saved.size() == n_tris;
    bvh.prev_differing = 0;
    bvh.refit_beyond = 0;
    const unsigned hw = host_threads(threads);
    // 1. mark, and the dirty records
    std::vector<uint8_t> mark(n_nodes, 0);
    for (size_t i = 0; i < n_tris; ++i) {
        BvhTri &tri = bvh.tris[i];
        const vhr_primitive &pr = primitives[tri.prim];
        uint32_t vi[3];
        record_corners(tri, indices, pr, vi);
        if (!(dirty.primitives.holds(tri.prim) || dirty.vertices.holds(vi[0]) || dirty.vertices.holds(vi[1]) || dirty.vertices.holds(vi[2]))) {
            // (a clean record saved by a failed attempt of this refit -- a whole-tree one -- keeps its previous; it is counted like a rewritten one)
            if (motion) { motion_settle(bvh, i, motion_epoch); if (bvh.prev_saved[i] == motion_epoch) bvh.prev_differing += motion_differs(bvh, i); }
            continue;
        }
        if (motion) motion_save(bvh, i, motion_epoch);
        counts[2] += refit_record(tri, vertices, vi, pr, bvh, bvh.refit_beyond);
        if (motion) bvh.prev_differing += motion_differs(bvh, i);
        ++out[0];
        for (uint32_t node = bvh.owner[i]; node != 0xffffffffu && !mark[node]; node = bvh.parent[node]) { mark[node] = 1; ++out[1]; }
    }
    // 2. + 3. the dirty nodes' boxes, bottom-up, from the boxes the clean ones keep
    for (size_t k = n_nodes; k-- > 0;)
        if (mark[k]) bvh_math::refit_slots(bvh.nodes[k], n_nodes == 1, bvh.tris.data(), bvh.self_box.data(), bvh.frame, bvh.frame_on, bvh_math::frame_pad_of(bvh.frame_magnitude), &bvh.self_box[6 * k], &bvh.self_box[6 * k + 3]);
    // 4. the scene centre from the root's two slots
    float centre[3];
    bvh_math::centre_of_root(bvh.nodes[0], centre);
    const bool moved = std::memcmp(centre, bvh.centre, sizeof(centre)) != 0;
    if (moved) derive_node_forms(bvh, threads);          // (the whole-tree reduction: the same centre)
    else derive_node_forms(bvh, threads, &mark);
    out[2] = moved ? n_nodes : out[1];
    out[3] = moved ? 1u : 0u;
    const uint64_t non_finite = counts[2];
    refit_check_pass(bvh, counts, hw);
    counts[2] = non_finite;
    return true;
}

double bvh_sah_cost(const HostBvh &bvh) {
    if (bvh.nodes.empty()) return 0.0;
    const bool single = bvh.nodes.size() == 1;
    double sum = 0.0;
    for (const BvhNode &nd : bvh.nodes) {
        sum += bvh_math::sah_term(nd.box0, nd.child0);
        if (!bvh_math::absent_child1(nd, single)) sum += bvh_math::sah_term(nd.box1, nd.child1);
    }
    return bvh_math::sah_cost(sum, bvh.nodes[0], single);
}

// ---- rebuild in place (vhr_rebuild_geometry): the host twins of k0_rebuild_finite_kernel / k0_rebuild_gather_kernel / k0_rebuild_scatter_kernel ----
uint64_t count_non_finite_positions(const vhr_vertex *vertices, uint32_t vertex_count) {
    uint64_t bad = 0;
    for (uint32_t v = 0; v < vertex_count; ++v)
        for (int a = 0; a < 3; ++a) bad += std::isfinite(vertices[v].pos[a]) ? 0u : 1u;
    return bad;
}

void rebuild_gather_records(const std::vector<BvhTri> &tris, const std::vector<BvhTri> &prev_tris, const std::vector<uint32_t> &prev_saved, uint32_t epoch,
                            uint32_t flat_count, std::vector<BvhTri> &flat) {
    flat.assign(flat_count, BvhTri{});
    const bool retry = prev_tris.size() == tris.size() && prev_saved.size() == tris.size();
    for (size_t k = 0; k < tris.size(); ++k) {
        const BvhTri &t = (retry && prev_saved[k] == epoch) ? prev_tris[k] : tris[k];      // (a presplit tree's references of one triangle hold the same words)
        if (t.flat < flat_count) flat[t.flat] = t;
    }
}

uint64_t rebuild_scatter_records(HostBvh &bvh, const std::vector<BvhTri> &flat, uint32_t epoch) {
    const size_t n = bvh.tris.size();
    bvh.prev_tris.resize(n);
    bvh.prev_saved.assign(n, 0u);
    uint64_t differing = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t f = bvh.tris[k].flat;
        bvh.prev_tris[k] = f < flat.size() ? flat[f] : bvh.tris[k];
        if (motion_differs(bvh, k)) { bvh.prev_saved[k] = epoch; ++differing; }
    }
    bvh.prev_differing = differing;
    return differing;
}

}  // namespace vhr
