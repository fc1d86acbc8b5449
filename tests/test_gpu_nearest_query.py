"""vhr_nearest_points_query on the device: a query's list equals, bit for bit, the first k of the brute force of tests/nearest_truth.py -- the
candidates of the closest-point query ordered by (d2, flat), every triangle once, miss records behind them -- on every tree the library builds,
on presplit trees (where the walk meets a triangle several times), in the builder's frame, after refits and a rebuild, with cull masks, from
host and device memory at every count around a wave and a block, between frames and inside a pass; and the k-th distance prunes the walk.
Scenes and queries are those of tests/test_gpu_point_query.py.

The "every tree" queries are queries_for(seed=18): with the default seed 51 of 1 024 lists hold between 1 and 15 entries, one short of the
twentieth the test demands of its truth; with 18 it is 62, 551 lists are full and 408 hold two neighbours of equal d2.

Measured on an MI355X: see test_the_kth_distance_prunes_the_walk."""
import numpy as np
import pytest

from tests import nearest_truth as nt
from tests.test_gpu_fuzz import soup
from tests.test_gpu_point_query import TREE_DEFAULTS, _vertex_block, flat_to_ids, outlier_soup, queries_for, triangle_grid
from vulkanhybridrenderer_amd import abi, lib, ray_queries, scenes

pytestmark = pytest.mark.gpu
MISS = abi.RAY_MISS
ERROR_GRAPH = -5          # include/vhr_amd.h


@pytest.fixture(scope="module")
def host():
    c = lib.Context(64, 64, host_only=True)
    yield c
    c.close()


def assert_lists_equal(got, want, what, fields=None):
    assert got.dtype == abi.ray_hit_dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if fields is None:
        g, w = got.view(np.uint32).reshape(len(got), -1), want.view(np.uint32).reshape(len(want), -1)          # raw 24-byte records
    else:
        g = np.concatenate([got[f].view(np.uint32) for f in fields], axis=1)
        w = np.concatenate([want[f].view(np.uint32) for f in fields], axis=1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} lists differ, first {bad[0]}:\n got {got[bad[0]]}\nwant {want[bad[0]]}"


def check(ctx, queries, want, entries, what, fields=None, **kw):
    k = want.shape[1]
    got = ctx.nearest_points_query(queries, k, **kw)
    s = ctx.nearest_query_statistics()
    assert_lists_equal(got, want, f"{what}, k {k}", fields)
    assert s[0] == len(queries) and s[1] == int(entries.sum()) and s[3] == 0, (what, k, s, int(entries.sum()))
    return s


# ---------------------------------------------------------------------------------------------
# tree independence
# ---------------------------------------------------------------------------------------------
def test_lists_equal_the_brute_force_on_every_tree(host):
    scene = outlier_soup(300.0)
    geometry, primitive = flat_to_ids(scene)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        records = ctx.triangle_records()
        assert len(records) == scene.triangle_count > 1400
        queries = queries_for(records, seed=18)
        assert len(queries) == 1024
        matrix = nt.distance_matrix(host, records, queries)
        truth = {k: nt.nearest(matrix, geometry, primitive, queries, k) for k in (1, 2, 5, 16)}
        # what the truth must hold for the comparison to mean something
        order, total = nt.ordered(matrix, nt.candidates(matrix, queries))
        entries = truth[16][1]
        assert np.array_equal(entries, np.minimum(total, 16))
        assert (entries == 16).mean() >= 1 / 5 and ((entries >= 1) & (entries <= 15)).mean() >= 1 / 20, ((entries == 16).sum(), ((entries >= 1) & (entries <= 15)).sum())
        d2 = np.take_along_axis(matrix[:, :, 0], order[:, :16], axis=1)
        ties = ((d2[:, 1:] == d2[:, :-1]) & (order[:, 1:16] != order[:, 0:15]) & (np.arange(1, 16)[None] < entries[:, None])).any(axis=1)
        assert ties.sum() >= 20, ties.sum()
        for what, options in (("device-built tree", {}), ("host-built tree", {"bvh_builder": 0}), ("world axes", {"bvh_frame": 0}),
                              ("leaves of 1", {"bvh_leaf_triangles": 1}), ("leaves of 4", {"bvh_leaf_triangles": 4}),
                              ("host-built, leaves of 1, world axes", {"bvh_builder": 0, "bvh_leaf_triangles": 1, "bvh_frame": 0})):
            for o, v in options.items():
                ctx.set_option(o, v)
            ctx.upload_scene(scene)
            assert ctx.bvh_builder_used() == options.get("bvh_builder", 1)
            assert np.array_equal(ctx.triangle_records(), records)
            for k, (want, n) in truth.items():
                check(ctx, queries, want, n, what)
            closest = ctx.closest_point_query(queries)
            assert_lists_equal(ctx.nearest_points_query(queries, 1), closest.reshape(-1, 1), what + ": k = 1 against vhr_closest_point_query")
            for o in options:
                ctx.set_option(o, TREE_DEFAULTS[o])
    finally:
        ctx.close()


def test_a_presplit_tree_lists_every_triangle_once(host):
    """A presplit tree holds a fat triangle in several leaves, each an identical record behind the box of its part: the same lists, compared on
    (t, geometry_index, primitive_index) as the closest-point query's presplit test compares, no triangle twice -- and the tree's own records say
    that the first 16 REFERENCES of at least 50 queries name a triangle twice, so the lists are these only because the walk drops them."""
    scene = scenes.rotated(soup(22, 1500, 6), rot_y=0.6, rot_x=0.25)
    geometry, primitive = flat_to_ids(scene)
    fields = ("t", "geometry_index", "primitive_index")
    ctx = lib.Context(64, 64)
    try:
        ctx.set_option("bvh_frame", 0)
        ctx.upload_scene(scene)
        records = ctx.triangle_records()
        queries = queries_for(records, seed=13)
        queries[::2, 3] = np.inf
        matrix = nt.distance_matrix(host, records, queries)
        want, entries = nt.nearest(matrix, geometry, primitive, queries, 16)
        assert (entries == 16).mean() > 0.5
        check(ctx, queries, want, entries, "one reference per triangle")
        for builder in (1, 0):
            ctx.set_option("bvh_presplit", 100)
            ctx.set_option("bvh_builder", builder)
            ctx.upload_scene(scene)
            assert ctx.bvh_builder_used() == builder and ctx.bvh_presplit_level() >= 0 and ctx.bvh_statistics()["triangles"] > scene.triangle_count
            got = ctx.nearest_points_query(queries, 16)
            s = ctx.nearest_query_statistics()
            assert_lists_equal(got, want, f"presplit, builder {builder}", fields)
            assert s[0] == len(queries) and s[1] == int(entries.sum()) and s[3] == 0, s
            ids = got["geometry_index"].astype(np.int64) << 32 | got["primitive_index"]
            for q in range(len(queries)):
                assert len(np.unique(ids[q, :entries[q]])) == entries[q], f"builder {builder}, query {q}: a triangle twice"
            # the references the walk meets: the tree's leaf records, one per reference
            raw = ctx.bvh_arrays()["records"]
            refs, ref_flat = raw[:, 0:36].copy().view(np.float32).reshape(-1, 9), raw[:, 44:48].copy().view(np.uint32).reshape(-1)
            assert len(refs) > scene.triangle_count and np.array_equal(np.unique(ref_flat), np.arange(scene.triangle_count))
            by_flat = np.argsort(ref_flat, kind="stable")
            refs, ref_flat = refs[by_flat], ref_flat[by_flat]
            assert np.array_equal(refs, records[ref_flat])                           # identical records, one flat index (presplit.hpp)
            ref_matrix = nt.distance_matrix(host, refs, queries)
            ref_order, ref_total = nt.ordered(ref_matrix, nt.candidates(ref_matrix, queries))
            repeats = 0
            for q in range(len(queries)):
                first = ref_flat[ref_order[q, :min(int(ref_total[q]), 16)]]
                repeats += len(np.unique(first)) < len(first)
            print(f"builder {builder}: {len(refs)} references of {scene.triangle_count} triangles, {repeats} of {len(queries)} queries' first 16 references repeat a triangle")
            assert repeats >= 50, repeats
    finally:
        ctx.close()


def test_lists_equal_the_brute_force_in_the_frame_after_refits_a_rebuild_and_beyond_the_half_range(host):
    """The rotated soup with "bvh_frame" on, both builders; then vertices move: vhr_refit_geometry, vhr_refit_geometry_partial,
    vhr_rebuild_geometry, the brute force over the records of each; then the scene whose outliers put it beyond the half-precision nodes."""
    rng = np.random.default_rng(43)
    scene = scenes.rotated(soup(32, 2000, 6), rot_y=0.6, rot_x=0.25)
    geometry, primitive = flat_to_ids(scene)
    ctx = lib.Context(64, 64)

    def judge(sc, ids, queries, what):
        records = ctx.triangle_records()
        matrix = nt.distance_matrix(host, records, queries)
        for k in (3, 16):
            want, entries = nt.nearest(matrix, ids[0], ids[1], queries, k)
            assert 0.3 < (entries > 0).mean() < 0.9 and (entries == k).mean() > 0.2
            check(ctx, queries, want, entries, what)
        return matrix

    try:
        queries = None
        for builder in (1, 0):
            ctx.set_option("bvh_builder", builder)
            ctx.upload_scene(scene)
            assert ctx.bvh_builder_used() == builder and not np.array_equal(ctx.bvh_frame(), np.eye(3, dtype=np.float32))
            if queries is None:
                queries = queries_for(ctx.triangle_records(), seed=9)
            judge(scene, (geometry, primitive), queries, f"frame on, builder {builder}")
        ctx.set_option("bvh_builder", 1)
        ctx.upload_scene(scene)
        pts = lib.Context._points_array(queries)
        out = np.zeros((len(queries), 3), abi.ray_hit_dtype)
        v = scene.vertices.copy()
        for step, p in enumerate((2, 5, 1)):
            a, b = _vertex_block(scene, p)
            v["pos"][a:b] += rng.normal(scale=0.3, size=(b - a, 3)).astype(np.float32)
            ctx.update_vertices(v[a:b], first_vertex=a)
            rc = ctx.L.vhr_nearest_points_query(ctx.handle, pts.ctypes.data, len(pts), 3, abi.POINT_QUERY_HOST_MEMORY, 0xFF, out.ctypes.data)      # an update is pending
            assert rc == ERROR_GRAPH and "vhr_nearest_points_query" in ctx.L.vhr_last_error(ctx.handle).decode(), rc
            if step == 0:
                ctx.refit_geometry()
            elif step == 1:
                ctx.refit_geometry_partial(force=True)
                assert ctx.partial_refit_statistics()["partial_refits"] >= 1
            else:
                ctx.rebuild_geometry()
                assert ctx.rebuild_statistics()[0] >= 1
            matrix = judge(scene, (geometry, primitive), queries, ("refit", "partial refit", "rebuild")[step])
            want, _ = nt.nearest(matrix, geometry, primitive, queries, 3)
            assert (want["geometry_index"] == p).sum() > 10                          # the moved block is found
        # beyond the half range
        far = outlier_soup(3.0e5)
        ctx.upload_scene(far)
        far_ids = flat_to_ids(far)
        far_queries = queries_for(ctx.triangle_records(), seed=10)
        fv = far.vertices.copy()
        a, b = _vertex_block(far, 2)
        fv["pos"][a:b] += rng.normal(scale=0.3, size=(b - a, 3)).astype(np.float32)
        ctx.update_vertices(fv[a:b], first_vertex=a)
        ctx.refit_geometry()
        st = ctx.refit_statistics()
        assert (st["records_outside"], st["children_outside"], st["non_finite"], st["half_nodes"]) == (0, 0, 0, 0), st
        judge(far, far_ids, far_queries, "beyond the half range, refitted")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# cull masks
# ---------------------------------------------------------------------------------------------
def test_cull_masks_restrict_the_brute_force(host):
    """The masks of the closest-point query's mask test.  Which instantiation ran has no counter of its own; the evaluations tell: with a cull mask
    that shares a bit with every primitive's mask the call is the call before masks were set, evaluation for evaluation (the plain kernel), and
    with cull_mask 0 the walks evaluate nothing, which only the kernel that looks at the masks before it evaluates can do."""
    scene = outlier_soup(300.0)
    geometry, primitive = flat_to_ids(scene)
    K = 5
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        records = ctx.triangle_records()
        queries = queries_for(records, seed=11)
        matrix = nt.distance_matrix(host, records, queries)
        plain, plain_entries = nt.nearest(matrix, geometry, primitive, queries, K)
        before = ctx.ray_mask_statistics()
        s_plain = check(ctx, queries, plain, plain_entries, "no masks set")
        assert ctx.ray_mask_statistics() == before == [0, 0, 0, 0] and s_plain[2] > 0
        prim_masks = np.array([0x01, 0x02, 0x06][:3] * 3, np.uint8)[:len(scene.primitives)]
        assert len(prim_masks) == len(scene.primitives) and len(np.unique(prim_masks)) == 3
        ctx.set_primitive_masks(prim_masks)
        stats = ctx.ray_mask_statistics()
        for cull in (0xFF, 0x04, 0x02, 0):
            visible = (prim_masks[geometry] & cull) != 0
            want, entries = nt.nearest(matrix, geometry, primitive, queries, K, visible)
            s = check(ctx, queries, want, entries, f"cull_mask {cull:#x}", cull_mask=cull)
            if cull == 0xFF:
                assert np.array_equal(want, plain) and s == s_plain                  # the mask does not act: the plain kernel, the same walk
            elif cull == 0:
                assert not entries.any() and (want["geometry_index"] == MISS).all() and s[1:] == [0, 0, 0]
            else:
                assert entries.any() and entries.sum() < plain_entries.sum() and not np.array_equal(want, plain)
                found = want["geometry_index"][want["geometry_index"] != MISS]
                assert ((prim_masks[found] & cull) != 0).all() and 0 < s[2]
        assert ctx.ray_mask_statistics() == stats                                   # the ray statistics are the rays'
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# memory, streams and side effects
# ---------------------------------------------------------------------------------------------
def test_host_and_device_memory_agree_at_every_count_around_a_wave_and_a_block(host):
    import torch
    torch.cuda.set_device(0)
    scene = outlier_soup(300.0)
    geometry, primitive = flat_to_ids(scene)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = lib.Context(64, 64, stream=torch.cuda.current_stream().cuda_stream)
        try:
            assert ctx.current_stream() == stream.cuda_stream
            assert ctx.nearest_query_statistics() == [0, 0, 0, 0]
            empty = ctx.nearest_points_query(np.float32([[0, 1, 0, np.inf]] * 70), 3)            # a context without geometry: only miss records
            assert empty.shape == (70, 3) and (empty["geometry_index"] == MISS).all() and (empty["primitive_index"] == MISS).all()
            assert not empty.view(np.uint32).reshape(-1, 6)[:, [0, 1, 2, 5]].any() and ctx.nearest_query_statistics() == [70, 0, 0, 0]
            ctx.upload_scene(scene)
            records = ctx.triangle_records()
            queries = queries_for(records, n=1000, seed=12)
            matrix = nt.distance_matrix(host, records, queries)
            d_queries = torch.from_numpy(queries).cuda()
            assert d_queries.data_ptr() % 16 == 0
            tail = 7                                                                 # records behind the last entry, which stay as they were
            for k in (1, 3, 16):
                want, entries = nt.nearest(matrix, geometry, primitive, queries, k)
                for n in (1, 63, 64, 65, 127, 128, 129, 1000):
                    from_host = ctx.nearest_points_query(queries[:n], k)
                    assert_lists_equal(from_host, want[:n], f"host memory, count {n}, k {k}")
                    out = torch.full(((n * k + tail) * 24,), 0xCD, dtype=torch.uint8, device="cuda")
                    ctx.nearest_points_query_device(d_queries.data_ptr(), n, k, out.data_ptr())
                    raw = out.cpu().numpy()                                          # (.cpu() waits on the current stream)
                    assert (raw[n * k * 24:] == 0xCD).all(), f"count {n}, k {k}: bytes behind entry count * k were written"
                    assert np.array_equal(raw[:n * k * 24], from_host.view(np.uint8).reshape(-1)), f"count {n}, k {k}: host and device memory differ"
                    assert ctx.nearest_query_statistics()[:2] == [n, int(entries[:n].sum())] and ctx.nearest_query_statistics()[3] == 0
            # count == 0 launches nothing
            out = torch.full((24 * 4,), 0xCD, dtype=torch.uint8, device="cuda")
            ctx.nearest_points_query_device(d_queries.data_ptr(), 0, 4, out.data_ptr())
            assert (out.cpu().numpy() == 0xCD).all() and ctx.L.vhr_nearest_points_query(ctx.handle, None, 0, 4, 0, 0xFF, None) == 0
            assert ctx.nearest_points_query(queries[:0], 4).shape == (0, 4)
            # the argument checks on a device context
            assert ctx.L.vhr_nearest_points_query(ctx.handle, 0x1008, 5, 4, 0, 0xFF, 0x2000) == -1 and "16-byte" in ctx.L.vhr_last_error(ctx.handle).decode()
            assert ctx.L.vhr_nearest_points_query(ctx.handle, 0x1000, 5, 4, abi.POINT_QUERY_ANY_WITHIN, 0xFF, 0x2000) == -1
            assert ctx.L.vhr_nearest_points_query(ctx.handle, 0x1000, 5, 17, 0, 0xFF, 0x2000) == -1 and "k 17" in ctx.L.vhr_last_error(ctx.handle).decode()
        finally:
            ctx.close()


_frame_truth = {}          # the frames test's brute force over sponza_proc(0.2), computed once and shared by its two cases


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_queries_between_and_inside_frames_leave_the_frames_identical(host, frames_in_flight):
    """The rig of the closest-point query's test of the same name: a k = 4 query from the G-Buffer Pass's epilogue (on the stream the next pass is
    ordered on) and one between frames (on the context's) -- the frames are the frames without them, the lists are the brute force's, and the two
    streams' counters are their own."""
    import torch
    from vulkanhybridrenderer_amd.harness import HybridFrameLoop
    W, H, N, K = 480, 270, 5, 4
    scene = scenes.sponza_proc(0.2)
    rng = np.random.default_rng(17)
    lo, hi = ray_queries.scene_bounds(scene)
    inside_q = np.zeros((1000, 4), np.float32)
    inside_q[:, 0:3], inside_q[:, 3] = rng.uniform(lo, hi, (1000, 3)), 0.5
    between_q = np.zeros((1900, 4), np.float32)
    between_q[:, 0:3], between_q[:, 3] = rng.uniform(lo - 2.0, hi + 2.0, (1900, 3)), np.inf
    between_q[::7, 3] = 0.1

    def run(with_queries):
        loop = HybridFrameLoop(scene, W, H, N, shadow=True, ao_spp=2, reflections=1, denoise=True, frames_in_flight=frames_in_flight)
        ctx = loop.ctx
        results, stats = [], []
        try:
            d_inside, d_between = torch.from_numpy(inside_q).cuda(), torch.from_numpy(between_q).cuda()
            out_between = torch.zeros((len(between_q), K, 6), dtype=torch.int32, device="cuda")
            out_inside = torch.zeros((len(inside_q), K, 6), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            streams = set()
            if with_queries:
                def inside(c):
                    streams.add(c.current_stream())
                    c.nearest_points_query_device(d_inside.data_ptr(), len(inside_q), K, out_inside.data_ptr())
                ctx.set_pass_epilogue("G-Buffer Pass", inside)
            images = []
            for i in range(N):
                loop.frame(i)
                if with_queries:
                    streams.add(ctx.current_stream())
                    ctx.nearest_points_query_device(d_between.data_ptr(), len(between_q), K, out_between.data_ptr())
                if i % 2 == 1 or i == N - 1:
                    ctx.synchronize()
                    images.append([ctx.download(lib.RAYTRACED), ctx.download(lib.DENOISED), ctx.download(lib.REFLECTIONS)])
                    if with_queries:
                        results.append((out_between.cpu().numpy().copy(), out_inside.cpu().numpy().copy()))
                        stats.append(ctx.nearest_query_statistics())
            records = ctx.triangle_records() if with_queries else None
            return images, results, stats, records, len(streams)
        finally:
            loop.close()

    plain, _, _, _, _ = run(False)
    queried, results, stats, records, n_streams = run(True)
    assert n_streams == frames_in_flight                      # one stream, or the front stream and the context's
    for c, (a, b) in enumerate(zip(plain, queried)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), f"checkpoint {c}, image {j}: a frame around queries differs"
    geometry, primitive = flat_to_ids(scene)
    key = records.tobytes()
    if key not in _frame_truth:
        _frame_truth.clear()
        _frame_truth[key] = (nt.nearest(nt.distance_matrix(host, records, between_q), geometry, primitive, between_q, K),
                             nt.nearest(nt.distance_matrix(host, records, inside_q), geometry, primitive, inside_q, K))
    (want, entries), (want_inside, entries_inside) = _frame_truth[key]
    assert 0.01 < (entries_inside > 0).mean() < 0.99 and 0.5 < (entries == K).mean() <= 1.0
    for (between, inside), s in zip(results, stats):
        assert_lists_equal(between.view(abi.ray_hit_dtype).reshape(-1, K), want, "between frames")
        assert_lists_equal(inside.view(abi.ray_hit_dtype).reshape(-1, K), want_inside, "inside a pass")
        assert s[:2] == [len(between_q), int(entries.sum())] and s[3] == 0, s     # the last query's counters: the pass's query did not touch them


# ---------------------------------------------------------------------------------------------
# pruning
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [1, 0])
def test_the_kth_distance_prunes_the_walk(builder):
    """32 x 32 disjoint triangles of side 0.5 at pitch 2, a query 0.02 above each centroid.  k = 4 without a max_distance: the list fills with the
    triangle and three neighbours (1.5 and more away), and from then on the 4th distance closes every box farther than it -- a mean of at most 128
    evaluations of 1 024 is a condition that the k-th distance prunes, which a walk that only had max_distance = inf to go by misses by a factor
    of eight; it is no performance figure.  k = 16 within 1.0: one entry per query, so the list never fills and max_distance alone prunes.

    Measured on an MI355X, mean evaluations per query: k = 4, inf: 9.188 on the device-built and on the host-built tree; k = 16, 1.0: 2.000 on both."""
    scene, tri = triangle_grid()
    centroid = tri.astype(np.float64).mean(axis=1)
    ctx = lib.Context(64, 64)
    try:
        ctx.set_option("bvh_builder", builder)
        ctx.upload_scene(scene)
        assert ctx.bvh_builder_used() == builder and ctx.bvh_statistics()["triangles"] == 1024
        q = np.zeros((1024, 4), np.float32)
        q[:, 0:3], q[:, 3] = centroid + [0, 0.02, 0], np.inf
        got = ctx.nearest_points_query(q, 4)
        s = ctx.nearest_query_statistics()
        print(f"builder {builder}, k 4, inf: {s[2]} evaluations for {s[0]} queries, mean {s[2] / s[0]:.3f}")
        assert s[0] == 1024 and s[1] == 4 * 1024 and s[3] == 0                       # every list is full
        assert (got["geometry_index"] == 0).all() and np.array_equal(got["primitive_index"][:, 0], np.arange(1024))
        assert np.allclose(got["t"][:, 0], 0.02, rtol=1e-4) and np.allclose(got["u"][:, 0], 1 / 3, atol=1e-5) and np.allclose(got["v"][:, 0], 1 / 3, atol=1e-5)
        assert (got["t"][:, 1] >= 1.5 - 0.5).all() and (np.diff(got["t"], axis=1) >= 0).all()
        assert s[2] / s[0] <= 128.0, s
        q[:, 3] = 1.0
        got = ctx.nearest_points_query(q, 16)
        s = ctx.nearest_query_statistics()
        print(f"builder {builder}, k 16, 1.0: {s[2]} evaluations for {s[0]} queries, mean {s[2] / s[0]:.3f}")
        assert s[0] == s[1] == 1024 and s[3] == 0                                    # exactly one entry per query
        assert np.array_equal(got["primitive_index"][:, 0], np.arange(1024)) and (got["primitive_index"][:, 1:] == MISS).all() and (got["geometry_index"][:, 1:] == MISS).all()
        assert s[2] / s[0] <= 128.0, s
        q[:, 3] = 0.01
        got = ctx.nearest_points_query(q, 16)
        assert (got["geometry_index"] == MISS).all() and not got.view(np.uint32).reshape(-1, 6)[:, [0, 1, 2, 5]].any()
        assert ctx.nearest_query_statistics() == [1024, 0, 0, 0]
    finally:
        ctx.close()
