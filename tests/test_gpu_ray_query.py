"""vhr_ray_query on the device (Context.ray_query / ray_query_device) against the CPU oracle's one-ray-at-a-time answers
(orc_scene_closest / orc_scene_occluded): t, u and v compared as bits, the geometry / primitive index of the committed hit, the
any-hit boolean.  Random soups on every tree the library builds, rays grazing triangles (decision (vi)'s binary64 launch),
degenerate rays, the rayquery path's shadow rays on sponza_proc, 8 M-ray batches, the device path on torch's stream, and frames
around queries that stay bit-identical."""
import numpy as np
import pytest

from tests.test_gpu_fuzz import soup
from vulkanhybridrenderer_amd import abi, lib, ray_queries, scenes

pytestmark = pytest.mark.gpu
MISS = abi.RAY_MISS


def _oracle(osc, rays, use_bvh):
    """Closest hit as a ray_hit_dtype array and the any-hit booleans, one ray at a time."""
    n = len(rays)
    want = np.zeros(n, abi.ray_hit_dtype)
    want["geometry_index"] = MISS
    want["primitive_index"] = MISS
    occ = np.zeros(n, bool)
    for i, r in enumerate(rays):
        o, d, tmin, tmax = r[0:3], r[4:7], float(r[3]), float(r[7])
        h = osc.closest(o, d, tmin, tmax, use_bvh=use_bvh)
        if h is not None:
            want[i] = (h[0], h[1], h[2], h[3], h[4], 0)
        occ[i] = osc.occluded(o, d, tmin, tmax, use_bvh=use_bvh)
    return want, occ


def _assert_hits_equal(got, want, what):
    assert got.dtype == abi.ray_hit_dtype
    g, w = got.view(np.uint32).reshape(-1, 6), want.view(np.uint32).reshape(-1, 6)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} rays differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _check(ctx, rays, want, occ, what):
    got = ctx.ray_query(rays)
    _assert_hits_equal(got, want, what + " closest hit")
    stats_closest = ctx.ray_query_statistics()
    assert stats_closest[0] == len(rays) and stats_closest[1] == int((want["geometry_index"] != MISS).sum()) and stats_closest[3] == 0, stats_closest
    any_hit = ctx.ray_query(rays, any_hit=True)
    assert any_hit.dtype == bool and np.array_equal(any_hit, occ), f"{what}: any hit differs for {int((any_hit != occ).sum())} rays"
    stats = ctx.ray_query_statistics()
    assert stats[1] == int(occ.sum()) and stats[3] == 0, stats
    assert np.array_equal(occ, want["geometry_index"] != MISS), what      # any hit == "closest hit found"
    return stats_closest, stats


def _soup_rays(rng, scene, n):
    lo, hi = ray_queries.scene_bounds(scene)
    return ray_queries.random_rays(rng, n, lo, hi, margin=0.2, tmins=(0.0, 0.01), tmaxs=(np.inf, 3.0, 20.0, 1e4))


@pytest.mark.parametrize("seed,n_tris,n_prims", [(1, 60, 3), (2, 400, 5), (3, 2000, 8), (4, 9000, 12)])
def test_soup_rays_equal_the_oracle_on_every_tree(oracle, seed, n_tris, n_prims):
    scene = soup(seed, n_tris, n_prims)
    rng = np.random.default_rng(100 + seed)
    rays = _soup_rays(rng, scene, 20000)
    osc = oracle.Scene(scene)
    want, occ = _oracle(osc, rays, use_bvh=osc.triangle_count > 2000)
    assert 0.1 < occ.mean() < 0.95
    ctx = lib.Context(64, 64)
    try:
        for what, options in (("device-built tree", {}), ("host-built tree", {"bvh_builder": 0}), ("presplit", {"bvh_presplit": 100}),
                              ("world axes", {"bvh_frame": 0}), ("2 LDS levels", {"lds_stack_levels": 2})):
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.upload_scene(scene)
            _check(ctx, rays, want, occ, f"soup {seed}, {what}")
            for k in options:
                ctx.set_option(k, {"bvh_builder": 1, "bvh_presplit": 0, "bvh_frame": 1, "lds_stack_levels": 8}[k])
    finally:
        ctx.close()


def _grazing_rays(scene, rng, n):
    """Rays in or within 1e-7..1e-3 of the planes of the scene's (non-degenerate) triangles, through their interiors, edges and corners."""
    tris = ray_queries.world_triangles(scene)
    k = rng.integers(0, len(tris), n)
    v0, e1, e2 = tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]
    keep = np.linalg.norm(np.cross(e1, e2), axis=1) > 1e-6
    v0, e1, e2 = v0[keep], e1[keep], e2[keep]
    n = len(v0)
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    kind = rng.integers(0, 4, n)
    bu, bv = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = bu + bv > 1
    bu[flip], bv[flip] = 1 - bu[flip], 1 - bv[flip]
    bu[kind == 1] = 0.0
    bv[kind == 2] = 1.0 - bu[kind == 2]
    bu[kind == 3], bv[kind == 3] = 0.0, 0.0
    point = v0 + bu[:, None] * e1 + bv[:, None] * e2
    along = e1 * rng.normal(size=(n, 1)) + e2 * rng.normal(size=(n, 1))
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    d = along + rng.choice([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3], n)[:, None] * nrm
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = point - 10.0 ** rng.uniform(-2, 0.5, (n, 1)) * d
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3], rays[:, 7] = rng.choice([0.0, 1e-3], n), rng.choice([np.inf, 1e4], n)
    return rays


def test_grazing_rays_take_the_binary64_launch(oracle):
    """Rays in or within 1e-7..1e-3 of soup triangles' planes, through their interiors, edges and corners: some candidates contradict
    themselves, the second launch decides those rays again, and every answer is still the oracle's."""
    scene = soup(3, 2000, 8)
    rays = _grazing_rays(scene, np.random.default_rng(7), 12000)
    osc = oracle.Scene(scene)
    want, occ = _oracle(osc, rays, use_bvh=False)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        s_closest, s_any = _check(ctx, rays, want, occ, "grazing rays")
        assert s_closest[2] > 0 and s_any[2] > 0, (s_closest, s_any)
    finally:
        ctx.close()


def test_degenerate_rays_empty_scene_and_odd_counts(oracle):
    scene = soup(2, 400, 5)
    rng = np.random.default_rng(11)
    base = _soup_rays(rng, scene, 64)
    special = []
    for r in base[:12]:
        z = r.copy(); z[4:7] = 0.0; special.append(z)                                  # zero direction
        q = r.copy(); q[4 + int(rng.integers(0, 3))] = np.nan; special.append(q)        # a NaN component
        e = r.copy(); e[3] = e[7] = 1.5; special.append(e)                              # tmin == tmax
        g = r.copy(); g[3], g[7] = 5.0, 1.0; special.append(g)                          # tmin > tmax
    n_miss = len(special)
    for r in base[:12]:
        s = r.copy(); s[4 + int(rng.integers(0, 3))] = np.float32(1e-40); special.append(s)    # a denormal component
        s = r.copy(); s[4:7] = [1e-39, -1.0, 2e-41]; special.append(s)
        s = r.copy(); s[4:7] = [0.0, -1.0, 0.0]; special.append(s)                             # axis-aligned
    rays = np.array(special, np.float32)
    osc = oracle.Scene(scene)
    want, occ = _oracle(osc, rays, use_bvh=False)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        _check(ctx, rays, want, occ, "degenerate rays")
        assert (want["geometry_index"][:n_miss] == MISS).all() and not occ[:n_miss].any()
        assert occ[n_miss:].any()
        # counts that are not a multiple of 64 (nor of a wave's 256 rays)
        many = _soup_rays(rng, scene, 1000)
        w2, o2 = _oracle(osc, many, use_bvh=False)
        for n in (1, 63, 65, 255, 257, 1000):
            _assert_hits_equal(ctx.ray_query(many[:n]), w2[:n], f"count {n}")
            assert np.array_equal(ctx.ray_query(many[:n], any_hit=True), o2[:n])
        # count == 0: VHR_OK, nothing launched
        assert len(ctx.ray_query(np.zeros((0, 8), np.float32))) == 0
        assert ctx.L.vhr_ray_query(ctx.handle, None, 0, 0, None) == 0
        # the argument checks on a device context
        assert ctx.L.vhr_ray_query(ctx.handle, 0x1008, 5, 0, 0x2000) == -1 and "16-byte" in ctx.L.vhr_last_error(ctx.handle).decode()
        assert ctx.L.vhr_ray_query(ctx.handle, 0x1000, 5, 8, 0x2000) == -1
    finally:
        ctx.close()
    empty = lib.Context(64, 64)                                   # no geometry: every ray misses
    try:
        got = empty.ray_query(many)
        assert (got["geometry_index"] == MISS).all() and (got["primitive_index"] == MISS).all()
        assert np.all(got.view(np.uint32).reshape(-1, 6)[:, [0, 1, 2, 5]] == 0)          # t = u = v = 0, reserved 0
        assert not empty.ray_query(many, any_hit=True).any()
        assert empty.ray_query_statistics() == [len(many), 0, 0, 0]
    finally:
        empty.close()


def _sponza_shadow_rays(W=1920, H=1080, grid=None):
    """The rayquery path's shadow rays on frame 1 of sponza_proc's camera path (its stand-in G-buffer at W x H)."""
    from vulkanhybridrenderer_amd.harness import HybridFrameLoop
    scene = scenes.sponza_proc()
    loop = HybridFrameLoop(scene, W, H, 2, shadow=True, ao_spp=0, reflections=0, denoise=False)
    try:
        pfd, depth = loop.pfds[1], loop.gbuffers[1][2].cpu().numpy()
    finally:
        loop.close()
    if grid is None:
        return scene, ray_queries.rayquery_shadow_rays(pfd, depth)
    gx, gy = grid
    ys, xs = np.meshgrid((np.arange(gy) * H) // gy, (np.arange(gx) * W) // gx, indexing="ij")
    return scene, ray_queries.rayquery_shadow_rays(pfd, depth, xs, ys)


def test_sponza_rayquery_shadow_rays_equal_the_oracle(oracle):
    scene, (rays, pix) = _sponza_shadow_rays(grid=(256, 144))
    assert len(rays) > 20000
    osc = oracle.Scene(scene)
    want, occ = _oracle(osc, rays, use_bvh=True)
    assert 0.05 < occ.mean() < 0.95
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        _check(ctx, rays, want, occ, "sponza_proc shadow rays")
    finally:
        ctx.close()


def test_large_batches_are_consistent():
    scene = scenes.sponza_proc()
    lo, hi = ray_queries.scene_bounds(scene)
    rng = np.random.default_rng(5)
    n = 8 << 20
    rays = ray_queries.random_rays(rng, n, lo, hi, margin=0.05, tmins=(0.0, 0.01), tmaxs=(np.inf, 1e4, 5.0))
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        full = ctx.ray_query(rays)
        stats = ctx.ray_query_statistics()
        assert stats[0] == n and stats[1] == int((full["geometry_index"] != MISS).sum()) and stats[3] == 0, stats
        occ = ctx.ray_query(rays, any_hit=True)
        assert ctx.ray_query_statistics()[3] == 0
        assert np.array_equal(occ, full["geometry_index"] != MISS)
        assert 0.2 < occ.mean() < 0.99
        perm = rng.permutation(n)
        shuffled = ctx.ray_query(rays[perm])
        assert shuffled.tobytes() == full[perm].tobytes()
        assert np.array_equal(ctx.ray_query(rays[perm], any_hit=True), occ[perm])
        half = n // 2 + 77
        a, b = ctx.ray_query(rays[:half]), ctx.ray_query(rays[half:])
        assert np.concatenate([a, b]).tobytes() == full.tobytes()
    finally:
        ctx.close()


def test_device_path_on_torchs_stream_sees_updated_geometry():
    import torch
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    scene_a, scene_b = soup(2, 400, 5), soup(4, 9000, 12)
    rng = np.random.default_rng(9)
    rays = _soup_rays(rng, scene_a, 5000)
    host = lib.Context(64, 64)
    try:
        host.upload_scene(scene_a)
        want_a, occ_a = host.ray_query(rays), host.ray_query(rays, any_hit=True)
        host.upload_scene(scene_b)
        want_b, occ_b = host.ray_query(rays), host.ray_query(rays, any_hit=True)
    finally:
        host.close()
    assert not np.array_equal(occ_a, occ_b)
    with torch.cuda.stream(stream):
        ctx = lib.Context(64, 64, stream=torch.cuda.current_stream().cuda_stream)
        try:
            assert ctx.current_stream() == stream.cuda_stream
            ctx.upload_scene(scene_a)
            d_rays = torch.from_numpy(rays).cuda()
            hits = torch.empty((len(rays), 6), dtype=torch.int32, device="cuda")
            occ = torch.empty(len(rays), dtype=torch.uint8, device="cuda")
            ctx.ray_query_device(d_rays.data_ptr(), len(rays), hits.data_ptr())
            ctx.ray_query_device(d_rays.data_ptr(), len(rays), occ.data_ptr(), any_hit=True)
            got_a = hits.cpu().numpy().view(abi.ray_hit_dtype).reshape(-1)         # (.cpu() waits on the current stream)
            got_occ_a = occ.cpu().numpy().astype(bool)
            ctx.upload_scene(scene_b)                                              # ... and the next query, enqueued behind it, sees it
            ctx.ray_query_device(d_rays.data_ptr(), len(rays), hits.data_ptr())
            ctx.ray_query_device(d_rays.data_ptr(), len(rays), occ.data_ptr(), any_hit=True)
            got_b = hits.cpu().numpy().view(abi.ray_hit_dtype).reshape(-1)
            got_occ_b = occ.cpu().numpy().astype(bool)
            assert ctx.ray_query_statistics()[0] == len(rays)
        finally:
            ctx.close()
    assert got_a.tobytes() == want_a.tobytes() and np.array_equal(got_occ_a, occ_a)
    assert got_b.tobytes() == want_b.tobytes() and np.array_equal(got_occ_b, occ_b)


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_queries_between_and_inside_frames_leave_the_frames_identical(frames_in_flight):
    import torch
    from vulkanhybridrenderer_amd.harness import HybridFrameLoop
    W, H, N = 1920, 1080, 8
    scene = scenes.sponza_proc()

    def run(with_queries):
        loop = HybridFrameLoop(scene, W, H, N, shadow=True, ao_spp=2, reflections=1, denoise=True, frames_in_flight=frames_in_flight)
        ctx = loop.ctx
        results = []
        try:
            n, m, d = loop.gbuffers[1]
            rays, _ = ray_queries.rayquery_shadow_rays(loop.pfds[1], d.cpu().numpy())
            rays = np.concatenate([rays, _grazing_rays(scene, np.random.default_rng(17), 20000)])   # (some for the binary64 launch)
            d_rays = torch.from_numpy(rays).cuda()
            out_between = torch.zeros((len(rays), 6), dtype=torch.int32, device="cuda")
            out_inside = torch.zeros(len(rays), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if with_queries:                                       # inside the frame: from the Raytrace Pass's epilogue, on its stream
                ctx.set_pass_epilogue("Raytrace Pass", lambda c: c.ray_query_device(d_rays.data_ptr(), len(rays), out_inside.data_ptr(), any_hit=True))
            images = []
            for i in range(N):
                loop.frame(i)
                if with_queries:                                   # between frames, on the context's stream
                    ctx.ray_query_device(d_rays.data_ptr(), len(rays), out_between.data_ptr())
                if i % 3 == 2 or i == N - 1:
                    ctx.synchronize()
                    images.append([ctx.download(lib.RAYTRACED), ctx.download(lib.DENOISED), ctx.download(lib.REFLECTIONS)])
                    if with_queries:
                        results.append((out_between.cpu().numpy().copy(), out_inside.cpu().numpy().copy()))
            return images, results, rays
        finally:
            loop.close()

    plain, _, _ = run(False)
    queried, results, rays = run(True)
    for k, (a, b) in enumerate(zip(plain, queried)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), f"checkpoint {k}, image {j}: a frame around queries differs"
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        want = ctx.ray_query(rays)
        stats_closest = ctx.ray_query_statistics()
        occ = ctx.ray_query(rays, any_hit=True)
        stats = ctx.ray_query_statistics()
        assert stats_closest[2] + stats[2] > 0 and stats_closest[3] == stats[3] == 0, (stats_closest, stats)
    finally:
        ctx.close()
    for between, inside in results:
        assert between.view(abi.ray_hit_dtype).reshape(-1).tobytes() == want.tobytes()
        assert np.array_equal(inside.astype(bool), occ)


def test_host_memory_calls_share_one_staging_buffer_and_keep_their_statistics():
    """The three host-memory paths stage through ONE buffer per context: a sequence in which it grows, is reused by a smaller call of another
    layout and grows again -- counts on either side of a workgroup of each kernel (2 x 256 rays, 128 points, 256 hits) -- and after every step the
    answer is, bit for bit, the device-memory call's on torch tensors, the step's statistics are that call's, and the other two getters
    still report their own last call."""
    import torch
    from tests import ray_truth as rt
    scene = rt.soup_scene(2)
    rays = rt.soup_rays(scene, 2, 1025)
    rng = np.random.default_rng(23)
    masks = rng.integers(0, 256, len(rays)).astype(np.uint8)
    lo, hi = ray_queries.scene_bounds(scene)
    points = np.concatenate([rng.uniform(lo - 0.2, hi + 0.2, (129, 3)), rng.choice([np.inf, 0.05, 0.5], (129, 1))], axis=1).astype(np.float32)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        ctx.set_primitive_masks(rng.integers(1, 256, len(scene.primitives)).astype(np.uint8))
        getters = {"ray": ctx.ray_query_statistics, "point": ctx.point_query_statistics, "surface": ctx.surface_statistics}
        last = {k: g() for k, g in getters.items()}
        assert all(v == [0, 0, 0, 0] for v in last.values())

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()

        def step(kind, count, device_call, host_call, what):
            want = device_call()
            want_stats = getters[kind]()
            got = host_call()
            assert got.dtype == want.dtype and len(got) == count and got.tobytes() == want.tobytes(), f"{what}: host-memory and device-memory answers differ"
            stats = getters[kind]()
            assert stats[0] == count and stats == want_stats, (what, stats, want_stats)
            last[kind] = stats
            for other, g in getters.items():
                assert g() == last[other], (what, other, g(), last[other])
            return got

        def ray_device(n, any_hit=False, with_masks=True, **kw):
            d_rays, d_masks = dev(rays[:n]), dev(masks[:n])
            out = torch.zeros(n, dtype=torch.uint8, device="cuda") if any_hit else torch.zeros((n, 6), dtype=torch.int32, device="cuda")
            ctx.ray_query_device(d_rays.data_ptr(), n, out.data_ptr(), any_hit=any_hit, ray_masks_ptr=d_masks.data_ptr() if with_masks else 0, **kw)
            return out.cpu().numpy().astype(bool) if any_hit else out.cpu().numpy().view(abi.ray_hit_dtype).reshape(-1)

        def point_device(n):
            d_points = dev(points[:n])
            out = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
            ctx.closest_point_query_device(d_points.data_ptr(), n, out.data_ptr())
            return out.cpu().numpy().view(abi.ray_hit_dtype).reshape(-1)

        def resolve_device(hits, material):
            d_hits = dev(hits.view(np.uint32).reshape(-1, 6))
            out = torch.zeros((len(hits), 20), dtype=torch.float32, device="cuda")
            ctx.resolve_hits_device(d_hits.data_ptr(), len(hits), out.data_ptr(), material=material)
            return out.cpu().numpy().view(abi.surface_point_dtype).reshape(-1)

        hits = step("ray", 513, lambda: ray_device(513, cull_mask=0x7F), lambda: ctx.ray_query(rays[:513], cull_mask=0x7F, ray_masks=masks[:513]), "1: masked, 513 rays")
        assert 0 < int((hits["geometry_index"] != MISS).sum()) < 513 and ctx.ray_mask_statistics()[2] == 1
        found = step("point", 129, lambda: point_device(129), lambda: ctx.closest_point_query(points), "2: 129 points")
        assert 0 < int((found["geometry_index"] != MISS).sum()) < 129
        surf = step("surface", 513, lambda: resolve_device(hits, False), lambda: ctx.resolve_hits(hits), "3: resolve 513 hits")
        assert ctx.surface_statistics()[1] == int((hits["geometry_index"] != MISS).sum()) == int((surf["flags"] & abi.SURFACE_VALID != 0).sum())
        step("ray", 3, lambda: ray_device(3, any_hit=True, with_masks=False), lambda: ctx.ray_query(rays[:3], any_hit=True), "4: any hit, 3 rays")
        one = hits[hits["geometry_index"] != MISS][:1]
        step("surface", 1, lambda: resolve_device(one, True), lambda: ctx.resolve_hits(one, material=True), "5: resolve 1 hit")
        assert ctx.surface_statistics() == [1, 1, ctx.surface_statistics()[2], 1]
        faces = step("ray", 1025, lambda: ray_device(1025, face_cull=abi.FACE_CULL_BACK), lambda: ctx.ray_query(rays, ray_masks=masks, face_cull=abi.FACE_CULL_BACK),
                     "6: faces, 1025 rays")
        assert ctx.face_cull_statistics()[1] == 1 and set(np.unique(faces["reserved"])) <= {0, abi.HIT_KIND_FRONT_FACING}
    finally:
        ctx.close()
