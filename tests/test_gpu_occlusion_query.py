"""vhr_occlusion_query on the device: a point's mask equals, bit for bit, the truth of tests/occlusion_truth.py -- the rays restated from the
oracle's primitives, each judged by the oracle's brute force -- on every tree the library builds, after a refit and a rebuild; it equals the bits
of vhr_ray_query on the rays vhr_debug_occlusion_rays reports, which are the host-only context's; at every count around a wave and a workgroup
from host and device memory; through the binary64 launch on triangles built around the rays; under cull masks; without geometry; and frames
around queries stay bit-identical."""
import copy

import numpy as np
import pytest

from tests import occlusion_truth as ot
from tests.test_gpu_fuzz import soup
from tests.test_gpu_point_query import _vertex_block
from vulkanhybridrenderer_amd import abi, lib, ray_queries, scenes
from vulkanhybridrenderer_amd.camera import directional_light

pytestmark = pytest.mark.gpu
SAMPLES = (1, 5, 16, 64)
SEED = 0x51ED
TREE_DEFAULTS = {"bvh_builder": 1, "bvh_presplit": 0, "bvh_frame": 1, "lds_stack_levels": 8}


@pytest.fixture(scope="module")
def host():
    c = lib.Context(64, 64, host_only=True)
    yield c
    c.close()


def soup_points(scene, rng, n=400):
    """n query points: half on the scene's (non-degenerate) triangles pushed 1e-3 along their normals, which are their axes; half uniform in the
    scene's bounds with random unit axes.  tmin 0, tmax one of 0.5, 3, inf."""
    tris = ray_queries.world_triangles(scene)
    nrm = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    good = np.nonzero(area > 1e-6)[0]
    k = rng.choice(good, n // 2)
    bu, bv = rng.uniform(0, 1, n // 2), rng.uniform(0, 1, n // 2)
    flip = bu + bv > 1
    bu[flip], bv[flip] = 1 - bu[flip], 1 - bv[flip]
    unit = nrm[k] / area[k, None]
    on = tris[k, 0] + bu[:, None] * (tris[k, 1] - tris[k, 0]) + bv[:, None] * (tris[k, 2] - tris[k, 0]) + 1e-3 * unit
    lo, hi = ray_queries.scene_bounds(scene)
    free = rng.uniform(lo, hi, (n - n // 2, 3))
    axes = rng.normal(size=(n - n // 2, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    pts = np.zeros((n, 8), np.float32)
    pts[:, 0:3] = np.concatenate([on, free])
    pts[:, 4:7] = np.concatenate([unit, axes])
    pts[:, 7] = rng.choice(np.float32([0.5, 3.0, np.inf]), n)
    return pts


def assert_masks_equal(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} masks differ, first {bad[0]}: got {int(got[bad[0]]):#018x}, want {int(want[bad[0]]):#018x}"


def check(ctx, pts, samples, want, what, **kw):
    got = ctx.occlusion_query(pts, samples, SEED, **kw)
    s = ctx.occlusion_statistics()
    assert_masks_equal(got, want, f"{what}, samples {samples}")
    assert s[0] == len(pts) and s[1] == ot.popcount(want) and s[2] <= len(pts) and s[3] == 0, (what, samples, s, ot.popcount(want))
    return s


# ---------------------------------------------------------------------------------------------
# soups and trees
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_tris,n_prims", [(1, 60, 3), (2, 400, 5), (3, 2000, 8)])
def test_masks_equal_the_oracle_on_every_tree(oracle, seed, n_tris, n_prims):
    scene = soup(seed, n_tris, n_prims)
    rng = np.random.default_rng(200 + seed)
    pts = soup_points(scene, rng)
    osc = oracle.Scene(scene)
    rays = {s: ot.rays(pts, s, SEED) for s in SAMPLES}
    truth = {s: ot.masks_of_rays(osc, rays[s]) for s in SAMPLES}
    for s in SAMPLES:                                  # the truth is not trivial, by the oracle alone
        share = ot.popcount(truth[s]) / (len(pts) * s)
        assert 0.1 <= share <= 0.9, (s, share)
        assert s == 64 or not (truth[s] >> np.uint64(s)).any()             # bits from `samples` up are 0
    # one primitive's vertices move: the truth of the refitted and of the rebuilt tree
    moved = copy.copy(scene)
    moved.vertices = scene.vertices.copy()
    a, b = _vertex_block(scene, 1)
    moved.vertices["pos"][a:b] += rng.normal(scale=0.3, size=(b - a, 3)).astype(np.float32)
    moved_truth = {s: ot.masks_of_rays(oracle.Scene(moved), rays[s]) for s in SAMPLES}
    assert any(not np.array_equal(moved_truth[s], truth[s]) for s in SAMPLES)
    ctx = lib.Context(64, 64)
    try:
        for what, options in (("device-built tree", {}), ("host-built tree", {"bvh_builder": 0}), ("presplit", {"bvh_presplit": 100}),
                              ("world axes", {"bvh_frame": 0}), ("2 LDS levels", {"lds_stack_levels": 2})):
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.upload_scene(scene)
            assert ctx.bvh_builder_used() == options.get("bvh_builder", 1)
            for s in SAMPLES:
                check(ctx, pts, s, truth[s], f"soup {seed}, {what}")
            for k in options:
                ctx.set_option(k, TREE_DEFAULTS[k])
        ctx.upload_scene(scene)
        ctx.update_vertices(moved.vertices[a:b], first_vertex=a)
        packed = lib.Context._occlusion_points_array(pts)
        out = np.zeros(len(pts), np.uint64)
        rc = ctx.L.vhr_occlusion_query(ctx.handle, packed.ctypes.data, len(packed), 16, SEED, abi.OCCLUSION_HOST_MEMORY, 0xFF, out.ctypes.data)    # an update is pending
        assert rc == -5 and "vhr_occlusion_query" in ctx.L.vhr_last_error(ctx.handle).decode(), rc
        ctx.refit_geometry()
        for s in SAMPLES:
            check(ctx, pts, s, moved_truth[s], f"soup {seed}, refitted")
        ctx.rebuild_geometry()
        assert ctx.rebuild_statistics()[0] >= 1
        for s in SAMPLES:
            check(ctx, pts, s, moved_truth[s], f"soup {seed}, rebuilt")
    finally:
        ctx.close()


def test_masks_are_the_ray_querys_bits_and_the_devices_rays_are_the_hosts(host):
    scene = soup(2, 400, 5)
    rng = np.random.default_rng(31)
    pts = soup_points(scene, rng)
    pts[::7, 4:7] *= np.float32(0.5)                    # axes that are no unit vectors
    pts[3::11, 4:7] = np.float32([1e-8, -1e-8, -1.0])   # the fixed basis
    pts[5::13, 4:7] = 0.0                               # the zero axis
    pts[6::17, 3] = 4.0                                 # tmin >= tmax where tmax is 0.5 or 3
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        for samples in SAMPLES:
            rays = ctx.debug_occlusion_rays(pts, samples, SEED)
            want = host.debug_occlusion_rays(pts, samples, SEED)
            assert np.array_equal(rays.view(np.uint32), want.view(np.uint32)), f"samples {samples}: the device's rays are not the host's"
            occ = ctx.ray_query(rays.reshape(-1, 8), any_hit=True).reshape(len(pts), samples)
            bits = (occ.astype(np.uint64) << np.arange(samples, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
            got = ctx.occlusion_query(pts, samples, SEED)
            assert_masks_equal(got, bits, f"samples {samples} against vhr_ray_query")
            assert ctx.occlusion_statistics()[1] == int(occ.sum())
        # a NaN axis: every ray has a NaN direction and hits nothing
        nan = pts[:70].copy()
        nan[:, 4] = np.nan
        assert not ctx.occlusion_query(nan, 16, SEED).any()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# every shape of a wave, from host and device memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 3, 64])
def test_every_shape_of_a_wave_from_host_and_device_memory(oracle, samples):
    import torch
    torch.cuda.set_device(0)
    P = max(1, 256 // samples)                          # the points a wave owns; a workgroup is two waves
    counts = sorted({1, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1, 4 * P + 3} - {0})
    scene = soup(2, 400, 5)
    rng = np.random.default_rng(77)
    pts = soup_points(scene, rng, counts[-1])
    want = ot.masks(oracle.Scene(scene), pts, samples, SEED)
    assert 0.1 <= ot.popcount(want) / (len(pts) * samples) <= 0.9
    stream = torch.cuda.Stream()
    tail = 5
    with torch.cuda.stream(stream):
        ctx = lib.Context(64, 64, stream=torch.cuda.current_stream().cuda_stream)
        try:
            assert ctx.current_stream() == stream.cuda_stream
            ctx.upload_scene(scene)
            d_pts = torch.from_numpy(pts).cuda()
            assert d_pts.data_ptr() % 16 == 0
            for n in counts:
                from_host = ctx.occlusion_query(pts[:n], samples, SEED)
                assert_masks_equal(from_host, want[:n], f"host memory, count {n}, samples {samples}")
                out = torch.full(((n + tail) * 8,), 0xCD, dtype=torch.uint8, device="cuda")
                assert out.data_ptr() % 8 == 0
                ctx.occlusion_query_device(d_pts.data_ptr(), n, samples, out.data_ptr(), SEED)
                raw = out.cpu().numpy()                                          # (.cpu() waits on the current stream)
                assert (raw[n * 8:] == 0xCD).all(), f"count {n}: bytes behind mask `count` were written"
                assert_masks_equal(raw[:n * 8].view(np.uint64), want[:n], f"device memory, count {n}, samples {samples}")
                s = ctx.occlusion_statistics()
                assert s[0] == n and s[1] == ot.popcount(want[:n]) and s[3] == 0, (n, s)
            # count == 0 launches nothing
            out = torch.full((32,), 0xCD, dtype=torch.uint8, device="cuda")
            ctx.occlusion_query_device(d_pts.data_ptr(), 0, samples, out.data_ptr(), SEED)
            assert (out.cpu().numpy() == 0xCD).all() and ctx.L.vhr_occlusion_query(ctx.handle, None, 0, samples, SEED, 0, 0xFF, None) == 0
            assert ctx.occlusion_query(pts[:0], samples).shape == (0,)
            # the argument checks on a device context
            assert ctx.L.vhr_occlusion_query(ctx.handle, 0x1008, 5, 4, SEED, 0, 0xFF, 0x2000) == -1 and "16-byte" in ctx.L.vhr_last_error(ctx.handle).decode()
            assert ctx.L.vhr_occlusion_query(ctx.handle, 0x1000, 5, 4, SEED, 0, 0xFF, 0x2004) == -1 and "8-byte" in ctx.L.vhr_last_error(ctx.handle).decode()
            assert ctx.L.vhr_occlusion_query(ctx.handle, 0x1000, 5, 65, SEED, 0, 0xFF, 0x2000) == -1 and "samples 65" in ctx.L.vhr_last_error(ctx.handle).decode()
        finally:
            ctx.close()


# ---------------------------------------------------------------------------------------------
# the binary64 launch
# ---------------------------------------------------------------------------------------------
def grazing_scene(rays, rng, n):
    """One triangle for each of n of the rays: its plane contains the ray's line, tilted by 0 or 1e-7 .. 1e-3, it sits 0.5 - 2 along the ray and the
    ray crosses it through its interior, an edge or a corner (the mirror image of _grazing_rays in tests/test_gpu_ray_query.py)."""
    k = rng.choice(len(rays), n, replace=False)
    o, d = rays[k, 0:3].astype(np.float64), rays[k, 4:7].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = np.cross(d, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    nrm = np.cross(d, w)
    a = d + rng.choice([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3], n)[:, None] * nrm          # in the triangle's plane, the ray's direction up to the tilt
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    c = o + rng.uniform(0.5, 2.0, (n, 1)) * d                                         # where the ray meets the plane
    size = 10.0 ** rng.uniform(-1.5, 0.0, (n, 1))
    th, ph = rng.uniform(0, 2 * np.pi, (n, 1)), rng.uniform(0.3, np.pi - 0.3, (n, 1))
    e1 = size * (np.cos(th) * a + np.sin(th) * w)
    e2 = size * (np.cos(th + ph) * a + np.sin(th + ph) * w)
    kind = rng.integers(0, 4, n)
    bu, bv = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = bu + bv > 1
    bu[flip], bv[flip] = 1 - bu[flip], 1 - bv[flip]
    bu[kind == 1] = 0.0
    bv[kind == 2] = 1.0 - bu[kind == 2]
    bu[kind == 3], bv[kind == 3] = 0.0, 0.0
    v0 = c - bu[:, None] * e1 - bv[:, None] * e2
    tri = np.stack([v0, v0 + e1, v0 + e2], axis=1).astype(np.float32)
    pos = tri.reshape(-1, 3)
    normals = np.repeat(nrm, 3, axis=0).astype(np.float32)
    uv = np.zeros((len(pos), 2), np.float32)
    idx = np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)
    b = scenes._Builder()
    half = (n // 2) * 3
    b.add((pos[:half], normals[:half], uv[:half], idx[:n // 2]))
    b.add((pos[half:], normals[half:], uv[half:], idx[:n - n // 2]))
    camera = dict(position=(0.0, 2.0, 8.0), yaw=0.0, pitch=0.0, yfov=0.9, znear=0.1, dolly=(0.0, 0.0, -0.01))
    return b.finish("grazing", camera, directional_light((0.25, -0.9, 0.3)))


def test_grazing_triangles_take_the_binary64_launch(oracle, host):
    rng = np.random.default_rng(23)
    n, samples = 500, 8
    pts = np.zeros((n, 8), np.float32)
    gx, gz = np.divmod(np.arange(n), 25)
    pts[:, 0:3] = np.stack([gx * 10.0, np.zeros(n), gz * 10.0], axis=1) + rng.uniform(-1, 1, (n, 3))      # well separated: 10 apart, reach 5
    axes = rng.normal(size=(n, 3))
    pts[:, 4:7] = axes / np.linalg.norm(axes, axis=1, keepdims=True)
    pts[:, 7] = 5.0
    rays = host.debug_occlusion_rays(pts, samples, SEED)
    scene = grazing_scene(rays.reshape(-1, 8), rng, 2000)
    assert scene.triangle_count == 2000
    want = ot.masks_of_rays(oracle.Scene(scene), ot.rays(pts, samples, SEED))
    assert 0.1 <= ot.popcount(want) / (n * samples) <= 0.9
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        # the precondition, held against the existing kernel: these rays do send vhr_ray_query to its binary64 launch
        occ = ctx.ray_query(rays.reshape(-1, 8), any_hit=True)
        assert ctx.ray_query_statistics()[2] > 0, ctx.ray_query_statistics()
        s = check(ctx, pts, samples, want, "grazing triangles")
        print(f"binary64: vhr_ray_query redid {ctx.ray_query_statistics()[2]} rays, vhr_occlusion_query {s[2]} of {n} points")
        assert 0 < s[2] <= n, s
        assert int(occ.sum()) == s[1]
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# cull masks
# ---------------------------------------------------------------------------------------------
def test_cull_masks_restrict_the_truth(oracle):
    scene = soup(2, 400, 5)
    rng = np.random.default_rng(41)
    pts = soup_points(scene, rng)
    samples = 16
    rays = ot.rays(pts, samples, SEED)
    plain = ot.masks_of_rays(oracle.Scene(scene), rays)
    prim_masks = np.array([0x01, 0x02, 0x03, 0x01, 0x02, 0x03], np.uint8)[:len(scene.primitives)]
    assert len(prim_masks) == len(scene.primitives) == 6
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        s_plain = check(ctx, pts, samples, plain, "no masks set")
        ctx.set_primitive_masks(prim_masks)
        for cull in (0xFF, 0x01, 0x02, 0):
            keep = (prim_masks & cull) != 0
            if keep.any():
                part = copy.copy(scene)
                part.primitives = scene.primitives[keep]
                want = ot.masks_of_rays(oracle.Scene(part), rays)
            else:
                want = np.zeros(len(pts), np.uint64)
            s = check(ctx, pts, samples, want, f"cull_mask {cull:#x}", cull_mask=cull)
            if cull == 0xFF:
                assert np.array_equal(want, plain) and s == s_plain              # the mask does not act: the plain kernels, the same statistics
            elif cull == 0:
                assert s[1:] == [0, 0, 0]
            else:
                assert 0 < ot.popcount(want) < ot.popcount(plain)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# no geometry, and no side effects
# ---------------------------------------------------------------------------------------------
def test_a_context_without_geometry_returns_zeros():
    ctx = lib.Context(64, 64)
    try:
        assert ctx.occlusion_statistics() == [0, 0, 0, 0]
        pts = np.zeros((300, 8), np.float32)
        pts[:, 6], pts[:, 7] = 1.0, np.inf
        for samples in (1, 7, 64):
            got = ctx.occlusion_query(pts, samples, SEED)
            assert got.shape == (300,) and not got.any() and ctx.occlusion_statistics() == [300, 0, 0, 0]
    finally:
        ctx.close()


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_queries_between_and_inside_frames_leave_the_frames_identical(frames_in_flight):
    """The rig of the other queries' tests of the same name: an occlusion query from the G-Buffer Pass's epilogue (on the stream the next pass is
    ordered on) and one between frames (on the context's) -- the frames are the frames without them, and the masks are a fresh context's."""
    import torch
    from vulkanhybridrenderer_amd.harness import HybridFrameLoop
    W, H, N = 480, 270, 5
    scene = scenes.sponza_proc(0.2)
    rng = np.random.default_rng(19)
    inside_p, between_p = soup_points(scene, rng, 1000), soup_points(scene, rng, 1900)

    def run(with_queries):
        loop = HybridFrameLoop(scene, W, H, N, shadow=True, ao_spp=2, reflections=1, denoise=True, frames_in_flight=frames_in_flight)
        ctx = loop.ctx
        results, stats = [], []
        try:
            d_inside, d_between = torch.from_numpy(inside_p).cuda(), torch.from_numpy(between_p).cuda()
            out_between = torch.zeros(len(between_p), dtype=torch.int64, device="cuda")
            out_inside = torch.zeros(len(inside_p), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            streams = set()
            if with_queries:
                def inside(c):
                    streams.add(c.current_stream())
                    c.occlusion_query_device(d_inside.data_ptr(), len(inside_p), 8, out_inside.data_ptr(), SEED)
                ctx.set_pass_epilogue("G-Buffer Pass", inside)
            images = []
            for i in range(N):
                loop.frame(i)
                if with_queries:
                    streams.add(ctx.current_stream())
                    ctx.occlusion_query_device(d_between.data_ptr(), len(between_p), 16, out_between.data_ptr(), SEED)
                if i % 2 == 1 or i == N - 1:
                    ctx.synchronize()
                    images.append([ctx.download(lib.RAYTRACED), ctx.download(lib.DENOISED), ctx.download(lib.REFLECTIONS)])
                    if with_queries:
                        results.append((out_between.cpu().numpy().view(np.uint64).copy(), out_inside.cpu().numpy().view(np.uint64).copy()))
                        stats.append(ctx.occlusion_statistics())
            return images, results, stats, len(streams)
        finally:
            loop.close()

    plain, _, _, _ = run(False)
    queried, results, stats, n_streams = run(True)
    assert n_streams == frames_in_flight                      # one stream, or the front stream and the context's
    for c, (a, b) in enumerate(zip(plain, queried)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), f"checkpoint {c}, image {j}: a frame around queries differs"
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        want_between, want_inside = ctx.occlusion_query(between_p, 16, SEED), ctx.occlusion_query(inside_p, 8, SEED)
    finally:
        ctx.close()
    assert 0.05 < ot.popcount(want_between) / (16 * len(between_p)) < 0.95
    for (between, inside), s in zip(results, stats):
        assert_masks_equal(between, want_between, "between frames")
        assert_masks_equal(inside, want_inside, "inside a pass")
        assert s[:2] == [len(between_p), ot.popcount(want_between)] and s[3] == 0, s     # the last query's counters: the pass's query did not touch them
