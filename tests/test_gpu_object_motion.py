""""object_motion_vectors" on the device: the contract of the previous records (the refit kernels' motion instantiations against truths read
before each update, and against the host twin), a failed refit, and the stand-in G-buffer -- static scenes untouched bit for bit, moved
surfaces against a float64 truth built from the unchanged oracle's depth and the known affine maps, stopped objects, and the SVGF history
following geometry that moves with the camera."""
import numpy as np
import pytest

from tests import f2_scene
from tests import object_motion_cases as omc
from tests import partial_refit_cases as cases
from tests.helpers import GpuHybrid, f16
from tests.test_gpu_fuzz import soup
from tests.test_gpu_refit import _with
from vulkanhybridrenderer_amd import abi, camera, lib, scenes

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1
KEY = "object_motion_vectors"
SIZES = [(128, 80), (67, 45)]


# ---- the previous records ----
def _ctx(vertices, indices, primitives, host_only=False, **options):
    c = lib.Context(64, 64, host_only=host_only)
    for k, v in options.items():
        c.set_option(k, v)
    c.update_geometry(vertices, indices, primitives)
    return c


def _warm(scene, host_only=False, **options):
    c = _ctx(scene.vertices, scene.indices, scene.primitives, host_only=host_only, **options)
    c.set_option(KEY, 1)                                      # after the build: switching on makes the arrays
    c.update_vertices(scene.vertices)
    c.refit_geometry()
    return c


@pytest.mark.parametrize("builder", [1, 0])
def test_previous_is_the_last_state_bit_for_bit(oracle, builder):
    """Tests 2-4 of tests/test_object_motion_host.py on device contexts: A (dirty path), B (whole tree) and, for the host-built tree, the
    host-only H, whose previous records the walk holds equal to the device's bit for bit (all equal the same truth)."""
    scene = soup(3, 2000, 8)
    a, b = _warm(scene, bvh_builder=builder), _warm(scene, bvh_builder=builder)
    h = _warm(scene, host_only=True) if builder == 0 else None

    def fresh(vertices, primitives):
        c = _ctx(vertices, scene.indices, primitives, bvh_builder=builder)
        try:
            return c.triangle_records()
        finally:
            c.close()
    try:
        contexts = [(a, lambda c: c.refit_geometry_partial(force=True)), (b, lambda c: c.refit_geometry())]
        if h:
            contexts.append((h, lambda c: c.refit_geometry_partial(force=True)))
        for c, _ in contexts:
            omc.assert_settled(c, "after the warm-up refit")
        omc.walk(scene, contexts, fresh)
        assert a.partial_refit_statistics()["partial_refits"] == len(omc.SEQUENCE)
        if h:
            assert omc.same(a.triangle_records(previous=True), h.triangle_records(previous=True))
    finally:
        for c in (a, b, h):
            if c:
                c.close()


@pytest.mark.parametrize("partial", [True, False])
def test_a_failed_refit_does_not_count(oracle, partial):
    """Primitive 0's block with one NaN through the device-memory route: the refit refuses (an existing refusal), the records hold the attempt's
    values; after a finite block and a refit that succeeds, previous is the state before the failed attempt."""
    import torch
    scene = soup(3, 2000, 8)
    first, end = cases.vertex_blocks(scene)[0]
    moved = cases._moved(scene, first, end, np.random.default_rng(8))[2]
    bad = moved.copy()
    bad["pos"][3, 1] = np.nan
    a = _warm(scene)
    refit = (lambda: a.L.vhr_refit_geometry_partial(a.handle, lib.REFIT_FORCE_PARTIAL)) if partial else (lambda: a.L.vhr_refit_geometry(a.handle))
    try:
        # one refit that moves something else first, so that previous != current where the failed attempt will not look
        cases.apply(a, cases.updates(scene)[omc.SEQUENCE[0]])
        assert refit() == 0
        truth = a.triangle_records()
        stats = a.object_motion_statistics()
        dev = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).cuda()
        a.update_vertices_device(dev.data_ptr(), len(bad), first_vertex=first)
        assert refit() == INVALID_ARGUMENT and "non-finite" in a.L.vhr_last_error(a.handle).decode()
        assert a.object_motion_statistics() == stats
        good = torch.from_numpy(moved.view(np.uint8).reshape(-1).copy()).cuda()
        a.update_vertices_device(good.data_ptr(), len(moved), first_vertex=first)
        assert refit() == 0
        cur, prev = a.triangle_records(), a.triangle_records(previous=True)
        assert omc.same(prev, truth), "previous is not the state before the failed attempt"
        changed = omc.differing_rows(truth, cur)
        assert changed.sum() == cases.expected_dirty_records(scene, ("v", first, moved)) and np.isfinite(cur).all()
        assert a.object_motion_statistics()["differing_records"] == int(changed.sum())
    finally:
        a.close()


# ---- the G-buffer ----
class _Rig:
    """The hybrid path (shadows + AO + SVGF) behind the stand-in G-buffer with albedo."""

    def __init__(self, scene, W, H):
        self.ctx = lib.Context(W, H)
        self.ctx.upload_scene(scene)
        self.path = lib.HybridRenderPath(self.ctx, 0, 0, 2, True, 5, lambda c: c.standin_gbuffer_with_albedo(0))
        self.path.build()

    def frame(self, pfd):
        self.ctx.update_per_frame_ubo(0, pfd)
        self.ctx.execute(0, 0)
        self.ctx.synchronize()
        return {k: self.ctx.download(v) for k, v in (("normals", lib.NORMALS), ("motion", lib.MOTION), ("depth", lib.DEPTH), ("albedo", lib.ALBEDO),
                                                      ("denoised", lib.DENOISED))}

    def close(self):
        self.path.destroy()
        self.ctx.close()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("W,H", SIZES)
def test_static_scenes_are_untouched(oracle, W, H):
    sc = f2_scene.scene()
    frames = {}
    for on in (0, 1):
        rig = _Rig(sc, W, H)
        try:
            rig.ctx.set_option(KEY, on)
            frames[on] = []
            for pfd in camera.dolly_frames(sc, W, H, 3):
                rig.ctx.refit_geometry()                      # one refit call per frame, with nothing pending
                frames[on].append(rig.frame(pfd))
            assert rig.ctx.object_motion_statistics() == dict(active=on, differing_records=0, motion_launches=0)
        finally:
            rig.close()
    for i, (off, on) in enumerate(zip(frames[0], frames[1])):
        for name in off:
            assert _same_bits(off[name], on[name]), f"frame {i}: {name} differs with the option on and nothing moved"


def _motion64(pfd, depth, W, H, previous_position=None):
    """Float64 motion vectors from a depth image: P through the inverse of camera_proj * camera_view, then c - (ndc(prev_projview * P_prev) *
    0.5 + 0.5) with P_prev = previous_position(P) (default: P, camera motion only).  Returns (mv (H, W, 2), previous clip w, P)."""
    pv = abi.glm_to_mat(pfd["camera_proj"]) @ abi.glm_to_mat(pfd["camera_view"])
    ppv = abi.glm_to_mat(pfd["camera_proj_prev_frame"]) @ abi.glm_to_mat(pfd["camera_view_prev_frame"])
    y, x = np.mgrid[0:H, 0:W]
    c = np.stack([(x + 0.5) / W, (y + 0.5) / H], -1)
    ndc = np.concatenate([c * 2.0 - 1.0, depth.astype(np.float64)[..., None], np.ones((H, W, 1))], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        pw = ndc @ np.linalg.inv(pv).T
        P = pw[..., :3] / pw[..., 3:4]
        Pp = P if previous_position is None else previous_position(P)
        rp = np.concatenate([Pp, np.ones((H, W, 1))], -1) @ ppv.T
        mv = c - (rp[..., :2] / rp[..., 3:4] * 0.5 + 0.5)
    return mv, rp[..., 3], P


def _noise_floor(oracle_motion, mv64, covered):
    """E0: the largest residual beyond fp16 storage between the oracle's own motion.xy and the float64 construction from its depth."""
    res = np.abs(f16(oracle_motion)[..., :2].astype(np.float64) - mv64) - 2.0 ** -10 * np.abs(mv64)
    return float(max(res[covered].max(), 0.0))


def _affine(m):
    m = np.asarray(m, np.float64)
    return lambda P: P @ m[:3, :3].T + m[:3, 3]


def _moved_f2(sc):
    """FENCE: a new transform (rotation about y of 0.2 rad plus a translation).  FLOOR: an affine map of its vertex block (scale 1.05, a shear,
    a shift).  Returns (moved scene, the fence's (1, 16) transform, (first vertex, the floor's records), {primitive: world map of now -> before})."""
    fence_now = scenes.trs((0.35, 0.12, 0.2), rot_y=0.2)
    floor_map = np.eye(4)
    floor_map[:3, :3] = 1.05 * np.eye(3)
    floor_map[0, 2] = 0.06                                     # shear: x += 0.06 z
    floor_map[:3, 3] = (0.3, 0.04, 0.25)
    prims = sc.primitives.copy()
    fence_before = abi.glm_to_mat(prims["transform"][f2_scene.FENCE])
    prims["transform"][f2_scene.FENCE] = abi.mat_to_glm(fence_now @ fence_before)
    first, end = cases.vertex_blocks(sc)[f2_scene.FLOOR]
    v = sc.vertices.copy()
    v["pos"][first:end] = (v["pos"][first:end].astype(np.float64) @ floor_map[:3, :3].T + floor_map[:3, 3]).astype(np.float32)
    floor_t = abi.glm_to_mat(prims["transform"][f2_scene.FLOOR])
    back = {f2_scene.FENCE: fence_before @ np.linalg.inv(abi.glm_to_mat(prims["transform"][f2_scene.FENCE])),
            f2_scene.FLOOR: floor_t @ np.linalg.inv(floor_map) @ np.linalg.inv(floor_t)}
    return _with(sc, vertices=v, primitives=prims), prims["transform"][f2_scene.FENCE].reshape(1, 16), (first, v[first:end]), back


@pytest.mark.parametrize("W,H", SIZES)
def test_moved_geometry_reprojects_and_stopped_objects_stop(oracle, W, H):
    """Tests 11 and 12 of the issue.  Frames 0 and 1 static; FENCE and FLOOR move, one partial refit, frame 2; a refit call with nothing
    pending, frame 3.  On frame 2 everything but motion.xy equals the oracle's G-buffer of the moved scene bit for bit, motion.xy of the WALL
    too, and motion.xy of FENCE and FLOOR lies within 2^-10 |mv| + 4 E0 of the float64 truth (P from the oracle's depth, P_prev = A_prev
    A_cur^-1 P), E0 being the oracle's own residual against the same construction on the unmoved scene.  Frame 3 equals the oracle's bit for
    bit, from the plain kernel."""
    sc = f2_scene.scene()
    moved, fence_transform, (floor_first, floor_records), back = _moved_f2(sc)
    pfds = camera.dolly_frames(sc, W, H, 4)
    osc, osc2 = oracle.Scene(sc), oracle.Scene(moved)
    # E0, from the oracle alone, on the unmoved scene's frame 2
    n0, m0, d0 = osc.gbuffer(pfds[2], W, H)
    mv0, _, _ = _motion64(pfds[2], d0, W, H)
    E0 = _noise_floor(m0, mv0, d0 != 0)
    print(f"{W}x{H}: E0 = {E0:.3e} (cap {0.05 / max(W, H):.3e})")
    assert E0 < 0.05 / max(W, H), "the oracle alone breaks the cap: the scene is ill-conditioned"
    # the truth on frame 2
    n2, m2, d2, al2 = osc2.gbuffer(pfds[2], W, H, with_albedo=True)
    ids, covered = f16(n2)[..., 3], d2 != 0
    maps = {p: _affine(m) for p, m in back.items()}

    def before(P):
        out = P.copy()
        for p, f in maps.items():
            out[ids == p] = f(P[ids == p])
        return out
    truth, prev_w, _ = _motion64(pfds[2], d2, W, H, before)
    camera_only, _, _ = _motion64(pfds[2], d2, W, H)
    assert (prev_w[covered] > 0).all(), "a previous clip w <= 0: choose another motion"
    for p in (f2_scene.FENCE, f2_scene.FLOOR):
        on = covered & (ids == p)
        assert on.sum() > 20, p
        px = np.abs(truth - camera_only)[on] * (W, H)
        assert px.max() >= 1.0, f"primitive {p}: the true motion is within a pixel of the camera-only motion everywhere ({px.max():.2f} px)"
    assert (covered & (ids == f2_scene.WALL)).sum() > 20
    rig = _Rig(sc, W, H)
    try:
        ctx = rig.ctx
        ctx.set_option(KEY, 1)
        ctx.update_vertices(sc.vertices)                      # the first refit since the build is whole-tree: made here, so that the one below takes the dirty path
        ctx.refit_geometry()
        for pfd in pfds[:2]:
            ctx.refit_geometry()
            rig.frame(pfd)
        assert ctx.object_motion_statistics()["motion_launches"] == 0
        ctx.update_primitive_transforms(fence_transform, first_primitive=f2_scene.FENCE)
        ctx.update_vertices(floor_records, first_vertex=floor_first)
        ctx.refit_geometry_partial(force=True)
        assert ctx.partial_refit_statistics()["ran_as"] == 0
        fence_tris, floor_tris = (int(sc.primitives["index_count"][p]) // 3 for p in (f2_scene.FENCE, f2_scene.FLOOR))
        assert ctx.object_motion_statistics()["differing_records"] == fence_tris + floor_tris
        got = rig.frame(pfds[2])
        launches = ctx.object_motion_statistics()["motion_launches"]
        assert launches > 0
        # (a) nothing but motion.xy may change
        assert _same_bits(got["normals"], n2) and _same_bits(got["depth"], d2) and _same_bits(got["albedo"], al2)
        assert _same_bits(got["motion"][..., 2:], m2[..., 2:])
        # (b) what did not move keeps its bits
        wall = ids == f2_scene.WALL
        assert _same_bits(got["motion"][wall], m2[wall])
        assert _same_bits(got["motion"][~covered], m2[~covered])
        # (c) what moved, against the float64 truth
        mv = f16(got["motion"])[..., :2].astype(np.float64)
        on = covered & ((ids == f2_scene.FENCE) | (ids == f2_scene.FLOOR))
        err, bound = np.abs(mv - truth)[on], (2.0 ** -10 * np.abs(truth) + 4.0 * E0)[on]
        print(f"{W}x{H}: largest error {err.max():.3e}, largest error / bound {(err / bound).max():.3f}, "
              f"the oracle's camera-only motion misses the truth by up to {(np.abs(f16(m2)[..., :2] - truth)[on] * (W, H)).max():.2f} px")
        assert (err <= bound).all(), f"{int((err > bound).sum())} of {int(on.sum())} moved pixels miss the bound, worst by {(err / bound).max():.2f} x"
        # test 12: a refit call with nothing pending, and the objects have stopped
        ctx.refit_geometry_partial()
        assert ctx.object_motion_statistics() == dict(active=1, differing_records=0, motion_launches=launches)
        got3 = rig.frame(pfds[3])
        n3, m3, d3, al3 = osc2.gbuffer(pfds[3], W, H, with_albedo=True)
        assert _same_bits(got3["motion"], m3) and _same_bits(got3["normals"], n3) and _same_bits(got3["depth"], d3) and _same_bits(got3["albedo"], al3)
        assert ctx.object_motion_statistics()["motion_launches"] == launches, "the plain kernel was to run"
    finally:
        rig.close()


# ---- end to end ----
RIG_STEP = (0.3, 0.1, 0.0)          # metres per frame, geometry and camera alike: about four pixels of camera-only motion at 128 x 80
RIG_FACTOR = 64.9                   # k of rmse_on < rmse_off / k: the geometric mean of 1 and the ratio measured on an MI355X (4212.6), see the test


def _rig_run(scene, W, H, frames, option, step):
    """`frames` frames of shadows + AO + SVGF; every primitive's transform and the camera translated by f * step at frame f (step None: nothing
    moves).  Returns (final denoised, final depth, the largest |motion.xy| over covered pixels of frames >= 1)."""
    g = GpuHybrid(scene, W, H, reflections=False, gbuffer="standin")
    try:
        g.ctx.set_option(KEY, option)
        drv = camera.FrameDriver(W, H, scene.camera["yfov"], scene.camera["znear"], scene.light, aspect=scene.camera.get("aspect"))
        pos = np.asarray(scene.camera["position"], np.float64)
        base = [abi.glm_to_mat(t) for t in scene.primitives["transform"]]
        largest = 0.0
        for f in range(frames):
            offset = np.zeros(3) if step is None else f * np.asarray(step, np.float64)
            if step is not None and f > 0:
                shift = np.eye(4)
                shift[:3, 3] = offset
                g.ctx.update_primitive_transforms(np.stack([abi.mat_to_glm(shift @ m) for m in base]))
            g.ctx.refit_geometry_partial()                    # one refit call per frame
            g.frame(drv.next(pos + offset, scene.camera["yaw"], scene.camera["pitch"]))
            depth = g.ctx.download(lib.DEPTH)
            if f > 0:
                largest = max(largest, float(np.abs(f16(g.ctx.download(lib.MOTION))[..., :2][depth != 0]).max()))
        return f16(g.ctx.download(lib.DENOISED))[..., :2].astype(np.float64), depth, largest
    finally:
        g.close()


def test_the_history_follows_the_geometry(oracle):
    """Test 13 of the issue: tiny_scene at 128 x 80, 6 frames.  Run R moves every primitive and the camera together, so the picture stands
    still; run S is static.  RMSE of R's final denoised image against S's over covered pixels, with the option on and off (off is what the
    library did before the option existed: camera-only motion vectors of several pixels on a picture that does not move).

    Measured on an MI355X (also in profiles/object_motion_rate.jsonl): rmse_on = 3.5109e-05, rmse_off = 1.4790e-01, ratio 4212.6, so k =
    sqrt(4212.6) = 64.9.  With the option on the differences are rounding-level (the largest |motion.xy| is 3.2e-06 against 2.3e-06 on the
    static scene and a bound of 4 E0 = 9.1e-06); with it off the camera-only motion is 9.5 pixels and the history is fetched from there."""
    scene = scenes.tiny_scene()
    W, H, frames = 128, 80, 6
    den_s, depth_s, still = _rig_run(scene, W, H, frames, 0, None)
    den_on, depth_on, moving_on = _rig_run(scene, W, H, frames, 1, RIG_STEP)
    den_off, _, moving_off = _rig_run(scene, W, H, frames, 0, RIG_STEP)
    covered = (depth_s != 0) & (depth_on != 0)
    assert covered.mean() > 0.5                           # (the camera sees sky above the back wall: the oracle covers 72 % of the pixels)
    rmse_on = float(np.sqrt(np.mean((den_on - den_s)[covered] ** 2)))
    rmse_off = float(np.sqrt(np.mean((den_off - den_s)[covered] ** 2)))
    # E0 as in the test above, from the oracle alone: its own motion.xy on the static scene under the static camera, where the truth is 0
    drv = camera.FrameDriver(W, H, scene.camera["yfov"], scene.camera["znear"], scene.light, aspect=scene.camera.get("aspect"))
    pfd = [drv.next(scene.camera["position"], scene.camera["yaw"], scene.camera["pitch"]) for _ in range(2)][1]
    _, m0, d0 = oracle.Scene(scene).gbuffer(pfd, W, H)
    E0 = _noise_floor(m0, _motion64(pfd, d0, W, H)[0], d0 != 0)
    assert 0 < E0 < 0.05 / max(W, H)
    print(f"rmse_on {rmse_on:.4e}, rmse_off {rmse_off:.4e}, ratio {rmse_off / max(rmse_on, 1e-300):.1f}; largest |motion.xy|: static {still:.3e}, "
          f"rig with the option on {moving_on:.3e}, off {moving_off:.3e} ({moving_off * max(W, H):.1f} px)")
    assert moving_off * max(W, H) >= 3.0, "the camera-only motion was to be several pixels"
    assert rmse_on < rmse_off / RIG_FACTOR
    assert moving_on <= 4.0 * E0, f"with the option on the picture stands still: |motion.xy| {moving_on:.3e} > 4 E0 = {4 * E0:.3e}"
