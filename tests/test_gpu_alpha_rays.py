"""Alpha-tested rays on the GPU: "alpha_test_rays" (the hybrid path's shadow, AO and mirror rays skip what gbuf.frag:20-32 discards) and
VHR_RAY_QUERY_ALPHA_TEST.  The oracle's rays know no alpha and stay as they are, so three independent legs carry the proof:

  L1  the rule is sampled correctly: rays through the texel centres of a 16 x 16 checker, by ray query;
  L2  every kernel applies it: scene A (occluders of CONSTANT alpha, tests/alpha_scenes.uniform_pair) with the switch on is, bit for
      bit, the EXISTING oracle on scene B = A without the occluders the rule discards (one G-buffer: tests/test_alpha_rays_host.py);
  L3  all forms of a kernel agree where alpha varies per texel (fence_scene): against the literal per-pixel kernels.

Then alpha with the deferred binary64 decision, no side effects on contexts that have the switch off, and the plain kernels where
nothing can discard."""
import json
import os

import numpy as np
import pytest

from tests import alpha_scenes
from tests.alpha_scenes import assert_hits_equal, grazing_rays, oracle_hits
from tests.helpers import GpuHybrid, assert_reflections_identical, oracle_frames
from vulkanhybridrenderer_amd import abi, camera, lib, ray_queries, scenes
from vulkanhybridrenderer_amd.scenes import _Builder, plane

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = abi.RAY_MISS
W, H, FRAMES = 72, 56, 3

# every form of the six kernels and every option that changes how they walk: (name, options, ray statistics)
SETTINGS = [
    ("defaults", {}, False),
    ("per-pixel kernels", {"raygen_variant": 0, "reflection_variant": 0}, False),
    ("raygen_variant 0", {"raygen_variant": 0}, False),
    ("reflection_variant 0", {"reflection_variant": 0}, False),
    ("compact_nodes 0", {"compact_nodes": 0}, False),
    ("raygen_steal 0", {"raygen_steal": 0}, False),
    ("raygen_steal 8", {"raygen_steal": 8}, False),
    ("1 wave per block", {"raygen_waves_per_block": 1}, False),
    ("2 waves per block", {"raygen_waves_per_block": 2}, False),
    ("4 waves per block", {"raygen_waves_per_block": 4}, False),
    ("5 tile rows", {"raygen_tile_rows": 5}, False),
    ("spill instantiations", {"lds_stack_levels": 1, "reflection_lds_stack_levels": 1}, False),
    ("statistics", {}, True),
    ("statistics, compact_nodes 0, spill", {"compact_nodes": 0, "lds_stack_levels": 1, "reflection_lds_stack_levels": 1}, True),
]
IDS = [s[0] for s in SETTINGS]


class Rig:
    """One hybrid context per scene for the whole module (host-supplied G-buffers, no denoiser): every case sets its options, runs its
    frames and puts the defaults back -- the switch is read at every launch."""

    def __init__(self, scene):
        self.g = GpuHybrid(scene, W, H, denoise=False)
        self.defaults = lib.option_table()

    def run(self, frames, options=None, stats=False, alpha=1, bounces=1):
        ctx = self.g.ctx
        options = options or {}
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_ray_statistics(stats)
        ctx.set_trace_params(abi.default_trace_params(reflections=bounces))
        out = []
        try:
            for f in frames:
                ctx.set_option("alpha_test_rays", alpha)
                self.g.frame(f["pfd"], f["gbuf"])
                out.append(dict(raytraced=ctx.download(lib.RAYTRACED).copy(), reflections=ctx.download(lib.REFLECTIONS).copy(),
                                alpha_launches=ctx.alpha_launches(), b64=ctx.binary64_statistics() if stats else None,
                                overflows=ctx.ray_statistics()["stack_overflows"] if stats else 0))
        finally:
            for k in options:
                ctx.set_option(k, self.defaults[k][0])
            ctx.set_ray_statistics(False)
            ctx.set_option("alpha_test_rays", 0)
        return out


@pytest.fixture(scope="module")
def pair(oracle):
    """Scenes A and B, the oracle's frames of both (one and two bounces on B), and a context holding A."""
    A, B = alpha_scenes.uniform_pair()
    want = {("A", 1): oracle_frames(oracle, A, W, H, FRAMES, abi.default_trace_params(), denoise=False)[0]}
    for bounces in (1, 2):
        want[("B", bounces)] = oracle_frames(oracle, B, W, H, FRAMES, abi.default_trace_params(reflections=bounces), denoise=False)[0]
    rig = Rig(A)
    yield dict(A=A, B=B, want=want, rig=rig)
    rig.g.close()


def _assert_frames(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        diff = (g["raytraced"] != w["shadow_ao"]).any(-1)
        assert not diff.any(), f"{what}, frame {i}: {int(diff.sum())} RAYTRACED texels differ from the oracle, first at {np.argwhere(diff)[:4].tolist()}"
        assert_reflections_identical(g["reflections"], w["reflections"], f"{what}, frame {i}: reflections")
        assert g["overflows"] == 0


# ---------------------------------------------------------------------------------------------
# L2: every hybrid kernel against the existing oracle, through the cut-out scene
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name,options,stats", SETTINGS, ids=IDS)
def test_L2_rays_on_A_see_the_oracles_B(pair, name, options, stats, bounces):
    want = pair["want"][("B", bounces)]                  # (its G-buffers are A's: tests/test_alpha_rays_host.py)
    got = pair["rig"].run(want, options, stats, alpha=1, bounces=bounces)
    _assert_frames(got, want, f"alpha_test_rays 1, {name}, {bounces} bounce(s)")
    # the alpha instantiations ran: the shadow / AO launch and -- where the mirror ray has a launch of its own -- that one
    assert all(g["alpha_launches"] == (1 if options.get("raygen_variant", 1) == 0 else 2) for g in got), [g["alpha_launches"] for g in got]


def test_L2_the_switch_toggles_per_launch_both_ways(pair):
    a, b = pair["want"][("A", 1)], pair["want"][("B", 1)]
    rig = pair["rig"]
    for i in range(FRAMES):
        for alpha in (1, 0, 1, 0):
            got = rig.run([a[i]], alpha=alpha)
            _assert_frames(got, [(b if alpha else a)[i]], f"frame {i}, alpha_test_rays {alpha}")
            assert got[0]["alpha_launches"] == (2 if alpha else 0)
    for name, options, stats in SETTINGS[:2]:            # off: today's images on A, solid occluders and all
        _assert_frames(rig.run(a, options, stats, alpha=0), a, f"alpha_test_rays 0, {name}")


def _scene_rays(scene, seed, n):
    lo, hi = ray_queries.scene_bounds(scene)
    return ray_queries.random_rays(np.random.default_rng(seed), n, lo, hi, margin=0.2, tmins=(0.0, 0.01), tmaxs=(np.inf, 3.0, 20.0, 1e4))


def test_L2_flagged_query_on_A_equals_the_plain_query_on_B(pair):
    rays = _scene_rays(pair["A"], 5, 1000)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(pair["B"])
        want, occ = ctx.ray_query(rays), ctx.ray_query(rays, any_hit=True)
        ctx.upload_scene(pair["A"])
        plain, plain_occ = ctx.ray_query(rays), ctx.ray_query(rays, any_hit=True)
        got, got_occ = ctx.ray_query(rays, alpha_test=True), ctx.ray_query(rays, any_hit=True, alpha_test=True)
        assert ctx.ray_query_statistics()[3] == 0
    finally:
        ctx.close()
    assert_hits_equal(got, want, "flagged closest hit on A against the plain one on B")
    assert np.array_equal(got_occ, occ)
    # the flag acts (the discarded occluders stop rays of the plain query) and the batch is no trivial one
    assert (plain.view(np.uint32).reshape(-1, 6) != want.view(np.uint32).reshape(-1, 6)).any(1).sum() >= 20 and (plain_occ != occ).sum() >= 20
    assert 0.2 < occ.mean() < 0.98


# ---------------------------------------------------------------------------------------------
# L1: texel centres, by ray query
# ---------------------------------------------------------------------------------------------
def _checker_scenes():
    """Primitive 0: an opaque wall at z = -1; primitive 1: a masked quad at z = 0, one uv unit across, under a 16 x 16-texel NEAREST /
    CLAMP checker of alpha 255 / 0.  Returns (both, wall only, quad only, alpha[ty, tx])."""
    yy, xx = np.mgrid[0:16, 0:16]
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., :3] = [200, 150, 50]
    img[..., 3] = np.where((xx + yy) % 2 == 0, 255, 0)
    tex = [dict(rgba8=img, format=abi.FORMAT_R8G8B8A8_SRGB, mag=abi.FILTER_NEAREST, min=abi.FILTER_NEAREST,
                address_u=abi.ADDRESS_CLAMP_TO_EDGE, address_v=abi.ADDRESS_CLAMP_TO_EDGE)]

    def build(wall, quad):
        b = _Builder()
        if wall:
            b.add(plane([-1, -1, -1], [3, 0, 0], [0, 3, 0], 1, 1), base_color=(0.5, 0.5, 0.5, 1.0))
        if quad:
            b.add(plane([0, 0, 0], [1, 0, 0], [0, 1, 0], 1, 1), base_color_texture=0)
            b.p[-1]["material"]["alpha_mask"] = 1
        return b.finish("checker", scenes.tiny_scene().camera, scenes.tiny_scene().light, tex)
    return build(True, True), build(True, False), build(False, True), img[..., 3]


def _checker_rays():
    """256 perpendicular rays through the texel centres, then 744 tilted ones aimed at points at least 0.2 texel inside a texel and 0.1
    texel off the quad's diagonal: 1 000 rays (no multiple of 64), none near an edge of either quad.  Returns (rays, texel x, texel y)."""
    rng = np.random.default_rng(16)
    ty, tx = np.mgrid[0:16, 0:16]
    cx, cy = (tx.reshape(-1) + 0.5) / 16.0, (ty.reshape(-1) + 0.5) / 16.0
    rx, ry = np.zeros(0), np.zeros(0)
    while len(rx) < 744:
        ix, iy = rng.integers(0, 16, 2000), rng.integers(0, 16, 2000)
        px, py = (ix + rng.uniform(0.2, 0.8, 2000)) / 16.0, (iy + rng.uniform(0.2, 0.8, 2000)) / 16.0
        keep = np.abs(px - py) > 0.1 / 16.0                       # plane()'s two triangles meet on the diagonal u == v
        rx, ry = np.concatenate([rx, px[keep]]), np.concatenate([ry, py[keep]])
    tgt = np.stack([np.concatenate([cx, rx[:744]]), np.concatenate([cy, ry[:744]]), np.zeros(1000)], 1)
    org = tgt + np.array([0.0, 0.0, 1.0])
    org[256:, :2] += rng.uniform(-0.3, 0.3, (744, 2))
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((1000, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = org, d, 0.0, np.inf
    return rays, np.floor(tgt[:, 0] * 16).astype(int), np.floor(tgt[:, 1] * 16).astype(int)


@pytest.mark.parametrize("route", ["host memory", "device pointers"])
def test_L1_texel_centres_of_a_checker(oracle, route):
    import torch
    both, wall_only, quad_only, alpha = _checker_scenes()
    rays, tx, ty = _checker_rays()
    opaque = alpha[ty, tx] == 255
    assert opaque[:256].sum() == 128 and 300 < opaque[256:].sum() < 450
    ctx = lib.Context(64, 64)

    def query(any_hit=False, alpha_test=False):
        if route == "host memory":
            return ctx.ray_query(rays, any_hit=any_hit, alpha_test=alpha_test)
        d_rays = torch.from_numpy(rays).cuda()
        out = torch.zeros(len(rays) if any_hit else (len(rays), 6), dtype=torch.uint8 if any_hit else torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.ray_query_device(d_rays.data_ptr(), len(rays), out.data_ptr(), any_hit=any_hit, alpha_test=alpha_test)
        ctx.synchronize()
        return out.cpu().numpy().astype(bool) if any_hit else out.cpu().numpy().view(abi.ray_hit_dtype).reshape(-1)
    try:
        ctx.upload_scene(wall_only)
        on_wall = query()
        ctx.upload_scene(quad_only)
        assert np.array_equal(query(any_hit=True, alpha_test=True), opaque)            # without the wall: any hit == the texel is opaque
        assert query(any_hit=True).all()
        ctx.upload_scene(both)
        plain, plain_any = query(), query(any_hit=True)
        got, got_any = query(alpha_test=True), query(any_hit=True, alpha_test=True)
    finally:
        ctx.close()
    # without the flag: today's results, the oracle's
    want, occ = oracle_hits(oracle.Scene(both), rays, use_bvh=False)
    assert_hits_equal(plain, want, "unflagged query")
    assert np.array_equal(plain_any, occ) and (plain["geometry_index"] == 1).all() and (on_wall["geometry_index"] == 0).all()
    # with it: every ray ends on something (the wall), over an opaque texel on the quad exactly as the plain query does, over a hole on the
    # wall exactly as the plain query on the wall-only scene does (t, u, v, geometry_index, primitive_index as bits)
    assert got_any.all()
    assert_hits_equal(got[opaque], plain[opaque], "over opaque texels")
    assert_hits_equal(got[~opaque], on_wall[~opaque], "over holes")


# ---------------------------------------------------------------------------------------------
# L3: per-texel alpha, the forms against each other
# ---------------------------------------------------------------------------------------------
def _fence_frames(oracle, scene):
    """pfd + the oracle's G-buffer (which cuts the holes) per dolly frame"""
    osc = oracle.Scene(scene)
    return [dict(pfd=pfd, gbuf=osc.gbuffer(pfd, W, H)) for pfd in camera.dolly_frames(scene, W, H, FRAMES)]


@pytest.fixture(scope="module")
def fence(oracle):
    scene = alpha_scenes.fence_scene()
    rig = Rig(scene)
    frames = _fence_frames(oracle, scene)
    literal = {b: rig.run(frames, {"raygen_variant": 0, "reflection_variant": 0}, alpha=1, bounces=b) for b in (1, 2)}
    yield dict(scene=scene, rig=rig, frames=frames, literal=literal)
    rig.g.close()


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name,options,stats", SETTINGS[:1] + SETTINGS[2:], ids=IDS[:1] + IDS[2:])
def test_L3_every_form_equals_the_literal_kernels_on_the_fence(fence, name, options, stats, bounces):
    got = fence["rig"].run(fence["frames"], options, stats, alpha=1, bounces=bounces)
    for i, (g, w) in enumerate(zip(got, fence["literal"][bounces])):
        assert np.array_equal(g["raytraced"], w["raytraced"]), f"{name}, frame {i}: {int((g['raytraced'] != w['raytraced']).any(-1).sum())} RAYTRACED texels differ from raygen_kernel's"
        assert_reflections_identical(g["reflections"], w["reflections"], f"{name}, frame {i}: reflections against reflection_kernel's")
        assert g["overflows"] == 0 and g["alpha_launches"] >= 1


def test_L3_the_switch_acts_on_the_fence(oracle, fence):
    """The oracle's opaque rays on the fence scene are today's images (asserted); with the switch on the shadow of the fence's holes, of the
    masked quad, of the ramp's transparent side and of the awning's cells is gone: at least 100 shadow texels of every frame differ.
    Measured on an MI355X at 72 x 56: 378, 408 and 395 shadow texels differ in frames 0, 1 and 2 (of ~3 630 covered; the oracle with the
    masked primitives solid against the oracle without them differs in 824, 889 and 878: an upper bound, about half of which is hole)."""
    osc = oracle.Scene(fence["scene"])
    tp = abi.default_trace_params()
    off = fence["rig"].run(fence["frames"], alpha=0)
    for i, (f, o, on) in enumerate(zip(fence["frames"], off, fence["literal"][1])):
        sa, refl, _, _ = osc.raygen(f["pfd"], tp, f["gbuf"][0], f["gbuf"][2])
        assert np.array_equal(o["raytraced"], sa), f"frame {i}: alpha_test_rays 0 differs from the oracle"
        assert_reflections_identical(o["reflections"], refl, f"frame {i}: alpha_test_rays 0")
        changed = int((on["raytraced"][..., 0] != sa[..., 0]).sum())
        print(f"fence frame {i}: {changed} shadow texels differ between alpha_test_rays 0 and 1")
        assert changed >= 100, (i, changed)
        # a ray can only LOSE occluders: no texel lit with the switch off is shadowed with it on
        assert not ((sa[..., 0] == 0x3c00) & (on["raytraced"][..., 0] != 0x3c00)).any()


def test_L3_a_cutoff_above_one_makes_the_masked_primitives_vanish(oracle, fence):
    """alpha_cutoff = 1.5 on every masked primitive: all of their texels are discarded, and the rays see the scene without them -- which is
    the oracle's on that scene (payloads do not depend on primitive indices), under the G-buffer of the scene with them."""
    gone = alpha_scenes.fence_scene(cutoff_scale=1.5)
    without = alpha_scenes.fence_scene(without_masked=True)
    frames = _fence_frames(oracle, gone)
    osc = oracle.Scene(without)
    tp = abi.default_trace_params()
    rig = Rig(gone)
    try:
        for name, options, stats in (SETTINGS[0], SETTINGS[1], SETTINGS[11]):
            got = rig.run(frames, options, stats, alpha=1)
            for i, (f, g) in enumerate(zip(frames, got)):
                sa, refl, _, _ = osc.raygen(f["pfd"], tp, f["gbuf"][0], f["gbuf"][2])
                assert np.array_equal(g["raytraced"], sa), f"{name}, frame {i}"
                assert_reflections_identical(g["reflections"], refl, f"{name}, frame {i}")
    finally:
        rig.g.close()


# ---------------------------------------------------------------------------------------------
# alpha with the deferred binary64 decision
# ---------------------------------------------------------------------------------------------
def test_ray_query_alpha_with_the_binary64_launch():
    """The grazing pairs of tests/golden/kat_decision_vi.json as a scene -- the pairs' triangles, the odd ones on a primitive the rule
    discards (untextured, alpha 0) that comes last -- and as rays, with rays grazing those triangles around them: some take the second
    launch (decision (vi)'s binary64 half), and the flagged query still equals the plain query on the scene without the discarded half."""
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_decision_vi.json")))
    h = lambda xs: np.array([float.fromhex(x) for x in xs], np.float32)     # noqa: E731

    def prim_mesh(ks):
        pos = np.concatenate([np.stack([h(k["v0"]), h(k["v0"]) + h(k["e1"]), h(k["v0"]) + h(k["e2"])]) for k in ks]).astype(np.float64)
        nrm = np.tile([[0.0, 1.0, 0.0]], (len(pos), 1))
        return pos, nrm, np.zeros((len(pos), 2)), np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)

    def build(with_discarded):
        b = _Builder()
        b.add(prim_mesh(kats[0::2]), base_color=(0.5, 0.5, 0.5, 1.0))
        if with_discarded:
            b.add(prim_mesh(kats[1::2]), base_color=(0.5, 0.5, 0.5, 0.0))
        return b.finish("kats", scenes.tiny_scene().camera, scenes.tiny_scene().light)
    full, kept = build(True), build(False)
    rays = np.array([np.concatenate([h(k["o"]), [float.fromhex(k["tmin"])], h(k["d"]), [float.fromhex(k["tmax"])]]) for k in kats], np.float32)
    rays = np.concatenate([rays, grazing_rays(full, np.random.default_rng(23), 6000)])
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(kept)
        want, occ = ctx.ray_query(rays), ctx.ray_query(rays, any_hit=True)
        ctx.upload_scene(full)
        plain = ctx.ray_query(rays)
        got = ctx.ray_query(rays, alpha_test=True)
        s_closest = ctx.ray_query_statistics()
        got_occ = ctx.ray_query(rays, any_hit=True, alpha_test=True)
        s_any = ctx.ray_query_statistics()
    finally:
        ctx.close()
    assert s_closest[2] > 0 and s_any[2] > 0 and s_closest[3] == 0 and s_any[3] == 0, (s_closest, s_any)
    assert_hits_equal(got, want, "flagged query on the grazing scene")
    assert np.array_equal(got_occ, occ)
    assert (plain["geometry_index"] == 1).sum() > 100            # the discarded half stops rays of the plain query


def test_hybrid_alpha_with_pixels_computed_again():
    """The queue kernels' deferred decision with the switch on.  No input of a few hundred triangles has a ray with a self-contradicting
    candidate (the fence scene at 1080p: none), so this one is sponza_hard_rot at 1080p -- where every frame has such pixels
    (tests/test_gpu_full_size.py) -- with 30 % of its primitives cut out: the pixels are computed again by redo_pixel_visibility /
    redo_pixel_reflection WITH the rule, and both images are the per-pixel kernels', bit for bit."""
    W2, H2 = 1920, 1080
    scene = scenes.alpha_masked(scenes.sponza_hard_rot(), 30)
    g = GpuHybrid(scene, W2, H2, denoise=False, gbuffer="standin")
    try:
        g.ctx.set_ray_statistics(True)
        g.ctx.set_option("alpha_test_rays", 1)
        pfd = camera.dolly_frames(scene, W2, H2, 2)[1]
        images, again = {}, None
        for variant in (1, 0):
            g.ctx.set_option("raygen_variant", variant)
            g.ctx.set_option("reflection_variant", variant)
            g.frame(pfd)
            images[variant] = (g.ctx.download(lib.RAYTRACED).copy(), g.ctx.download(lib.REFLECTIONS).copy())
            if variant == 1:
                again = g.ctx.binary64_statistics()
                assert g.ctx.alpha_launches() == 2 and g.ctx.ray_statistics()["stack_overflows"] == 0
        print("pixels computed again with alpha_test_rays 1:", again)
        assert again["pixels_again"] > 0 and again["mirror_pixels_again"] > 0, again        # (measured: 6 and 69)
        assert np.array_equal(images[1][0], images[0][0]), int((images[1][0] != images[0][0]).any(-1).sum())
        assert np.array_equal(images[1][1], images[0][1]), int((images[1][1] != images[0][1]).any(-1).sum())
        g.ctx.set_option("alpha_test_rays", 0)                      # and the switch acts on this scene
        g.frame(pfd)
        assert (g.ctx.download(lib.RAYTRACED) != images[0][0]).any(-1).sum() > 1000
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------
# no side effects; neutral where nothing can discard
# ---------------------------------------------------------------------------------------------
def test_switch_off_frames_do_not_depend_on_other_contexts_alpha_work(pair):
    """A denoised frame sequence with the switch off is bit-identical whether or not flagged queries and switch-on frames of ANOTHER
    context run in between."""
    frames = pair["want"][("A", 1)]
    rays = _scene_rays(pair["A"], 9, 1000)

    def sequence(disturb):
        g = GpuHybrid(pair["A"], W, H, denoise=True)
        other = pair["rig"]
        out = []
        try:
            for f in frames + frames:
                g.frame(f["pfd"], f["gbuf"])
                out.append([g.ctx.download(k).copy() for k in (lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED)])
                if disturb:
                    other.run([f], alpha=1)
                    other.g.ctx.ray_query(rays, alpha_test=True)
                    g.ctx.ray_query(rays, any_hit=True, alpha_test=True)         # a flagged query of its own is no switch
            assert g.ctx.get_option("alpha_test_rays") == 0 and g.ctx.alpha_launches() == 0
        finally:
            g.close()
        return out
    quiet, disturbed = sequence(False), sequence(True)
    for i, (a, b) in enumerate(zip(quiet, disturbed)):
        for x, y, what in zip(a, b, ("RAYTRACED", "REFLECTIONS", "DENOISED")):
            assert np.array_equal(x, y), f"frame {i}: {what} differs"


def test_neutral_where_nothing_can_discard(oracle):
    """tiny_scene() has no masked, textured or alpha-0 primitive: alpha_test_rays = 1 launches the plain kernels (alpha_launches == 0: no
    launch ran an alpha instantiation) and the images are the oracle's."""
    scene = scenes.tiny_scene()
    want = oracle_frames(oracle, scene, W, H, FRAMES, abi.default_trace_params(), denoise=False)[0]
    rig = Rig(scene)
    try:
        for name, options, stats in (SETTINGS[0], SETTINGS[1], SETTINGS[12]):
            got = rig.run(want, options, stats, alpha=1)
            _assert_frames(got, want, f"tiny_scene, {name}")
            assert [g["alpha_launches"] for g in got] == [0] * FRAMES
        rays = _scene_rays(scene, 3, 1000)
        assert rig.g.ctx.ray_query(rays, alpha_test=True).tobytes() == rig.g.ctx.ray_query(rays).tobytes()
    finally:
        rig.g.close()
