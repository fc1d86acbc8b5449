"""Ray cull masks on the GPU: vhr_set_primitive_masks, vhr_ray_query_masked and the hybrid path's "shadow_ray_mask" / "ao_ray_mask" /
"reflection_ray_mask".  One truth everywhere, and no oracle change: a ray of mask m on scene A sees, bit for bit, what the plain ray sees
on the scene made of A's primitives p with masks[p] & m != 0 (tests/ray_mask_cases.sub_scene; results never depend on the tree).  A frame
with three different class masks has the composite truth -- shadow from sub(shadow mask), AO from sub(AO mask), reflections from
sub(reflection mask) -- because the oracle's channels do not depend on each other (tests/test_ray_masks_host.py)."""
import json
import os

import numpy as np
import pytest

from tests import alpha_scenes
from tests import ray_mask_cases as cases
from tests.alpha_scenes import assert_hits_equal, grazing_rays
from tests.helpers import GpuHybrid, assert_reflections_identical, oracle_frames
from vulkanhybridrenderer_amd import abi, camera, lib, scenes
from vulkanhybridrenderer_amd.scenes import _Builder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = abi.RAY_MISS
W, H, FRAMES = cases.W, cases.H, cases.FRAMES
GRAPH = -5
CLASS_MASKS = (cases.SHADOW_MASK, cases.AO_MASK, cases.REFLECTION_MASK)
KEYS = ("shadow_ray_mask", "ao_ray_mask", "reflection_ray_mask")

# every form of the six kernels and every option that changes how they walk: (name, options, ray statistics) -- the list of
# tests/test_gpu_alpha_rays.py, copied
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
    """One hybrid context per scene for the whole module (host-supplied G-buffers, no denoiser): every case sets its options and class
    masks, runs its frames and puts the defaults back -- the masks are read at every launch."""

    def __init__(self, scene, prim_masks=None):
        self.g = GpuHybrid(scene, W, H, denoise=False)
        self.defaults = lib.option_table()
        if prim_masks is not None:
            self.g.ctx.set_primitive_masks(prim_masks)

    def run(self, frames, options=None, stats=False, class_masks=CLASS_MASKS, bounces=1, alpha=0):
        ctx = self.g.ctx
        options = options or {}
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_ray_statistics(stats)
        ctx.set_trace_params(abi.default_trace_params(reflections=bounces))
        out = []
        try:
            for f in frames:
                for k, v in zip(KEYS, class_masks):
                    ctx.set_option(k, v)
                ctx.set_option("alpha_test_rays", alpha)
                self.g.frame(f["pfd"], f["gbuf"])
                out.append(dict(raytraced=ctx.download(lib.RAYTRACED).copy(), reflections=ctx.download(lib.REFLECTIONS).copy(),
                                mask_launches=ctx.ray_mask_statistics()[1], alpha_launches=ctx.alpha_launches(),
                                overflows=ctx.ray_statistics()["stack_overflows"] if stats else 0))
        finally:
            for k in options:
                ctx.set_option(k, self.defaults[k][0])
            for k in KEYS:
                ctx.set_option(k, 255)
            ctx.set_ray_statistics(False)
            ctx.set_option("alpha_test_rays", 0)
        return out


def composite_truth(oracle, frames, sc, prim_masks, class_masks, bounces):
    """Per frame of `frames` (pfd + the FULL scene's G-buffer): shadow from sub(shadow mask), AO from sub(AO mask), reflections from
    sub(reflection mask), each the oracle's own channel on that sub-scene."""
    subs = [oracle.Scene(cases.sub_scene(sc, prim_masks, m)[0]) for m in class_masks]
    tp = abi.default_trace_params
    out = []
    for f in frames:
        n, d = f["gbuf"][0], f["gbuf"][2]
        sa = np.empty_like(subs[0].raygen(f["pfd"], tp(ao_spp=0, reflections=False), n, d)[0])
        sa[..., 0] = subs[0].raygen(f["pfd"], tp(ao_spp=0, reflections=False), n, d)[0][..., 0]
        sa[..., 1] = subs[1].raygen(f["pfd"], tp(shadow=False, reflections=False), n, d)[0][..., 1]
        refl = subs[2].raygen(f["pfd"], tp(shadow=False, ao_spp=0, reflections=bounces), n, d)[1]
        out.append(dict(pfd=f["pfd"], gbuf=f["gbuf"], shadow_ao=sa, reflections=refl))
    return out


@pytest.fixture(scope="module")
def A(oracle):
    """Scene A with its masks on a hybrid context, the oracle's frames on A (all-255 truth) and the composite truths for one and two bounces."""
    sc = cases.scene()
    full = {b: oracle_frames(oracle, sc, W, H, FRAMES, abi.default_trace_params(reflections=b), denoise=False)[0] for b in (1, 2)}
    want = {b: composite_truth(oracle, full[1], sc, cases.masks(), CLASS_MASKS, b) for b in (1, 2)}
    rig = Rig(sc, cases.masks())
    cache = {}

    def truth(class_masks, bounces=1):
        if (class_masks, bounces) not in cache:
            cache[(class_masks, bounces)] = composite_truth(oracle, full[1], sc, cases.masks(), class_masks, bounces)
        return cache[(class_masks, bounces)]
    yield dict(scene=sc, full=full, want=want, rig=rig, rays=cases.rays(sc), truth=truth)
    rig.g.close()


@pytest.fixture(scope="module")
def truth_ctx():
    """A second context that holds whatever sub-scene a test wants the plain query's answers on."""
    c = lib.Context(64, 64)
    yield c
    c.close()


def plain_on(truth_ctx, sub, keep, rays):
    """(closest hits with A's geometry indices, any-hit) of the plain query on a sub-scene; on no scene at all: every ray misses"""
    if sub is None:
        want = np.zeros(len(rays), abi.ray_hit_dtype)
        want["geometry_index"] = want["primitive_index"] = MISS
        return want, np.zeros(len(rays), bool)
    truth_ctx.upload_scene(sub)
    return cases.remap_hits(truth_ctx.ray_query(rays), keep), truth_ctx.ray_query(rays, any_hit=True)


def _assert_frames(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        for ch, name in ((0, "shadow"), (1, "AO")):
            diff = g["raytraced"][..., ch] != w["shadow_ao"][..., ch]
            assert not diff.any(), f"{what}, frame {i}: {int(diff.sum())} {name} texels differ from the oracle on the sub-scene, first at {np.argwhere(diff)[:4].tolist()}"
        assert_reflections_identical(g["reflections"], w["reflections"], f"{what}, frame {i}: reflections")
        assert g["overflows"] == 0


# ---------------------------------------------------------------------------------------------
# 1, 2: queries
# ---------------------------------------------------------------------------------------------
def _query(ctx, route, rays, any_hit=False, **kw):
    if route == "host memory":
        return ctx.ray_query(rays, any_hit=any_hit, **kw)
    import torch
    d_rays = torch.from_numpy(rays).cuda()
    out = torch.zeros(len(rays) if any_hit else (len(rays), 6), dtype=torch.uint8 if any_hit else torch.int32, device="cuda")
    ray_masks = kw.pop("ray_masks", None)
    d_masks = torch.from_numpy(np.concatenate([[0], ray_masks]).astype(np.uint8)).cuda()[1:] if ray_masks is not None else None    # (odd address: no alignment needed)
    torch.cuda.synchronize()
    ctx.ray_query_device(d_rays.data_ptr(), len(rays), out.data_ptr(), any_hit=any_hit, ray_masks_ptr=d_masks.data_ptr() if d_masks is not None else 0, **kw)
    ctx.synchronize()
    return out.cpu().numpy().astype(bool) if any_hit else out.cpu().numpy().view(abi.ray_hit_dtype).reshape(-1)


@pytest.mark.parametrize("route", ["host memory", "device pointers"])
def test_masked_query_equals_the_plain_query_on_the_sub_scene(A, truth_ctx, route):
    ctx, rays = A["rig"].g.ctx, A["rays"]
    assert len(rays) % 64 != 0
    for m in cases.QUERY_MASKS:
        sub, keep = cases.sub_scene(A["scene"], cases.masks(), m)
        want, occ = plain_on(truth_ctx, sub, keep, rays)
        got = _query(ctx, route, rays, cull_mask=m)
        s = ctx.ray_query_statistics()
        got_occ = _query(ctx, route, rays, any_hit=True, cull_mask=m)
        assert s[3] == 0 and ctx.ray_query_statistics()[3] == 0 and ctx.ray_mask_statistics()[2] == 1
        assert_hits_equal(got, want, f"cull_mask {m:#04x}, closest hit")
        assert np.array_equal(got_occ, occ), f"cull_mask {m:#04x}, any hit: {int((got_occ != occ).sum())} differ"
        if m == 0:
            assert (got["geometry_index"] == MISS).all() and not got_occ.any() and s[1] == 0


@pytest.mark.parametrize("route", ["host memory", "device pointers"])
def test_per_ray_masks(A, truth_ctx, route):
    ctx, rays = A["rig"].g.ctx, A["rays"]
    ray_masks = np.array(cases.QUERY_MASKS, np.uint8)[np.arange(len(rays)) % len(cases.QUERY_MASKS)]
    for cull in (0xFF, 0x03):
        got = _query(ctx, route, rays, cull_mask=cull, ray_masks=ray_masks)
        got_occ = _query(ctx, route, rays, any_hit=True, cull_mask=cull, ray_masks=ray_masks)
        assert ctx.ray_query_statistics()[3] == 0 and ctx.ray_mask_statistics()[2] == 1
        effective = ray_masks & np.uint8(cull)
        for m in np.unique(effective):
            group = np.nonzero(effective == m)[0]
            sub, keep = cases.sub_scene(A["scene"], cases.masks(), int(m))
            want, occ = plain_on(truth_ctx, sub, keep, rays[group])
            assert_hits_equal(got[group], want, f"cull_mask {cull:#04x}, rays of effective mask {int(m):#04x}")
            assert np.array_equal(got_occ[group], occ)


def test_a_ray_of_mask_zero_misses_primitives_at_ff():
    """With ray_masks given the filtering kernels run whatever the primitives carry: a ray's mask may be 0."""
    sc = cases.scene()
    rays = cases.rays(sc)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(sc)                                    # every primitive at 0xFF, no set call at all
        plain, plain_occ = ctx.ray_query(rays), ctx.ray_query(rays, any_hit=True)
        assert ctx.ray_mask_statistics() == [0, 0, 0, 0]
        ray_masks = np.where(np.arange(len(rays)) % 3 == 0, 0, 0x40).astype(np.uint8)
        got, got_occ = ctx.ray_query(rays, ray_masks=ray_masks), ctx.ray_query(rays, any_hit=True, ray_masks=ray_masks)
        assert ctx.ray_mask_statistics() == [0, 0, 1, 0]
        none = ctx.ray_query(rays, cull_mask=0)
        assert (none["geometry_index"] == MISS).all() and not ctx.ray_query(rays, any_hit=True, cull_mask=0).any()
    finally:
        ctx.close()
    zero = ray_masks == 0
    assert (got["geometry_index"][zero] == MISS).all() and (got["t"][zero] == 0).all() and not got_occ[zero].any()
    assert_hits_equal(got[~zero], plain[~zero], "rays of mask 0x40 on primitives at 0xFF")
    assert np.array_equal(got_occ[~zero], plain_occ[~zero]) and plain_occ[zero].sum() > 50


# ---------------------------------------------------------------------------------------------
# 3, 4, 5: the hybrid path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name,options,stats", SETTINGS, ids=IDS)
def test_every_form_sees_the_three_sub_scenes(A, name, options, stats, bounces):
    want = A["want"][bounces]
    got = A["rig"].run(want, options, stats, bounces=bounces)
    _assert_frames(got, want, f"class masks 0x01 / 0x02 / 0x04, {name}, {bounces} bounce(s)")
    # the mask instantiations ran: the shadow / AO launch and -- where the mirror ray has a launch of its own -- that one
    assert all(g["mask_launches"] == (1 if options.get("raygen_variant", 1) == 0 else 2) for g in got), [g["mask_launches"] for g in got]
    assert all(g["alpha_launches"] == 0 for g in got)


def test_the_masks_toggle_per_launch_both_ways(A):
    on, off, rig = A["want"][1], A["full"][1], A["rig"]
    for i in range(FRAMES):
        for acting in (True, False, True, False):
            got = rig.run([on[i]], class_masks=CLASS_MASKS if acting else (255, 255, 255))
            # all-255 on this scene still hides the 0x00 primitive: its truth is sub(0xFF), not A
            _assert_frames(got, [on[i]] if acting else A["truth"]((255, 255, 255))[i:i + 1], f"frame {i}, masks {'acting' if acting else '255'}")
            assert got[0]["mask_launches"] == 2


def test_class_masks_0x07_act_only_on_the_0x00_primitive(A):
    want = A["truth"]((0x07, 0x07, 0x07))
    for name, options, stats in (SETTINGS[0], SETTINGS[1], SETTINGS[12]):
        got = A["rig"].run(want, options, stats, class_masks=(0x07, 0x07, 0x07))
        _assert_frames(got, want, f"class masks 0x07, {name}")
        assert all(g["mask_launches"] == (1 if options.get("raygen_variant", 1) == 0 else 2) for g in got)
    # ... which is A without its last primitive: the canopy's shadow is gone
    assert sum(int((w["shadow_ao"][..., 0] != f["shadow_ao"][..., 0]).sum()) for w, f in zip(want, A["full"][1])) > 300


def test_neutral_where_every_primitive_is_at_ff(A):
    """Every primitive mask at 0xFF and any non-zero class masks: no mask acts, the launches are the plain ones (mask_launches == 0), the
    images the oracle's on A, and a masked query's bytes the plain query's."""
    rig = Rig(A["scene"])
    try:
        for prim_masks in (None, [0xFF] * 12):
            if prim_masks is not None:
                rig.g.ctx.set_primitive_masks(cases.masks())               # set, then put back: the device array exists, nothing acts
                rig.g.ctx.set_primitive_masks(prim_masks)
            for class_masks in ((255, 255, 255), CLASS_MASKS, (0x80, 0x10, 0x7F)):
                for name, options, stats in (SETTINGS[0], SETTINGS[1], SETTINGS[12]):
                    got = rig.run(A["full"][1], options, stats, class_masks=class_masks)
                    _assert_frames(got, A["full"][1], f"all primitives at 0xFF, class masks {class_masks}, {name}")
                    assert [g["mask_launches"] for g in got] == [0] * FRAMES
            assert rig.g.ctx.ray_query(A["rays"], cull_mask=0x10).tobytes() == rig.g.ctx.ray_query(A["rays"]).tobytes()
            assert rig.g.ctx.ray_mask_statistics()[2] == 0
            assert rig.g.ctx.ray_query(A["rays"], any_hit=True, cull_mask=0x10).tobytes() == rig.g.ctx.ray_query(A["rays"], any_hit=True).tobytes()
    finally:
        rig.g.close()


def test_set_primitive_masks_is_refused_inside_a_pass(A):
    """Refused with VHR_ERROR_GRAPH in a pass callback (a graphics pass's: no stamps, no recording); as with every failed call of a
    callback, vhr_graph_execute then returns that error.  Nothing was stored, and the next frame is the oracle's."""
    seen = {}

    class InPass(GpuHybrid):
        def _gbuffer_pass(self, ctx):
            if not seen:
                m = cases.masks()
                seen["rc"] = ctx.L.vhr_set_primitive_masks(ctx.handle, 0, len(m), m.ctypes.data)
                seen["msg"] = ctx.L.vhr_last_error(ctx.handle).decode()
            super()._gbuffer_pass(ctx)
    g = InPass(A["scene"], W, H, denoise=False)
    try:
        f = A["full"][1][0]
        with pytest.raises(lib.VhrError, match="vhr_set_primitive_masks: called from inside a pass"):
            g.frame(f["pfd"], f["gbuf"])
        assert seen["rc"] == GRAPH and "vhr_set_primitive_masks" in seen["msg"] and "inside a pass" in seen["msg"], seen
        g.ctx.synchronize()
        assert g.ctx.primitive_masks().tolist() == [0xFF] * 12 and g.ctx.ray_mask_statistics()[0] == 0
        g.frame(f["pfd"], f["gbuf"])                            # outside a pass again: the call works, and the frame before it is A's
        assert np.array_equal(g.ctx.download(lib.RAYTRACED), f["shadow_ao"])
        g.ctx.set_primitive_masks(cases.masks())
        assert g.ctx.primitive_masks().tolist() == cases.masks().tolist()
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------
# 6: with alpha
# ---------------------------------------------------------------------------------------------
def test_masks_with_alpha_test_rays(oracle, truth_ctx):
    """alpha_scenes.uniform_pair()'s A with "alpha_test_rays" 1 and masks that hide two of the occluders the alpha rule KEEPS: the frames
    are the oracle's on B minus those two (A and B have one G-buffer), the flagged masked query the plain one on that scene."""
    sa, sb = alpha_scenes.uniform_pair()
    hidden = [5, 7]                                             # two of B's three occluders (B is A cut short: the indices are A's too)
    prim_masks = np.full(len(sa.primitives), 0xFF, np.uint8)
    prim_masks[hidden] = 0x08
    keep = np.array([p for p in range(len(sb.primitives)) if p not in hidden])
    truth_scene = alpha_scenes.subset(sb, keep)
    frames = oracle_frames(oracle, sa, W, H, FRAMES, abi.default_trace_params(), denoise=False)[0]
    osc = oracle.Scene(truth_scene)
    rig = Rig(sa, prim_masks)
    try:
        for bounces in (1, 2):
            tp = abi.default_trace_params(reflections=bounces)
            want = []
            for f in frames:
                s, r, _, _ = osc.raygen(f["pfd"], tp, f["gbuf"][0], f["gbuf"][2])
                want.append(dict(pfd=f["pfd"], gbuf=f["gbuf"], shadow_ao=s, reflections=r))
            for name, options, stats in (SETTINGS[0], SETTINGS[1], SETTINGS[11], SETTINGS[12]):
                got = rig.run(want, options, stats, class_masks=(0x07, 0x07, 0x07), bounces=bounces, alpha=1)
                _assert_frames(got, want, f"alpha_test_rays 1 with masks, {name}, {bounces} bounce(s)")
                n = 1 if options.get("raygen_variant", 1) == 0 else 2
                assert all(g["mask_launches"] == n and g["alpha_launches"] == n for g in got)
        rays = cases.rays(sa)
        want, occ = plain_on(truth_ctx, truth_scene, keep, rays)
        ctx = rig.g.ctx
        assert_hits_equal(ctx.ray_query(rays, alpha_test=True, cull_mask=0x07), want, "flagged masked query")
        assert np.array_equal(ctx.ray_query(rays, any_hit=True, alpha_test=True, cull_mask=0x07), occ)
        only_alpha = ctx.ray_query(rays, alpha_test=True)
        assert cases.hit_bits_differ(only_alpha, want).sum() >= 20              # the mask acts on top of the alpha rule
    finally:
        rig.g.close()


# ---------------------------------------------------------------------------------------------
# 7: with the deferred binary64 decision
# ---------------------------------------------------------------------------------------------
def test_masked_query_with_the_binary64_launch():
    """The grazing pairs of tests/golden/kat_decision_vi.json as a scene, the odd triangles on a primitive of mask 0x02 that comes last, and
    as rays with rays grazing those triangles around them: some take the second launch, and cull_mask 0x01 still equals the plain query
    on the kept half."""
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_decision_vi.json")))
    h = lambda xs: np.array([float.fromhex(x) for x in xs], np.float32)     # noqa: E731

    def prim_mesh(ks):
        pos = np.concatenate([np.stack([h(k["v0"]), h(k["v0"]) + h(k["e1"]), h(k["v0"]) + h(k["e2"])]) for k in ks]).astype(np.float64)
        nrm = np.tile([[0.0, 1.0, 0.0]], (len(pos), 1))
        return pos, nrm, np.zeros((len(pos), 2)), np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)

    def build(with_odd):
        b = _Builder()
        b.add(prim_mesh(kats[0::2]), base_color=(0.5, 0.5, 0.5, 1.0))
        if with_odd:
            b.add(prim_mesh(kats[1::2]), base_color=(0.5, 0.5, 0.5, 1.0))
        return b.finish("kats", scenes.tiny_scene().camera, scenes.tiny_scene().light)
    full, kept = build(True), build(False)
    rays = np.array([np.concatenate([h(k["o"]), [float.fromhex(k["tmin"])], h(k["d"]), [float.fromhex(k["tmax"])]]) for k in kats], np.float32)
    rays = np.concatenate([rays, grazing_rays(full, np.random.default_rng(23), 6000)])
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(kept)
        want, occ = ctx.ray_query(rays), ctx.ray_query(rays, any_hit=True)
        ctx.upload_scene(full)
        ctx.set_primitive_masks([0xFF, 0x02])
        plain = ctx.ray_query(rays)
        got = ctx.ray_query(rays, cull_mask=0x01)
        s_closest = ctx.ray_query_statistics()
        got_occ = ctx.ray_query(rays, any_hit=True, cull_mask=0x01)
        s_any = ctx.ray_query_statistics()
        assert ctx.ray_mask_statistics() == [1, 0, 1, 0]
    finally:
        ctx.close()
    assert s_closest[2] > 0 and s_any[2] > 0 and s_closest[3] == 0 and s_any[3] == 0, (s_closest, s_any)
    assert_hits_equal(got, want, "masked query on the grazing scene")
    assert np.array_equal(got_occ, occ)
    assert (plain["geometry_index"] == 1).sum() > 100            # the hidden half stops rays of the plain query


def test_hybrid_masks_with_pixels_computed_again():
    """The queue kernels' deferred decision with masks acting: sponza_hard_rot at 1080p (the smallest input known to have such pixels,
    tests/test_gpu_alpha_rays.py) with 30 % of its primitives hidden from all three classes -- the pixels are computed again by
    redo_pixel_visibility / redo_pixel_reflection WITH the filter, and both images are the per-pixel kernels', bit for bit."""
    W2, H2 = 1920, 1080
    scene = scenes.sponza_hard_rot()
    n = len(scene.primitives)
    count = int(round(n * 0.3))
    prim_masks = np.full(n, 0xFF, np.uint8)
    prim_masks[np.unique((np.arange(count) * n) // count)] = 0x08            # evenly spread, as scenes.alpha_masked chooses
    g = GpuHybrid(scene, W2, H2, denoise=False, gbuffer="standin")
    try:
        g.ctx.set_primitive_masks(prim_masks)
        g.ctx.set_ray_statistics(True)
        for k in KEYS:
            g.ctx.set_option(k, 0x07)
        pfd = camera.dolly_frames(scene, W2, H2, 2)[1]
        images, again = {}, None
        for variant in (1, 0):
            g.ctx.set_option("raygen_variant", variant)
            g.ctx.set_option("reflection_variant", variant)
            g.frame(pfd)
            images[variant] = (g.ctx.download(lib.RAYTRACED).copy(), g.ctx.download(lib.REFLECTIONS).copy())
            if variant == 1:
                again = g.ctx.binary64_statistics()
                assert g.ctx.ray_mask_statistics()[1] == 2 and g.ctx.ray_statistics()["stack_overflows"] == 0
        print("pixels computed again with masks acting:", again)
        assert again["pixels_again"] > 0 and again["mirror_pixels_again"] > 0, again
        assert np.array_equal(images[1][0], images[0][0]), int((images[1][0] != images[0][0]).any(-1).sum())
        assert np.array_equal(images[1][1], images[0][1]), int((images[1][1] != images[0][1]).any(-1).sum())
        for k in KEYS:                                              # and the masks act on this scene
            g.ctx.set_option(k, 255)
        g.frame(pfd)
        assert g.ctx.ray_mask_statistics()[1] == 0
        assert (g.ctx.download(lib.RAYTRACED) != images[0][0]).any(-1).sum() > 1000
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------
# 8, 9, 10: fuse_temporal, refits, side effects
# ---------------------------------------------------------------------------------------------
def test_fuse_temporal_with_a_shadow_mask_that_acts(A):
    """The epilogue form has no filter: with a shadow mask that acts the launch is not held back -- svgf.comp keeps its own dispatch --
    and the denoised frames are those of fuse_temporal 0, bit for bit.  (Stand-in G-buffer on the context's stream, no mirror ray: the
    schedule in which the launch WOULD fuse, tests/test_gpu_svgf.py.)"""
    pfds = camera.dolly_frames(A["scene"], W, H, 2 * FRAMES)

    def sequence(fuse):
        g = GpuHybrid(A["scene"], W, H, reflections=False, denoise=True, gbuffer="standin", trace_params=abi.default_trace_params(reflections=False))
        out = []
        try:
            g.ctx.set_primitive_masks(cases.masks())
            g.ctx.set_option("fuse_temporal", fuse)
            g.ctx.set_option("shadow_ray_mask", cases.SHADOW_MASK)
            g.ctx.set_kernel_timing(["svgf_temporal"])
            g.ctx.kernel_time("svgf_temporal", reset=True)
            for pfd in pfds:
                g.frame(pfd)
                out.append([g.ctx.download(k).copy() for k in (lib.RAYTRACED, lib.DENOISED)])
                assert g.ctx.ray_mask_statistics()[1] == 1
            assert g.ctx.kernel_time("svgf_temporal")[1] == len(pfds)            # svgf.comp ran as a dispatch of its own in every frame
        finally:
            g.close()
        return out
    plain, fused = sequence(0), sequence(1)
    for i, (a, b) in enumerate(zip(plain, fused)):
        assert np.array_equal(a[0], b[0]), f"frame {i}: RAYTRACED differs"
        assert np.array_equal(a[1], b[1]), f"frame {i}: DENOISED differs"


def test_masks_stay_in_force_after_a_partial_refit(A, truth_ctx):
    sc, rays = A["scene"], A["rays"]
    moved = scenes.Scene(sc.name + "_moved", sc.vertices, sc.indices, sc.primitives.copy(), list(sc.textures), sc.camera, sc.light)
    moved.primitives["transform"][cases.N_TINY:, 12] += 0.35                  # every occluder 0.35 along x and 0.2 up
    moved.primitives["transform"][cases.N_TINY:, 13] += 0.2
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(sc)
        ctx.set_primitive_masks(cases.masks())
        before = ctx.ray_query(rays, cull_mask=0x01)
        ctx.update_primitive_transforms(moved.primitives["transform"][cases.N_TINY:], first_primitive=cases.N_TINY)
        ctx.refit_geometry_partial()
        assert ctx.primitive_masks().tolist() == cases.masks().tolist()
        for m in (0x01, 0x06):
            sub, keep = cases.sub_scene(moved, cases.masks(), m)
            want, occ = plain_on(truth_ctx, sub, keep, rays)
            got = ctx.ray_query(rays, cull_mask=m)
            assert_hits_equal(got, want, f"cull_mask {m:#04x} after the refit")
            assert np.array_equal(ctx.ray_query(rays, any_hit=True, cull_mask=m), occ)
            if m == 0x01:
                assert cases.hit_bits_differ(got, before).sum() >= 20            # the occluders did move
    finally:
        ctx.close()


def test_default_frames_do_not_depend_on_other_contexts_mask_work(A):
    """A denoised frame sequence of a context at defaults is bit-identical whether or not ANOTHER context runs masked frames and masked
    queries in between (and a masked query of its own is no class mask)."""
    frames, rays = A["full"][1], A["rays"]

    def sequence(disturb):
        g = GpuHybrid(A["scene"], W, H, denoise=True)
        out = []
        try:
            for f in frames + frames:
                g.frame(f["pfd"], f["gbuf"])
                out.append([g.ctx.download(k).copy() for k in (lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED)])
                if disturb:
                    A["rig"].run([f])
                    A["rig"].g.ctx.ray_query(rays, cull_mask=0x02)
                    g.ctx.ray_query(rays, any_hit=True, cull_mask=0x00)
            assert [g.ctx.get_option(k) for k in KEYS] == [255] * 3 and g.ctx.ray_mask_statistics()[:2] == [0, 0]
        finally:
            g.close()
        return out
    quiet, disturbed = sequence(False), sequence(True)
    for i, (a, b) in enumerate(zip(quiet, disturbed)):
        for x, y, what in zip(a, b, ("RAYTRACED", "REFLECTIONS", "DENOISED")):
            assert np.array_equal(x, y), f"frame {i}: {what} differs"
    for i in range(FRAMES):
        assert np.array_equal(quiet[i][0], frames[i]["shadow_ao"])
