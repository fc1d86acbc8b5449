"""vhr_ray_query_faces on the device: the device's copy of the facing function equals the host's; culled queries judged against the exact
truth with the culled pairs removed (tests/face_cull_cases.py) at three scene scales, with and without a cull mask that acts, every
reported hit kind against the exact sign; identities between the cull modes that need no truth; tree independence; transforms that mirror at
run time; the face rule combined with the alpha rule and the masks; memory routes, streams, statistics and side effects.

Scenes: ray_truth.SOUPS with a seeded half of their primitives mirrored (60 / 400 / 2 000 triangles, degenerate and duplicate ones
included); rays: soup_rays plus soup_grazing, cut to 1, 255, 257, 513 and the full set."""
import dataclasses

import numpy as np
import pytest

from tests import alpha_scenes, face_cull_cases as fc, ray_mask_cases, ray_truth as rt
from vulkanhybridrenderer_amd import abi, lib, scenes

pytestmark = pytest.mark.gpu
MISS = abi.RAY_MISS
GRAPH = -5
MODES = ((fc.BACK, "BACK"), (fc.FRONT, "FRONT"))
SEEDS = [s[0] for s in rt.SOUPS]
TREE_DEFAULTS = {"bvh_builder": 1, "bvh_presplit": 0, "bvh_frame": 1, "bvh_leaf_triangles": 2}


def bits(hits):
    return hits.view(np.uint32).reshape(-1, 6)


def assert_hits_equal(got, want, what, kind=True):
    """vhr_ray_hit records equal as bits (kind=False: all but `reserved`)."""
    g, w = bits(got), bits(want)
    if not kind:
        g, w = g[:, :5], w[:, :5]
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} rays differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def assert_cuts_equal(ctx, rays, full, what, **kw):
    """The batch cut to 1, 255, 257 and 513 rays (across the 256-ray wave and the 512-ray block) gives the first rays' answers of the full batch."""
    any_hit = kw.get("any_hit", False)
    for n in fc.COUNTS[:-1]:
        got = ctx.ray_query(rays[:n], **{k: (v[:n] if k == "ray_masks" else v) for k, v in kw.items()})
        assert np.array_equal(got, full[:n]) if any_hit else bits(got).tobytes() == bits(full[:n]).tobytes(), f"{what}: the first {n} rays alone differ"


def assert_kinds(osc, scene, rays, hits, flips, what, mode=fc.NONE):
    want, either = fc.expected_kinds(osc, scene, rays, hits, flips)
    got = hits["reserved"]
    miss = hits["geometry_index"] == MISS
    assert (got[miss] == 0).all(), f"{what}: a miss with a hit kind"
    assert np.isin(got[~miss], (fc.KIND_FRONT, fc.KIND_BACK)).all(), what
    bad = np.nonzero((got != want) & ~either)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} hit kinds differ from the exact sign's, first ray {bad[0]}: got {got[bad[0]]:#x}, want {want[bad[0]]:#x}"
    if mode == fc.BACK:
        assert (got[~miss & ~either] == fc.KIND_FRONT).all(), f"{what}: a back-facing hit with VHR_FACE_CULL_BACK"
    if mode == fc.FRONT:
        assert (got[~miss & ~either] == fc.KIND_BACK).all(), f"{what}: a front-facing hit with VHR_FACE_CULL_FRONT"


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(64, 64)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------
# 1: the device's copy of the function
# ---------------------------------------------------------------------------------------------
def test_the_devices_facing_function_is_the_hosts(ctx):
    pairs, sign = fc.pair_set()
    n = len(pairs)
    host = lib.Context(64, 64, host_only=True)
    try:
        mixed = (np.arange(n) % 3 == 0).astype(np.uint8)
        for flips in (None, np.ones(n, np.uint8), mixed):
            got, want = ctx.debug_ray_facing(pairs, flips), host.debug_ray_facing(pairs, flips)
            assert got.tobytes() == want.tobytes(), f"{int((got != want).sum())} of {n} pairs differ between device and host"
        wrong = (ctx.debug_ray_facing(pairs) != fc.kind_of_sign(sign, np.zeros(n))) & (sign != 0)
        assert wrong.sum() == 0
        for k in (1, 255, 257):                                    # one block and a bit
            assert ctx.debug_ray_facing(pairs[:k], mixed[:k]).tobytes() == host.debug_ray_facing(pairs[:k], mixed[:k]).tobytes()
        special = np.array([[np.nan, 0, -1, 1, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, -1, 0, 0, 0, 0, 0, 0], [0, 0, -1, 1, 0, 0, 0, 1, 0]], np.float32)
        assert ctx.debug_ray_facing(special).tolist() == host.debug_ray_facing(special).tolist() == [fc.KIND_BACK, fc.KIND_BACK, fc.KIND_BACK, fc.KIND_FRONT]
    finally:
        host.close()


# ---------------------------------------------------------------------------------------------
# 2: against the exact truth
# ---------------------------------------------------------------------------------------------
def _judge(ctx, osc, scene, rays, truth, flips, mode, what, **kw):
    culled, removed, total = fc.culled_truth(truth, osc, rays, flips, mode)
    assert total > 200 and removed >= total / 4, f"{what}: the truth has too little to cull ({removed} of {total} exact hits)"
    hits = ctx.ray_query(rays, face_cull=mode, **kw)
    s_closest = ctx.ray_query_statistics()
    assert ctx.face_cull_statistics()[1] == 1
    occ = ctx.ray_query(rays, any_hit=True, face_cull=mode, **kw)
    s_any = ctx.ray_query_statistics()
    assert ctx.face_cull_statistics()[1] == 1
    assert s_closest[3] == 0 and s_any[3] == 0, (what, s_closest, s_any)
    hit, flat = rt.flat_of_hits(scene, hits)
    assert s_closest[:2] == [len(rays), int(hit.sum())] and s_any[:2] == [len(rays), int(occ.sum())], (what, s_closest, s_any)
    vc = rt.judge_closest(culled, hit, flat, hits["t"], hits["u"], hits["v"])
    va = rt.judge_any(culled, occ)
    print(f"{what}: {removed} of {total} exact hits culled; closest {vc.violations} violations (D explained {vc.explained_d}, passed over explained "
          f"{vc.explained_lost}), any hit {va.violations}; binary64 rays {s_closest[2]} / {s_any[2]}")
    assert vc.violations == 0, f"{what}, closest hit: {vc.describe()}"
    assert va.violations == 0, f"{what}, any hit: {va.describe()}"
    assert_kinds(osc, scene, rays, hits, flips, what, mode)
    return hits, occ


@pytest.mark.parametrize("scale", rt.SCALES)
@pytest.mark.parametrize("seed", SEEDS)
def test_culled_queries_against_the_exact_truth(oracle, ctx, seed, scale):
    scene, rays = fc.soup_case(seed, scale)
    osc = oracle.Scene(scene)
    flips = fc.expected_flips(scene)
    ctx.upload_scene(scene)
    assert ctx.primitive_facing_flips().tolist() == flips.tolist() and ctx.face_cull_statistics()[0] == flips.sum() == len(flips) // 2
    prim_masks = np.where(np.arange(len(scene.primitives)) % 2 == 0, 0x01, 0x02).astype(np.uint8)
    plain = rt.Truth(oracle, osc, rays)
    for what, kw, tkw in (("no masks", {}, {}), ("cull_mask 0x02", dict(cull_mask=0x02), dict(prim_masks=prim_masks, cull_mask=0x02))):
        if kw:
            ctx.set_primitive_masks(prim_masks)
            truth = rt.Truth(oracle, osc, rays, **tkw)
            assert 0.2 * plain.hit.sum() < truth.hit.sum() < 0.8 * plain.hit.sum()            # the mask acts
        else:
            truth = plain
        for mode, name in MODES:
            hits, occ = _judge(ctx, osc, scene, rays, truth, flips, mode, f"soup {seed} x {scale}, {what}, {name}", **kw)
            assert ctx.ray_mask_statistics()[2] == (1 if kw else 0)
            assert_cuts_equal(ctx, rays, hits, f"soup {seed} x {scale}, {what}, {name}", face_cull=mode, **kw)
            assert_cuts_equal(ctx, rays, occ, f"soup {seed} x {scale}, {what}, {name}, any hit", any_hit=True, face_cull=mode, **kw)
            if kw:
                seen = hits["geometry_index"][hits["geometry_index"] != MISS]
                assert ((prim_masks[seen] & 0x02) != 0).all()
        # the unculled query through the new entry point reports every hit's kind
        none = ctx.ray_query(rays, face_cull=fc.NONE, **kw)
        assert_kinds(osc, scene, rays, none, flips, f"soup {seed} x {scale}, {what}, NONE")
        both = np.bincount(none["reserved"][none["geometry_index"] != MISS], minlength=256)
        assert both[fc.KIND_FRONT] > 50 and both[fc.KIND_BACK] > 50


# ---------------------------------------------------------------------------------------------
# 3: exact identities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", rt.SCALES)
@pytest.mark.parametrize("seed", SEEDS)
def test_identities_between_the_cull_modes(ctx, seed, scale):
    scene, rays = fc.soup_case(seed, scale)
    ctx.upload_scene(scene)
    prim_masks = np.where(np.arange(len(scene.primitives)) % 2 == 0, 0x01, 0x03).astype(np.uint8)
    ray_masks = np.where(np.arange(len(rays)) % 3 == 0, 0x02, 0xFF).astype(np.uint8)
    for what, kw in (("no masks", {}), ("cull_mask 0xFF, nothing set", dict(cull_mask=0xFF)), ("per-ray masks", dict(ray_masks=ray_masks))):
        if "ray_masks" in kw:
            ctx.set_primitive_masks(prim_masks)
        what = f"soup {seed} x {scale}, {what}"
        masked_kw = kw or dict(cull_mask=0xFF)
        # (a) NONE through the new entry point is vhr_ray_query_masked, and its any-hit launch is the masked one's
        plain, plain_occ = ctx.ray_query(rays, **masked_kw), ctx.ray_query(rays, any_hit=True, **masked_kw)
        assert ctx.face_cull_statistics()[1] == 0 and (plain["reserved"] == 0).all()
        none = ctx.ray_query(rays, face_cull=fc.NONE, **kw)
        assert ctx.face_cull_statistics()[1] == 1
        none_occ = ctx.ray_query(rays, any_hit=True, face_cull=fc.NONE, **kw)
        assert ctx.face_cull_statistics()[1] == 0 and ctx.ray_mask_statistics()[2] == (1 if "ray_masks" in kw else 0)
        assert_hits_equal(none, plain, f"{what}: NONE against vhr_ray_query_masked", kind=False)
        assert none_occ.tobytes() == plain_occ.tobytes()
        hit = none["geometry_index"] != MISS
        front, back = hit & (none["reserved"] == fc.KIND_FRONT), hit & (none["reserved"] == fc.KIND_BACK)
        assert (front | back).tolist() == hit.tolist() and front.sum() > 50 and back.sum() > 50 and (none["reserved"][~hit] == 0).all()
        culled = {mode: (ctx.ray_query(rays, face_cull=mode, **kw), ctx.ray_query(rays, any_hit=True, face_cull=mode, **kw)) for mode, _ in MODES}
        (b_hits, b_occ), (f_hits, f_occ) = culled[fc.BACK], culled[fc.FRONT]
        # (b) a ray whose unculled closest hit faces it keeps that hit under BACK, bit for bit, kind included; symmetrically for FRONT
        assert_hits_equal(b_hits[front], none[front], f"{what}: BACK on rays whose closest hit is front-facing")
        assert_hits_equal(f_hits[back], none[back], f"{what}: FRONT on rays whose closest hit is back-facing")
        # (c) the two modes partition a ray's candidates
        assert np.array_equal(b_occ | f_occ, none_occ), f"{what}: any(BACK) | any(FRONT) != any(NONE)"
        assert np.array_equal(b_occ, b_hits["geometry_index"] != MISS) and np.array_equal(f_occ, f_hits["geometry_index"] != MISS)
        # (d) culling never brings a hit nearer, a ray that misses misses either way, and the other mode finds what this one does not
        tn = np.where(hit, none["t"], np.inf)
        tb, tf = np.where(b_occ, b_hits["t"], np.inf), np.where(f_occ, f_hits["t"], np.inf)
        assert (tb >= tn).all() and (tf >= tn).all() and (np.minimum(tb, tf) == tn).all()
        assert (b_hits["reserved"][b_occ] == fc.KIND_FRONT).all() and (f_hits["reserved"][f_occ] == fc.KIND_BACK).all()
        assert (hit & ~b_occ).sum() > 20 and (hit & ~f_occ).sum() > 20 and ((tb > tn) & b_occ).sum() > 0 and ((tf > tn) & f_occ).sum() > 0
        for mode, name in MODES:
            assert_cuts_equal(ctx, rays, culled[mode][0], f"{what}, {name}", face_cull=mode, **kw)


# ---------------------------------------------------------------------------------------------
# 4: tree independence
# ---------------------------------------------------------------------------------------------
def _answers(c, rays):
    return {mode: (c.ray_query(rays, face_cull=mode), c.ray_query(rays, any_hit=True, face_cull=mode)) for mode in (fc.NONE, fc.BACK, fc.FRONT)}


def _assert_answers(got, want, what):
    for mode in want:
        assert_hits_equal(got[mode][0], want[mode][0], f"{what}, face_cull {mode}, closest hit")
        assert np.array_equal(got[mode][1], want[mode][1]), f"{what}, face_cull {mode}, any hit"


def _vertex_block(scene, p):
    off = scene.primitives["vertex_offset"].astype(np.int64)
    return int(off[p]), int(off[p + 1]) if p + 1 < len(off) else len(scene.vertices)


def test_culled_answers_do_not_depend_on_the_tree():
    scene, rays = fc.soup_case(3, 1.0)
    c = lib.Context(64, 64)
    fresh = lib.Context(64, 64)
    try:
        c.upload_scene(scene)
        want = _answers(c, rays)
        assert (want[fc.BACK][0]["geometry_index"] != MISS).sum() > 300 and c.ray_query_statistics()[3] == 0
        for what, options in (("host-built tree", {"bvh_builder": 0}), ("world axes", {"bvh_frame": 0}), ("leaves of 1", {"bvh_leaf_triangles": 1}),
                              ("leaves of 4", {"bvh_leaf_triangles": 4}), ("presplit", {"bvh_presplit": 100}), ("presplit, host-built", {"bvh_presplit": 100, "bvh_builder": 0}),
                              ("host-built, leaves of 1, world axes", {"bvh_builder": 0, "bvh_leaf_triangles": 1, "bvh_frame": 0})):
            for k, v in options.items():
                c.set_option(k, v)
            c.upload_scene(scene)
            assert c.bvh_builder_used() == options.get("bvh_builder", 1)
            _assert_answers(_answers(c, rays), want, what)
            assert c.ray_query_statistics()[3] == 0
            for k in options:
                c.set_option(k, TREE_DEFAULTS[k])
        # moved vertices and a refit, a partial refit, a rebuild: the answers of a fresh build of the moved scene
        c.upload_scene(scene)
        rng = np.random.default_rng(41)
        v = scene.vertices.copy()
        for step, p in enumerate((2, 5, 7)):
            a, b = _vertex_block(scene, p)
            v["pos"][a:b] += rng.normal(scale=0.3, size=(b - a, 3)).astype(np.float32)
            c.update_vertices(v[a:b], first_vertex=a)
            (c.refit_geometry, lambda: c.refit_geometry_partial(force=True), c.rebuild_geometry)[step]()
            moved = dataclasses.replace(scene, vertices=v.copy())
            fresh.upload_scene(moved)
            now = _answers(fresh, rays)
            assert c.primitive_facing_flips().tolist() == fc.expected_flips(scene).tolist()
            _assert_answers(_answers(c, rays), now, ("refit", "partial refit", "rebuild")[step] + f" after primitive {p} moved")
            assert bits(now[fc.BACK][0]).tobytes() != bits(want[fc.BACK][0]).tobytes()
            assert (now[fc.NONE][0]["geometry_index"] == p).sum() > 20
            assert step != 1 or c.partial_refit_statistics()["partial_refits"] >= 1           # (a rebuild clears the refits' statistics)
    finally:
        c.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------
# 5: transforms that mirror at run time
# ---------------------------------------------------------------------------------------------
def test_a_transform_that_mirrors_at_run_time(oracle):
    scene, rays = fc.soup_case(2, 1.0)
    flips = fc.expected_flips(scene)
    c = lib.Context(64, 64)
    try:
        c.upload_scene(scene)
        before = c.ray_query(rays, face_cull=fc.NONE)              # (makes the device copy of the flips, which the update below has to keep right)
        assert c.face_cull_statistics() == [int(flips.sum()), 1, 0, 0]
        targets = [int(np.nonzero(flips == 0)[0][1]), int(np.nonzero(flips == 1)[0][0])]      # one primitive gets mirrored, one loses its mirror
        p = scene.primitives.copy()
        for k in targets:
            p["transform"][k] = fc.mirror_transform(p["transform"][k])
            c.update_primitive_transforms(p["transform"][k:k + 1], first_primitive=k)
        rc = c.L.vhr_ray_query_faces(c.handle, np.zeros(1, abi.ray_dtype).ctypes.data, 1, abi.RAY_QUERY_HOST_MEMORY, 0xFF, None, fc.BACK, np.zeros(1, abi.ray_hit_dtype).ctypes.data)
        assert rc == GRAPH and "vhr_refit_geometry" in c.L.vhr_last_error(c.handle).decode() and "vhr_ray_query_faces" in c.L.vhr_last_error(c.handle).decode()
        c.refit_geometry()
        st = c.refit_statistics()
        assert (st["records_outside"], st["children_outside"], st["non_finite"]) == (0, 0, 0), st
        moved = dataclasses.replace(scene, primitives=p)
        new_flips = fc.expected_flips(moved)
        assert (new_flips != flips).sum() == 2 and c.primitive_facing_flips().tolist() == new_flips.tolist() and c.face_cull_statistics()[0] == new_flips.sum()
        osc = oracle.Scene(moved)
        truth = rt.Truth(oracle, osc, rays)
        for mode, name in MODES:
            _judge(c, osc, moved, rays, truth, new_flips, mode, f"soup 2 after two transforms mirrored, {name}")
        after = c.ray_query(rays, face_cull=fc.NONE)
        assert_kinds(osc, moved, rays, after, new_flips, "soup 2 after two transforms mirrored, NONE")
        for k in targets:
            assert (after["geometry_index"] == k).sum() > 20 and (before["geometry_index"] == k).sum() > 20
        # the same transforms on a fresh build: the same answers
        fresh = lib.Context(64, 64)
        try:
            fresh.upload_scene(moved)
            _assert_answers(_answers(c, rays), _answers(fresh, rays), "refit against a fresh build")
        finally:
            fresh.close()
    finally:
        c.close()


def test_mirroring_a_planar_primitive_in_its_plane_swaps_its_kinds():
    """A quad in the plane y = 1 whose transform becomes diag(-1, 1, 1): the world triangles are the same set of points mirrored in x, the winding of
    each is reversed in world space, and the flip undoes it -- every ray still meets the same side.  Without the flip byte every kind would swap."""
    b = scenes._Builder()
    b.add(scenes.plane([-2, 1, 2], [4, 0, 0], [0, 0, -4], 4, 4), base_color=(0.7, 0.7, 0.7, 1))
    tiny = scenes.tiny_scene()
    scene = b.finish("mirror_quad", tiny.camera, tiny.light, [])
    rng = np.random.default_rng(3)
    n = 600
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = np.stack([rng.uniform(-1.9, 1.9, n), np.where(np.arange(n) % 2 == 0, 3.0, -1.0), rng.uniform(-1.9, 1.9, n)], 1)
    rays[:, 4:7] = np.stack([rng.uniform(-0.01, 0.01, n), np.where(np.arange(n) % 2 == 0, -1.0, 1.0), rng.uniform(-0.01, 0.01, n)], 1)
    rays[:, 7] = np.inf
    c = lib.Context(64, 64)
    try:
        c.upload_scene(scene)
        a = c.ray_query(rays, face_cull=fc.NONE)
        assert (a["geometry_index"] == 0).all() and len(np.unique(a["reserved"][0::2])) == 1 and len(np.unique(a["reserved"][1::2])) == 1
        assert a["reserved"][0] != a["reserved"][1]
        c.update_primitive_transforms(abi.mat_to_glm(np.diag([-1.0, 1, 1, 1]))[None])
        c.refit_geometry()
        assert c.primitive_facing_flips().tolist() == [1]
        m = c.ray_query(rays, face_cull=fc.NONE)
        assert (m["geometry_index"] == 0).all() and np.array_equal(m["reserved"], a["reserved"])
        for mode, kind in ((fc.BACK, fc.KIND_FRONT), (fc.FRONT, fc.KIND_BACK)):
            got = c.ray_query(rays, face_cull=mode)
            assert np.array_equal(got["geometry_index"] != MISS, a["reserved"] == kind) and np.array_equal(c.ray_query(rays, any_hit=True, face_cull=mode), a["reserved"] == kind)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# 6: with the alpha rule and the masks
# ---------------------------------------------------------------------------------------------
def _on_sub_scene(c, sub, keep, rays, mode, **kw):
    """The query on the scene made of the primitives `keep`, geometry indices in the full scene's numbering; nothing kept: every ray misses."""
    if sub is None:
        miss = np.zeros(len(rays), abi.ray_hit_dtype)
        miss["geometry_index"] = miss["primitive_index"] = MISS
        return miss, np.zeros(len(rays), bool)
    c.upload_scene(sub)
    return ray_mask_cases.remap_hits(c.ray_query(rays, face_cull=mode, **kw), keep), c.ray_query(rays, any_hit=True, face_cull=mode, **kw)


def test_face_culling_with_masks_equals_culling_the_sub_scene():
    sc = ray_mask_cases.scene()
    masks, rays = ray_mask_cases.masks(), ray_mask_cases.rays(sc)
    c, sub_ctx = lib.Context(64, 64), lib.Context(64, 64)
    try:
        c.upload_scene(sc)
        c.set_primitive_masks(masks)
        for m in ray_mask_cases.QUERY_MASKS:
            sub, keep = ray_mask_cases.sub_scene(sc, masks, m)
            plain = kinds = None
            for mode in (fc.NONE, fc.BACK, fc.FRONT):
                want, occ = _on_sub_scene(sub_ctx, sub, keep, rays, mode)
                got, got_occ = c.ray_query(rays, cull_mask=m, face_cull=mode), c.ray_query(rays, any_hit=True, cull_mask=m, face_cull=mode)
                assert c.ray_query_statistics()[3] == 0
                assert_hits_equal(got, want, f"cull_mask {m:#04x}, face_cull {mode}, closest hit")
                assert np.array_equal(got_occ, occ), f"cull_mask {m:#04x}, face_cull {mode}, any hit"
                if sub is None:                                    # mask 0: every ray misses
                    assert (got["geometry_index"] == MISS).all() and (got["reserved"] == 0).all() and not got_occ.any()
                elif mode == fc.NONE:                              # against the PLAIN query on the sub-scene (sub_ctx holds it) ...
                    plain = ray_mask_cases.remap_hits(sub_ctx.ray_query(rays), keep)
                    assert_hits_equal(got, plain, f"cull_mask {m:#04x}: NONE against the plain query on the sub-scene", kind=False)
                    kinds = got["reserved"].copy()
                else:                                              # ... restricted as identity (b): the rays whose plain hit the mode leaves
                    facing = kinds == (fc.KIND_FRONT if mode == fc.BACK else fc.KIND_BACK)
                    assert facing.sum() > 30
                    assert_hits_equal(got[facing], plain[facing], f"cull_mask {m:#04x}, face_cull {mode}: rays whose plain hit survives", kind=False)
    finally:
        c.close()
        sub_ctx.close()


def test_face_culling_with_the_alpha_rule_and_masks():
    """alpha_scenes.uniform_pair()'s A: the alpha rule removes its last four occluders, masks hide two of those it keeps (the set-up of
    tests/test_gpu_ray_masks.py::test_masks_with_alpha_test_rays); the face rule then culls among what is left -- the culled query on A
    equals the culled query on the scene holding what the other two rules leave."""
    sa, sb = alpha_scenes.uniform_pair()
    hidden = [5, 7]
    prim_masks = np.full(len(sa.primitives), 0xFF, np.uint8)
    prim_masks[hidden] = 0x08
    keep = np.array([p for p in range(len(sb.primitives)) if p not in hidden])
    truth_scene = alpha_scenes.subset(sb, keep)
    rays = ray_mask_cases.rays(sa)
    c, sub_ctx = lib.Context(64, 64), lib.Context(64, 64)
    try:
        c.upload_scene(sa)
        c.set_primitive_masks(prim_masks)
        differ = 0
        for mode in (fc.NONE, fc.BACK, fc.FRONT):
            want, occ = _on_sub_scene(sub_ctx, truth_scene, keep, rays, mode)
            got, got_occ = c.ray_query(rays, alpha_test=True, cull_mask=0x07, face_cull=mode), c.ray_query(rays, any_hit=True, alpha_test=True, cull_mask=0x07, face_cull=mode)
            assert c.face_cull_statistics()[1] == (1 if mode else 0) and c.ray_mask_statistics()[2] == 1 and c.ray_query_statistics()[3] == 0
            assert_hits_equal(got, want, f"alpha + masks, face_cull {mode}, closest hit")
            assert np.array_equal(got_occ, occ), f"alpha + masks, face_cull {mode}, any hit"
            # each of the other two rules acts under this mode: without it the answer differs
            no_alpha, no_mask = c.ray_query(rays, cull_mask=0x07, face_cull=mode), c.ray_query(rays, alpha_test=True, face_cull=mode)
            # (rays that meet the two small hidden quads from one side only are few: 20 for the unculled query, as tests/test_gpu_ray_masks.py has it)
            least = 20 if mode == fc.NONE else 1
            assert ray_mask_cases.hit_bits_differ(no_alpha, got).sum() >= least and ray_mask_cases.hit_bits_differ(no_mask, got).sum() >= least
            if mode:
                differ += int(ray_mask_cases.hit_bits_differ(got, none).sum())
            else:
                none = got
        assert differ >= 40                                        # ... and so does the face rule
        # alpha alone with the face rule: B itself
        for mode in (fc.BACK, fc.FRONT):
            want, occ = _on_sub_scene(sub_ctx, sb, np.arange(len(sb.primitives)), rays, mode)
            c.set_primitive_masks(np.full(len(sa.primitives), 0xFF, np.uint8))
            assert_hits_equal(c.ray_query(rays, alpha_test=True, face_cull=mode), want, f"alpha alone, face_cull {mode}")
            assert np.array_equal(c.ray_query(rays, any_hit=True, alpha_test=True, face_cull=mode), occ) and c.ray_mask_statistics()[2] == 0
    finally:
        c.close()
        sub_ctx.close()


# ---------------------------------------------------------------------------------------------
# 7: plumbing
# ---------------------------------------------------------------------------------------------
def test_host_and_device_memory_agree_and_an_empty_context_misses():
    import torch
    torch.cuda.set_device(0)
    scene, rays = fc.soup_case(2, 1.0)
    rays = rays[:1025]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = lib.Context(64, 64, stream=torch.cuda.current_stream().cuda_stream)
        try:
            assert c.current_stream() == stream.cuda_stream and c.face_cull_statistics() == [0, 0, 0, 0]
            for mode in (fc.NONE, fc.BACK, fc.FRONT):              # a context without geometry: every ray misses, no kind
                empty = c.ray_query(rays[:70], face_cull=mode)
                assert (empty["geometry_index"] == MISS).all() and (empty["primitive_index"] == MISS).all() and np.all(bits(empty)[:, [0, 1, 2, 5]] == 0)
                assert not c.ray_query(rays[:70], any_hit=True, face_cull=mode).any() and c.ray_query_statistics() == [70, 0, 0, 0]
            c.upload_scene(scene)
            ray_masks = np.where(np.arange(len(rays)) % 3 == 0, 0x02, 0xFF).astype(np.uint8)
            c.set_primitive_masks(np.where(np.arange(len(scene.primitives)) % 2 == 0, 0x01, 0x03).astype(np.uint8))
            d_rays = torch.from_numpy(rays).cuda()
            d_masks = torch.from_numpy(np.concatenate([[0], ray_masks]).astype(np.uint8)).cuda()[1:]          # (an odd address)
            assert d_rays.data_ptr() % 16 == 0
            for mode in (fc.NONE, fc.BACK, fc.FRONT):
                for n in (0, 1, 255, 257, 513, 1025):
                    want, want_occ = c.ray_query(rays[:n], ray_masks=ray_masks[:n], face_cull=mode), c.ray_query(rays[:n], any_hit=True, ray_masks=ray_masks[:n], face_cull=mode)
                    hits = torch.full((max(n, 1), 6), 0x7F, dtype=torch.int32, device="cuda")
                    occ = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
                    c.ray_query_device(d_rays.data_ptr(), n, hits.data_ptr(), ray_masks_ptr=d_masks.data_ptr(), face_cull=mode)
                    c.ray_query_device(d_rays.data_ptr(), n, occ.data_ptr(), any_hit=True, ray_masks_ptr=d_masks.data_ptr(), face_cull=mode)
                    got, got_occ = hits.cpu().numpy(), occ.cpu().numpy()                                     # (.cpu() waits on the current stream)
                    if n == 0:
                        assert (got == 0x7F).all() and (got_occ == 7).all()                                  # count == 0 launches nothing
                        assert c.L.vhr_ray_query_faces(c.handle, None, 0, 0, 0xFF, None, mode, None) == 0
                    else:
                        assert_hits_equal(got.view(abi.ray_hit_dtype).reshape(-1), want, f"device memory, face_cull {mode}, count {n}")
                        assert np.array_equal(got_occ.astype(bool), want_occ)
                        assert c.ray_query_statistics()[:2] == [n, int(want_occ.sum())] and c.ray_query_statistics()[3] == 0
            # the argument checks on a device context
            assert c.L.vhr_ray_query_faces(c.handle, d_rays.data_ptr(), 5, 0, 0xFF, None, 3, 0x2000) == -1 and "face_cull" in c.L.vhr_last_error(c.handle).decode()
            assert c.L.vhr_ray_query_faces(c.handle, d_rays.data_ptr() + 8, 5, 0, 0xFF, None, 3, 0x2000) == -1 and "16-byte" in c.L.vhr_last_error(c.handle).decode()
            # which launches ran: the statistics of the last query of any kind
            c.ray_query(rays, face_cull=fc.BACK)
            assert c.face_cull_statistics()[1] == 1
            c.ray_query(rays)
            assert c.face_cull_statistics()[1] == 0
            c.ray_query(rays, any_hit=True, face_cull=fc.FRONT)
            assert c.face_cull_statistics()[1] == 1
            c.ray_query(rays, any_hit=True, face_cull=fc.NONE)
            assert c.face_cull_statistics()[1] == 0
            c.ray_query(rays, face_cull=fc.NONE)
            assert c.face_cull_statistics()[1] == 1
            c.ray_query(rays, cull_mask=0x01)
            assert c.face_cull_statistics()[1] == 0
        finally:
            c.close()


def test_culled_queries_on_two_streams_leave_the_frames_identical():
    """Three frames of the hybrid path, two in flight: a BACK-culled any-hit query from the G-Buffer Pass's epilogue (on the front stream) and a
    FRONT-culled closest-hit query between frames (on the context's).  The frames are the frames without them, and each query's answers are
    its own mode's."""
    import torch
    from vulkanhybridrenderer_amd import ray_queries
    from vulkanhybridrenderer_amd.harness import HybridFrameLoop
    W, H, N = 480, 270, 3
    scene = scenes.sponza_proc(0.2)
    lo, hi = ray_queries.scene_bounds(scene)
    rng = np.random.default_rng(17)
    inside_rays = ray_queries.random_rays(rng, 3000, lo, hi, margin=0.0, tmaxs=(np.inf, 2.0))
    between_rays = np.concatenate([ray_queries.random_rays(rng, 1900, lo, hi, margin=0.1), alpha_scenes.grazing_rays(scene, rng, 600)])

    def run(with_queries):
        loop = HybridFrameLoop(scene, W, H, N, shadow=True, ao_spp=2, reflections=1, denoise=True, frames_in_flight=2)
        c = loop.ctx
        results = []
        try:
            d_inside, d_between = torch.from_numpy(inside_rays).cuda(), torch.from_numpy(between_rays).cuda()
            out_between = torch.zeros((len(between_rays), 6), dtype=torch.int32, device="cuda")
            out_inside = torch.zeros(len(inside_rays), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            streams = set()
            if with_queries:
                def inside(cc):
                    streams.add(cc.current_stream())
                    cc.ray_query_device(d_inside.data_ptr(), len(inside_rays), out_inside.data_ptr(), any_hit=True, face_cull=fc.BACK)
                c.set_pass_epilogue("G-Buffer Pass", inside)
            images = []
            for i in range(N):
                loop.frame(i)
                if with_queries:
                    streams.add(c.current_stream())
                    c.ray_query_device(d_between.data_ptr(), len(between_rays), out_between.data_ptr(), face_cull=fc.FRONT)
                c.synchronize()
                images.append([c.download(lib.RAYTRACED), c.download(lib.DENOISED), c.download(lib.REFLECTIONS)])
                if with_queries:
                    results.append((out_between.cpu().numpy().copy(), out_inside.cpu().numpy().copy()))
                    assert c.face_cull_statistics()[1] == 1
            return images, results, len(streams)
        finally:
            loop.close()

    plain, _, _ = run(False)
    queried, results, n_streams = run(True)
    assert n_streams == 2
    for k, (a, b) in enumerate(zip(plain, queried)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), f"frame {k}, image {j}: a frame around culled queries differs"
    c = lib.Context(64, 64)
    try:
        c.upload_scene(scene)
        want = c.ray_query(between_rays, face_cull=fc.FRONT)
        other = c.ray_query(between_rays, face_cull=fc.BACK)
        occ, other_occ = c.ray_query(inside_rays, any_hit=True, face_cull=fc.BACK), c.ray_query(inside_rays, any_hit=True, face_cull=fc.FRONT)
    finally:
        c.close()
    assert ray_mask_cases.hit_bits_differ(want, other).sum() > 100 and (occ != other_occ).sum() > 100          # the two modes' answers are not each other's
    for between, inside in results:
        assert_hits_equal(between.view(abi.ray_hit_dtype).reshape(-1), want, "between frames, FRONT")
        assert np.array_equal(inside.astype(bool), occ)
