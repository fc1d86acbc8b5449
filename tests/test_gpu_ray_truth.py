"""The device's ray answers judged against exact arithmetic (tests/ray_truth.py) at three units of length -- millimetres, metres,
kilometres -- and on the 1000-fold mixed scene: ray queries on every tree the library builds, after refits, with cull masks, and the
hybrid path's own walkers (the queue kernels with the 32-byte nodes and with the 48-byte ones) through the rays the oracle logs.  No
bit-identity with the oracle is asked here (scale 1 keeps those tests): a verdict needs no tree-independence, so it holds where the
oracle's own BVH and brute force part ways."""
import numpy as np
import pytest

from tests import ray_truth as rt
from tests.helpers import GpuHybrid, f16
from vulkanhybridrenderer_amd import abi, camera, lib, scenes

pytestmark = pytest.mark.gpu
TREES = (("device-built tree", {}), ("host-built tree", {"bvh_builder": 0}), ("presplit", {"bvh_presplit": 100}), ("world axes", {"bvh_frame": 0}))
TREE_DEFAULTS = {"bvh_builder": 1, "bvh_presplit": 0, "bvh_frame": 1}


def _judge_queries(ctx, scene, rays, truth, what, **masks):
    """Closest hit and terminate-on-first-hit of one batch: zero violations, no stack overflow.  -> (closest verdict, any-hit verdict, hits, occluded)"""
    hits = ctx.ray_query(rays, **masks)
    s_closest = ctx.ray_query_statistics()
    occ = ctx.ray_query(rays, any_hit=True, **masks)
    s_any = ctx.ray_query_statistics()
    assert s_closest[3] == 0 and s_any[3] == 0, (what, s_closest, s_any)
    hit, flat = rt.flat_of_hits(scene, hits)
    vc = rt.judge_closest(truth, hit, flat, hits["t"], hits["u"], hits["v"])
    va = rt.judge_any(truth, occ)
    print(f"{what}: closest {vc.violations} violations (D explained {vc.explained_d}, true hits passed over explained {vc.explained_lost}), "
          f"any hit {va.violations}; binary64 rays {s_closest[2]} / {s_any[2]}")
    assert vc.violations == 0, f"{what}, closest hit: {vc.describe()}"
    assert va.violations == 0, f"{what}, any hit: {va.describe()}"
    return vc, va, hits, occ


@pytest.mark.parametrize("scale", rt.SCALES)
@pytest.mark.parametrize("seed", [s[0] for s in rt.SOUPS])
def test_ray_queries_on_every_tree(oracle, seed, scale):
    """8 000 random rays per soup (and 1 500 grazing ones on soup 3), every length times `scale`, on the four trees."""
    base = rt.soup_scene(seed)
    scene = rt.scaled_scene(base, scale)
    osc = oracle.Scene(scene)
    sets = [("random", rt.scaled_rays(rt.soup_rays(base, seed), scale))]
    if seed == 3:
        sets.append(("grazing", rt.scaled_rays(rt.soup_grazing(base), scale)))
    sets = [(name, rays, rt.Truth(oracle, osc, rays)) for name, rays in sets]
    ctx = lib.Context(64, 64)
    try:
        for tree, options in TREES:
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.upload_scene(scene)
            for name, rays, truth in sets:
                _, _, _, occ = _judge_queries(ctx, scene, rays, truth, f"soup {seed} x {scale}, {tree}, {name} rays")
                if name == "random":
                    assert 0.1 < occ.mean() < 0.95
            for k in options:
                ctx.set_option(k, TREE_DEFAULTS[k])
    finally:
        ctx.close()


def _vertex_block(scene, p):
    off = scene.primitives["vertex_offset"].astype(np.int64)
    return int(off[p]), int(off[p + 1]) if p + 1 < len(off) else len(scene.vertices)


@pytest.mark.parametrize("scale", [rt.SCALES[0], rt.SCALES[2]])
def test_ray_queries_after_a_refit_and_a_partial_refit(oracle, scale):
    """Soup 3: one primitive's vertex block moves, vhr_refit_geometry; a second block moves, vhr_refit_geometry_partial.  The truth is of
    the moved triangles."""
    base = rt.soup_scene(3)
    scene = rt.scaled_scene(base, scale)
    rays = rt.scaled_rays(rt.soup_rays(base, 3), scale)
    rng = np.random.default_rng(41)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        v = scene.vertices.copy()
        for step, p in enumerate((2, 5)):
            a, b = _vertex_block(scene, p)
            v["pos"][a:b] += (rng.normal(scale=0.3, size=(b - a, 3)) * scale).astype(np.float32)
            ctx.update_vertices(v[a:b], first_vertex=a)
            if step == 0:
                ctx.refit_geometry()
            else:
                ctx.refit_geometry_partial(force=True)
            st = ctx.refit_statistics()
            assert (st["records_outside"], st["children_outside"], st["non_finite"]) == (0, 0, 0), st
            moved = scenes.Scene(scene.name, v.copy(), scene.indices, scene.primitives, scene.textures, scene.camera, scene.light)
            truth = rt.Truth(oracle, oracle.Scene(moved), rays)
            _, _, hits, _ = _judge_queries(ctx, moved, rays, truth, f"soup 3 x {scale}, {'refit' if step == 0 else 'partial refit'} of primitive {p}")
            assert (hits["geometry_index"] == p).sum() > 20                   # the moved block is hit
        assert ctx.partial_refit_statistics()["partial_refits"] >= 1
    finally:
        ctx.close()


@pytest.mark.parametrize("scale", rt.SCALES)
def test_masked_ray_queries(oracle, scale):
    """Soup 2 with its primitives alternately at 0x01 and 0x02 and rays alternately of mask 0x01 and 0x02 (each ray sees about half the
    primitives), and with cull_mask 0x02 alone: vhr_ray_query_masked against the truth over the visible subset."""
    base = rt.soup_scene(2)
    scene = rt.scaled_scene(base, scale)
    osc = oracle.Scene(scene)
    rays = rt.scaled_rays(rt.soup_rays(base, 2), scale)
    prim_masks = np.where(np.arange(len(scene.primitives)) % 2 == 0, 0x01, 0x02).astype(np.uint8)
    ray_masks = np.where(np.arange(len(rays)) % 2 == 0, 0x01, 0x02).astype(np.uint8)
    plain = rt.Truth(oracle, osc, rays)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        ctx.set_primitive_masks(prim_masks)
        for what, kw, tkw in (("per-ray masks", dict(ray_masks=ray_masks), dict(ray_masks=ray_masks)), ("cull_mask 0x02", dict(cull_mask=0x02), dict(cull_mask=0x02))):
            truth = rt.Truth(oracle, osc, rays, prim_masks=prim_masks, **tkw)
            assert 0.25 * plain.hit.sum() < truth.hit.sum() < 0.75 * plain.hit.sum()        # about half the scene is hidden
            _, _, hits, occ = _judge_queries(ctx, scene, rays, truth, f"soup 2 x {scale}, {what}", **kw)
            assert ctx.ray_mask_statistics()[2] == 1 and 0.03 < occ.mean() < 0.95
            seen = hits["geometry_index"][hits["geometry_index"] != abi.RAY_MISS]
            m = ray_masks[hits["geometry_index"] != abi.RAY_MISS] if "ray_masks" in kw else np.uint8(0x02)
            assert ((prim_masks[seen] & m) != 0).all()
    finally:
        ctx.close()


def test_ray_queries_on_the_1000_fold_mix(oracle):
    """tiny_far with its vertices scaled by 1e-3 .. 1e3 around 12 345: the case the bit-identity test had to leave out."""
    scene = rt.tiny_far()
    rays = rt.tiny_far_rays(scene)
    truth = rt.Truth(oracle, oracle.Scene(scene), rays)
    ctx = lib.Context(64, 64)
    try:
        for tree, options in TREES:
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.upload_scene(scene)
            _, _, _, occ = _judge_queries(ctx, scene, rays, truth, f"tiny_far, {tree}")
            assert 0.1 < occ.mean() < 0.95
            for k in options:
                ctx.set_option(k, TREE_DEFAULTS[k])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# the hybrid path's own walkers
# ---------------------------------------------------------------------------------------------
def _rays_of(log, kind, n_pixels):
    sel = log[log["kind"] == kind]
    assert len(np.unique(sel["pixel"])) == len(sel) and (sel["pixel"] < n_pixels).all()
    rays = np.zeros((len(sel), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = sel["o"], sel["tmin"], sel["d"], sel["tmax"]
    return sel["pixel"].astype(np.int64), rays


HYBRID_SCENES = {"tiny_scene": scenes.tiny_scene, "sponza_proc_rot": lambda: scenes.rotated(scenes.sponza_proc(0.15), rot_y=0.6, rot_x=0.25)}


@pytest.mark.parametrize("scale", rt.SCALES)
@pytest.mark.parametrize("name", sorted(HYBRID_SCENES))
def test_the_hybrid_paths_walkers(oracle, name, scale):
    """96 x 64, camera and trace parameters scaled with the scene.  Frame A: shadows and one AO ray, no mirror ray -- both channels of
    Raytraced are 0 or 1 per pixel, each judged as an any-hit answer for the ray the oracle logged for that pixel.  Frame B: the mirror
    ray -- the alpha of Reflections judged as hit / miss.  With the 32-byte nodes (in use: half_nodes) and with compact_nodes 0.  The
    device traces from the oracle's G-buffer (read back and compared bit for bit), so the logged rays are its rays."""
    W, H = 96, 64
    scene = rt.scaled_scene(HYBRID_SCENES[name](), scale)
    osc = oracle.Scene(scene)
    pfd = camera.dolly_frames(scene, W, H, 2)[1]
    gbuf = osc.gbuffer(pfd, W, H)
    tp_a = rt.scaled_trace_params(abi.default_trace_params(shadow=True, ao_spp=1, reflections=False), scale)
    tp_b = rt.scaled_trace_params(abi.default_trace_params(shadow=False, ao_spp=0, reflections=True), scale)
    with oracle.Audit(ray_log=4 * W * H) as a:
        osc.raygen(pfd, tp_a, gbuf[0], gbuf[2], want_reflections=False)
    with oracle.Audit(ray_log=4 * W * H) as b:
        osc.raygen(pfd, tp_b, gbuf[0], gbuf[2])
    covered = int((gbuf[2] != 0).sum())
    assert covered > W * H // 4 and len(a.ray_log) == 2 * covered and len(b.ray_log) == covered
    judged = []
    for kind, log in ((oracle.RAY_KIND_SHADOW, a.ray_log), (oracle.RAY_KIND_AO, a.ray_log), (oracle.RAY_KIND_MIRROR, b.ray_log)):
        pix, rays = _rays_of(log, kind, W * H)
        judged.append((kind, pix, rt.Truth(oracle, osc, rays)))
    g = GpuHybrid(scene, W, H, denoise=False, trace_params=tp_a)
    try:
        g.ctx.update_vertices(scene.vertices)                       # an identity refit: the tree stays bit for bit, and the refit's statistics
        g.ctx.refit_geometry()                                      # say which node form the walkers are on
        assert g.ctx.refit_statistics()["half_nodes"] == 1 and g.ctx.bvh_form_checks()[1:] == (0, 0, 0)
        for compact in (1, 0):
            g.ctx.set_option("compact_nodes", compact)
            g.ctx.set_trace_params(tp_a)
            g.frame(pfd, gbuf)
            for image, want in ((lib.NORMALS, gbuf[0]), (lib.DEPTH, gbuf[2])):
                assert np.array_equal(g.ctx.download(image).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), "the device's G-buffer is not the oracle's"
            visibility = f16(g.ctx.download(lib.RAYTRACED)).reshape(W * H, 2)
            g.ctx.set_trace_params(tp_b)
            g.frame(pfd, gbuf)
            alpha = f16(g.ctx.download(lib.REFLECTIONS)).reshape(W * H, 4)[:, 3]
            for kind, pix, truth in judged:
                values = alpha[pix] if kind == oracle.RAY_KIND_MIRROR else visibility[pix, 0 if kind == oracle.RAY_KIND_SHADOW else 1]
                assert np.isin(values, (0.0, 1.0)).all()
                occluded = values == 1.0 if kind == oracle.RAY_KIND_MIRROR else values == 0.0
                v = rt.judge_any(truth, occluded)
                what = f"{name} x {scale}, compact_nodes {compact}, {('shadow', 'AO', 'mirror')[kind]} rays"
                print(f"{what}: {v.violations} violations of {len(pix)}; occluded without an exact hit (explained) {v.explained_d}, true hits passed over (explained) {v.explained_lost}")
                assert v.violations == 0, f"{what}: {v.describe()}; first pixels {pix[v.bad][:4].tolist()}"
                assert 0.02 < occluded.mean() < 0.999, (what, occluded.mean())
    finally:
        g.close()
