"""The trees tests/test_tree_truth.py (host builder, host-only contexts) and tests/test_gpu_tree_truth.py (device builder and device refits) hand to
the judge of tests/tree_truth.py, and the routine that judges one context at every stage of a case.  No tests here."""
import dataclasses

import numpy as np

from tests import ray_truth as rt
from tests import tree_truth as tt
from tests.partial_refit_cases import form_scenes, vertex_blocks
from tests.test_gpu_fuzz import soup
from vulkanhybridrenderer_amd import abi, lib, scenes


def one_leaf_scene():
    b = scenes._Builder()
    pos = np.float32([[0.25, 0.5, -1.0], [1.5, 0.75, -1.25], [0.5, 2.0, -0.5]])
    nrm = np.tile(np.float32([0, 0, 1]), (3, 1))
    b.add((pos, nrm, np.zeros((3, 2), np.float32), np.uint32([[0, 1, 2]])), base_color=(0.5, 0.5, 0.5, 1))
    return b.finish("one_leaf", scenes.tiny_scene().camera, scenes.tiny_scene().light)


def outlier_soup():
    from tests.test_gpu_point_query import outlier_soup as make
    return make(3.0e5)


def translated(scene, offset):
    """Every primitive's translation plus `offset` (world axes)."""
    p = scene.primitives.copy()
    p["transform"][:, 12:15] += np.asarray(offset, np.float32)
    return dataclasses.replace(scene, primitives=p)


def framed_scenes():
    """Scenes turned off the world axes for which the frame search finds a frame."""
    return {"tiny_rot": scenes.tiny_rot, "soup1_rot": lambda: scenes.rotated(rt.soup_scene(1))}


# name -> (scene, options).  Every tree is built once and judged; LIFECYCLES below go on to refit and rebuild theirs.
def build_cases():
    cases = {"tiny": (scenes.tiny_scene, {}), "one leaf": (one_leaf_scene, {}), "far, mixed scales": (lambda: form_scenes()["far"][0], {}),
             "outliers beyond the half range": (outlier_soup, {}),
             "presplit 100": (lambda: scenes.rotated(soup(22, 1500, 6)), {"bvh_presplit": 100, "bvh_frame": 0})}
    for seed in (1, 2, 3):
        for leaf in (1, 2, 4):
            cases[f"soup{seed} leaf {leaf}"] = (lambda seed=seed: rt.soup_scene(seed), {"bvh_leaf_triangles": leaf})
    for name, make in framed_scenes().items():                  # (frame 1: the search finds a frame for both, the tests assert it)
        for frame in (0, 1):
            cases[f"{name} frame {frame}"] = (make, {"bvh_frame": frame})
    for seed in (1, 2, 3):
        for s in rt.SCALES:
            if s != 1.0:                                        # (x 1: the leaf cases above)
                cases[f"soup{seed} x {s:g}"] = (lambda seed=seed, s=s: rt.scaled_scene(rt.soup_scene(seed), s), {})
    return cases


def check_built_case(ctx, scene, name, options, what):
    """One build case on the context that has built it: the verdict, and what the case is there for."""
    arrays, _ = judge_context(ctx, scene, what, leaf=options.get("bvh_leaf_triangles", 2))
    if " frame " in name:
        assert arrays["frame_on"] == bool(options["bvh_frame"]), what
    if name.startswith("presplit"):
        assert ctx.bvh_presplit_level() >= 0 and arrays["record_count"] > scene.triangle_count, what
    if name.startswith("outliers"):
        assert not arrays["half_nodes"], what


LIFECYCLES = ("soup2", "soup1_rot", "tiny_rot")
# (scene, how it is moved, whether the frame search still finds a frame there)
FAR = tuple((name, how, not (name == "soup1_rot" and how == "x 2^10")) for name in ("tiny_rot", "soup1_rot") for how in ("along the frame 2^14", "along the frame 2^17", "x 2^10"))


def lifecycle_scene(name):
    return rt.soup_scene(2) if name == "soup2" else framed_scenes()[name]()


def far_scene(name, how, frame):
    """The far-frame scenes: translated along the frame's third row (so the other two frame coordinates stay small), or scaled about the origin."""
    scene = framed_scenes()[name]()
    if how == "x 2^10":
        return rt.scaled_scene(scene, 2.0 ** 10)
    row = np.asarray(frame, np.float32).reshape(3, 3)[2]
    return translated(scene, row * np.float32(2.0 ** (14 if how.endswith("14") else 17)))


def judge_context(ctx, scene, what, leaf=2, refitted=False):
    """The judge's verdict on the tree `ctx` holds, asserted clean, with T7: the library's own counters and its surface-area cost say the same.
    refitted: the tree has been refitted since it was built (the refit's counters are compared too; the frame's world magnitude is the build's)."""
    arrays = ctx.bvh_arrays()
    stats = ctx.bvh_statistics()
    verdict = tt.judge(arrays, scene, leaf_triangles=leaf, presplit=ctx.bvh_presplit_level() >= 0, statistics=stats)
    print(f"{what}: {verdict.summary()}")
    assert verdict.clean(), (what, verdict.failed(), {r: w[:5] for r, w in verdict.where.items() if w})
    assert verdict.faces > 0, what
    assert ctx.bvh_form_checks() == (2 * stats["nodes"], 0, 0, 0), (what, ctx.bvh_form_checks())
    if refitted:
        st = ctx.refit_statistics()
        assert (st["records_outside"], st["children_outside"], st["non_finite"]) == (0, 0, 0), (what, st)
        assert st["half_nodes"] == int(arrays["half_nodes"]), (what, st)
    else:
        # the world magnitude the tightness rule takes from the header, held from outside: the power of two in [2 W, 4 W) for the judge's own W
        # (W from exact corners, the builders' from the fp32 ones: 2^-20 of slack), 0 on the world axes
        w, magnitude = verdict.world_magnitude, arrays["frame_magnitude"]
        if arrays["frame_on"]:
            assert 2.0 * w * (1 - 2.0 ** -20) <= magnitude < 4.0 * w * (1 + 2.0 ** -20) and np.log2(magnitude) % 1 == 0, (what, w, magnitude)
        else:
            assert magnitude == 0.0, (what, magnitude)
    mine, theirs = tt.sah_cost(arrays), ctx.bvh_sah_cost()[1]
    assert abs(mine - theirs) <= 1e-12 * abs(mine), (what, mine, theirs)
    return arrays, verdict


def run_lifecycle(ctx, scene, name):
    """build -> whole refit of every vertex -> forced partial refit of the last primitive's block -> a mirrored transform through
    vhr_update_primitive_transforms -> vhr_rebuild_geometry; judged after each.  Returns the verdicts by stage."""
    out = {"build": judge_context(ctx, scene, f"{name} build")[1]}
    rng = np.random.default_rng(5)
    v = scene.vertices.copy()
    v["pos"] += rng.normal(scale=0.05, size=v["pos"].shape).astype(np.float32)
    ctx.update_vertices(v)
    ctx.refit_geometry()
    scene = dataclasses.replace(scene, vertices=v)
    out["refit"] = judge_context(ctx, scene, f"{name} refit", refitted=True)[1]
    first, end = vertex_blocks(scene)[-1]
    v = v.copy()
    v["pos"][first:end] += rng.normal(scale=0.3, size=(end - first, 3)).astype(np.float32)
    ctx.update_vertices(v[first:end], first_vertex=first)
    ctx.refit_geometry_partial(force=True)
    assert ctx.partial_refit_statistics()["ran_as"] == 0, name
    scene = dataclasses.replace(scene, vertices=v)
    out["partial refit"] = judge_context(ctx, scene, f"{name} partial refit", refitted=True)[1]
    p = scene.primitives.copy()
    last = len(p) - 1
    m = np.asarray(p["transform"][last], np.float64).reshape(4, 4).T
    p["transform"][last] = abi.mat_to_glm(m @ np.diag([-1.0, 1.0, 1.0, 1.0]))                 # mirrors the primitive in its own x
    ctx.update_primitive_transforms(p["transform"][last:last + 1], first_primitive=last)
    ctx.refit_geometry()
    assert ctx.primitive_facing_flips()[last] == 1, name
    scene = dataclasses.replace(scene, primitives=p)
    out["mirrored transform"] = judge_context(ctx, scene, f"{name} mirrored transform", refitted=True)[1]
    v = v.copy()
    v["pos"] += rng.normal(scale=0.5, size=v["pos"].shape).astype(np.float32)
    ctx.update_vertices(v)
    ctx.rebuild_geometry()
    scene = dataclasses.replace(scene, vertices=v)
    out["rebuild"] = judge_context(ctx, scene, f"{name} rebuild")[1]
    return out


def check_far(ctx, name, how, keeps_frame, what=None):
    """A far-frame scene on `ctx`, which holds the scene at the origin: the frame is read there, the scene moved along its third row (or scaled)
    and handed over again.  -> (scene, arrays, verdict)"""
    at_origin = ctx.bvh_arrays()
    assert at_origin["frame_on"], name
    scene = far_scene(name, how, at_origin["frame"])
    ctx.update_geometry(scene.vertices, scene.indices, scene.primitives)
    arrays, verdict = judge_context(ctx, scene, what or f"{name} {how}")
    assert arrays["frame_on"] == keeps_frame, (name, how)
    if keeps_frame:
        assert not np.array_equal(arrays["frame"], np.eye(3, dtype=np.float32).reshape(9)), "the far scene lost its frame"
    assert verdict.min_margin_over_rho > 1.0
    return scene, arrays, verdict


def check_leaving_the_magnitude(ctx, scene, partial):
    """The frame's padding is sized by the world magnitude W' of the build; a refit keeps it (so that a partial refit leaves what a whole one
    leaves) and refuses records beyond it, as it refuses non-finite ones, with a message that tells the two apart.  On `ctx`, which has built
    the framed `scene`: a move to just inside W' refits to a clean tree, a move by 3 W' fails, and a rebuild recovers with a larger W'.
    partial: through vhr_refit_geometry_partial's dirty path (an identity refit first: the first refit after a build is whole-tree)."""
    def refit():
        ctx.refit_geometry_partial(force=True) if partial else ctx.refit_geometry()
        assert not partial or ctx.partial_refit_statistics()["ran_as"] == 0
    magnitude = ctx.bvh_arrays()["frame_magnitude"]
    world = tt.judge(ctx.bvh_arrays(), scene).world_magnitude
    assert 2 * world <= magnitude < 4 * world
    if partial:
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
    inside = translated(scene, [0.9 * magnitude - world, 0, 0])                     # the largest |coordinate| stays below 0.9 W'
    ctx.update_primitive_transforms(inside.primitives["transform"])
    refit()
    arrays, verdict = judge_context(ctx, inside, "moved to just inside the magnitude", refitted=True)
    assert arrays["frame_magnitude"] == magnitude and 0.5 * magnitude < verdict.world_magnitude < magnitude
    outside = translated(scene, [3.0 * magnitude, 0, 0])
    ctx.update_primitive_transforms(outside.primitives["transform"])
    try:
        refit()
        raise AssertionError("a refit beyond the frame's world magnitude succeeded")
    except lib.VhrError as e:
        assert "beyond the world magnitude" in str(e) and "vhr_rebuild_geometry" in str(e) and "non-finite" not in str(e), str(e)
    assert ctx.refit_statistics()["non_finite"] > 0
    ctx.rebuild_geometry()
    arrays, _ = judge_context(ctx, outside, "rebuilt after leaving the magnitude")
    assert arrays["frame_magnitude"] >= 2 * 3.0 * magnitude
