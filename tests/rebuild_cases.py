"""What tests/test_rebuild_host.py and tests/test_gpu_rebuild.py share: the soups, the updates applied before a vhr_rebuild_geometry, the arrays
those updates leave, and the state that must equal a fresh context's.  The truth of every comparison is a FRESH context given the updated
arrays through update_geometry (and, for the previous records, triangle_records() read before the call), never the context under test."""
import numpy as np

from tests import object_motion_cases as omc
from tests import partial_refit_cases as cases
from tests.test_gpu_fuzz import soup
from vulkanhybridrenderer_amd import scenes

SOUPS = {"soup3": (3, 2000, 8), "soup5": (5, 2800, 11)}          # 2 000 / 2 800 triangles in 9 / 12 primitives (the floor is one)
UPDATE_KINDS = ("vertices", "transforms", "both")


def make_soup(name, rotated=False):
    s = soup(*SOUPS[name])
    return scenes.rotated(s, rot_y=0.6, rot_x=0.25) if rotated else s


def presplit_scene():
    """The scene tests/test_refit_host.py builds its presplit tree from (with "bvh_presplit" 100 and "bvh_frame" 0 its level is >= 0)."""
    return scenes.rotated(soup(22, 1500, 6), rot_y=0.6, rot_x=0.25)


def update_calls(scene, kind):
    """Vertex updates over two disjoint ranges, one primitive's transform, or both (tests/partial_refit_cases.py makes them)."""
    ups = cases.updates(scene)
    v, t = ups["4 two disjoint ranges"], ups["6 one primitive's transform"]
    return {"vertices": v, "transforms": t, "both": v + t}[kind]


def updated_arrays(scene, calls):
    """(vertices, primitives) as the context holds them after `calls`."""
    vertices, primitives = scene.vertices.copy(), scene.primitives.copy()
    omc.apply_to_arrays(vertices, primitives, calls)
    return vertices, primitives


def tree_state(ctx):
    """Everything the issue lists as equal to a fresh context's after a rebuild."""
    return dict(fingerprint=ctx.bvh_fingerprint(), tree=ctx.bvh_tree_fingerprint(), forms=ctx.bvh_forms_fingerprint(), form_checks=ctx.bvh_form_checks(),
                statistics=ctx.bvh_statistics(), frame=ctx.bvh_frame().view(np.uint32).tolist(), presplit_level=ctx.bvh_presplit_level(),
                builder=ctx.bvh_builder_used(), sah=ctx.bvh_sah_cost())


def assert_reads_as_after_a_build(ctx, what):
    """The refit bookkeeping after a rebuild: "refits since the last build" = 0, nothing of a last refit, nothing pending."""
    st, pst = ctx.refit_statistics(), ctx.partial_refit_statistics()
    assert all(v == 0 for v in st.values()), (what, st)
    assert all(v == 0 for v in pst.values()), (what, pst)
    built, now = ctx.bvh_sah_cost()
    assert built == now, what


def moved_subset(scene, seed=3):
    """("v", first, records): the last primitive's first 40 vertices displaced -- a known subset of the triangles moves."""
    rng = np.random.default_rng(seed)
    first, end = cases.vertex_blocks(scene)[-1]
    v = scene.vertices[first:min(end, first + 40)].copy()
    v["pos"] += rng.normal(scale=0.3, size=v["pos"].shape).astype(np.float32)
    return [("v", first, v)]
