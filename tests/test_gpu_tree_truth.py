"""The judge of tests/tree_truth.py on the trees in DEVICE memory: the device builder's (k0_emit_kernel, k0_forms_kernel), the device refits'
(the k0_refit_* kernels), the rebuild's, with "object_motion_vectors" on and off, and a host-built tree after its upload -- the case list of
tests/test_tree_truth.py.  Then, end to end on the far-frame scenes: the answers of vhr_ray_query on the tree in
its frame, on the world-axes tree and the oracle's brute force, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import ray_truth as rt
from tests import tree_truth as tt
from tests import tree_truth_cases as cases
from tests.helpers import GpuHybrid
from vulkanhybridrenderer_amd import camera, lib

pytestmark = pytest.mark.gpu
GRAPH = -5          # include/vhr_amd.h


def _ctx(scene, **options):
    c = lib.Context(64, 64)
    for k, v in options.items():
        c.set_option(k, v)
    c.upload_scene(scene)
    return c


@pytest.mark.parametrize("builder", [1, 0])
@pytest.mark.parametrize("name", sorted(cases.build_cases()))
def test_built_trees_are_clean(vhr, name, builder):
    make, options = cases.build_cases()[name]
    scene = make()
    c = _ctx(scene, bvh_builder=builder, **options)
    try:
        assert c.bvh_builder_used() == (builder if name != "one leaf" else 0)          # (a one-leaf scene goes to the host builder)
        cases.check_built_case(c, scene, name, options, f"{name}, builder {builder}")
    finally:
        c.close()


@pytest.mark.parametrize("builder", [1, 0])
@pytest.mark.parametrize("name,how,keeps_frame", cases.FAR)
def test_the_frame_far_from_the_origin(vhr, name, how, keeps_frame, builder):
    """tests/test_tree_truth.py's far-frame scenes in device memory: the device builder's trees, and the host builder's after their upload."""
    c = _ctx(cases.framed_scenes()[name](), bvh_builder=builder)
    try:
        cases.check_far(c, name, how, keeps_frame, what=f"{name}, builder {builder}, {how}")
        assert c.bvh_builder_used() == builder
    finally:
        c.close()


@pytest.mark.parametrize("partial", [False, True])
@pytest.mark.parametrize("builder", [1, 0])
def test_a_refit_that_leaves_the_frame_magnitude_fails_and_a_rebuild_recovers(vhr, builder, partial):
    """The device refits' own refusal (coordinates_beyond in k0_refit_records_kernel and k0_refit_mark_kernel): just inside the build's world
    magnitude a refit of either kind succeeds and leaves a clean tree, beyond it the refit fails, and a rebuild recovers."""
    scene = cases.framed_scenes()["soup1_rot"]()
    c = _ctx(scene, bvh_builder=builder)
    try:
        cases.check_leaving_the_magnitude(c, scene, partial)
        assert c.bvh_builder_used() == builder
    finally:
        c.close()


@pytest.mark.parametrize("motion", [0, 1])
@pytest.mark.parametrize("builder", [1, 0])
@pytest.mark.parametrize("name", cases.LIFECYCLES)
def test_refitted_and_rebuilt_trees_are_clean(vhr, name, builder, motion):
    scene = cases.lifecycle_scene(name)
    c = _ctx(scene, bvh_builder=builder, object_motion_vectors=motion)
    try:
        assert c.bvh_arrays()["frame_on"] == (name != "soup2")
        cases.run_lifecycle(c, scene, f"{name}, builder {builder}, motion {motion}")
        assert c.bvh_builder_used() == builder
    finally:
        c.close()


def test_host_and_device_builders_leave_the_same_slots(vhr):
    """The frame's world magnitude and the slots it pads, from both builders: the same bits (the leaves' order in memory may differ)."""
    scene = cases.far_scene("tiny_rot", "x 2^10", None)
    seen = []
    for builder in (1, 0):
        c = _ctx(scene, bvh_builder=builder)
        try:
            a = c.bvh_arrays()
            seen.append((a["frame_on"], a["frame_magnitude"], a["frame"].tobytes(), a["centre"].tobytes(), c.bvh_tree_fingerprint()))
        finally:
            c.close()
    assert seen[0] == seen[1] and seen[0][0] and seen[0][1] > 0


def test_refused_from_inside_a_pass(vhr):
    scene = rt.soup_scene(1)
    seen = {}

    class InPass(GpuHybrid):
        def _gbuffer_pass(self, ctx):
            if not seen:
                header, counts = (C.c_uint32 * 24)(), (C.c_uint32 * 2)()
                bufs = [np.zeros((ctx.bvh_statistics()["nodes"] + ctx.bvh_statistics()["triangles"]) * 64, np.uint8) for _ in range(5)]
                seen["rc"] = ctx.L.vhr_debug_bvh_arrays(ctx.handle, header, *[b.ctypes.data for b in bufs], ctx.bvh_statistics()["nodes"],
                                                        ctx.bvh_statistics()["triangles"], counts)
                seen["msg"] = ctx.L.vhr_last_error(ctx.handle).decode()
            super()._gbuffer_pass(ctx)
    g = InPass(scene, 96, 64, gbuffer="standin")
    try:
        try:
            g.frame(camera.dolly_frames(scene, 96, 64, 1)[0])
        except lib.VhrError as e:                             # (the refusal's message is the context's last error when the graph returns)
            assert "vhr_debug_bvh_arrays" in str(e)
        assert seen["rc"] == GRAPH and "vhr_debug_bvh_arrays: called from inside a pass" in seen["msg"], seen
        g.ctx.synchronize()
        assert tt.judge(g.ctx.bvh_arrays(), scene, statistics=g.ctx.bvh_statistics()).clean()
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------
# end to end on the far-frame scenes
# ---------------------------------------------------------------------------------------------
def _moved_rays(rays, how, offset):
    """The base scene's rays where the far scene is: every length times 2^10, or the origins moved with the scene."""
    if how == "x 2^10":
        return rt.scaled_rays(rays, 2.0 ** 10)
    out = np.array(rays, np.float32)
    out[:, 0:3] += np.asarray(offset, np.float32)
    return out


@pytest.mark.parametrize("name,how,keeps_frame", [f for f in cases.FAR if f[0] == "tiny_rot"])
def test_far_frame_rays_equal_the_world_axes_and_the_brute_force(oracle, name, how, keeps_frame):
    """2 000 of the soups' random rays and up to 1 000 grazing ones aimed at the records that attain slot extremes (the judge names them: where a
    box that is too small loses a hit first): closest hit and terminate-on-first-hit on the tree in its frame, on the world-axes tree and by
    the oracle's brute force, bit for bit.  A ray has to graze a sliver of a millimetre to lose a hit to a box that is too small: the judge
    is the deterministic detector, this is what its verdict means for an answer."""
    base = cases.framed_scenes()[name]()
    c = _ctx(base)
    try:
        frame = c.bvh_arrays()["frame"]
        scene = cases.far_scene(name, how, frame)
        offset = scene.primitives["transform"][0, 12:15] - base.primitives["transform"][0, 12:15]
        c.upload_scene(scene)
        arrays, verdict = cases.judge_context(c, scene, f"{name} {how}")
        assert arrays["frame_on"] == keeps_frame
        rec = np.frombuffer(arrays["records"].tobytes(), tt.RECORD)[verdict.extreme_records]
        v0 = rec["v0"].astype(np.float64)
        tris = np.stack([v0, v0 + rec["e1"], v0 + rec["e2"]], 1)
        scale = 2.0 ** 10 if how == "x 2^10" else 1.0
        grazing = rt.grazing_rays((tris - (0 if how == "x 2^10" else offset.astype(np.float64))) / scale, np.random.default_rng(7), 1000)
        rays = _moved_rays(np.concatenate([rt.soup_rays(base, 1, n=2000), grazing]), how, offset)
        framed = (c.ray_query(rays), c.ray_query(rays, any_hit=True))
        assert c.ray_query_statistics()[3] == 0
        c.set_option("bvh_frame", 0)
        c.upload_scene(scene)
        assert not c.bvh_arrays()["frame_on"]
        world = (c.ray_query(rays), c.ray_query(rays, any_hit=True))
        for what, a, b in (("closest", framed[0], world[0]), ("any hit", framed[1], world[1])):
            differ = np.nonzero((np.ascontiguousarray(a).view(np.uint8).reshape(len(rays), -1) != np.ascontiguousarray(b).view(np.uint8).reshape(len(rays), -1)).any(1))[0]
            assert len(differ) == 0, f"{what}: {len(differ)} rays answer differently in the frame and on the world axes, first {differ[:5]}"
        (ohit, oflat, ot, ou, ov), oocc = rt.oracle_answers(oracle.Scene(scene), rays, use_bvh=False)
        hit, flat = rt.flat_of_hits(scene, framed[0])
        assert 0.05 < hit.mean() < 0.99 and np.array_equal(hit, ohit), f"{(hit != ohit).sum()} rays hit / miss unlike the brute force"
        assert np.array_equal(flat[hit], oflat[hit])
        for f, want in (("t", ot), ("u", ou), ("v", ov)):
            assert np.array_equal(np.ascontiguousarray(framed[0][f][hit]).view(np.uint32), np.ascontiguousarray(want[hit], np.float32).view(np.uint32)), f
        assert np.array_equal(np.asarray(framed[1]).astype(bool), oocc)
    finally:
        c.close()
