"""WHICH triangle the closest-hit kernels commit, judged against exact arithmetic (tests/ray_truth.py judge_closest_triangle) at three
units of length and on the 1000-fold mix: the mirror ray (reflection_kernel / reflection_queue_kernel, with the pixels the queue kernel
marks and computes again), the stand-in G-buffer's primary ray (gbuffer_kernel) and the raytraced path's (raytraced_kernel /
raytraced_queue_kernel).  The scenes have one primitive per triangle and a colour that spells the primitive's index
(tests/probe_scenes.py), so each kernel's ordinary image names the triangle it committed -- duplicates included: every 15th triangle of
a soup repeats its predecessor, and "min t, then the smaller flat index" is judged with no excuse.

The device's ray is taken to be the one the oracle logged for the pixel: for the mirror ray the device traces from the oracle's G-buffer
(read back and compared bit for bit); a primary ray is a function of the PerFrameData alone.  Where a verdict finds a violation the
logged rays of the offending pixels go to vhr_ray_query on the same context, and the message says whether the query agrees with the
truth (then the kernel's ray set-up differs and its walk is not at fault) or not.

The raytraced path is judged at 2^-4, not 2^-10: raygen.rgen:20 hard-codes tmin = 0.1, and 0.1 m lies behind a 6 mm scene."""
import numpy as np
import pytest

from tests import probe_scenes as ps
from tests import ray_truth as rt
from tests.helpers import GpuHybrid
from tests.test_gpu_ray_truth import TREE_DEFAULTS, TREES
from vulkanhybridrenderer_amd import lib

pytestmark = pytest.mark.gpu
W, H = ps.W, ps.H
HYBRID_CASES = [(name, scale) for name in ps.NAMES for scale in rt.SCALES] + [("tiny_far", 1.0)]
RAYTRACED_CASES = [(name, scale) for name in ps.NAMES for scale in ps.RAYTRACED_SCALES]


def _judge(oracle, case, ctx, probe, hit, flat, what, again=None):
    """Zero violations, the tie clause included; the counts go to the log."""
    v = rt.judge_closest_triangle(probe.truth, hit, flat)
    print(f"{what}: {v.violations} violations of {len(probe.rays)} rays; hit share {hit.mean():.3f}, explained as class D {v.explained_d}, true hits passed over "
          f"(explained) {v.explained_lost}, ties checked {v.ties}" + (f", pixels computed again {again}" if again is not None else ""))
    if v.violations:
        bad = np.nonzero(v.bad)[0]
        qhit, qflat = rt.flat_of_hits(case["scene"], ctx.ray_query(probe.rays[bad]))
        sub = rt.Truth(oracle, case["osc"], probe.rays[bad])
        q = rt.judge_closest_triangle(sub, qhit, qflat)
        where = ("vhr_ray_query answers the logged rays in keeping with the truth: the kernel's ray differs from the logged one, its walk is not at fault"
                 if q.violations == 0 else f"vhr_ray_query on the logged rays carries {q.violations} violations too: the walk is at fault")
        raise AssertionError(f"{what}: {v.describe()}; first pixels {probe.pix[bad][:4].tolist()}, answered {flat[bad][:4].tolist()} "
                             f"(hit {hit[bad][:4].tolist()}), the oracle {probe.flat[bad][:4].tolist()}.  {where}")
    return v


@pytest.mark.parametrize("name,scale", HYBRID_CASES)
def test_the_mirror_ray_commits_the_right_triangle(oracle, name, scale):
    """Frame B of tests/test_gpu_ray_truth.py::test_the_hybrid_paths_walkers (no shadow, no AO, the mirror ray) with the light's intensity 0:
    reflection_hit.rchit leaves albedo * 0.2 / pi, which decodes to the triangle.  Every combination of reflection_variant (the queue kernel
    with its deferred decision and redo_pixel_reflection; the per-pixel kernel), compact_nodes and bvh_builder."""
    c = ps.hybrid_case(oracle, name, scale)
    scene, pfd, gbuf, p = c["scene"], c["pfd"], c["gbuf"], c["mirror"]
    n = len(scene.primitives)
    g = GpuHybrid(scene, W, H, denoise=False, trace_params=c["tp"])
    try:
        g.ctx.set_ray_statistics(True)
        for builder in (1, 0):
            g.ctx.set_option("bvh_builder", builder)
            g.ctx.upload_scene(scene)
            assert g.ctx.bvh_builder_used() == builder and g.ctx.bvh_form_checks()[1:] == (0, 0, 0)
            for compact in (1, 0):
                g.ctx.set_option("compact_nodes", compact)
                for variant in (1, 0):
                    g.ctx.set_option("reflection_variant", variant)
                    g.frame(pfd, gbuf)
                    for image, want in ((lib.NORMALS, gbuf[0]), (lib.DEPTH, gbuf[2])):
                        assert np.array_equal(g.ctx.download(image).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), "the device's G-buffer is not the oracle's"
                    assert g.ctx.ray_statistics()["stack_overflows"] == 0
                    again = g.ctx.binary64_statistics()["mirror_pixels_again"]
                    texels = np.asarray(g.ctx.download(lib.REFLECTIONS)).view(np.uint16).reshape(W * H, 4)
                    uncovered = np.setdiff1d(np.arange(W * H), p.pix)
                    assert not texels[uncovered].any()                                  # raygen.rgen:20-24
                    hit, flat = ps.decode_mirror(texels[p.pix], n)
                    what = f"{name} x {scale}, mirror ray, reflection_variant {variant}, compact_nodes {compact}, bvh_builder {builder}"
                    _judge(oracle, c, g.ctx, p, hit, flat, what, again)
                    assert hit.mean() >= 0.5, what
                    if variant == 1 and name == "soup 3" and scale == 2.0 ** 10:
                        assert again > 0, f"{what}: no pixel was marked and computed again -- redo_pixel_reflection was not judged"
    finally:
        g.close()


@pytest.mark.parametrize("name,scale", HYBRID_CASES)
def test_the_standin_gbuffer_commits_the_right_triangle(oracle, name, scale):
    """gbuffer_kernel's primary ray on the four trees: NORMALS.w is the primitive, DEPTH != 0 the coverage."""
    c = ps.hybrid_case(oracle, name, scale)
    scene, pfd, p = c["scene"], c["pfd"], c["primary"]
    g = GpuHybrid(scene, W, H, denoise=False, gbuffer="standin")
    try:
        for tree, options in TREES:
            for k, v in options.items():
                g.ctx.set_option(k, v)
            g.ctx.upload_scene(scene)
            g.frame(pfd)
            normals = np.asarray(g.ctx.download(lib.NORMALS)).view(np.uint16).reshape(W * H, 4)
            depth = np.asarray(g.ctx.download(lib.DEPTH)).reshape(W * H)
            hit, flat = ps.decode_ids(normals[p.pix], depth[p.pix] != 0, len(scene.primitives))
            _judge(oracle, c, g.ctx, p, hit, flat, f"{name} x {scale}, stand-in G-buffer, {tree}")
            assert hit.mean() >= 0.8
            for k in options:
                g.ctx.set_option(k, TREE_DEFAULTS[k])
    finally:
        g.close()


@pytest.mark.parametrize("name,scale", RAYTRACED_CASES)
def test_the_raytraced_path_commits_the_right_triangle(oracle, name, scale):
    """raytraced_kernel (raytraced_variant 0) and raytraced_queue_kernel (1), which decides a candidate that contradicts itself inline, on the
    device-built and the host-built tree, with the light's colour 0: closesthit.rchit leaves albedo / pi.  The miss colour is miss.rmiss's."""
    c = ps.raytraced_case(oracle, name, scale)
    scene, pfd, p = c["scene"], c["pfd"], c["primary"]
    ctx = lib.Context(W, H)
    path = None
    try:
        ctx.upload_scene(scene)
        ctx.set_ray_statistics(True)
        path = lib.RaytracedRenderPath(ctx, use_anyhit_shader=False)
        path.build()
        for builder in (1, 0):
            ctx.set_option("bvh_builder", builder)
            ctx.upload_scene(scene)
            assert ctx.bvh_builder_used() == builder
            for variant in (1, 0):
                ctx.set_option("raytraced_variant", variant)
                ctx.update_per_frame_ubo(0, pfd)
                ctx.execute(0, 0)
                ctx.synchronize()
                assert ctx.ray_statistics()["stack_overflows"] == 0
                image = np.asarray(ctx.download(lib.RAYTRACED_OUTPUT)).reshape(W * H, 4)
                hit, flat = ps.decode_raytraced(image[p.pix], len(scene.primitives))
                _judge(oracle, c, ctx, p, hit, flat, f"{name} x {scale}, raytraced path, raytraced_variant {variant}, bvh_builder {builder}")
                assert hit.sum() >= 0.9 * W * H
    finally:
        if path is not None:
            path.destroy()
        ctx.close()
