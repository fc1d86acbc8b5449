"""vhr_refit_geometry_partial on the device: context A takes the dirty path, context B the whole-tree refit, from the same update calls --
fingerprints, form checks, cost and counters equal, and equal to the host twin's; ray queries equal the oracle's; the device-memory route and
its NaN refusal; the half-precision fallback and return; hybrid frames bit-identical to a context that uploads the arrays in full."""
import numpy as np
import pytest

from tests import partial_refit_cases as cases
from tests.helpers import GpuHybrid
from tests.test_gpu_fuzz import soup
from tests.test_gpu_ray_query import _check, _oracle, _soup_rays
from tests.test_gpu_refit import HYBRID_IMAGES, _hybrid_images, _with
from vulkanhybridrenderer_amd import abi, camera, lib, scenes

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, GRAPH = -1, -5
DIRTY = 0


def _warm(scene, host_only=False, **options):
    c = lib.Context(64, 64, host_only=host_only)
    for k, v in options.items():
        c.set_option(k, v)
    c.update_geometry(scene.vertices, scene.indices, scene.primitives)
    c.update_vertices(scene.vertices)
    c.refit_geometry()
    return c


@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("builder", [1, 0])
def test_partial_refit_equals_the_whole_tree_refit_and_the_host_twin(oracle, builder, frame):
    """Updates 1, 3, 4 and 6 one after the other on the same three contexts: A (device, dirty path), B (device, whole tree) and, for the
    host-built tree, H (host-only, dirty path), whose arrays must hash like the device's."""
    scene = soup(3, 2000, 8)
    a, b = _warm(scene, bvh_builder=builder, bvh_frame=frame), _warm(scene, bvh_builder=builder, bvh_frame=frame)
    h = _warm(scene, host_only=True, bvh_frame=frame) if builder == 0 else None
    try:
        stats = a.bvh_statistics()
        whole_launches = a.refit_statistics()["upward_launches"]
        ups = cases.updates(scene)
        for i, name in enumerate(n for n in sorted(ups) if n[0] in "1346"):
            for c in (a, b, h):
                if c:
                    cases.apply(c, ups[name])
            a.refit_geometry_partial(force=True)
            b.refit_geometry()
            sa, sb = cases.state(a), cases.state(b)
            assert sa == sb, (name, sa, sb)
            assert sa["outside"] == (0, 0, 0) and sa["form_checks"][1:] == (0, 0, 0), (name, sa)
            ps, st = a.partial_refit_statistics(), a.refit_statistics()
            assert ps["ran_as"] == DIRTY and ps["partial_refits"] == i + 1, (name, ps)
            assert 0 < ps["dirty_records"] < stats["triangles"] and 0 < ps["dirty_nodes"] < stats["nodes"], (name, ps)
            assert (st["records"], st["nodes"]) == (ps["dirty_records"], ps["dirty_nodes"]) and 1 <= st["upward_launches"] <= whole_launches, (name, st)
            if len(ups[name]) == 1:
                assert ps["dirty_records"] == cases.expected_dirty_records(scene, ups[name][0]), (name, ps)
            forms = [c.bvh_forms_fingerprint() for c in (a, b)]
            assert forms[0] == forms[1] and forms[0][0] == forms[0][1], (name, forms)
            if h:
                h.refit_geometry_partial(force=True)
                assert h.bvh_forms_fingerprint() == forms[0], name
                hp = h.partial_refit_statistics()
                assert h.bvh_fingerprint() == sa["fingerprint"] and h.bvh_tree_fingerprint() == sa["tree"], name
                assert (hp["dirty_records"], hp["dirty_nodes"], hp["centre_moved"]) == (ps["dirty_records"], ps["dirty_nodes"], ps["centre_moved"]), (name, hp, ps)
    finally:
        for c in (a, b, h):
            if c:
                c.close()


def test_ray_queries_after_successive_partial_refits_equal_the_oracle(oracle):
    """Three partial refits without a rebuild, one primitive displaced further each time; 20 000 rays each, closest hit and any hit."""
    scene = soup(3, 2000, 8)
    first, end = cases.vertex_blocks(scene)[4]
    rng = np.random.default_rng(303)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
        for i, scale in enumerate((0.05, 0.4, 1.5)):
            v = scene.vertices.copy()
            v["pos"][first:end] += rng.normal(scale=scale, size=(end - first, 3)).astype(np.float32)
            sc = _with(scene, vertices=v)
            rays = _soup_rays(rng, sc, 20000)
            want, occ = _oracle(oracle.Scene(sc), rays, use_bvh=False)
            ctx.update_vertices(v[first:end], first_vertex=first)
            ctx.refit_geometry_partial(force=True)
            ps = ctx.partial_refit_statistics()
            assert ps["ran_as"] == DIRTY and ps["partial_refits"] == i + 1 and ps["dirty_records"] == (end - first) // 3, ps
            assert ctx.bvh_form_checks()[1:] == (0, 0, 0)
            _check(ctx, rays, want, occ, f"soup 3, partial refit {i + 1}")
    finally:
        ctx.close()


def test_the_device_memory_route_refuses_a_nan_and_recovers(oracle):
    import torch
    scene = soup(2, 400, 5)
    first, end = cases.vertex_blocks(scene)[2]
    moved = cases._moved(scene, first, end, np.random.default_rng(8))[2]
    bad = moved.copy()
    bad["pos"][3, 1] = np.nan
    a, b = _warm(scene), _warm(scene)
    try:
        L, hd = a.L, a.handle
        dev = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).cuda()
        a.update_vertices_device(dev.data_ptr(), len(bad), first_vertex=first)
        assert L.vhr_refit_geometry_partial(hd, lib.REFIT_FORCE_PARTIAL) == INVALID_ARGUMENT and "non-finite" in L.vhr_last_error(hd).decode()
        assert a.refit_statistics()["refits"] == 1 and a.partial_refit_statistics()["partial_refits"] == 0
        # updates stay pending: tracing calls refuse until a refit succeeds
        rays, out = np.zeros(4, abi.ray_dtype), np.zeros(4, abi.ray_hit_dtype)
        assert L.vhr_ray_query(hd, rays.ctypes.data, 4, abi.RAY_QUERY_HOST_MEMORY, out.ctypes.data) == GRAPH and "vhr_refit_geometry" in L.vhr_last_error(hd).decode()
        assert L.vhr_graph_execute(hd, 0, 0) == GRAPH
        good = torch.from_numpy(moved.view(np.uint8).reshape(-1).copy()).cuda()
        a.update_vertices_device(good.data_ptr(), len(moved), first_vertex=first)
        a.refit_geometry_partial(force=True)
        assert a.partial_refit_statistics()["ran_as"] == DIRTY and a.refit_statistics()["refits"] == 2
        assert L.vhr_ray_query(hd, rays.ctypes.data, 4, abi.RAY_QUERY_HOST_MEMORY, out.ctypes.data) == 0
        b.update_vertices(moved, first_vertex=first)
        b.refit_geometry()
        assert cases.state(a) == cases.state(b)
    finally:
        a.close()
        b.close()


def test_half_precision_nodes_fall_back_and_return(oracle):
    """tests/test_gpu_refit.py's input: x times 32768 puts the scene past the half range.  One primitive's block stretched that way is enough: A's
    half_nodes word and form checks equal B's after the partial refit, and again after the vertices return."""
    scene = soup(2, 400, 5)
    first, end = cases.vertex_blocks(scene)[3]
    wide = scene.vertices[first:end].copy()
    wide["pos"][:, 0] *= np.float32(32768.0)
    a, b = _warm(scene), _warm(scene)
    try:
        home = cases.state(a)
        assert home["half_nodes"] == 1
        for block in (wide, scene.vertices[first:end]):
            a.update_vertices(block, first_vertex=first)
            b.update_vertices(block, first_vertex=first)
            a.refit_geometry_partial(force=True)
            b.refit_geometry()
            ps = a.partial_refit_statistics()
            assert ps["ran_as"] == DIRTY and ps["centre_moved"] == 1, ps          # (the root's box changes both ways: all forms and form checks are redone;
            sa, sb = cases.state(a), cases.state(b)                             #  the restricted update is the next test's)
            assert sa == sb and sa["outside"] == (0, 0, 0), (sa, sb)
            assert sa["half_nodes"] == (0 if block is wide else 1), sa
        assert cases.state(a) == home
    finally:
        a.close()
        b.close()


def test_check_totals_follow_by_difference_while_the_scene_centre_stays(oracle):
    """The per-node status words and the new - old counter update with values other than 0.  tiny_scene's back wall spans x = -4 .. 4 about an
    identity transform, like the floor, so the root's x slots are symmetric and the scene centre's x is +0.  The wall's x times a power of two
    (exact) keeps them symmetric: the centre keeps its bits, the dirty pass stays restricted, and the wall's ancestors -- the root among them --
    leave the half range, so their nodes add to the form-check counters (old 0, new > 0).  A wider wall (old > 0, new > 0), another primitive
    moved meanwhile (the root again: old > 0, new > 0), the wall back (old > 0, new 0: the totals must return to exactly 0, or the walkers
    would stay off the half-precision nodes where context B is back on them), that primitive back.  After every step A's half_nodes word, form
    checks and arrays equal B's, which refits the whole tree."""
    scene = scenes.tiny_scene()
    blocks = cases.vertex_blocks(scene)
    wall, quad = blocks[1], blocks[4]

    def scaled(block, factor):
        v = scene.vertices[block[0]:block[1]].copy()
        v["pos"][:, 0] *= np.float32(factor)
        return v

    def shifted(block, dx):
        v = scene.vertices[block[0]:block[1]].copy()
        v["pos"][:, 0] += np.float32(dx)
        return v

    steps = [("wall x 32768", wall, scaled(wall, 32768.0), 0), ("wall x 65536", wall, scaled(wall, 65536.0), 0), ("quad moved", quad, shifted(quad, 0.1), 0),
             ("wall back", wall, scaled(wall, 1.0), 1), ("quad back", quad, shifted(quad, 0.0), 1)]
    a, b = _warm(scene, bvh_frame=0), _warm(scene, bvh_frame=0)
    try:
        home = cases.state(a)
        nodes = a.bvh_statistics()["nodes"]
        assert home["half_nodes"] == 1 and home["form_checks"][1:] == (0, 0, 0)
        for i, (what, block, v, half) in enumerate(steps):
            a.update_vertices(v, first_vertex=block[0])
            b.update_vertices(v, first_vertex=block[0])
            a.refit_geometry_partial(force=True)
            b.refit_geometry()
            ps = a.partial_refit_statistics()
            print(what, ps, a.refit_statistics(), a.bvh_form_checks())
            assert ps["ran_as"] == DIRTY and ps["centre_moved"] == 0 and ps["partial_refits"] == i + 1, (what, ps)
            assert 0 < ps["dirty_nodes"] == ps["forms_rewritten"] < nodes, (what, ps)
            sa, sb = cases.state(a), cases.state(b)
            assert sa == sb, (what, sa, sb)
            assert sa["half_nodes"] == half and sa["outside"] == (0, 0, 0), (what, sa)
        assert cases.state(a) == home
    finally:
        a.close()
        b.close()


def test_hybrid_frames_of_a_partially_refitted_context_equal_a_rebuilt_one(oracle):
    """Context A: one primitive's vertices updated per frame, then the partial refit.  Context B: a full upload of the same arrays.  Four dolly
    frames of the hybrid path at 240 x 136: every image the path publishes or keeps is bit-identical."""
    scene = scenes.sponza_proc(detail=0.3)
    W, H = 240, 136
    tp = abi.default_trace_params()
    blocks = cases.vertex_blocks(scene)
    rng = np.random.default_rng(17)
    a = GpuHybrid(scene, W, H, trace_params=tp, gbuffer="standin")
    b = GpuHybrid(scene, W, H, trace_params=tp, gbuffer="standin")
    try:
        v = scene.vertices.copy()
        for i, pfd in enumerate(camera.dolly_frames(scene, W, H, 4)):
            first, end = blocks[(3 * i + 1) % len(blocks)]
            v["pos"][first:end, 0] += (0.1 * np.sin(3.0 * v["pos"][first:end, 1] + 0.7 * i + rng.random())).astype(np.float32)
            a.ctx.update_vertices(v[first:end], first_vertex=first)
            a.ctx.refit_geometry_partial(force=True)
            ps = a.ctx.partial_refit_statistics()
            assert ps["ran_as"] == (1 if i == 0 else DIRTY), ps                  # (the first refit since the build is whole-tree)
            b.ctx.update_geometry(v, scene.indices, scene.primitives)
            a.frame(pfd)
            b.frame(pfd)
            for name, x, y in zip(HYBRID_IMAGES, _hybrid_images(a), _hybrid_images(b)):
                assert np.array_equal(x, y), f"frame {i}: {name} differs between the partially refitted and the rebuilt context"
        assert a.ctx.partial_refit_statistics()["partial_refits"] == 3
    finally:
        a.close()
        b.close()


def test_stage_times_and_launch_count(oracle):
    scene = soup(3, 2000, 8)
    ctx = _warm(scene)
    try:
        ctx.set_kernel_timing(False, refit=True)
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
        whole = ctx.refit_statistics()["upward_launches"]
        cases.apply(ctx, cases.updates(scene)["1 one primitive's block"])
        ctx.refit_geometry_partial(force=True)
        t = ctx.refit_times_ms()
        print("partial refit times (wall, leaf, upward, forms + checks) ms:", t)
        assert len(t) == 4 and all(np.isfinite(x) and x >= 0.0 for x in t) and t[0] > 0.0, t
        assert 1 <= ctx.refit_statistics()["upward_launches"] <= whole
    finally:
        ctx.close()
