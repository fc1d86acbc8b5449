"""vhr_rebuild_geometry on the device: the tree equals a fresh context's whichever builder makes it, queries and frames do not see the
rebuild, the object-motion records travel across the new tree's slot permutation (the gather / scatter kernels of csrc/kernels_bvh_refit.hip), and
a non-finite device-memory vertex is met by the check pass before anything is freed or built."""
import numpy as np
import pytest

from tests import object_motion_cases as omc
from tests import partial_refit_cases as cases
from tests import rebuild_cases as rc
from tests.helpers import GpuHybrid
from vulkanhybridrenderer_amd import camera, lib, ray_queries

pytestmark = pytest.mark.gpu
OK, INVALID_ARGUMENT, GRAPH = 0, -1, -5          # include/vhr_amd.h
KEY = "object_motion_vectors"
W, H = 96, 64


def _ctx(vertices, indices, primitives, **options):
    c = lib.Context(W, H)
    for k, v in options.items():
        c.set_option(k, v)
    c.update_geometry(vertices, indices, primitives)
    return c


def _scene_ctx(scene, **options):
    return _ctx(scene.vertices, scene.indices, scene.primitives, **options)


def _fresh_state(scene, vertices, primitives, **options):
    f = _ctx(vertices, scene.indices, primitives, **options)
    try:
        return rc.tree_state(f)
    finally:
        f.close()


def _apply_through_device_memory(c, calls):
    """The first vertex call through update_vertices_device from a torch tensor (no host copy of it exists), the others as host arrays."""
    import torch
    keep = []
    for i, (kind, first, data) in enumerate(calls):
        if kind == "v" and not keep:
            keep.append(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()).cuda())
            c.update_vertices_device(keep[0].data_ptr(), len(data), first_vertex=first)
        else:
            cases.apply(c, [(kind, first, data)])
    c.synchronize()                                           # the copy is on the context's stream: done before the tensor goes
    return keep


# ---- 1. the tree ----
BUILDERS = {"device": (dict(), 1, 0), "host": (dict(bvh_builder=0), 0, 1), "handed over": (dict(bvh_device_max_depth=8), 0, 1)}


@pytest.mark.parametrize("refitted", [False, True], ids=["pending", "refitted"])
@pytest.mark.parametrize("kind", rc.UPDATE_KINDS)
@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_rebuild_equals_a_fresh_build(vhr, builder, kind, refitted):
    options, used, fetched = BUILDERS[builder]
    scene = rc.make_soup("soup5")
    calls = rc.update_calls(scene, kind)
    vertices, primitives = rc.updated_arrays(scene, calls)
    want = _fresh_state(scene, vertices, primitives, **options)
    assert want["builder"] == used
    c = _scene_ctx(scene, **options)
    try:
        _apply_through_device_memory(c, calls)
        if refitted:
            c.refit_geometry()
        c.rebuild_geometry()
        assert rc.tree_state(c) == want
        rc.assert_reads_as_after_a_build(c, (builder, kind, refitted))
        assert c.rebuild_statistics() == (1, fetched, 0, 0, 0, 0, 0, 0)
        build_ms, transfer_ms = c.build_times_ms()
        assert build_ms > 0 and (transfer_ms > 0) == bool(fetched)
    finally:
        c.close()


@pytest.mark.parametrize("leaf,frame", [(1, 0), (4, 1), (2, 0)])
def test_rebuild_equals_a_fresh_build_on_a_rotated_soup(vhr, leaf, frame):
    scene = rc.make_soup("soup3", rotated=True)
    calls = rc.update_calls(scene, "both")
    vertices, primitives = rc.updated_arrays(scene, calls)
    options = dict(bvh_leaf_triangles=leaf, bvh_frame=frame, bvh_host_checks=1)
    want = _fresh_state(scene, vertices, primitives, **options)
    c = _scene_ctx(scene, bvh_leaf_triangles=2, bvh_frame=1 - frame, bvh_host_checks=1)          # built with other options: the rebuild reads the current ones
    try:
        for k, v in options.items():
            c.set_option(k, v)
        cases.apply(c, calls)
        c.rebuild_geometry()
        assert rc.tree_state(c) == want and c.rebuild_statistics()[:2] == (1, 0)
    finally:
        c.close()


# ---- 2. queries ----
def _queries(c, rays, points, masked):
    out = dict(closest=c.ray_query(rays), any=c.ray_query(rays, any_hit=True), points=c.closest_point_query(points),
               within=c.closest_point_query(points, any_within=True))
    if masked:
        out.update(closest_masked=c.ray_query(rays, cull_mask=0x0F), any_masked=c.ray_query(rays, any_hit=True, cull_mask=0x0F),
                   points_masked=c.closest_point_query(points, cull_mask=0x0F))
    return out


def _same_answers(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), f"{what}: {k}"


def _rays_and_points(scene):
    lo, hi = ray_queries.scene_bounds(scene)
    rng = np.random.default_rng(41)
    rays = ray_queries.random_rays(rng, 4096, lo, hi, margin=0.2, tmins=(0.0, 2.0 ** -7), tmaxs=(np.inf, 4.0, 16.0))
    points = np.empty((1024, 4), np.float32)
    points[:, :3] = rng.uniform(lo - 0.5, hi + 0.5, (1024, 3))
    points[:, 3] = rng.choice(np.array([0.25, 1.0, np.inf], np.float32), 1024)
    return rays, points


def test_queries_do_not_see_the_rebuild(vhr):
    scene = rc.make_soup("soup3")
    calls = rc.update_calls(scene, "both")
    vertices, primitives = rc.updated_arrays(scene, calls)
    rays, points = _rays_and_points(scene)
    masks = np.full(len(scene.primitives), 0xFF, np.uint8)
    masks[0], masks[2], masks[5] = 0xF0, 0x30, 0x01          # against the cull mask 0x0F: the floor and primitive 2 do not exist
    rebuilt, refitted, fresh = _scene_ctx(scene), _scene_ctx(scene), _ctx(vertices, scene.indices, primitives)
    try:
        for c in (rebuilt, refitted, fresh):
            c.set_primitive_masks(masks)
        cases.apply(rebuilt, calls)
        rebuilt.rebuild_geometry()
        cases.apply(refitted, calls)
        refitted.refit_geometry()
        assert np.array_equal(rebuilt.primitive_masks(), masks) and rebuilt.ray_mask_statistics()[0] == fresh.ray_mask_statistics()[0] == 3
        want = _queries(fresh, rays, points, True)
        assert not np.array_equal(want["closest"].view(np.uint8), want["closest_masked"].view(np.uint8)), "the cull mask was to act"
        _same_answers(_queries(rebuilt, rays, points, True), want, "rebuilt against fresh")
        _same_answers(_queries(refitted, rays, points, True), want, "refitted against fresh")
    finally:
        for c in (rebuilt, refitted, fresh):
            c.close()


def test_a_presplit_tree_with_object_motion_on(vhr):
    scene = rc.presplit_scene()
    rays, points = _rays_and_points(scene)
    options = dict(bvh_presplit=100, bvh_frame=0)
    c, fresh = _scene_ctx(scene, **options, **{KEY: 1}), _scene_ctx(scene, **options)
    try:
        assert c.bvh_presplit_level() >= 0 and c.object_motion_statistics()["active"] == 1
        c.rebuild_geometry()                                  # nothing pending; several records per triangle, each takes its flat triangle's record
        assert c.rebuild_statistics() == (1, 0, 0, 0, 0, 0, 0, 0) and c.object_motion_statistics()["differing_records"] == 0
        assert rc.tree_state(c) == rc.tree_state(fresh)
        _same_answers(_queries(c, rays, points, False), _queries(fresh, rays, points, False), "a rebuilt presplit tree against a fresh one")
        c.set_option("bvh_presplit", 0)                       # ... and out of it, to a tree a refit can keep
        c.rebuild_geometry()
        assert c.bvh_presplit_level() == -1
        omc.assert_settled(c, "from a presplit tree to a plain one")
        _same_answers(_queries(c, rays, points, False), _queries(fresh, rays, points, False), "rebuilt without presplit against the fresh presplit tree")
    finally:
        c.close()
        fresh.close()


# ---- 3. frames ----
IMAGES = ("NORMALS", "MOTION", "DEPTH", "RAYTRACED", "REFLECTIONS", "DENOISED")


def _three_frames(scene, calls, how, option):
    """Three frames of the hybrid path (shadows, AO, reflections, SVGF) behind the stand-in G-buffer; `calls` then how(ctx) before frame 2."""
    g = GpuHybrid(scene, W, H, gbuffer="standin")
    try:
        g.ctx.set_option(KEY, option)
        out = []
        for i, pfd in enumerate(camera.dolly_frames(scene, W, H, 3)):
            if i == 1:
                cases.apply(g.ctx, calls)
                how(g.ctx)
            elif option:
                g.ctx.refit_geometry()                        # "object_motion_vectors": one refit call per frame
            g.frame(pfd)
            out.append({name: g.ctx.download(getattr(lib, name)) for name in IMAGES})
        return out, g.ctx.object_motion_statistics()
    finally:
        g.close()


@pytest.mark.parametrize("option", [0, 1])
def test_frames_after_a_rebuild_are_the_frames_after_a_refit(vhr, option):
    """The SVGF history and the other frame state survive the rebuild: frames 2 and 3 of update + rebuild are update + refit's, bit for bit.
    With "object_motion_vectors" 1 that includes the stand-in G-buffer's motion image, which reads the carried previous records."""
    scene = rc.make_soup("soup3")
    calls = rc.update_calls(scene, "both")
    a, st_a = _three_frames(scene, calls, lambda c: c.refit_geometry(), option)
    b, st_b = _three_frames(scene, calls, lambda c: c.rebuild_geometry(), option)
    for i in (1, 2):
        for name in IMAGES:
            assert np.array_equal(a[i][name].view(np.uint8), b[i][name].view(np.uint8)), f"frame {i + 1}: {name}"
    assert not np.array_equal(a[0]["DEPTH"].view(np.uint8), a[1]["DEPTH"].view(np.uint8))
    assert st_a == st_b
    if option:
        assert st_b["motion_launches"] > 0, "the moved records were to reach the G-buffer's motion instantiation"


# ---- 4. object motion ----
def test_object_motion_is_carried_across_the_slot_permutation(vhr):
    scene = rc.make_soup("soup3")
    vertices, primitives = scene.vertices.copy(), scene.primitives.copy()

    def fresh_records():
        f = _ctx(vertices, scene.indices, primitives)
        try:
            return f.triangle_records()
        finally:
            f.close()

    def rebuild_and_check(c, calls, what):
        r0 = c.triangle_records()
        _apply_through_device_memory(c, calls)
        omc.apply_to_arrays(vertices, primitives, calls)
        c.rebuild_geometry()
        want = fresh_records()
        cur, prev = c.triangle_records(), c.triangle_records(previous=True)
        assert omc.same(prev, r0), f"{what}: the previous records are not the records before the rebuild"
        assert omc.same(cur, want), f"{what}: the current records are not a fresh build's"
        differing = int(omc.differing_rows(r0, want).sum())
        assert c.object_motion_statistics()["differing_records"] == differing == c.rebuild_statistics()[3], what
        return differing
    c = _scene_ctx(scene, **{KEY: 1})
    try:
        moved = rebuild_and_check(c, rc.moved_subset(scene), "a known subset moves")
        assert 0 < moved < len(c.triangle_records())
        c.refit_geometry()
        omc.assert_settled(c, "a refit with nothing pending after a rebuild")
        c.update_vertices(vertices)
        c.refit_geometry()                                    # (the first refit since a build is whole-tree)
        cases.apply(c, rc.update_calls(scene, "vertices"))
        omc.apply_to_arrays(vertices, primitives, rc.update_calls(scene, "vertices"))
        c.refit_geometry_partial(force=True)
        assert c.partial_refit_statistics()["ran_as"] == 0 and c.object_motion_statistics()["differing_records"] > 0
        rebuild_and_check(c, rc.update_calls(scene, "transforms"), "after a partial refit")
        r0 = c.triangle_records()
        c.rebuild_geometry()
        omc.assert_settled(c, "a rebuild with nothing pending")
        assert omc.same(c.triangle_records(), r0) and c.rebuild_statistics()[3] == 0
    finally:
        c.close()


# ---- 5. non-finite input ----
def test_a_non_finite_vertex_is_met_before_anything_is_freed_or_built(vhr):
    """One NaN through the device-memory route.  The check pass only reads; the builder is never reached with the NaN."""
    import torch
    scene = rc.make_soup("soup3")
    first = cases.vertex_blocks(scene)[3][0] + 7
    good = scene.vertices[first:first + 1].copy()
    good["pos"][0] += np.float32(0.25)
    bad = good.copy()
    bad["pos"][0, 2] = np.nan
    vertices = scene.vertices.copy()
    vertices[first:first + 1] = good
    g = GpuHybrid(scene, W, H, gbuffer="standin", geometry_options={KEY: 1})
    c = g.ctx
    try:
        pfds = camera.dolly_frames(scene, W, H, 2)
        g.frame(pfds[0])
        before = (c.bvh_forms_fingerprint(), c.bvh_statistics(), c.triangle_records().copy(), c.triangle_records(previous=True).copy())
        dev = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).cuda()
        c.update_vertices_device(dev.data_ptr(), 1, first_vertex=first)
        assert c.L.vhr_rebuild_geometry(c.handle, 0) == INVALID_ARGUMENT
        err = c.L.vhr_last_error(c.handle).decode()
        assert "vhr_rebuild_geometry" in err and "non-finite" in err
        st = c.rebuild_statistics()
        assert st[0] == 0 and st[2] >= 1
        assert c.L.vhr_graph_execute(c.handle, 0, 0) == GRAPH and "pending" in c.L.vhr_last_error(c.handle).decode()
        after = (c.bvh_forms_fingerprint(), c.bvh_statistics(), c.triangle_records(), c.triangle_records(previous=True))
        assert after[:2] == before[:2] and omc.same(after[2], before[2]) and omc.same(after[3], before[3]), "the old tree was to stay untouched"
        dev2 = torch.from_numpy(good.view(np.uint8).reshape(-1).copy()).cuda()
        c.update_vertices_device(dev2.data_ptr(), 1, first_vertex=first)
        c.rebuild_geometry()
        assert c.rebuild_statistics()[:3] == (1, 0, 0)
        want = _fresh_state(scene, vertices, scene.primitives)
        assert rc.tree_state(c) == want
        assert omc.same(c.triangle_records(previous=True), before[2]) and c.rebuild_statistics()[3] == c.object_motion_statistics()["differing_records"] > 0
        g.frame(pfds[1])                                      # and it traces again
    finally:
        g.close()


# ---- 6. from inside a pass ----
def test_refused_from_inside_a_pass(vhr):
    scene = rc.make_soup("soup3")
    seen = {}

    class InPass(GpuHybrid):
        def _gbuffer_pass(self, ctx):
            if not seen:
                seen["rc"] = ctx.L.vhr_rebuild_geometry(ctx.handle, 0)
                seen["msg"] = ctx.L.vhr_last_error(ctx.handle).decode()
            super()._gbuffer_pass(ctx)
    g = InPass(scene, W, H, gbuffer="standin")
    try:
        state = rc.tree_state(g.ctx)
        pfds = camera.dolly_frames(scene, W, H, 2)
        try:
            g.frame(pfds[0])
        except lib.VhrError as e:                             # (the refusal's message is the context's last error when the graph returns)
            assert "vhr_rebuild_geometry" in str(e)
        assert seen["rc"] == GRAPH and "vhr_rebuild_geometry" in seen["msg"] and "inside a pass" in seen["msg"], seen
        g.ctx.synchronize()
        assert g.ctx.rebuild_statistics() == (0,) * 8 and rc.tree_state(g.ctx) == state
        g.ctx.rebuild_geometry()                              # outside a pass again: the call works
        assert g.ctx.rebuild_statistics()[0] == 1 and rc.tree_state(g.ctx) == state
        g.frame(pfds[1])
    finally:
        g.close()
