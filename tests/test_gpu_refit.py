"""vhr_refit_geometry on the device: a refitted tree answers ray queries like the oracle's scene built from the moved arrays, bit for bit,
and publishes the frames a rebuild publishes; rigid motion through the primitive transforms (the G-buffer stand-in's normals follow); the
half-precision nodes' fallback and return; pending updates refuse every tracing call; the device-memory route; no side effects on frames."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import GpuHybrid
from tests.test_gpu_fuzz import soup
from tests.test_gpu_ray_query import _check, _oracle, _soup_rays
from vulkanhybridrenderer_amd import abi, camera, lib, scenes

pytestmark = pytest.mark.gpu
GRAPH, UNSUPPORTED = -5, -7


def _with(scene, vertices=None, primitives=None):
    return scenes.Scene(scene.name, scene.vertices if vertices is None else vertices, scene.indices, scene.primitives if primitives is None else primitives,
                        scene.textures, scene.camera, scene.light)


def _displaced(scene, rng, scale):
    v = scene.vertices.copy()
    v["pos"] += rng.normal(scale=scale, size=v["pos"].shape).astype(np.float32)
    return v


def _clean(ctx):
    st = ctx.refit_statistics()
    assert (st["records_outside"], st["children_outside"], st["non_finite"]) == (0, 0, 0), st
    assert ctx.bvh_form_checks()[1:] == (0, 0, 0), ctx.bvh_form_checks()
    return st


@pytest.mark.parametrize("seed,n_tris,n_prims", [(1, 60, 3), (2, 400, 5), (3, 2000, 8), (4, 9000, 12)])
def test_ray_queries_after_successive_refits_equal_the_oracle(oracle, seed, n_tris, n_prims):
    """Three refits without a rebuild in between, each further from the geometry the tree was built for; 20 000 rays each, closest hit and any
    hit, on the device-built tree, the host-built tree, boxes along the world axes, and with 2 LDS stack levels."""
    scene = soup(seed, n_tris, n_prims)
    rng = np.random.default_rng(300 + seed)
    moved = []
    for scale in (0.05, 0.4, 1.5):
        sc = _with(scene, vertices=_displaced(scene, rng, scale))
        rays = _soup_rays(rng, sc, 20000)
        osc = oracle.Scene(sc)
        want, occ = _oracle(osc, rays, use_bvh=osc.triangle_count > 2000)
        moved.append((sc, rays, want, occ))
    ctx = lib.Context(64, 64)
    try:
        for what, options in (("device-built tree", {}), ("host-built tree", {"bvh_builder": 0}), ("world axes", {"bvh_frame": 0}), ("2 LDS levels", {"lds_stack_levels": 2})):
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.upload_scene(scene)
            stats = ctx.bvh_statistics()
            for i, (sc, rays, want, occ) in enumerate(moved):
                ctx.update_vertices(sc.vertices)
                ctx.refit_geometry()
                st = _clean(ctx)
                assert st["refits"] == i + 1 and st["records"] == stats["triangles"] and st["nodes"] == stats["nodes"] and ctx.bvh_statistics() == stats
                _check(ctx, rays, want, occ, f"soup {seed}, {what}, refit {i + 1}")
            cost = ctx.bvh_sah_cost()
            assert np.isfinite(cost[1]) and cost[1] > 0 and cost[0] > 0
            for k in options:
                ctx.set_option(k, {"bvh_builder": 1, "bvh_frame": 1, "lds_stack_levels": 8}[k])
    finally:
        ctx.close()


def test_identity_refit_keeps_the_device_tree_bit_for_bit(oracle):
    """The device kernels against the device builder: the same vertices again give the same arrays (both fingerprints), on both builders' trees."""
    scene = soup(3, 2000, 8)
    ctx = lib.Context(64, 64)
    try:
        for builder in (1, 0):
            ctx.set_option("bvh_builder", builder)
            ctx.upload_scene(scene)
            built = (ctx.bvh_fingerprint(), ctx.bvh_tree_fingerprint(), ctx.bvh_form_checks())
            forms = ctx.bvh_forms_fingerprint()
            ctx.update_vertices(scene.vertices)
            ctx.refit_geometry()
            _clean(ctx)
            assert (ctx.bvh_fingerprint(), ctx.bvh_tree_fingerprint(), ctx.bvh_form_checks()) == built, builder
            assert ctx.bvh_forms_fingerprint() == forms and forms[0] == forms[1], (builder, forms)
            cost = ctx.bvh_sah_cost()
            assert cost[0] == cost[1] > 0
    finally:
        ctx.close()


HYBRID_IMAGES = ("raytraced", "reflections", "denoised", "integrated 0", "integrated 1", "previous normals", "history", "moments history")


def _hybrid_images(g):
    """Every image the hybrid path publishes or keeps: the Raytraced output, the reflections, the denoised output and the five storage images
    of the SVGF pass (both integration buffers, last frame's normals, the history and the moments history)."""
    pc = g.path.push_constants()
    ids = [int(pc["integrated_shadow_and_ao"][0]), int(pc["integrated_shadow_and_ao"][1]), int(pc["prev_frame_normals_and_object_ids"]),
           int(pc["shadow_and_ao_history"]), int(pc["shadow_and_ao_moments_history"])]
    return [g.ctx.download(k) for k in (lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED)] + [g.ctx.download(i) for i in ids]


def _wave(scene, phase, amplitude=0.15):
    """Every vertex above 1 m pushed along x by a travelling wave in (y, z): normals left as they are."""
    v = scene.vertices.copy()
    p = v["pos"]
    up = p[:, 1] > 1.0
    p[up, 0] += (amplitude * np.sin(3.0 * p[up, 1] + 2.0 * p[up, 2] + phase)).astype(np.float32)
    return v


def test_frames_of_a_refitted_context_equal_a_rebuilt_one(oracle):
    """Context A: update_vertices + refit per frame.  Context B: a full upload of the same arrays per frame.  Eight frames of the hybrid path
    (stand-in G-buffer, which reads the moved vertices too) over the dolly: every image of every frame is bit-identical, the SVGF history and
    moments included.  Frame 0's visibility image of A also equals the oracle's for the moved scene (traced from A's own G-buffer)."""
    scene = scenes.sponza_proc(detail=0.3)
    W, H = 480, 270
    tp = abi.default_trace_params()
    a = GpuHybrid(scene, W, H, trace_params=tp, gbuffer="standin")
    b = GpuHybrid(scene, W, H, trace_params=tp, gbuffer="standin")
    try:
        for i, pfd in enumerate(camera.dolly_frames(scene, W, H, 8)):
            v = _wave(scene, 0.7 * i)
            a.ctx.update_vertices(v)
            a.ctx.refit_geometry()
            _clean(a.ctx)
            b.ctx.update_geometry(v, scene.indices, scene.primitives)
            a.frame(pfd)
            b.frame(pfd)
            for name, x, y in zip(HYBRID_IMAGES, _hybrid_images(a), _hybrid_images(b)):
                assert np.array_equal(x, y), f"frame {i}: {name} differs between the refitted and the rebuilt context"
            if i == 0:
                osc = oracle.Scene(_with(scene, vertices=v))
                want = osc.raygen(pfd, tp, a.ctx.download(lib.NORMALS), a.ctx.download(lib.DEPTH))[0]
                assert np.array_equal(a.ctx.download(lib.RAYTRACED), want), "frame 0: visibility differs from the oracle's for the moved scene"
            for img in (lib.NORMALS, lib.DEPTH):
                assert np.array_equal(a.ctx.download(img), b.ctx.download(img)), f"frame {i}: {img}"
        assert a.ctx.refit_statistics()["refits"] == 8
    finally:
        a.close()
        b.close()


class _OtherPath:
    """One of the three other render paths on a context, its stand-ins as pass bodies; images(): what it publishes."""

    def __init__(self, kind, scene, W, H):
        self.ctx = ctx = lib.Context(W, H)
        ctx.upload_scene(scene)
        self.present = present = ctx.upload_new_storage_image(W, H, abi.FORMAT_B8G8R8A8_SRGB)
        if kind == "raytraced":
            self.path = lib.RaytracedRenderPath(ctx, use_anyhit_shader=False, composition_pass=lambda c: c.standin_raytraced_composition(present))
            self.names = (lib.RAYTRACED_OUTPUT, present)
        elif kind == "rayquery":
            self.path = lib.RayqueryRenderPath(ctx, forward_pass=lambda c: c.standin_rayquery_forward(present, 0))
            self.names = (lib.DEPTH, present)
        else:
            self.path = lib.ForwardRasterRenderPath(ctx, depth_prepass=lambda c: c.standin_shadow_map(0, "ShadowMap"),
                                                    forward_pass=lambda c: c.standin_forward_raster(present, 0, msaa="Forward Pass_MSAA"), enable_msaa=1)
            self.names = (lib.DEPTH, "ShadowMap", "Forward Pass_MSAA", present)
        self.path.build()

    def images(self, pfd):
        self.ctx.update_per_frame_ubo(0, pfd)
        self.ctx.execute(0, 0)
        self.ctx.synchronize()
        return [self.ctx.download(n) for n in self.names]

    def close(self):
        self.path.destroy()
        self.ctx.close()


@pytest.mark.parametrize("kind", ["raytraced", "rayquery", "forward_raster"])
def test_the_other_paths_after_a_refit_equal_a_rebuild(oracle, kind):
    """The raytraced, the rayquery and the forward raster path, two frames each: A refits, B rebuilds from the same arrays; every image equal."""
    scene = scenes.sponza_proc(detail=0.3)
    W, H = 480, 270
    a, b = _OtherPath(kind, scene, W, H), _OtherPath(kind, scene, W, H)
    try:
        for i, pfd in enumerate(camera.dolly_frames(scene, W, H, 2)):
            v = _wave(scene, 0.9 * i + 0.4)
            a.ctx.update_vertices(v)
            a.ctx.refit_geometry()
            _clean(a.ctx)
            b.ctx.update_geometry(v, scene.indices, scene.primitives)
            for name, x, y in zip(a.names, a.images(pfd), b.images(pfd)):
                assert np.array_equal(x, y), f"{kind}, frame {i}: {name} differs between the refitted and the rebuilt context"
    finally:
        a.close()
        b.close()


def test_rigid_motion_through_the_primitive_transforms(oracle):
    """A third of the primitives rotated and translated: ray queries equal the oracle's scene with those transforms, and the G-buffer stand-in's
    normals equal a fresh upload's bit for bit (the normal matrices followed)."""
    scene = scenes.tiny_scene()
    prims = scene.primitives.copy()
    t = np.ascontiguousarray(prims["transform"], np.float32).reshape(-1, 16)
    for p in range(0, len(t), 3):
        t[p] = abi.mat_to_glm(abi.glm_to_mat(t[p]) @ scenes.trs((0.3, 0.2 + 0.1 * p, -0.4), rot_y=0.9, rot_x=0.35))
    prims["transform"] = t.reshape(prims["transform"].shape)
    moved = _with(scene, primitives=prims)
    rng = np.random.default_rng(5)
    rays = _soup_rays(rng, moved, 20000)
    want, occ = _oracle(oracle.Scene(moved), rays, use_bvh=False)
    W, H = 96, 64
    pfd = camera.dolly_frames(scene, W, H, 1)[0]
    a = GpuHybrid(scene, W, H, gbuffer="standin")
    b = GpuHybrid(moved, W, H, gbuffer="standin")
    try:
        for p in range(0, len(t), 3):
            a.ctx.update_primitive_transforms(t[p:p + 1], first_primitive=p)
        a.ctx.refit_geometry()
        _clean(a.ctx)
        _check(a.ctx, rays, want, occ, "tiny_scene, moved primitives")
        a.frame(pfd)
        b.frame(pfd)
        for img in (lib.NORMALS, lib.MOTION, lib.DEPTH, lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED):
            assert np.array_equal(a.ctx.download(img), b.ctx.download(img)), img
    finally:
        a.close()
        b.close()


def test_half_precision_nodes_fall_back_and_return(oracle):
    """A refit that stretches the scene past the half range leaves the 32-byte nodes unusable: the statistics say so, no violation is counted,
    ray queries still equal the oracle.  A refit back to the original vertices makes them valid again, with the build's arrays, and the next
    frame equals the frame of a context that never refitted, bit for bit (the scene centre and the walkers' node form are back too)."""
    scene = soup(2, 400, 5)
    wide = scene.vertices.copy()
    wide["pos"][:, 0] *= np.float32(32768.0)              # +-3 m -> +-98 304 > 65 504
    wsc = _with(scene, vertices=wide)
    rng = np.random.default_rng(9)
    rays = _soup_rays(rng, wsc, 20000)
    want, occ = _oracle(oracle.Scene(wsc), rays, use_bvh=False)
    W, H = 96, 64
    pfds = camera.dolly_frames(scene, W, H, 2)
    g, ref = GpuHybrid(scene, W, H, gbuffer="standin"), GpuHybrid(scene, W, H, gbuffer="standin")
    ctx = g.ctx
    try:
        built = (ctx.bvh_fingerprint(), ctx.bvh_tree_fingerprint())
        g.frame(pfds[0])
        ref.frame(pfds[0])
        ctx.update_vertices(wide)
        ctx.refit_geometry()
        st = _clean(ctx)
        assert st["half_nodes"] == 0, st
        _check(ctx, rays, want, occ, "wide scene after a refit")
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
        st = _clean(ctx)
        assert st["half_nodes"] == 1 and st["refits"] == 2, st
        assert (ctx.bvh_fingerprint(), ctx.bvh_tree_fingerprint()) == built
        g.frame(pfds[1])
        ref.frame(pfds[1])
        for name, x, y in zip(HYBRID_IMAGES, _hybrid_images(g), _hybrid_images(ref)):
            assert np.array_equal(x, y), f"{name} differs from the original build's after the refit back"
    finally:
        g.close()
        ref.close()


def test_pending_updates_refuse_tracing_and_the_device_route_matches(oracle):
    import torch
    scene = soup(2, 400, 5)
    moved = _with(scene, vertices=_displaced(scene, np.random.default_rng(3), 0.3))
    W, H = 96, 64
    pfd = camera.dolly_frames(scene, W, H, 1)[0]
    g = GpuHybrid(scene, W, H, gbuffer="standin")
    h = GpuHybrid(scene, W, H, gbuffer="standin")
    try:
        g.ctx.update_vertices(moved.vertices)
        g.ctx.update_per_frame_ubo(0, pfd)
        L, hd = g.ctx.L, g.ctx.handle
        rays = np.zeros(4, abi.ray_dtype)
        out = np.zeros(4, abi.ray_hit_dtype)
        assert L.vhr_graph_execute(hd, 0, 0) == GRAPH and "vhr_refit_geometry" in L.vhr_last_error(hd).decode()
        assert L.vhr_ray_query(hd, rays.ctypes.data, 4, abi.RAY_QUERY_HOST_MEMORY, out.ctypes.data) == GRAPH and "vhr_refit_geometry" in L.vhr_last_error(hd).decode()
        assert L.vhr_standin_gbuffer(hd, 0, lib.NORMALS.encode(), lib.MOTION.encode(), lib.DEPTH.encode()) == GRAPH and "vhr_refit_geometry" in L.vhr_last_error(hd).decode()
        g.ctx.refit_geometry()
        _clean(g.ctx)
        g.frame(pfd)
        # the same vertices handed over as a device pointer
        dev = torch.from_numpy(moved.vertices.view(np.uint8).reshape(-1).copy()).cuda()
        h.ctx.update_vertices_device(dev.data_ptr(), len(moved.vertices))
        h.ctx.refit_geometry()
        _clean(h.ctx)
        h.frame(pfd)
        for img in (lib.NORMALS, lib.DEPTH, lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED):
            assert np.array_equal(g.ctx.download(img), h.ctx.download(img)), img
        assert g.ctx.bvh_fingerprint() == h.ctx.bvh_fingerprint()
    finally:
        g.close()
        h.close()


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_an_identity_refit_between_frames_changes_nothing(oracle, frames_in_flight):
    scene = scenes.tiny_scene()
    W, H = 96, 64
    ctxs = []
    try:
        for _ in range(2):
            g = GpuHybrid.__new__(GpuHybrid)
            g.ctx = lib.Context(W, H)
            g.ctx.set_option("frames_in_flight", frames_in_flight)
            g.ctx.upload_scene(scene)
            g.gbuf, g.mode = None, "standin"
            g.path = lib.HybridRenderPath(g.ctx, shadow_mode=0, ambient_occlusion_mode=0, reflection_mode=0, denoise=True, gbuffer_pass=g._gbuffer_pass)
            g.path.build()
            ctxs.append(g)
        a, b = ctxs
        for i, pfd in enumerate(camera.dolly_frames(scene, W, H, 4)):
            a.ctx.update_vertices(scene.vertices)
            a.ctx.refit_geometry()
            for g in (a, b):
                g.ctx.update_per_frame_ubo(i % frames_in_flight, pfd)
                g.ctx.execute(i % frames_in_flight, 0)
                g.ctx.synchronize()
            for img in (lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED):
                assert np.array_equal(a.ctx.download(img), b.ctx.download(img)), (i, img)
    finally:
        for g in ctxs:
            g.close()


def test_resize_keeps_the_refitted_tree(oracle):
    scene = soup(2, 400, 5)
    moved = _with(scene, vertices=_displaced(scene, np.random.default_rng(4), 0.3))
    W, H = 96, 64
    a = GpuHybrid(scene, 64, 48, gbuffer="standin")
    b = None
    try:
        a.ctx.update_vertices(moved.vertices)
        a.ctx.refit_geometry()
        a.path.destroy()
        a.ctx.resize(W, H)
        a.path = lib.HybridRenderPath(a.ctx, shadow_mode=0, ambient_occlusion_mode=0, reflection_mode=0, denoise=True, gbuffer_pass=a._gbuffer_pass)
        a.path.build()
        b = GpuHybrid(moved, W, H, gbuffer="standin", denoise=True)
        for pfd in camera.dolly_frames(scene, W, H, 2):
            a.frame(pfd)
            b.frame(pfd)
            for img in (lib.RAYTRACED, lib.REFLECTIONS, lib.DENOISED):
                assert np.array_equal(a.ctx.download(img), b.ctx.download(img)), img
    finally:
        a.close()
        if b:
            b.close()


def test_a_presplit_tree_refuses_on_the_device(oracle):
    scene = scenes.rotated(soup(22, 1500, 6), rot_y=0.6, rot_x=0.25)
    ctx = lib.Context(64, 64)
    try:
        ctx.set_option("bvh_presplit", 100)
        ctx.set_option("bvh_frame", 0)
        ctx.upload_scene(scene)
        assert ctx.bvh_presplit_level() >= 0
        v = scene.vertices
        assert ctx.L.vhr_update_vertices(ctx.handle, 0, len(v), v.ctypes.data_as(C.c_void_p), 0) == UNSUPPORTED
        assert "bvh_presplit" in ctx.L.vhr_last_error(ctx.handle).decode()
        assert ctx.L.vhr_refit_geometry(ctx.handle) == UNSUPPORTED
    finally:
        ctx.close()
