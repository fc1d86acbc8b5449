"""Ray cull masks without a GPU: vhr_set_primitive_masks / vhr_get_primitive_masks, the three "*_ray_mask" options and the argument checks of
vhr_ray_query_masked on a host-only context, the C++ facade's two methods, and the conditions tests/test_gpu_ray_masks.py relies on in
tests/ray_mask_cases: the oracle's channels are independent of each other, every class mask and every single-bit query mask changes
what the rays see, and every occluder is met by rays of the plain query.  (The refusal inside a pass needs a graph that runs: GPU test.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ray_mask_cases as cases
from tests.alpha_scenes import oracle_hits
from vulkanhybridrenderer_amd import abi, camera, lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, GRAPH, NO_DEVICE = -1, -5, -6          # include/vhr_amd.h
KEYS = ("shadow_ray_mask", "ao_ray_mask", "reflection_ray_mask")
W, H, FRAMES = cases.W, cases.H, cases.FRAMES


@pytest.fixture
def host_ctx():
    c = lib.Context(64, 64, host_only=True)
    yield c
    c.close()


@pytest.fixture
def scene_ctx(host_ctx):
    sc = cases.scene()
    host_ctx.update_geometry(sc.vertices, sc.indices, sc.primitives)
    return host_ctx, sc


def _err(c):
    return c.L.vhr_last_error(c.handle).decode()


def test_the_scene_is_the_one_described():
    sc = cases.scene()
    tiny = scenes.tiny_scene()
    assert len(tiny.primitives) == cases.N_TINY and len(sc.primitives) == 12 and int((sc.primitives["index_count"] // 3).sum()) == 396
    assert sc.primitives[:cases.N_TINY].tobytes() == tiny.primitives.tobytes()
    m = sc.primitives["material"][cases.N_TINY:]
    assert (m["alpha_mask"] == 0).all() and (m["base_color_texture"] == -1).all() and (m["base_color"][:, 3] == 1.0).all()      # opaque, untextured
    assert cases.masks().tolist() == [0xFF] * 5 + [0x01, 0x02, 0x04, 0x03, 0x06, 0x05, 0x00]
    sub, keep = cases.sub_scene(sc, cases.masks(), 0x01)
    assert keep.tolist() == [0, 1, 2, 3, 4, 5, 8, 10] and len(sub.primitives) == 8
    assert cases.sub_scene(sc, cases.masks(), 0x00)[0] is None and len(cases.sub_scene(sc, cases.masks(), 0xFF)[1]) == 11


def test_masks_default_to_ff_and_round_trip(scene_ctx):
    c, sc = scene_ctx
    assert c.primitive_masks().tolist() == [0xFF] * 12 and c.ray_mask_statistics() == [0, 0, 0, 0]
    c.set_primitive_masks(cases.masks())
    assert c.primitive_masks().tolist() == cases.masks().tolist() and c.ray_mask_statistics()[0] == 7
    c.set_primitive_masks([0x10, 0xFF, 0x20], first_primitive=6)                  # a partial range: the others keep their values
    want = cases.masks().copy()
    want[6:9] = [0x10, 0xFF, 0x20]
    assert c.primitive_masks().tolist() == want.tolist()
    assert c.primitive_masks(first_primitive=7, count=3).tolist() == want[7:10].tolist()
    assert c.primitive_masks(first_primitive=11).tolist() == [0x00]
    assert c.ray_mask_statistics()[0] == 6
    c.set_primitive_masks([0xFF] * 12)
    assert c.primitive_masks().tolist() == [0xFF] * 12 and c.ray_mask_statistics()[0] == 0


def test_storing_ff_on_untouched_masks_stores_nothing(scene_ctx):
    c, _ = scene_ctx
    c.set_primitive_masks([0xFF] * 4, first_primitive=3)
    assert c.primitive_masks().tolist() == [0xFF] * 12 and c.ray_mask_statistics()[0] == 0


def test_update_geometry_resets_resize_and_refit_keep(scene_ctx):
    c, sc = scene_ctx
    c.set_primitive_masks(cases.masks())
    c.resize(96, 48)
    assert c.primitive_masks().tolist() == cases.masks().tolist()
    t = sc.primitives["transform"][cases.N_TINY:].copy()
    t[:, 13] += 0.25                                                             # the occluders a quarter unit up
    c.update_primitive_transforms(t, first_primitive=cases.N_TINY)
    c.refit_geometry()
    assert c.primitive_masks().tolist() == cases.masks().tolist()
    c.update_primitive_transforms(sc.primitives["transform"][cases.N_TINY:], first_primitive=cases.N_TINY)
    c.refit_geometry_partial(force=True)
    assert c.primitive_masks().tolist() == cases.masks().tolist() and c.ray_mask_statistics()[0] == 7
    c.update_geometry(sc.vertices, sc.indices, sc.primitives)
    assert c.primitive_masks().tolist() == [0xFF] * 12 and c.ray_mask_statistics()[0] == 0
    tiny = scenes.tiny_scene()                                                   # ... and the count follows the new scene
    c.set_primitive_masks(cases.masks())
    c.update_geometry(tiny.vertices, tiny.indices, tiny.primitives)
    assert c.primitive_masks().tolist() == [0xFF] * 5
    assert c.L.vhr_set_primitive_masks(c.handle, 5, 1, cases.masks().ctypes.data) == INVALID_ARGUMENT


def test_refusals_argument_checks_first(host_ctx):
    c, L = host_ctx, host_ctx.L
    m = cases.masks()
    out = np.zeros(16, np.uint8)
    # the arguments first, on a context without geometry too
    assert L.vhr_set_primitive_masks(None, 0, 1, m.ctypes.data) == INVALID_ARGUMENT
    assert L.vhr_set_primitive_masks(c.handle, 0, 3, None) == INVALID_ARGUMENT and "vhr_set_primitive_masks" in _err(c) and "NULL" in _err(c)
    assert L.vhr_get_primitive_masks(c.handle, 0, 3, None) == INVALID_ARGUMENT and "vhr_get_primitive_masks" in _err(c) and "NULL" in _err(c)
    assert L.vhr_get_ray_mask_statistics(c.handle, None) == INVALID_ARGUMENT and L.vhr_get_ray_mask_statistics(None, None) == INVALID_ARGUMENT
    # no geometry yet
    assert L.vhr_set_primitive_masks(c.handle, 0, 1, m.ctypes.data) == GRAPH and "no geometry yet" in _err(c)
    assert L.vhr_get_primitive_masks(c.handle, 0, 1, out.ctypes.data) == GRAPH and "no geometry yet" in _err(c)
    sc = cases.scene()
    c.update_geometry(sc.vertices, sc.indices, sc.primitives)
    # a range outside the primitives
    for first, count in ((0, 13), (12, 1), (5, 8), (0xFFFFFFFF, 2)):
        assert L.vhr_set_primitive_masks(c.handle, first, count, np.zeros(16, np.uint8).ctypes.data) == INVALID_ARGUMENT and "exceeds the primitives (12)" in _err(c)
        assert L.vhr_get_primitive_masks(c.handle, first, count, out.ctypes.data) == INVALID_ARGUMENT and "exceeds the primitives (12)" in _err(c)
    assert c.primitive_masks().tolist() == [0xFF] * 12                           # nothing was stored
    # count == 0: VHR_OK, nothing done (NULL is fine then)
    assert L.vhr_set_primitive_masks(c.handle, 12, 0, None) == 0 and L.vhr_get_primitive_masks(c.handle, 0, 0, None) == 0
    assert L.vhr_set_primitive_masks(c.handle, 0, 12, m.ctypes.data) == 0 and c.primitive_masks().tolist() == m.tolist()


@pytest.mark.parametrize("key", KEYS)
def test_class_mask_options(host_ctx, key):
    c = host_ctx
    assert c.get_option(key) == 255
    for v in (0, 1, 0x80, 255, 7):
        c.set_option(key, v)
        assert c.get_option(key) == v
        assert [c.get_option(k) for k in KEYS if k != key] == [255, 255]         # three values, not one
    for bad in (-1, 256, 1 << 20):
        assert c.L.vhr_set_option(c.handle, key.encode(), bad) == INVALID_ARGUMENT and key in _err(c) and "0..255" in _err(c)
        assert c.get_option(key) == 7
    assert key not in lib.option_table()


def _raw(ctx, rays, count, flags, cull_mask, ray_masks, results):
    rc = ctx.L.vhr_ray_query_masked(ctx.handle, rays, count, flags, cull_mask, ray_masks, results)
    return rc, _err(ctx)


def test_masked_query_validation_order_is_the_plain_querys(host_ctx):
    c = host_ctx
    rays, out, rm = np.zeros(4, abi.ray_dtype), np.zeros(4, abi.ray_hit_dtype), np.zeros(5, np.uint8)
    assert rays.ctypes.data % 16 == 0
    cases_ = [  # (rays, count, flags, results) -> the plain query's answer, which the masked one must give with its own name in the message
        (0x1000, 5, 4, 0x2000), (0x1000, 5, 8, 0x2000), (0x1000, 5, 0x80000000, 0x2000), (0x1000, 5, 16 | 4, 0x2000),
        (None, 4, 0, out.ctypes.data), (rays.ctypes.data, 4, 2, None), (0x1008, 4, 0, out.ctypes.data), (rays.ctypes.data, 4, 0, out.ctypes.data + 2),
        (None, 4, 4, None),                                     # the flag check comes before the pointer checks
        (rays.ctypes.data, 4, 0, out.ctypes.data), (rays.ctypes.data, 4, 1 | 2 | 16, out.ctypes.data), (None, 0, 0, None),
    ]
    for r, n, flags, res in cases_:
        rc0 = c.L.vhr_ray_query(c.handle, r, n, flags, res)
        msg0 = _err(c)
        for masks_ptr in (None, rm.ctypes.data + 1):            # no alignment requirement
            rc1, msg1 = _raw(c, r, n, flags, 0x0F, masks_ptr, res)
            assert rc1 == rc0 and msg1 == msg0.replace("vhr_ray_query:", "vhr_ray_query_masked:"), (r, n, flags, rc0, rc1, msg0, msg1)
    for flags in (4, 8, 0x80000000):
        rc, msg = _raw(c, 0x1000, 5, flags, 0xFF, None, 0x2000)
        assert rc == INVALID_ARGUMENT and "unknown flag" in msg, (flags, rc, msg)
    # cull_mask beyond 8 bits: an argument check, before the device
    for bad in (256, 0x1FF, 0xFFFFFFFF):
        rc, msg = _raw(c, rays.ctypes.data, 4, 2, bad, None, out.ctypes.data)
        assert rc == INVALID_ARGUMENT and "cull_mask" in msg and "0xFF" in msg, (bad, rc, msg)
    # after validation: a host-only context has no device
    for cull, masks_ptr in ((0xFF, None), (0, None), (0x03, rm.ctypes.data)):
        rc, msg = _raw(c, rays.ctypes.data, 4, 2, cull, masks_ptr, out.ctypes.data)
        assert rc == NO_DEVICE and "host-only" in msg and "vhr_ray_query_masked" in msg, (rc, msg)


def test_binding_routes_to_the_masked_entry_point_only_when_asked(host_ctx):
    r = np.zeros((3, 8), np.float32)
    with pytest.raises(lib.VhrError, match="vhr_ray_query: host-only"):
        host_ctx.ray_query(r)
    with pytest.raises(lib.VhrError, match="vhr_ray_query_masked: host-only"):
        host_ctx.ray_query(r, cull_mask=0x01)
    with pytest.raises(lib.VhrError, match="vhr_ray_query_masked: host-only"):
        host_ctx.ray_query(r, any_hit=True, ray_masks=[1, 2, 3])
    with pytest.raises(ValueError):
        host_ctx.ray_query(r, ray_masks=[1, 2])
    with pytest.raises(lib.VhrError, match="vhr_ray_query: host-only"):
        host_ctx.ray_query_device(0x10000, 1, 0x20000)
    with pytest.raises(lib.VhrError, match="vhr_ray_query_masked: host-only"):
        host_ctx.ray_query_device(0x10000, 1, 0x20000, ray_masks_ptr=0x30001)
    with pytest.raises(lib.VhrError, match="cull_mask"):
        host_ctx.ray_query_device(0x10000, 1, 0x20000, cull_mask=300)


def test_struct_layout_call_is_unchanged():
    out = (C.c_uint32 * 8)()
    assert lib.load().vhr_ray_query_struct_layout(out) == 8
    assert list(out) == [32, 12, 16, 28, 24, 12, 16, 20]
    assert abi.ray_dtype.itemsize == 32 and abi.ray_hit_dtype.itemsize == 24


def test_exports_are_declared():
    text = open(os.path.join(ROOT, "include", "vhr_amd.h")).read()
    for name in ("vhr_set_primitive_masks", "vhr_get_primitive_masks", "vhr_ray_query_masked", "vhr_get_ray_mask_statistics"):
        assert name in lib.EXPORTS and f"int {name}(" in text and hasattr(lib.load(), name)


def test_facade_methods_compile(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    src = tmp_path / "ray_masks.cpp"
    src.write_text('''#include "vhr_render_graph.hpp"
#include <vector>
void colliders_only(vhr::DeviceContext &dc, const std::vector<vhr_ray> &rays, const std::vector<uint8_t> &ray_masks, std::vector<uint8_t> &occluded,
                    std::vector<vhr_ray_hit> &hits) {
    vhr::ResourceManager rm(dc);
    rm.SetPrimitiveMasks(3, std::vector<uint8_t>{ 0x01, 0x02, 0x00 });
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT | VHR_RAY_QUERY_HOST_MEMORY, 0x02, nullptr, occluded.data());
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_HOST_MEMORY, 0xFF, ray_masks.data(), hits.data());
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_HOST_MEMORY, hits.data());
}
''')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------
# the conditions the GPU tests' inputs must meet: the oracle alone
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_channels(oracle):
    """Per class mask: the oracle's frames on the full scene and on the mask's sub-scene, under the FULL scene's G-buffers."""
    sc = cases.scene()
    full = oracle.Scene(sc)
    subs = {m: oracle.Scene(cases.sub_scene(sc, cases.masks(), m)[0]) for m in (cases.SHADOW_MASK, cases.AO_MASK, cases.REFLECTION_MASK)}
    frames = []
    for pfd in camera.dolly_frames(sc, W, H, FRAMES):
        gbuf = full.gbuffer(pfd, W, H)
        frames.append(dict(pfd=pfd, gbuf=gbuf))
    return sc, full, subs, frames


def test_the_oracles_channels_do_not_depend_on_each_other(oracle_channels):
    sc, full, subs, frames = oracle_channels
    tp = abi.default_trace_params
    for f in frames:
        n, d = f["gbuf"][0], f["gbuf"][2]
        sa, refl, _, _ = full.raygen(f["pfd"], tp(), n, d)
        sa_no_ao, refl_no_ao, _, _ = full.raygen(f["pfd"], tp(ao_spp=0), n, d)
        sa_no_shadow, refl_no_shadow, _, _ = full.raygen(f["pfd"], tp(shadow=False), n, d)
        assert np.array_equal(sa[..., 0], sa_no_ao[..., 0])                      # the shadow channel does not depend on ao_spp
        assert np.array_equal(sa[..., 1], sa_no_shadow[..., 1])                  # the AO channel does not depend on shadow_enable
        assert refl.tobytes() == refl_no_ao.tobytes() == refl_no_shadow.tobytes()


def test_every_class_mask_changes_its_channel_in_every_frame(oracle_channels):
    """Conditions on the scene, not measurements: at least 300 texels of every frame and channel differ between the full scene and the
    channel's sub-scene."""
    sc, full, subs, frames = oracle_channels
    tp = abi.default_trace_params()
    for i, f in enumerate(frames):
        n, d = f["gbuf"][0], f["gbuf"][2]
        sa, refl, _, _ = full.raygen(f["pfd"], tp, n, d)
        shadow = int((subs[cases.SHADOW_MASK].raygen(f["pfd"], tp, n, d)[0][..., 0] != sa[..., 0]).sum())
        ao = int((subs[cases.AO_MASK].raygen(f["pfd"], tp, n, d)[0][..., 1] != sa[..., 1]).sum())
        mirror = int((subs[cases.REFLECTION_MASK].raygen(f["pfd"], tp, n, d)[1] != refl).any(-1).sum())
        print(f"frame {i}: shadow {shadow}, AO {ao}, reflection {mirror} texels differ of {int((d != 0).sum())} covered")
        assert shadow >= 300 and ao >= 300 and mirror >= 300, (i, shadow, ao, mirror)


def test_the_rays_meet_every_occluder_and_every_single_bit_mask_acts(oracle):
    sc = cases.scene()
    rays = cases.rays(sc)
    assert len(rays) == cases.N_RANDOM + 7 * cases.N_AIMED and len(rays) % 64 != 0
    plain, plain_occ = oracle_hits(oracle.Scene(sc), rays, use_bvh=True)
    for p in range(cases.N_TINY, 12):
        assert (plain["geometry_index"] == p).sum() >= 5, (p, int((plain["geometry_index"] == p).sum()))
    assert 0.2 < plain_occ.mean() < 0.98
    for m in (0x01, 0x02, 0x04):
        sub, keep = cases.sub_scene(sc, cases.masks(), m)
        want, occ = oracle_hits(oracle.Scene(sub), rays, use_bvh=True)
        closest = int(cases.hit_bits_differ(cases.remap_hits(want, keep), plain).sum())
        any_hit = int((occ != plain_occ).sum())
        print(f"mask {m:#04x}: {closest} closest hits and {any_hit} any-hit answers differ from the full scene's")
        assert closest >= 20 and any_hit >= 10, (m, closest, any_hit)
