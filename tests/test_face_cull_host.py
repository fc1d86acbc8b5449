"""vhr_ray_query_faces without a GPU: exports and layout, the argument checks on a host-only context, the facing function --
vhr_debug_ray_facing runs the HOST's copy of csrc/ray_facing.hpp on a host-only context -- against the sign of the determinant in exact
rational arithmetic, the primitives' flip bytes through builds, updates, refits, rebuilds and resizes, and the C++ facade and the C view.

Measured (the pair set of face_cull_cases.pair_set(): 12 KAT pairs + 31 092 grazing pairs on the three soups at 2^-10, 1, 2^10): the host
function disagrees with the exact sign on 0 pairs; the sign of the fp32 determinant (ray_triangle()'s det) on 989; no exact zero."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import face_cull_cases as fc
from vulkanhybridrenderer_amd import abi, lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, GRAPH, NO_DEVICE = -1, -5, -6          # include/vhr_amd.h
WHO = "vhr_ray_query_faces"
NAMES = ("vhr_ray_query_faces", "vhr_get_primitive_facing_flips", "vhr_get_face_cull_statistics", "vhr_debug_ray_facing")


@pytest.fixture(scope="module")
def host_ctx():
    c = lib.Context(64, 64, host_only=True)
    yield c
    c.close()


def _err(c):
    return c.L.vhr_last_error(c.handle).decode()


def test_exports_and_layout():
    text = open(os.path.join(ROOT, "include", "vhr_amd.h")).read()
    types = open(os.path.join(ROOT, "include", "vhr_types.h")).read()
    for name in NAMES:
        assert name in lib.EXPORTS and f"int {name}(" in text and hasattr(lib.load(), name), name
    for line in ("#define VHR_FACE_CULL_NONE  0u", "#define VHR_FACE_CULL_BACK  1u", "#define VHR_FACE_CULL_FRONT 2u",
                 "#define VHR_HIT_KIND_FRONT_FACING 0xFEu", "#define VHR_HIT_KIND_BACK_FACING  0xFFu"):
        assert line in types, line
    assert (abi.FACE_CULL_NONE, abi.FACE_CULL_BACK, abi.FACE_CULL_FRONT, abi.HIT_KIND_FRONT_FACING, abi.HIT_KIND_BACK_FACING) == (0, 1, 2, 0xFE, 0xFF)
    out = (C.c_uint32 * 8)()
    assert lib.load().vhr_ray_query_struct_layout(out) == 8
    assert out[4] == 24 and out[7] == 20                                      # vhr_ray_hit: 24 bytes, `reserved` at 20
    assert abi.ray_hit_dtype.itemsize == 24 and abi.ray_hit_dtype.fields["reserved"][1] == 20


def _raw(c, rays, count, flags, cull_mask, ray_masks, face_cull, results):
    rc = c.L.vhr_ray_query_faces(c.handle, rays, count, flags, cull_mask, ray_masks, face_cull, results)
    return rc, _err(c)


def test_validation_order_is_the_masked_querys_then_face_cull(host_ctx):
    c = host_ctx
    rays, out, rm = np.zeros(4, abi.ray_dtype), np.zeros(4, abi.ray_hit_dtype), np.zeros(5, np.uint8)
    R, O = rays.ctypes.data, out.ctypes.data
    assert R % 16 == 0
    assert c.L.vhr_ray_query_faces(None, R, 4, 0, 0xFF, None, 0, O) == INVALID_ARGUMENT                  # a NULL context
    cases_ = [  # (rays, count, flags, cull_mask, results): every refusal of vhr_ray_query_masked, and what passes its checks
        (0x1000, 5, 4, 0xFF, 0x2000), (0x1000, 5, 8, 0xFF, 0x2000), (0x1000, 5, 32, 0xFF, 0x2000), (0x1000, 5, 0x80000000, 0xFF, 0x2000), (0x1000, 5, 16 | 4, 0xFF, 0x2000),
        (None, 4, 0, 0xFF, O), (R, 4, 2, 0xFF, None), (0x1008, 4, 0, 0xFF, O), (R, 4, 0, 0xFF, O + 2),
        (None, 4, 4, 0x1FF, None),                              # the flag check comes before the pointer checks and the masks
        (R + 8, 4, 0, 0x1FF, O + 2), (R, 4, 0, 0x1FF, O + 2),   # ... the alignments before the cull mask
        (R, 4, 2, 256, O), (R, 4, 2, 0x1FF, O), (R, 4, 2, 0xFFFFFFFF, O),
        (R, 4, 0, 0x0F, O), (R, 4, 1 | 2 | 16, 0xFF, O), (None, 0, 0, 0xFF, None),
    ]
    for r, n, flags, cull, res in cases_:
        for masks_ptr in (None, rm.ctypes.data + 1):            # no alignment requirement
            rc0 = c.L.vhr_ray_query_masked(c.handle, r, n, flags, cull, masks_ptr, res)
            msg0 = _err(c)
            for face in (fc.NONE, fc.BACK, fc.FRONT):
                rc1, msg1 = _raw(c, r, n, flags, cull, masks_ptr, face, res)
                assert rc1 == rc0 and msg1 == msg0.replace("vhr_ray_query_masked:", WHO + ":"), (r, n, flags, cull, face, rc0, rc1, msg0, msg1)
            if rc0 == INVALID_ARGUMENT:                          # an earlier refusal wins over a bad face_cull
                rc1, msg1 = _raw(c, r, n, flags, cull, masks_ptr, 3, res)
                assert rc1 == rc0 and msg1 == msg0.replace("vhr_ray_query_masked:", WHO + ":") and "face_cull" not in msg1
    # then face_cull: an argument check, before the device, count == 0 included
    for bad in (3, 4, 0x80000000, 0xFFFFFFFF):
        for r, n, flags, res in ((R, 4, 2, O), (R, 4, 1, O), (None, 0, 0, None)):
            rc, msg = _raw(c, r, n, flags, 0xFF, None, bad, res)
            assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "face_cull" in msg, (bad, rc, msg)
    # valid arguments: a host-only context has no device (count == 0 as well, as for vhr_ray_query and vhr_ray_query_masked: it is VHR_OK where a
    # query could run, tests/test_gpu_face_cull.py)
    assert _raw(c, None, 0, 0, 0xFF, None, fc.BACK, None)[0] == NO_DEVICE
    for face in (fc.NONE, fc.BACK, fc.FRONT):
        for flags, cull, masks_ptr in ((0, 0xFF, None), (1, 0, None), (2 | 16, 0x03, rm.ctypes.data)):
            rc, msg = _raw(c, R, 4, flags, cull, masks_ptr, face, O)
            assert rc == NO_DEVICE and "host-only" in msg and msg.startswith(WHO + ":"), (rc, msg)


def test_binding_routes_to_the_new_entry_point_only_when_asked(host_ctx):
    r = np.zeros((3, 8), np.float32)
    with pytest.raises(lib.VhrError, match="vhr_ray_query: host-only"):
        host_ctx.ray_query(r)
    with pytest.raises(lib.VhrError, match="vhr_ray_query_masked: host-only"):
        host_ctx.ray_query(r, cull_mask=0x01)
    for face in (fc.NONE, fc.BACK, fc.FRONT):
        with pytest.raises(lib.VhrError, match="vhr_ray_query_faces: host-only"):
            host_ctx.ray_query(r, face_cull=face)
        with pytest.raises(lib.VhrError, match="vhr_ray_query_faces: host-only"):
            host_ctx.ray_query(r, any_hit=True, ray_masks=[1, 2, 3], face_cull=face)
        with pytest.raises(lib.VhrError, match="vhr_ray_query_faces: host-only"):
            host_ctx.ray_query_device(0x10000, 1, 0x20000, face_cull=face)
    with pytest.raises(lib.VhrError, match="face_cull"):
        host_ctx.ray_query(r, face_cull=3)
    with pytest.raises(lib.VhrError, match="cull_mask"):
        host_ctx.ray_query_device(0x10000, 1, 0x20000, cull_mask=300, face_cull=fc.BACK)
    with pytest.raises(lib.VhrError, match="vhr_ray_query: host-only"):
        host_ctx.ray_query_device(0x10000, 1, 0x20000)


def test_the_facing_function_against_exact_arithmetic(host_ctx):
    pairs, sign = fc.pair_set()
    n = len(pairs)
    assert n >= 30000
    zero = sign == 0
    print(f"{n} pairs, {int(zero.sum())} with an exact determinant of 0, {fc._PAIRS['settled']} settled by Fractions")
    assert zero.mean() < 0.01
    for flip in (0, 1):
        got = host_ctx.debug_ray_facing(pairs, None if flip == 0 else np.ones(n, np.uint8))
        assert np.isin(got, (fc.KIND_FRONT, fc.KIND_BACK)).all()
        want = fc.kind_of_sign(sign, np.full(n, flip))
        wrong = (got != want) & ~zero
        print(f"flip {flip}: {int(wrong.sum())} disagreements with the exact sign")
        assert wrong.sum() == 0, (flip, np.nonzero(wrong)[0][:5].tolist())
    # flips are per pair
    mixed = (np.arange(n) % 3 == 0).astype(np.uint8)
    assert np.array_equal(host_ctx.debug_ray_facing(pairs, mixed)[~zero], fc.kind_of_sign(sign, mixed)[~zero])
    # the fp32 determinant's sign is not good enough on these pairs (informational: nobody "simplifies" the function)
    fp32_wrong = int(((fc.fp32_det_sign(pairs[:, 0:3], pairs[:, 3:6], pairs[:, 6:9]) != sign) & ~zero).sum())
    print(f"the sign of the fp32 determinant is wrong on {fp32_wrong} of {n} pairs")
    assert fp32_wrong > 0


def test_simple_and_degenerate_pairs(host_ctx):
    # e1 = x, e2 = y: the normal e1 x e2 = +z; a ray travelling along -z sees the vertices counter-clockwise: front
    tri = [1, 0, 0, 0, 1, 0]
    pairs = np.array([[0, 0, -1] + tri, [0, 0, 1] + tri, [1, 0, 0] + tri, [0, 0, 0] + tri, [np.nan, 0, -1] + tri, [0, 0, -1, 0, 0, 0, 0, 0, 0],
                      [0, 0, -np.inf] + tri], np.float32)               # (the last: inf * 0 in d x e2, a NaN determinant)
    assert host_ctx.debug_ray_facing(pairs).tolist() == [fc.KIND_FRONT, fc.KIND_BACK, fc.KIND_BACK, fc.KIND_BACK, fc.KIND_BACK, fc.KIND_BACK, fc.KIND_BACK]
    # flip inverts, det == 0 and NaN included: (det > 0) != flip
    assert host_ctx.debug_ray_facing(pairs, np.ones(len(pairs), np.uint8)).tolist() == \
        [fc.KIND_BACK, fc.KIND_FRONT, fc.KIND_FRONT, fc.KIND_FRONT, fc.KIND_FRONT, fc.KIND_FRONT, fc.KIND_FRONT]
    # a NaN direction is back-facing
    assert host_ctx.debug_ray_facing(np.array([[np.nan, np.nan, np.nan] + tri], np.float32)).tolist() == [fc.KIND_BACK]
    # its own checks
    c = host_ctx
    assert c.L.vhr_debug_ray_facing(None, None, None, 0, None) == INVALID_ARGUMENT
    assert c.L.vhr_debug_ray_facing(c.handle, None, None, 3, None) == INVALID_ARGUMENT and "vhr_debug_ray_facing" in _err(c)
    assert c.L.vhr_debug_ray_facing(c.handle, None, None, 0, None) == 0 and c.debug_ray_facing(np.zeros((0, 9), np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        c.debug_ray_facing(pairs, [1, 0])


def _transforms():
    rot = scenes.trs((0.3, 0.2, -0.4), rot_y=0.7, rot_x=-0.3)
    return np.stack([abi.mat_to_glm(np.eye(4)), abi.mat_to_glm(np.diag([-1.0, 1, 1, 1])), abi.mat_to_glm(rot),
                     abi.mat_to_glm(rot @ np.diag([1.0, -2, 1, 1])), abi.mat_to_glm(np.diag([-1.0, -1, 1, 1]))])


def test_flips_follow_the_transforms():
    tiny = scenes.tiny_scene()
    assert len(tiny.primitives) == 5
    p = tiny.primitives.copy()
    p["transform"] = _transforms()
    c = lib.Context(64, 64, host_only=True)
    L = c.L
    out = np.zeros(16, np.uint8)
    try:
        # the arguments first, then "no geometry yet"
        assert L.vhr_get_primitive_facing_flips(None, 0, 1, out.ctypes.data) == INVALID_ARGUMENT
        assert L.vhr_get_primitive_facing_flips(c.handle, 0, 3, None) == INVALID_ARGUMENT and "vhr_get_primitive_facing_flips" in _err(c) and "NULL" in _err(c)
        assert L.vhr_get_face_cull_statistics(c.handle, None) == INVALID_ARGUMENT and L.vhr_get_face_cull_statistics(None, None) == INVALID_ARGUMENT
        assert L.vhr_get_primitive_facing_flips(c.handle, 0, 1, out.ctypes.data) == GRAPH and "no geometry yet" in _err(c)
        assert c.face_cull_statistics() == [0, 0, 0, 0]
        c.update_geometry(tiny.vertices, tiny.indices, p)
        assert c.primitive_facing_flips().tolist() == [0, 1, 0, 1, 0]
        assert c.primitive_facing_flips(1, 3).tolist() == [1, 0, 1] and c.primitive_facing_flips(4).tolist() == [0]
        assert c.face_cull_statistics() == [2, 0, 0, 0]
        # a range outside the primitives; count == 0 does nothing
        for first, count in ((0, 6), (5, 1), (3, 4), (0xFFFFFFFF, 2)):
            assert L.vhr_get_primitive_facing_flips(c.handle, first, count, out.ctypes.data) == INVALID_ARGUMENT and "exceeds the primitives (5)" in _err(c)
        assert L.vhr_get_primitive_facing_flips(c.handle, 5, 0, None) == 0
        # a sub-range of new transforms and a refit: the flips follow, the untouched ones stay
        t = _transforms()
        c.update_primitive_transforms(np.stack([t[0], t[3], t[1]]), first_primitive=1)       # primitives 1, 2, 3 := identity, mirrored rotation, mirror
        c.refit_geometry()
        assert c.primitive_facing_flips().tolist() == [0, 0, 1, 1, 0] and c.face_cull_statistics()[0] == 2
        c.update_primitive_transforms(t[1:2], first_primitive=4)
        c.refit_geometry_partial(force=True)
        assert c.primitive_facing_flips().tolist() == [0, 0, 1, 1, 1] and c.face_cull_statistics()[0] == 3
        # a rebuild and a resize keep them
        c.rebuild_geometry()
        assert c.primitive_facing_flips().tolist() == [0, 0, 1, 1, 1]
        c.resize(48, 40)
        assert c.primitive_facing_flips().tolist() == [0, 0, 1, 1, 1] and c.face_cull_statistics() == [3, 0, 0, 0]
        # a zero determinant and a tiny negative one
        z = np.stack([abi.mat_to_glm(np.diag([0.0, 1, 1, 1])), abi.mat_to_glm(np.diag([-1e-20, 1e-10, 1e-10, 1]))])
        c.update_primitive_transforms(z, first_primitive=0)
        c.refit_geometry()
        assert c.primitive_facing_flips().tolist() == [0, 1, 1, 1, 1]
        # vhr_update_geometry computes them again, and the count follows the new scene
        c.update_geometry(tiny.vertices, tiny.indices, tiny.primitives)
        assert c.primitive_facing_flips().tolist() == fc.expected_flips(tiny).tolist() == [0, 0, 0, 0, 0] and c.face_cull_statistics()[0] == 0
        # no part of a fingerprint: the tree of a mirrored scene is hashed as any tree, and the masks do not know the flips
        assert c.primitive_masks().tolist() == [0xFF] * 5
    finally:
        c.close()


def test_the_mirrored_soups_have_flips_on_a_seeded_half(host_ctx):
    from tests import ray_truth as rt
    for seed, _, n_prims in rt.SOUPS:
        scene, pick = fc.mirrored_half(rt.soup_scene(seed), seed)
        want = np.zeros(len(scene.primitives), np.uint8)
        want[pick] = 1
        assert len(pick) == (n_prims + 1) // 2 and fc.expected_flips(scene).tolist() == want.tolist()
        assert fc.expected_flips(rt.soup_scene(seed)).sum() == 0


FACADE = '''#include "vhr_render_graph.hpp"
#include <vector>
void probes(vhr::DeviceContext &dc, const std::vector<vhr_ray> &rays, const std::vector<uint8_t> &ray_masks, std::vector<vhr_ray_hit> &hits, std::vector<uint8_t> &occluded) {
    vhr::ResourceManager rm(dc);
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_HOST_MEMORY, 0xFFu, nullptr, VHR_FACE_CULL_BACK, hits.data());
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT | VHR_RAY_QUERY_HOST_MEMORY, 0x02u, ray_masks.data(), VHR_FACE_CULL_FRONT, occluded.data());
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_HOST_MEMORY, 0xFFu, nullptr, hits.data());       // the masked overload is still there
    bool front = hits[0].reserved == VHR_HIT_KIND_FRONT_FACING, back = hits[0].reserved == VHR_HIT_KIND_BACK_FACING;
    (void)front; (void)back;
}
'''
C_VIEW = '''#include "vhr_amd.h"
int f(vhr_context *c, const vhr_ray *r, vhr_ray_hit *h, uint8_t *w, uint64_t s[4], const float *pairs, const uint8_t *flips) {
    unsigned kinds[2] = { VHR_HIT_KIND_FRONT_FACING, VHR_HIT_KIND_BACK_FACING };
    (void)kinds;
    return vhr_ray_query_faces(c, r, 1, 0, 0xFFu, 0, VHR_FACE_CULL_NONE, h) + vhr_ray_query_faces(c, r, 1, VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT, 1u, w, VHR_FACE_CULL_FRONT, w) +
           vhr_ray_query_faces(c, r, 1, VHR_RAY_QUERY_HOST_MEMORY, 0xFFu, 0, VHR_FACE_CULL_BACK, h) +
           vhr_get_primitive_facing_flips(c, 0, 1, w) + vhr_get_face_cull_statistics(c, s) + vhr_debug_ray_facing(c, pairs, flips, 1, w);
}
'''


def test_facade_and_c_view_compile(tmp_path):
    cxx, cc = shutil.which("g++") or shutil.which("c++"), shutil.which("gcc") or shutil.which("cc")
    if not cxx or not cc:
        pytest.skip("no compiler")
    src = tmp_path / "face_cull.cpp"
    src.write_text(FACADE)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    csrc = tmp_path / "face_cull.c"
    csrc.write_text(C_VIEW)
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(csrc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
