"""vhr_resolve_hits without a GPU: the layout of vhr_surface_point, the argument checks, and the geometry part -- a host-only context runs the
HOST's copy of csrc/surface_point.hpp on the arrays it keeps -- against the numpy restatement of the contract (tests/surface_truth.py), the
oracle's own records, the binary64 position and its bound, mirrored primitives, the C++ facade and the C view of the types.

Measured (the host's copy, the mirrored soup and scene_f4, 2 090 + 500 hits): every field equals the restatement bit for bit; the largest
|position - binary64| / bound is 0.91 (soup) and 0.68 (scene_f4)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import f2_scene, face_cull_cases as fc, ray_truth as rt, surface_truth as st
from vulkanhybridrenderer_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, GRAPH, NO_DEVICE = 0, -1, -5, -6          # include/vhr_amd.h
WHO = "vhr_resolve_hits"
SOUP_SEED = 2
MISS = abi.RAY_MISS


def _host(scene):
    c = lib.Context(64, 64, host_only=True)
    c.update_geometry(scene.vertices, scene.indices, scene.primitives)
    return c


@pytest.fixture(scope="module")
def cases():
    """name -> (scene, host-only context, hits, the host twin's records): computed once, left unchanged."""
    soup, _ = fc.mirrored_half(rt.soup_scene(SOUP_SEED), SOUP_SEED)
    out = {}
    for name, scene in (("soup", soup), ("f4", f2_scene.scene_f4())):
        c = _host(scene)
        hits = st.triangle_hits(scene, 11)
        out[name] = (scene, c, hits, c.resolve_hits(hits))
    yield out
    for _, c, _, _ in out.values():
        c.close()


def _err(c):
    return c.L.vhr_last_error(c.handle).decode()


def _raw(c, hits, count, flags, out):
    rc = c.L.vhr_resolve_hits(c.handle, hits, count, flags, out)
    return rc, _err(c)


def test_layout_and_exports():
    text = open(os.path.join(ROOT, "include", "vhr_amd.h")).read()
    types = open(os.path.join(ROOT, "include", "vhr_types.h")).read()
    for name in ("vhr_resolve_hits", "vhr_get_surface_statistics", "vhr_surface_point_layout"):
        assert name in lib.EXPORTS and f"int {name}(" in text and hasattr(lib.load(), name), name
    out = (C.c_uint32 * 8)()
    assert lib.load().vhr_surface_point_layout(out) == 8 and lib.load().vhr_surface_point_layout(None) == INVALID_ARGUMENT
    d = abi.surface_point_dtype
    assert list(out) == [d.itemsize] + [d.fields[f][1] for f in ("flags", "geometric_normal", "metallic", "shading_normal", "roughness", "base_color", "uv0")]
    assert d.itemsize == 80 and d.fields["position"][1] == 0 and d.fields["uv1"][1] == 72 and d.names == st.FIELDS
    assert "sizeof(vhr_surface_point) == 80" in types
    for line in ("#define VHR_SURFACE_MATERIAL      1u", "#define VHR_SURFACE_HOST_MEMORY   2u", "#define VHR_SURFACE_VALID               1u",
                 "#define VHR_SURFACE_DEGENERATE          2u", "#define VHR_SURFACE_NO_SHADING_NORMAL   4u", "#define VHR_SURFACE_NORMAL_MAPPED       8u",
                 "#define VHR_SURFACE_DISCARDED          16u"):
        assert line in types, line
    assert (abi.SURFACE_MATERIAL, abi.SURFACE_HOST_MEMORY) == (1, 2)
    assert (abi.SURFACE_VALID, abi.SURFACE_DEGENERATE, abi.SURFACE_NO_SHADING_NORMAL, abi.SURFACE_NORMAL_MAPPED, abi.SURFACE_DISCARDED) == (1, 2, 4, 8, 16)


def test_validation_order_and_messages(cases):
    c = cases["soup"][1]
    hits, out = np.zeros(5, abi.ray_hit_dtype), c.resolve_hits(np.zeros(4, abi.ray_hit_dtype))
    Hp, Op = hits.ctypes.data, out.ctypes.data
    assert Hp % 4 == 0 and Op % 16 == 0
    assert c.L.vhr_resolve_hits(None, Hp, 4, 2, Op) == INVALID_ARGUMENT                                   # a NULL context
    for h, o in ((None, Op), (Hp, None), (None, None)):
        rc, msg = _raw(c, h, 4, 2, o)
        assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "NULL" in msg, (rc, msg)
    rc, msg = _raw(c, None, 4, 4, None)                                                                    # NULL comes first
    assert rc == INVALID_ARGUMENT and "NULL" in msg
    for flags in (4, 8, 16, 0x80000000, 1 | 4, 2 | 8):
        for n, h, o in ((4, Hp + 2, Op + 8), (0, None, None)):                                             # ... then the flags (count == 0 included)
            rc, msg = _raw(c, h, n, flags, o)
            assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "unknown flag" in msg, (flags, rc, msg)
    rc, msg = _raw(c, Hp + 2, 4, 2, Op + 8)                                                                # ... then the hits' alignment
    assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "hits must be 4-byte aligned" in msg, (rc, msg)
    for off in (4, 8, 12):
        rc, msg = _raw(c, Hp + 4, 4, 2, Op + off)                                                          # ... then out's (hits need 4 only)
        assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "out must be 16-byte aligned" in msg, (rc, msg)
    # count == 0 is VHR_OK on every context, whatever the valid flags and pointers
    for flags in (0, 1, 2, 3):
        assert _raw(c, None, 0, flags, None)[0] == OK and _raw(c, Hp + 2, 0, flags, Op + 8)[0] == OK
    # a host-only context samples no texture and has no device memory
    for flags in (1, 3):
        rc, msg = _raw(c, Hp, 4, flags, Op)
        assert rc == NO_DEVICE and msg.startswith(WHO + ":") and "host-only" in msg and "VHR_SURFACE_MATERIAL" in msg, (rc, msg)
    rc, msg = _raw(c, Hp, 4, 0, Op)
    assert rc == NO_DEVICE and msg.startswith(WHO + ":") and "host-only" in msg and "VHR_SURFACE_HOST_MEMORY" in msg, (rc, msg)
    with pytest.raises(lib.VhrError, match="vhr_resolve_hits: host-only"):
        c.resolve_hits(hits, material=True)
    with pytest.raises(lib.VhrError, match="vhr_resolve_hits: host-only"):
        c.resolve_hits_device(0x10000, 1, 0x20000)
    assert _raw(c, Hp + 4, 4, 2, Op)[0] == OK                                                              # 4-byte-aligned hits pass


def test_pending_updates_refuse_and_the_refit_releases():
    scene = rt.soup_scene(1)
    c = _host(scene)
    try:
        fresh = lib.Context(64, 64, host_only=True)
        assert fresh.surface_statistics() == [0, 0, 0, 0]
        none = fresh.resolve_hits(st.triangle_hits(scene, 3))                                              # a context without geometry resolves nothing
        assert not none.view(np.uint8).any() and fresh.surface_statistics() == [len(none), 0, 0, 0]
        fresh.close()
        hits = st.triangle_hits(scene, 3)
        before = c.resolve_hits(hits)
        assert c.surface_statistics() == [len(hits), len(hits), 0, 0]
        t = scene.primitives["transform"].copy()
        t[1] = fc.mirror_transform(t[1])
        c.update_primitive_transforms(t[1:2], first_primitive=1)
        out = c.resolve_hits(np.zeros(0, abi.ray_hit_dtype))                                               # count == 0 comes first
        assert len(out) == 0
        rc, msg = _raw(c, hits.ctypes.data, len(hits), 2, before.ctypes.data)
        assert rc == GRAPH and msg.startswith(WHO + ":") and "vhr_refit_geometry" in msg, (rc, msg)
        c.refit_geometry()
        import dataclasses
        moved = dataclasses.replace(scene, primitives=scene.primitives.copy())
        moved.primitives["transform"] = t
        after = c.resolve_hits(hits)
        assert not st.same_bits(after, st.resolve(moved, hits)) and st.same_bits(after, before)
    finally:
        c.close()


def test_host_twin_equals_the_restatement_bit_for_bit(cases):
    for name, (scene, c, hits, got) in cases.items():
        want = st.resolve(scene, hits, flips=c.primitive_facing_flips())
        assert (want["flags"] & st.VALID).all() and len(hits) == 5 * len(st.triangle_ids(scene)[0])
        assert not st.same_bits(got, want), (name, st.same_bits(got, want))
        assert not got["base_color"].any() and not got["metallic"].any() and not got["roughness"].any()
        assert not np.isnan(got["position"]).any() and not np.isnan(got["geometric_normal"]).any() and not np.isnan(got["shading_normal"]).any()
        assert not st.same_bits(c.resolve_hits(hits), got) and c.surface_statistics() == [len(hits), len(hits), 0, 0]      # the last call's
        fine = (got["flags"] & st.DEGENERATE) == 0
        length = np.linalg.norm(got["geometric_normal"][fine].astype(np.float64), axis=1)
        assert np.abs(length - 1).max() < 4e-7
        ok, _, unit, area = st.geometry64(scene, hits)
        # against binary64: each component of the fp32 cross product is off by at most 3 * 2^-24 |e1| |e2|, so the direction by about that over
        # the product's length (a thin triangle loses digits); 2^-21 leaves room for the three components and the normalisation
        _, _, e1, e2 = st.records(scene, hits)
        tol = 2.0 ** -21 * np.linalg.norm(e1.astype(np.float64), axis=1) * np.linalg.norm(e2.astype(np.float64), axis=1) / np.where(area > 0, area, 1.0) + 1e-6
        assert (np.abs(got["geometric_normal"][fine] - unit[fine]).max(1) <= tol[fine]).all()
    soup = cases["soup"][3]
    # the soup's records without area: every 20th triangle of 80 per primitive, of three kinds in turn; two equal corners and three equal
    # corners have no area in any arithmetic (a midpoint corner need not, once rounded and transformed): 2 or 3 of each primitive's 4
    assert ((soup["flags"] & st.DEGENERATE) != 0).sum() >= 5 * 10


def test_corners_are_the_oracles_records(cases, oracle):
    for name, (scene, c, hits, got) in cases.items():
        rec, prim = oracle.Scene(scene).triangles()
        assert len(rec) * 5 == len(hits) and np.array_equal(np.repeat(prim, 5), hits["geometry_index"])
        p = got["position"].reshape(len(rec), 5, 3)
        assert np.array_equal(p[:, 2], rec[:, 0]), name                                # (u, v) = (0, 0): v0
        assert np.array_equal(p[:, 3], rec[:, 0] + rec[:, 1]), name                    # (1, 0): fl(v0 + e1)
        assert np.array_equal(p[:, 4], rec[:, 0] + rec[:, 2]), name                    # (0, 1): fl(v0 + e2)


def test_unresolved_hits_are_all_zero(cases):
    scene, c, _, _ = cases["soup"]
    n_prims = len(scene.primitives)
    tris = int(scene.primitives["index_count"][1]) // 3
    prim = np.array([MISS, 1, MISS, n_prims, 0xFFFFFFFE, 1, 1, 1, 1, 1, 1, 1], np.uint32)
    tri = np.array([0, MISS, MISS, 0, 0, tris, 0xFFFFFFFE, 0, 0, 0, 0, tris - 1], np.uint32)
    u = np.array([0.2] * 7 + [np.nan, np.inf, 0.2, 0.2, 0.2], np.float32)
    v = np.array([0.3] * 7 + [0.3, 0.3, -np.inf, np.nan, 0.3], np.float32)
    hits = st.hits_of(prim, tri, u, v)
    hits["t"], hits["reserved"] = np.nan, 0xDEADBEEF                                   # neither is read
    got = c.resolve_hits(hits)
    assert not got[:-1].view(np.uint8).any()
    assert got["flags"][-1] == st.VALID and not st.same_bits(got, st.resolve(scene, hits))
    assert c.surface_statistics() == [len(hits), 1, 0, 0]
    # t and reserved do not matter
    plain = hits.copy()
    plain["t"], plain["reserved"] = 0, 0
    assert not st.same_bits(c.resolve_hits(plain), got)


def test_degenerate_records_say_so(cases):
    scene, c, hits, got = cases["soup"]
    _, _, _, area = st.geometry64(scene, hits)
    flat = area == 0
    assert flat.sum() >= 5 * 10
    assert ((got["flags"][flat] & st.DEGENERATE) != 0).all() and not got["geometric_normal"][flat].any() and np.isfinite(got["position"][flat]).all()
    assert ((got["flags"][area > 1e-12] & st.DEGENERATE) == 0).all()
    # products that underflow: edges of 1e-12 have a cross product of 1e-24, whose square is 0 in fp32
    import dataclasses
    tiny = dataclasses.replace(scene, vertices=scene.vertices.copy(), primitives=scene.primitives.copy())
    tiny.vertices["pos"] *= np.float32(1e-12)
    tiny.primitives["transform"][:, 12:15] = 0
    t = _host(tiny)
    try:
        small = t.resolve_hits(hits)
        assert ((small["flags"] & st.DEGENERATE) != 0).mean() > 0.9 and not st.same_bits(small, st.resolve(tiny, hits))
        assert not small["geometric_normal"][(small["flags"] & st.DEGENERATE) != 0].any()
    finally:
        t.close()


def test_position_lies_within_the_bound_of_the_binary64_value(cases):
    worst = 0.0
    for name, (scene, c, hits, got) in cases.items():
        ok, truth, _, _ = st.geometry64(scene, hits)
        ratio = (np.abs(got["position"].astype(np.float64) - truth) / st.position_bound(scene, hits)).max()
        print(f"{name}: {len(hits)} hits, largest |position - binary64| / bound = {ratio:.4f}")
        assert ok.all() and not st.position_violations(scene, hits, got).any(), name
        worst = max(worst, ratio)
    assert worst <= 1.0


def test_a_planted_error_of_four_bounds_is_caught(cases):
    for name, (scene, c, hits, got) in cases.items():
        b = st.position_bound(scene, hits)
        for axis in range(3):
            k = np.arange(axis, len(hits), 7)
            for sign in (1.0, -1.0):
                planted = got.copy()
                planted["position"][k, axis] = (got["position"][k, axis].astype(np.float64) + sign * 4 * b[k, axis]).astype(np.float32)
                moved = np.abs(planted["position"][k, axis].astype(np.float64) - got["position"][k, axis]) >= 3.5 * b[k, axis]
                assert moved.sum() > 50, (name, axis)
                bad = st.position_violations(scene, hits, planted)
                assert bad[k[moved]].all(), f"{name}: a planted error of {sign * 4:+g} bounds on axis {axis} passed"
                assert not np.delete(bad, k).any()


def test_mirroring_a_primitive_negates_its_geometric_normal(cases):
    import dataclasses
    base = rt.soup_scene(SOUP_SEED)
    hits = cases["soup"][2]
    plain = _host(base)
    try:
        a = plain.resolve_hits(hits)
        assert not plain.primitive_facing_flips().any()
        # the mirror of fc.mirror_transform moves the world geometry, so compare like with like: a primitive whose transform AND vertices are
        # mirrored in x keeps every world position bit for bit, and only its flip byte -- hence its normal's sign -- changes
        p = base.primitives.copy()
        v = base.vertices.copy()
        pick = [1, 3]
        for k in pick:
            p["transform"][k] = fc.mirror_transform(p["transform"][k])
            lo = int(p["vertex_offset"][k])
            hi = int(p["vertex_offset"][k + 1]) if k + 1 < len(p) else len(v)
            v["pos"][lo:hi, 0] = -v["pos"][lo:hi, 0]
        m = _host(dataclasses.replace(base, primitives=p, vertices=v))
        try:
            flips = m.primitive_facing_flips()
            assert flips.tolist() == [1 if k in pick else 0 for k in range(len(p))]
            b = m.resolve_hits(hits)
            mirrored = np.isin(hits["geometry_index"], pick)
            assert np.array_equal(a["position"], b["position"]) and np.array_equal(a["flags"], b["flags"])
            assert np.array_equal(b["geometric_normal"][~mirrored], a["geometric_normal"][~mirrored])
            fine = mirrored & ((a["flags"] & st.DEGENERATE) == 0)
            assert fine.sum() > 100 and np.array_equal(b["geometric_normal"][fine], -a["geometric_normal"][fine])
        finally:
            m.close()
    finally:
        plain.close()


FACADE = '''#include "vhr_render_graph.hpp"
#include <vector>
void pick_then_shade(vhr::DeviceContext &dc, const std::vector<vhr_ray> &rays, std::vector<vhr_ray_hit> &hits, vhr_surface_point *points) {
    vhr::ResourceManager rm(dc);
    rm.QueryRays(rays.data(), uint32_t(rays.size()), VHR_RAY_QUERY_HOST_MEMORY, hits.data());
    rm.ResolveHits(hits.data(), uint32_t(hits.size()), VHR_SURFACE_MATERIAL | VHR_SURFACE_HOST_MEMORY, points);
}
'''
C_VIEW = '''#include "vhr_amd.h"
int f(vhr_context *c, const vhr_ray_hit *h, vhr_surface_point *p, uint64_t s[4], uint32_t l[8]) {
    vhr_surface_point q = { { 0.0f, 1.0f, 2.0f }, VHR_SURFACE_VALID | VHR_SURFACE_DEGENERATE | VHR_SURFACE_NO_SHADING_NORMAL | VHR_SURFACE_NORMAL_MAPPED | VHR_SURFACE_DISCARDED };
    (void)q;
    return vhr_resolve_hits(c, h, 1, VHR_SURFACE_MATERIAL | VHR_SURFACE_HOST_MEMORY, p) + vhr_get_surface_statistics(c, s) + vhr_surface_point_layout(l);
}
'''


def test_facade_and_c_view_compile(tmp_path):
    cxx, cc = shutil.which("g++") or shutil.which("c++"), shutil.which("gcc") or shutil.which("cc")
    if not cxx or not cc:
        pytest.skip("no compiler")
    src = tmp_path / "resolve_hits.cpp"
    src.write_text(FACADE)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    csrc = tmp_path / "resolve_hits.c"
    csrc.write_text(C_VIEW)
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(csrc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
