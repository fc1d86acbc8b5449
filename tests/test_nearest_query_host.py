"""vhr_nearest_points_query without a GPU: the constant and the exports, every refusal of the argument checks on a host-only context and --
by calls with two faults -- their order, and the brute force the GPU tests judge by (tests/nearest_truth.py): at k = 1 it is the closest-point
query's brute force, and equal d2 are placed by flat index."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import nearest_truth as nt
from tests.test_gpu_fuzz import soup
from tests.test_gpu_point_query import brute_force, flat_to_ids, queries_for
from vulkanhybridrenderer_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, NO_DEVICE = 0, -1, -6          # include/vhr_amd.h
WHO = "vhr_nearest_points_query"


@pytest.fixture(scope="module")
def host_ctx():
    c = lib.Context(64, 64, host_only=True)
    yield c
    c.close()


def _raw(c, points, count, k, flags, cull_mask, results):
    rc = c.L.vhr_nearest_points_query(c.handle, points, count, k, flags, cull_mask, results)
    return rc, c.L.vhr_last_error(c.handle).decode()


def test_constant_and_exports():
    assert abi.NEAREST_MAX_K == 16
    text = open(os.path.join(ROOT, "include", "vhr_amd.h")).read()
    types = open(os.path.join(ROOT, "include", "vhr_types.h")).read()
    assert "#define VHR_NEAREST_MAX_K 16u" in types
    for name in ("vhr_nearest_points_query", "vhr_get_nearest_query_statistics"):
        assert name in lib.EXPORTS and f"int {name}(" in text and hasattr(lib.load(), name)


def test_every_refusal_and_the_order_of_the_checks(host_ctx):
    c = host_ctx
    pts, out = lib.Context._points_array(np.zeros((4, 4), np.float32)), np.zeros((4, 16), abi.ray_hit_dtype)
    P, R = pts.ctypes.data, out.ctypes.data
    assert P % 16 == 0 and R % 4 == 0
    assert c.L.vhr_nearest_points_query(None, P, 4, 1, 0, 0xFF, R) == INVALID_ARGUMENT                    # a NULL context

    def refused(what, *args):
        rc, msg = _raw(c, *args)
        assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and what in msg, (what, args, rc, msg)

    # 1. NULL with count > 0 -- before everything that follows, all of it wrong as well
    for points, results in ((None, R), (P, None), (None, None)):
        refused("NULL", points, 4, 1, 0, 0xFF, results)
    refused("NULL", None, 4, 0, 4, 0x1FF, None)
    # 2. unknown flag bits; VHR_POINT_QUERY_ANY_WITHIN is one here
    for flags in (abi.POINT_QUERY_ANY_WITHIN, abi.POINT_QUERY_ANY_WITHIN | abi.POINT_QUERY_HOST_MEMORY, 4, 8, 0x80000000):
        refused("unknown flag", P, 4, 1, flags, 0xFF, R)
        refused("unknown flag", P + 8, 4, 17, flags, 0x1FF, R + 2)
    # 3. the points' alignment
    refused("points must be 16-byte aligned", P + 8, 4, 1, 0, 0xFF, R)
    refused("points must be 16-byte aligned", P + 8, 4, 0, 2, 0x1FF, R + 2)
    # 4. the results'
    refused("results must be 4-byte aligned", P, 4, 1, 0, 0xFF, R + 2)
    refused("results must be 4-byte aligned", P, 4, 17, 2, 0x1FF, R + 2)
    # 5. the cull mask
    for bad in (256, 0x1FF, 0xFFFFFFFF):
        refused("cull_mask", P, 4, 1, 2, bad, R)
        refused("cull_mask", P, 4, 0, 0, bad, R)
        assert "0xFF" in _raw(c, P, 4, 17, 0, bad, R)[1]
    # 6. k
    for k in (0, 17, 18, 0xFFFFFFFF):
        refused(f"k {k} ", P, 4, k, 0, 0xFF, R)
        refused("VHR_NEAREST_MAX_K", P, 4, k, 2, 0, R)
        refused(f"k {k} ", None, 0, k, 0, 0xFF, None)                                                      # ... also of an empty call
    # behind the argument checks: a host-only context has no device.  Every k of the range, both values of the flag, any cull mask pass; so
    # does an empty call, whose pointers are not looked at
    for k in (1, 2, 15, 16):
        for points, count, flags, cull, results in ((P, 4, 0, 0xFF, R), (P, 4, 2, 0, R), (P, 4, 2, 0x03, R), (None, 0, 0, 0xFF, None), (None, 0, 2, 0, None), (P + 8, 0, 0, 0xFF, R + 2)):
            rc, msg = _raw(c, points, count, k, flags, cull, results)
            assert rc == NO_DEVICE and "host-only" in msg and msg.startswith(WHO + ":"), (k, rc, msg)
    with pytest.raises(lib.VhrError, match="vhr_nearest_points_query: host-only"):
        c.nearest_points_query(np.zeros((3, 4), np.float32), 4)
    with pytest.raises(lib.VhrError, match="vhr_nearest_points_query: host-only"):
        c.nearest_points_query_device(0x10000, 1, 16, 0x20000)
    with pytest.raises(lib.VhrError, match="vhr_nearest_points_query: k 0 "):
        c.nearest_points_query(np.zeros((3, 4), np.float32), 0)
    with pytest.raises(lib.VhrError, match="vhr_nearest_points_query: k 17 "):
        c.nearest_points_query(np.zeros((3, 4), np.float32), 17)
    with pytest.raises(lib.VhrError, match="cull_mask"):
        c.nearest_points_query_device(0x10000, 1, 4, 0x20000, cull_mask=300)
    assert c.nearest_query_statistics() == [0, 0, 0, 0]
    assert c.L.vhr_get_nearest_query_statistics(None, None) == INVALID_ARGUMENT and c.L.vhr_get_nearest_query_statistics(c.handle, None) == INVALID_ARGUMENT


def test_the_truth_at_k_1_is_the_closest_point_querys_brute_force(host_ctx):
    """256 queries of the 1 500-triangle soup; the records are a host-only context's own (it keeps the arrays a device context would build from)."""
    scene = soup(5, 1500, 6)
    c = lib.Context(64, 64, host_only=True)
    try:
        c.upload_scene(scene)
        records = c.triangle_records()
    finally:
        c.close()
    assert len(records) == scene.triangle_count >= 1500
    queries = queries_for(records, n=256)
    geometry, primitive = flat_to_ids(scene)
    matrix = nt.distance_matrix(host_ctx, records, queries)
    want, exists = brute_force(host_ctx, scene, records, queries)
    assert 0.3 < exists.mean() < 0.9
    got, entries = nt.nearest(matrix, geometry, primitive, queries, 1)
    assert got.shape == (256, 1) and np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32)) and np.array_equal(entries == 1, exists)
    # a longer list starts with the shorter one, never repeats a triangle and ascends in t
    long, n_long = nt.nearest(matrix, geometry, primitive, queries, 16)
    assert np.array_equal(long[:, :1], got) and (n_long >= entries).all() and n_long.max() == 16
    mid, n_mid = nt.nearest(matrix, geometry, primitive, queries, 5)
    assert np.array_equal(long[:, :5], mid) and np.array_equal(n_mid, np.minimum(n_long, 5))
    for q in range(256):
        ids = [(int(e["geometry_index"]), int(e["primitive_index"])) for e in long[q, :n_long[q]]]
        assert len(set(ids)) == len(ids) and (np.diff(long[q, :n_long[q]]["t"]) >= 0).all()
        assert (long[q, n_long[q]:]["geometry_index"] == nt.MISS).all() and not long[q, n_long[q]:].view(np.uint32).reshape(-1, 6)[:, [0, 1, 2, 5]].any()
    # a cull mask takes records out of the candidates
    visible = geometry % 2 == 0
    masked, n_masked = nt.nearest(matrix, geometry, primitive, queries, 16, visible)
    assert (masked["geometry_index"][masked["geometry_index"] != nt.MISS] % 2 == 0).all() and (n_masked <= n_long).all() and n_masked.sum() > 0


def test_the_truth_places_equal_d2_by_flat_index(host_ctx):
    """Five copies of one triangle among others, at flat indices 1, 3, 4, 6, 8: one d2, bit for bit, and the list names them in that order."""
    tri = np.float32([0, 0, 0, 1, 0, 0, 0, 0, 1])
    far, nearer = np.float32([0, -3, 0, 1, 0, 0, 0, 0, 1]), np.float32([0.1, 0.25, 0.1, 0.5, 0, 0, 0, 0, 0.5])
    records = np.stack([far, tri, nearer, tri, tri, far, tri, far, tri])
    queries = np.float32([[0.25, 0.5, 0.25, np.inf], [0.25, 0.5, 0.25, 0.6], [0.25, 0.5, 0.25, 0.3], [5, 5, 5, -1.0], [np.nan, 0, 0, np.inf]])
    geometry, primitive = np.zeros(9, np.uint32), np.arange(9, dtype=np.uint32)
    matrix = nt.distance_matrix(host_ctx, records, queries)
    assert len(np.unique(matrix[0, [1, 3, 4, 6, 8], 0])) == 1 and matrix[0, 2, 0] < matrix[0, 1, 0] < matrix[0, 0, 0]
    got, entries = nt.nearest(matrix, geometry, primitive, queries, 4)
    assert entries.tolist() == [4, 4, 1, 0, 0]
    assert got["primitive_index"][0].tolist() == [2, 1, 3, 4] and got["primitive_index"][1].tolist() == [2, 1, 3, 4]
    assert got["primitive_index"][2].tolist() == [2, nt.MISS, nt.MISS, nt.MISS]
    assert got["t"][0].tolist() == [np.float32(0.25), 0.5, 0.5, 0.5]
    got, entries = nt.nearest(matrix, geometry, primitive, queries, 16)
    assert entries.tolist() == [9, 6, 1, 0, 0] and got["primitive_index"][0, :9].tolist() == [2, 1, 3, 4, 6, 8, 0, 5, 7]
    assert (got["primitive_index"][0, 9:] == nt.MISS).all() and (got["geometry_index"][0, 9:] == nt.MISS).all()


FACADE = '''#include "vhr_render_graph.hpp"
#include <vector>
static_assert(VHR_NEAREST_MAX_K == 16u, "VHR_NEAREST_MAX_K");
void probes(vhr::DeviceContext &dc, const std::vector<vhr_point_query> &points, std::vector<vhr_ray_hit> &lists) {
    vhr::ResourceManager rm(dc);
    rm.QueryNearestPoints(points.data(), uint32_t(points.size()), 4u, VHR_POINT_QUERY_HOST_MEMORY, lists.data());
    rm.QueryNearestPoints(points.data(), uint32_t(points.size()), VHR_NEAREST_MAX_K, 0u, lists.data(), 0x02);
}
'''
C_VIEW = '''#include "vhr_amd.h"
int f(vhr_context *c, const vhr_point_query *p, vhr_ray_hit *h, uint64_t s[4]) {
    return vhr_nearest_points_query(c, p, 1, VHR_NEAREST_MAX_K, VHR_POINT_QUERY_HOST_MEMORY, 0xFFu, h) + vhr_get_nearest_query_statistics(c, s);
}
'''


def test_facade_and_c_view_compile(tmp_path):
    cxx, cc = shutil.which("g++") or shutil.which("c++"), shutil.which("gcc") or shutil.which("cc")
    if not cxx or not cc:
        pytest.skip("no compiler")
    src = tmp_path / "nearest_points.cpp"
    src.write_text(FACADE)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    csrc = tmp_path / "nearest_points.c"
    csrc.write_text(C_VIEW)
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(csrc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
