"""vhr_closest_point_query without a GPU: the layout of vhr_point_query, the argument checks on a host-only context, the C++ facade and the C
view of the types, and the query's point / triangle function -- vhr_debug_point_triangle runs the HOST's copy of csrc/closest_point.hpp on a
host-only context -- against the binary64 truth and the error bound of tests/point_truth.py.

Measured (the host's copy over point_truth.pair_sets(), 20 100 pairs): the largest |d2 - D^2| / bound is 0.126 (bound = 24 * 2^-24 * (A + E)^2)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import point_truth as pt
from vulkanhybridrenderer_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NO_DEVICE = -1, -6          # include/vhr_amd.h
WHO = "vhr_closest_point_query"


@pytest.fixture(scope="module")
def host_ctx():
    c = lib.Context(64, 64, host_only=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_outputs(host_ctx):
    """name -> (pairs, the host function's (d2, u, v)): computed once, left unchanged."""
    return {name: (pairs, host_ctx.debug_point_triangle(pairs)) for name, pairs in pt.pair_sets().items()}


def _err(c):
    return c.L.vhr_last_error(c.handle).decode()


def test_layout_and_exports():
    assert abi.point_query_dtype.itemsize == 16 and abi.point_query_dtype.fields["max_distance"][1] == 12 and abi.point_query_dtype.fields["point"][1] == 0
    assert (abi.POINT_QUERY_ANY_WITHIN, abi.POINT_QUERY_HOST_MEMORY) == (1, 2)
    text = open(os.path.join(ROOT, "include", "vhr_amd.h")).read()
    types = open(os.path.join(ROOT, "include", "vhr_types.h")).read()
    for name in ("vhr_closest_point_query", "vhr_get_point_query_statistics", "vhr_debug_point_triangle"):
        assert name in lib.EXPORTS and f"int {name}(" in text and hasattr(lib.load(), name)
    assert "sizeof(vhr_point_query) == 16 && offsetof(vhr_point_query, max_distance) == 12" in types
    assert "#define VHR_POINT_QUERY_ANY_WITHIN   1u" in types and "#define VHR_POINT_QUERY_HOST_MEMORY  2u" in types
    # the binding builds the records the header describes, 16-byte aligned whatever it is given
    raw = np.zeros(4 * 5 + 1, np.float32)[1:].reshape(5, 4)
    raw[:] = np.arange(20).reshape(5, 4)
    a = lib.Context._points_array(raw)
    assert a.dtype == abi.point_query_dtype and a.ctypes.data % 16 == 0 and a["max_distance"].tolist() == [3, 7, 11, 15, 19] and a["point"][2].tolist() == [8, 9, 10]
    with pytest.raises(ValueError):
        lib.Context._points_array(np.zeros((3, 8), np.float32))
    with pytest.raises(TypeError):
        lib.Context._points_array(np.zeros((3, 4), np.float64))


def _raw(c, points, count, flags, cull_mask, results):
    rc = c.L.vhr_closest_point_query(c.handle, points, count, flags, cull_mask, results)
    return rc, _err(c)


def test_validation_order_and_messages(host_ctx):
    c = host_ctx
    pts, out = lib.Context._points_array(np.zeros((4, 4), np.float32)), np.zeros(4, abi.ray_hit_dtype)
    P, R = pts.ctypes.data, out.ctypes.data
    assert P % 16 == 0 and R % 4 == 0
    assert c.L.vhr_closest_point_query(None, P, 4, 0, 0xFF, R) == INVALID_ARGUMENT                      # a NULL context
    for points, results in ((None, R), (P, None), (None, None)):
        rc, msg = _raw(c, points, 4, 0, 0xFF, results)
        assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "NULL" in msg, (rc, msg)
    rc, msg = _raw(c, None, 4, 4, 0x1FF, None)                                                            # NULL comes first
    assert rc == INVALID_ARGUMENT and "NULL" in msg
    for flags in (4, 8, 0x80000000, 1 | 4, 2 | 8):
        rc, msg = _raw(c, P + 8, 4, flags, 0x1FF, R + 2)                                                  # ... then the flags
        assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "unknown flag" in msg, (flags, rc, msg)
    rc, msg = _raw(c, P + 8, 4, 0, 0x1FF, R + 2)                                                          # ... then the points' alignment
    assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "points must be 16-byte aligned" in msg, (rc, msg)
    rc, msg = _raw(c, P, 4, 0, 0x1FF, R + 2)                                                              # ... then the results'
    assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "results must be 4-byte aligned" in msg, (rc, msg)
    for bad in (256, 0x1FF, 0xFFFFFFFF):                                                                  # ... then the cull mask
        rc, msg = _raw(c, P, 4, 2, bad, R)
        assert rc == INVALID_ARGUMENT and msg.startswith(WHO + ":") and "cull_mask" in msg and "0xFF" in msg, (bad, rc, msg)
    # after validation: a host-only context has no device; both flags pass, NULL pointers with count == 0 pass
    for points, count, flags, cull, results in ((P, 4, 0, 0xFF, R), (P, 4, 1, 0, R), (P, 4, 2, 0x03, R), (P, 4, 3, 0xFF, R), (None, 0, 0, 0xFF, None), (None, 0, 3, 0, None)):
        rc, msg = _raw(c, points, count, flags, cull, results)
        assert rc == NO_DEVICE and "host-only" in msg and msg.startswith(WHO + ":"), (rc, msg)
    with pytest.raises(lib.VhrError, match="vhr_closest_point_query: host-only"):
        c.closest_point_query(np.zeros((3, 4), np.float32))
    with pytest.raises(lib.VhrError, match="vhr_closest_point_query: host-only"):
        c.closest_point_query_device(0x10000, 1, 0x20000, any_within=True)
    with pytest.raises(lib.VhrError, match="cull_mask"):
        c.closest_point_query_device(0x10000, 1, 0x20000, cull_mask=300)
    assert c.point_query_statistics() == [0, 0, 0, 0]
    # vhr_debug_point_triangle's own checks
    assert c.L.vhr_debug_point_triangle(None, None, 0, None) == INVALID_ARGUMENT
    assert c.L.vhr_debug_point_triangle(c.handle, None, 3, None) == INVALID_ARGUMENT and "vhr_debug_point_triangle" in _err(c)
    assert c.L.vhr_debug_point_triangle(c.handle, None, 0, None) == 0 and c.debug_point_triangle(np.zeros((0, 12), np.float32)).shape == (0, 3)


def test_the_random_pairs_cover_all_seven_regions():
    for scale in pt.SCALES:
        _, _, _, region = pt.truth(pt.scaled(pt.random_pairs(), scale))
        counts = np.bincount(region, minlength=7)
        assert (counts >= 40).all(), dict(zip(pt.REGIONS, counts.tolist()))
    _, _, _, region = pt.truth(pt.boundary_pairs())
    assert (np.bincount(region, minlength=7)[1:] >= 40).all()


def test_the_truth_knows_simple_cases():
    tri = [0, 0, 0, 1, 0, 0, 0, 1, 0]                       # A = origin, B = (1, 0, 0), C = (0, 1, 0)
    pairs = np.array([[0.25, 0.25, 2] + tri, [-1, -1, 0] + tri, [2, -1, 0] + tri, [-1, 3, 0] + tri, [0.5, -2, 0] + tri, [-2, 0.5, 0] + tri, [1, 1, 1] + tri], np.float32)
    D2, u, v, region = pt.truth(pairs)
    assert D2.tolist() == [4, 2, 2, 5, 4, 4, 1.5] and region.tolist() == [0, 4, 5, 6, 1, 2, 3]
    assert u.tolist() == [0.25, 0, 1, 0, 0.5, 0, 0.5] and v.tolist() == [0.25, 0, 0, 1, 0, 0.5, 0.5]
    assert pt.inside_unit_triangle(np.float32([0, 1, 0.5, 0.75, 1, 0.25]), np.float32([0, 0, 0.5, np.float32(0.25) + np.float32(2.0 ** -24), 2.0 ** -30, 0.25])).tolist() == \
        [True, True, True, False, False, True]


def test_d2_lies_within_the_bound_of_the_binary64_truth(host_outputs):
    worst = 0.0
    for name, (pairs, out) in host_outputs.items():
        assert np.isfinite(out).all(), name
        bad = pt.violations(pairs, out)
        r = pt.ratio(pairs, out)
        print(f"{name}: {len(pairs)} pairs, largest |d2 - D^2| / bound = {r:.4f}")
        assert not bad.any(), f"{name}: {int(bad.sum())} of {len(pairs)} pairs break the contract, first {np.nonzero(bad)[0][0]}"
        worst = max(worst, r)
    print(f"largest error-to-bound ratio over {sum(len(p) for p, _ in host_outputs.values())} pairs: {worst:.4f}")
    assert worst <= 1.0


def test_a_planted_error_of_four_bounds_is_caught(host_outputs):
    for name, (pairs, out) in host_outputs.items():
        b = pt.bound(pairs)
        k = np.nonzero(b > 0)[0][::7]
        k = k[np.float32(out[k, 0].astype(np.float64) + 4 * b[k]) != out[k, 0]]          # (where fp32 can hold the planted value)
        assert len(k) > 50, name
        for sign in (1.0, -1.0):
            planted = out.copy()
            planted[k, 0] = (out[k, 0].astype(np.float64) + sign * 4 * b[k]).astype(np.float32)
            moved = np.abs(planted[k, 0].astype(np.float64) - out[k, 0]) >= 3.5 * b[k]
            assert moved.sum() > 50, name
            bad = pt.violations(pairs, planted)
            assert bad[k[moved]].all(), f"{name}: a planted error of {sign * 4:+g} bounds passed"
            assert not np.delete(bad, k).any()


def test_scaling_by_a_power_of_two_scales_the_answer_exactly(host_outputs):
    """Every operation of the function commutes with a power of two (nothing here underflows): d2 scales by its square, (u, v) stay."""
    for base in ("random", "boundary", "duplicate", "plane_far"):
        _, one = host_outputs[f"{base} x 1"]
        for scale in (pt.SCALES[0], pt.SCALES[2]):
            _, other = host_outputs[f"{base} x {scale:g}"]
            assert np.array_equal(other[:, 0], one[:, 0] * np.float32(scale * scale)) and np.array_equal(other[:, 1:], one[:, 1:]), (base, scale)


def test_degenerate_and_non_finite_inputs(host_ctx):
    pairs, n_point = pt.special_pairs()
    out = host_ctx.debug_point_triangle(pairs)
    assert not np.isnan(out).any()
    assert np.isposinf(out[:n_point, 0]).all() and (out[:n_point, 1:] == 0).all()                        # a non-finite point: no candidate
    assert pt.inside_unit_triangle(out[:, 1], out[:, 2]).all()
    assert (out[:, 0] >= 0).all()
    # records without area: the distance to the segment or the point they are
    p = np.float32([3, 4, 0])
    point_record = np.concatenate([p, [0, 0, 0], [0, 0, 0], [0, 0, 0]]).astype(np.float32)
    segment = np.concatenate([p, [-1, 0, 0], [2, 0, 0], [8, 0, 0]]).astype(np.float32)                   # A = -1, B = 1, C = 7 on the x axis
    collinear_mid = np.concatenate([np.float32([0, 2, 0]), [-1, 0, 0], [2, 0, 0], [1, 0, 0]]).astype(np.float32)
    out = host_ctx.debug_point_triangle(np.stack([point_record, segment, collinear_mid]))
    assert out[:, 0].tolist() == [25.0, 16.0, 4.0] and pt.inside_unit_triangle(out[:, 1], out[:, 2]).all()
    q = -1 + out[1, 1] * 2 + out[1, 2] * 8
    assert q == 3.0


FACADE = '''#include "vhr_render_graph.hpp"
#include <vector>
void probes(vhr::DeviceContext &dc, const std::vector<vhr_point_query> &points, std::vector<vhr_ray_hit> &nearest, std::vector<uint8_t> &within) {
    vhr::ResourceManager rm(dc);
    rm.QueryClosestPoints(points.data(), uint32_t(points.size()), VHR_POINT_QUERY_HOST_MEMORY, nearest.data());
    rm.QueryClosestPoints(points.data(), uint32_t(points.size()), VHR_POINT_QUERY_ANY_WITHIN | VHR_POINT_QUERY_HOST_MEMORY, within.data(), 0x02);
}
'''
C_VIEW = '''#include "vhr_amd.h"
int f(vhr_context *c, const vhr_point_query *p, vhr_ray_hit *h, uint8_t *w, uint64_t s[4], const float *pairs, float *out) {
    vhr_point_query q = { { 0.0f, 1.0f, 2.0f }, 0.5f };
    (void)q;
    return vhr_closest_point_query(c, p, 1, 0, 0xFFu, h) + vhr_closest_point_query(c, p, 1, VHR_POINT_QUERY_ANY_WITHIN | VHR_POINT_QUERY_HOST_MEMORY, 1u, w) +
           vhr_get_point_query_statistics(c, s) + vhr_debug_point_triangle(c, pairs, 1, out);
}
'''


def test_facade_and_c_view_compile(tmp_path):
    cxx, cc = shutil.which("g++") or shutil.which("c++"), shutil.which("gcc") or shutil.which("cc")
    if not cxx or not cc:
        pytest.skip("no compiler")
    src = tmp_path / "closest_points.cpp"
    src.write_text(FACADE)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    csrc = tmp_path / "closest_points.c"
    csrc.write_text(C_VIEW)
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(csrc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
