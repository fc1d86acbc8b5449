"""Which check wins when a vhr_occlusion_query call has two faults at once, in the manner of tests/test_query_validation_order.py: every adjacent
pair of its seven argument checks -- NULL context, NULL pointer, unknown flag, `points` alignment, `occluded` alignment, cull_mask, samples -- as
raw ctypes calls on a host-only context, on which "host-only" is itself the last fault of every row.  The expected codes and message fragments
are literals.  With them: count == 0, vhr_debug_occlusion_rays' own checks, and the statistics getter before any call."""
import ctypes as C

import numpy as np
import pytest

from tests import ray_truth as rt
from vulkanhybridrenderer_amd import lib

OK, INVALID_ARGUMENT, NO_DEVICE = 0, -1, -6                      # include/vhr_amd.h
BAD = 0x80000000                                                 # a flag bit no entry point knows
N = 4
SEED = 5


@pytest.fixture(scope="module")
def host():
    """A host-only context with geometry, and the addresses of two buffers that satisfy every alignment: A (points), B (masks)."""
    scene = rt.soup_scene(1)
    c = lib.Context(64, 64, host_only=True)
    c.update_geometry(scene.vertices, scene.indices, scene.primitives)
    keep = [np.zeros(1024, np.uint8) for _ in range(2)]
    a, b = (k.ctypes.data + (-k.ctypes.data % 16) for k in keep)
    yield c, a, b
    c.close()
    del keep


def rows(A, B):
    """(arguments behind the context: points, count, samples, seed, flags, cull_mask, occluded; return code; what vhr_last_error must contain)."""
    return [
        # NULL pointer before the flags
        ((None, N, 0, SEED, BAD, 0x100, None), INVALID_ARGUMENT, "points and occluded must not be NULL when count > 0"),
        ((A + 8, N, 0, SEED, BAD, 0x100, None), INVALID_ARGUMENT, "points and occluded must not be NULL when count > 0"),
        ((None, N, 8, SEED, 2, 0xFF, B), INVALID_ARGUMENT, "points and occluded must not be NULL when count > 0"),
        # the flags before the points' alignment
        ((A + 8, N, 0, SEED, BAD, 0x100, B + 4), INVALID_ARGUMENT, "unknown flag bits 2147483648"),
        ((A + 8, N, 8, SEED, 16, 0xFF, B), INVALID_ARGUMENT, "unknown flag bits 16"),          # VHR_RAY_QUERY_ALPHA_TEST's bit: out of scope
        ((A, N, 8, SEED, 1, 0xFF, B), INVALID_ARGUMENT, "unknown flag bits 1"),
        ((None, 0, 8, SEED, 4, 0xFF, None), INVALID_ARGUMENT, "unknown flag bits 4"),
        # the points' alignment before the masks'
        ((A + 8, N, 0, SEED, 2, 0x100, B + 4), INVALID_ARGUMENT, "points must be 16-byte aligned"),
        ((A + 4, N, 8, SEED, 0, 0xFF, B), INVALID_ARGUMENT, "points must be 16-byte aligned"),
        # the masks' alignment before cull_mask
        ((A, N, 0, SEED, 2, 0x100, B + 4), INVALID_ARGUMENT, "occluded must be 8-byte aligned"),
        ((A, N, 8, SEED, 2, 0xFF, B + 1), INVALID_ARGUMENT, "occluded must be 8-byte aligned"),
        # cull_mask before samples
        ((A, N, 0, SEED, 2, 0x100, B), INVALID_ARGUMENT, "cull_mask 256 exceeds 0xFF"),
        ((A, N, 65, SEED, 2, 0xFFFFFFFF, B + 8), INVALID_ARGUMENT, "cull_mask 4294967295 exceeds 0xFF"),
        ((None, 0, 0, SEED, 0, 0x100, None), INVALID_ARGUMENT, "cull_mask 256 exceeds 0xFF"),
        # samples before the context
        ((A, N, 0, SEED, 2, 0xFF, B), INVALID_ARGUMENT, "samples 0 is not in 1 .. VHR_OCCLUSION_MAX_SAMPLES (64)"),
        ((A, N, 65, SEED, 2, 0xFF, B), INVALID_ARGUMENT, "samples 65 is not in 1 .. VHR_OCCLUSION_MAX_SAMPLES (64)"),
        ((A, N, 0xFFFFFFFF, SEED, 0, 0, B), INVALID_ARGUMENT, "samples 4294967295 is not in 1 .. VHR_OCCLUSION_MAX_SAMPLES (64)"),
        ((None, 0, 0, SEED, 0, 0xFF, None), INVALID_ARGUMENT, "samples 0 is not in"),
        # nothing wrong with the arguments: the context has no device
        ((A, N, 1, SEED, 2, 0xFF, B), NO_DEVICE, "vhr_occlusion_query: host-only context: no device work"),
        ((A, N, 64, SEED, 0, 0, B + 8), NO_DEVICE, "host-only context: no device work"),
        # count == 0 asks nothing of the pointers, and is answered behind the context
        ((None, 0, 8, SEED, 0, 0xFF, None), NO_DEVICE, "host-only context: no device work"),
        ((A + 8, 0, 8, SEED, 2, 0xFF, B + 4), NO_DEVICE, "host-only context: no device work"),
    ]


def test_the_winning_check_of_every_adjacent_pair(host):
    c, A, B = host
    table = rows(A, B)
    wrong = []
    for args, want_rc, want in table:
        rc = c.L.vhr_occlusion_query(c.handle, *args)
        msg = c.L.vhr_last_error(c.handle).decode()
        if rc != want_rc or want not in msg or not msg.startswith("vhr_occlusion_query:"):
            wrong.append(f"vhr_occlusion_query{args}: got {rc} {msg!r}, want {want_rc} {want!r}")
    assert not wrong, "\n".join(wrong)
    assert {r[1] for r in table} == {INVALID_ARGUMENT, NO_DEVICE}
    # a NULL context has no error to keep: the bare code, whatever else is wrong
    assert c.L.vhr_occlusion_query(None, A, N, 8, SEED, 2, 0xFF, B) == INVALID_ARGUMENT
    assert c.L.vhr_occlusion_query(None, None, N, 0, SEED, BAD, 0x100, None) == INVALID_ARGUMENT
    assert c.occlusion_statistics() == [0, 0, 0, 0]                  # a refused query is no query


def test_the_python_wrapper_reports_the_same_faults(host):
    c = host[0]
    pts = np.zeros((N, 8), np.float32)
    with pytest.raises(lib.VhrError, match="samples 65"):
        c.occlusion_query(pts, 65)
    with pytest.raises(lib.VhrError, match="cull_mask 256"):
        c.occlusion_query(pts, 8, cull_mask=0x100)
    with pytest.raises(lib.VhrError, match="host-only context"):
        c.occlusion_query(pts, 8)
    with pytest.raises(lib.VhrError, match="host-only context"):
        c.occlusion_query(pts[:0], 8)


def test_the_debug_entry_points_checks(host):
    c, A, B = host
    L = c.L
    assert L.vhr_debug_occlusion_rays(None, A, N, 4, SEED, B) == INVALID_ARGUMENT
    for args, want in (((None, N, 4, SEED, B), "vhr_debug_occlusion_rays: null argument"), ((A, N, 4, SEED, None), "vhr_debug_occlusion_rays: null argument"),
                       ((A, N, 0, SEED, B), "vhr_debug_occlusion_rays: samples 0 is not in 1 .. VHR_OCCLUSION_MAX_SAMPLES (64)"),
                       ((A, N, 65, SEED, B), "vhr_debug_occlusion_rays: samples 65 is not in")):
        assert L.vhr_debug_occlusion_rays(c.handle, *args) == INVALID_ARGUMENT and want in L.vhr_last_error(c.handle).decode(), args
    assert L.vhr_debug_occlusion_rays(c.handle, None, 0, 4, SEED, None) == OK
    assert L.vhr_debug_occlusion_rays(c.handle, A, N, 4, SEED, B) == OK       # N * 4 rays of 32 bytes: 512 of B's 1008


def test_statistics_before_any_call():
    fresh = lib.Context(64, 64, host_only=True)
    try:
        out = (C.c_uint64 * 4)(7, 7, 7, 7)
        assert fresh.L.vhr_get_occlusion_statistics(fresh.handle, out) == OK and list(out) == [0, 0, 0, 0]
        assert fresh.L.vhr_get_occlusion_statistics(fresh.handle, None) == INVALID_ARGUMENT
        assert fresh.L.vhr_get_occlusion_statistics(None, out) == INVALID_ARGUMENT
        assert fresh.occlusion_statistics() == [0, 0, 0, 0]
    finally:
        fresh.close()
