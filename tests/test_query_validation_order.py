"""Which check wins when a query call has two faults at once: every pair of adjacent checks of vhr_ray_query, vhr_ray_query_masked,
vhr_ray_query_faces, vhr_closest_point_query and vhr_resolve_hits, as raw ctypes calls on a host-only context (on which "host-only" is itself
the last fault of every row).  The entry points do not share one order -- the ray queries test the flags before NULL, the other two NULL
before the flags; vhr_resolve_hits answers count == 0 before it looks at the context, the queries after -- and the order is behaviour a
caller can observe, so the expected return codes and messages stand here as literals, recorded from the library before the entry points came to
share their scaffold.  With them: the three debug pair entry points on NULL arguments and count == 0, and the three statistics getters
before any call."""
import ctypes as C

import numpy as np
import pytest

from tests import ray_truth as rt
from vulkanhybridrenderer_amd import abi, lib

OK, INVALID_ARGUMENT, DEVICE, NO_DEVICE = 0, -1, -2, -6          # include/vhr_amd.h
BAD = 0x80000000                                                 # a flag bit no entry point knows
N = 4


@pytest.fixture(scope="module")
def host():
    """A host-only context with geometry, and the addresses of buffers that satisfy every alignment: A (16 bytes, inputs), B (16 bytes,
    outputs), M (per-ray masks)."""
    scene = rt.soup_scene(1)
    c = lib.Context(64, 64, host_only=True)
    c.update_geometry(scene.vertices, scene.indices, scene.primitives)
    keep = [np.zeros(1024, np.uint8) for _ in range(3)]
    a, b, m = (k.ctypes.data + (-k.ctypes.data % 16) for k in keep)
    hits = np.frombuffer(keep[0], abi.ray_hit_dtype, N, offset=a - keep[0].ctypes.data)
    hits["geometry_index"], hits["u"], hits["v"] = 1, 0.25, 0.25
    yield c, a, b, m
    c.close()
    del keep


def rows(A, B, M):
    """(entry point, arguments behind the context, return code, what vhr_last_error must contain)."""
    rq, rm, rf, pq, rh = "vhr_ray_query", "vhr_ray_query_masked", "vhr_ray_query_faces", "vhr_closest_point_query", "vhr_resolve_hits"
    return [
        # vhr_ray_query: flags, NULL, rays' alignment, results' alignment, host-only
        (rq, (None, N, BAD, None), INVALID_ARGUMENT, "unknown flag bits 2147483648"),
        (rq, (A + 8, N, 4, B + 2), INVALID_ARGUMENT, "unknown flag bits 4"),
        (rq, (A + 8, N, 0, None), INVALID_ARGUMENT, "rays and results must not be NULL when count > 0"),
        (rq, (None, N, 2, B + 2), INVALID_ARGUMENT, "rays and results must not be NULL when count > 0"),
        (rq, (A + 8, N, 2, B + 2), INVALID_ARGUMENT, "rays must be 16-byte aligned"),
        (rq, (A, N, 2, B + 2), INVALID_ARGUMENT, "results must be 4-byte aligned"),
        (rq, (A, N, 2, B), NO_DEVICE, "vhr_ray_query: host-only context: no device work"),
        (rq, (A, 0, 2, B), NO_DEVICE, "vhr_ray_query: host-only context: no device work"),
        (rq, (None, 0, 0, None), NO_DEVICE, "vhr_ray_query: host-only context: no device work"),
        (rq, (A + 8, 0, 1, B + 2), NO_DEVICE, "host-only context"),
        (rq, (None, 0, 8, None), INVALID_ARGUMENT, "unknown flag bits 8"),
        # vhr_ray_query_masked: ..., results' alignment, cull_mask, host-only
        (rm, (None, N, BAD, 0x100, M, None), INVALID_ARGUMENT, "vhr_ray_query_masked: unknown flag bits"),
        (rm, (None, N, 2, 0x100, M, B), INVALID_ARGUMENT, "rays and results must not be NULL when count > 0"),
        (rm, (A + 8, N, 2, 0x100, M, B + 2), INVALID_ARGUMENT, "rays must be 16-byte aligned"),
        (rm, (A, N, 2, 0x100, M, B + 2), INVALID_ARGUMENT, "results must be 4-byte aligned"),
        (rm, (A, N, 2, 0x100, M, B), INVALID_ARGUMENT, "vhr_ray_query_masked: cull_mask 256 exceeds 0xFF"),
        (rm, (A, 0, 2, 0x100, None, B), INVALID_ARGUMENT, "cull_mask 256 exceeds 0xFF"),
        (rm, (A, N, 2, 0xFF, M, B), NO_DEVICE, "vhr_ray_query_masked: host-only context: no device work"),
        (rm, (A, N, 3, 0, None, B), NO_DEVICE, "host-only context"),
        (rm, (None, 0, 0, 0xFF, None, None), NO_DEVICE, "host-only context"),
        # vhr_ray_query_faces: ..., cull_mask, face_cull, host-only
        (rf, (None, N, BAD, 0x100, M, 3, None), INVALID_ARGUMENT, "vhr_ray_query_faces: unknown flag bits"),
        (rf, (A, N, 2, 0x100, M, 3, None), INVALID_ARGUMENT, "rays and results must not be NULL when count > 0"),
        (rf, (A + 4, N, 2, 0x100, M, 3, B + 1), INVALID_ARGUMENT, "rays must be 16-byte aligned"),
        (rf, (A, N, 2, 0x100, M, 3, B + 1), INVALID_ARGUMENT, "results must be 4-byte aligned"),
        (rf, (A, N, 2, 0x100, M, 3, B), INVALID_ARGUMENT, "vhr_ray_query_faces: cull_mask 256 exceeds 0xFF"),
        (rf, (A, N, 2, 0xFF, M, 3, B), INVALID_ARGUMENT, "face_cull 3 is none of VHR_FACE_CULL_NONE / BACK / FRONT"),
        (rf, (A, 0, 2, 0xFF, None, 0xFFFFFFFF, B), INVALID_ARGUMENT, "face_cull 4294967295 is none of"),
        (rf, (A, N, 2, 0xFF, M, 2, B), NO_DEVICE, "vhr_ray_query_faces: host-only context: no device work"),
        (rf, (None, 0, 0, 0xFF, None, 0, None), NO_DEVICE, "host-only context"),
        # vhr_closest_point_query: NULL, flags, points' alignment, results' alignment, cull_mask, host-only
        (pq, (None, N, BAD, 0x100, None), INVALID_ARGUMENT, "points and results must not be NULL when count > 0"),
        (pq, (A + 8, N, BAD, 0x100, None), INVALID_ARGUMENT, "points and results must not be NULL when count > 0"),
        (pq, (A + 8, N, 4, 0x100, B + 2), INVALID_ARGUMENT, "vhr_closest_point_query: unknown flag bits 4"),
        (pq, (None, 0, 4, 0x100, None), INVALID_ARGUMENT, "unknown flag bits 4"),
        (pq, (A + 8, N, 2, 0x100, B + 2), INVALID_ARGUMENT, "points must be 16-byte aligned"),
        (pq, (A, N, 2, 0x100, B + 2), INVALID_ARGUMENT, "results must be 4-byte aligned"),
        (pq, (A, N, 2, 0x100, B), INVALID_ARGUMENT, "vhr_closest_point_query: cull_mask 256 exceeds 0xFF"),
        (pq, (A, N, 2, 0xFF, B), NO_DEVICE, "vhr_closest_point_query: host-only context: no device work"),
        (pq, (A, 0, 3, 0xFF, B), NO_DEVICE, "host-only context"),
        (pq, (None, 0, 0, 0, None), NO_DEVICE, "host-only context"),
        (pq, (A + 8, 0, 0, 0xFF, B + 2), NO_DEVICE, "host-only context"),
        # vhr_resolve_hits: NULL, flags, hits' alignment, out's alignment, count == 0, host-only (material, then device memory)
        (rh, (None, N, BAD, None), INVALID_ARGUMENT, "hits and out must not be NULL when count > 0"),
        (rh, (A + 2, N, BAD, None), INVALID_ARGUMENT, "hits and out must not be NULL when count > 0"),
        (rh, (A + 2, N, 4, B + 8), INVALID_ARGUMENT, "vhr_resolve_hits: unknown flag bits 4"),
        (rh, (None, 0, BAD, None), INVALID_ARGUMENT, "unknown flag bits 2147483648"),
        (rh, (A + 2, N, 0, B + 8), INVALID_ARGUMENT, "hits must be 4-byte aligned"),
        (rh, (A + 4, N, 0, B + 8), INVALID_ARGUMENT, "out must be 16-byte aligned"),
        (rh, (A, N, 1, B + 4), INVALID_ARGUMENT, "out must be 16-byte aligned"),
        (rh, (A + 2, 0, 0, B + 8), OK, ""),
        (rh, (None, 0, 0, None), OK, ""),
        (rh, (None, 0, 1, None), OK, ""),
        (rh, (A, 0, 3, B), OK, ""),
        (rh, (A, N, 0, B), NO_DEVICE, "vhr_resolve_hits: host-only context: no device memory (VHR_SURFACE_HOST_MEMORY)"),
        (rh, (A, N, 1, B), NO_DEVICE, "host-only context: no textures are sampled without a device (VHR_SURFACE_MATERIAL)"),
        (rh, (A, N, 3, B), NO_DEVICE, "host-only context: no textures are sampled without a device (VHR_SURFACE_MATERIAL)"),
        (rh, (A, N, 2, B), OK, ""),
        (rh, (A + 4, N, 2, B), OK, ""),
        # the pair entry points: a null argument with count > 0; count == 0 asks for nothing
        ("vhr_debug_ray_triangle", (None, N, B, B), INVALID_ARGUMENT, "vhr_debug_ray_triangle: null argument"),
        ("vhr_debug_ray_triangle", (A, N, None, B), INVALID_ARGUMENT, "vhr_debug_ray_triangle: null argument"),
        ("vhr_debug_ray_triangle", (A, N, B, None), INVALID_ARGUMENT, "vhr_debug_ray_triangle: null argument"),
        ("vhr_debug_ray_triangle", (None, 0, None, None), DEVICE, "vhr_debug_ray_triangle: host-only context"),
        ("vhr_debug_ray_triangle", (A, N, B, B), DEVICE, "vhr_debug_ray_triangle: host-only context"),
        ("vhr_debug_ray_facing", (None, M, N, B), INVALID_ARGUMENT, "vhr_debug_ray_facing: null argument"),
        ("vhr_debug_ray_facing", (A, M, N, None), INVALID_ARGUMENT, "vhr_debug_ray_facing: null argument"),
        ("vhr_debug_ray_facing", (None, None, 0, None), OK, ""),
        ("vhr_debug_ray_facing", (A, None, N, B), OK, ""),
        ("vhr_debug_point_triangle", (None, N, B), INVALID_ARGUMENT, "vhr_debug_point_triangle: null argument"),
        ("vhr_debug_point_triangle", (A, N, None), INVALID_ARGUMENT, "vhr_debug_point_triangle: null argument"),
        ("vhr_debug_point_triangle", (None, 0, None), OK, ""),
        ("vhr_debug_point_triangle", (A, N, B), OK, ""),
    ]


def outcomes(c, table):
    """What the library answers to each row: (return code, vhr_last_error behind it)."""
    out = []
    for name, args, _, _ in table:
        rc = getattr(c.L, name)(c.handle, *args)
        out.append((rc, c.L.vhr_last_error(c.handle).decode()))
    return out


def test_statistics_before_any_call(host):
    c = host[0]
    fresh = lib.Context(64, 64, host_only=True)
    try:
        for name in ("vhr_get_ray_query_statistics", "vhr_get_point_query_statistics", "vhr_get_surface_statistics"):
            out = (C.c_uint64 * 4)(7, 7, 7, 7)
            assert getattr(fresh.L, name)(fresh.handle, out) == OK and list(out) == [0, 0, 0, 0], name
            assert getattr(fresh.L, name)(fresh.handle, None) == INVALID_ARGUMENT and getattr(fresh.L, name)(None, out) == INVALID_ARGUMENT, name
        assert fresh.ray_query_statistics() == fresh.point_query_statistics() == fresh.surface_statistics() == [0, 0, 0, 0]
    finally:
        fresh.close()
    assert c.ray_query_statistics() == c.point_query_statistics() == [0, 0, 0, 0]      # a refused query is no query


def test_the_winning_check_of_every_adjacent_pair(host):
    c, A, B, M = host
    table = rows(A, B, M)
    got = outcomes(c, table)
    wrong = [f"{name}{args}: got {rc} {msg!r}, want {want_rc} {want!r}" for (name, args, want_rc, want), (rc, msg) in zip(table, got)
             if rc != want_rc or (want_rc != OK and (want not in msg or not msg.startswith(name + ":")))]
    assert not wrong, "\n".join(wrong)
    # every entry point of the five is in the table with every code it can answer on this context
    for name in ("vhr_ray_query", "vhr_ray_query_masked", "vhr_ray_query_faces", "vhr_closest_point_query", "vhr_resolve_hits"):
        assert {r[2] for r in table if r[0] == name} >= {INVALID_ARGUMENT, NO_DEVICE}, name
    # a NULL context has no error to keep: the bare code
    assert c.L.vhr_ray_query(None, A, N, 2, B) == c.L.vhr_ray_query_masked(None, A, N, 2, 0xFF, None, B) == INVALID_ARGUMENT
    assert c.L.vhr_ray_query_faces(None, A, N, 2, 0xFF, None, 0, B) == c.L.vhr_closest_point_query(None, A, N, 2, 0xFF, B) == INVALID_ARGUMENT
    assert c.L.vhr_resolve_hits(None, A, N, 2, B) == c.L.vhr_debug_ray_triangle(None, A, N, B, B) == INVALID_ARGUMENT
    assert c.L.vhr_debug_ray_facing(None, A, None, N, B) == c.L.vhr_debug_point_triangle(None, A, N, B) == INVALID_ARGUMENT
    # the last resolve of the table was a host-memory call the host answered
    assert c.surface_statistics()[0] == N
