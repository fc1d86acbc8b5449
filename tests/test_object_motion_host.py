""""object_motion_vectors" without a GPU: the option, the previous records the host twin of the refits keeps (csrc/bvh_build.cpp) and the two
entry points, on host-only contexts.  The truths are the records read BEFORE each update and a fresh context's records after it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import object_motion_cases as omc
from tests import partial_refit_cases as cases
from tests.test_gpu_fuzz import soup
from vulkanhybridrenderer_amd import lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, GRAPH, UNSUPPORTED = 0, -1, -5, -7          # include/vhr_amd.h
KEY = "object_motion_vectors"


def _ctx(vertices, indices, primitives, **options):
    c = lib.Context(64, 64, host_only=True)
    for k, v in options.items():
        c.set_option(k, v)
    c.update_geometry(vertices, indices, primitives)
    return c


def _scene_ctx(scene, **options):
    return _ctx(scene.vertices, scene.indices, scene.primitives, **options)


def _fresh(scene):
    def records(vertices, primitives):
        c = _ctx(vertices, scene.indices, primitives)
        try:
            return c.triangle_records()
        finally:
            c.close()
    return records


def _warm(c, scene):
    c.update_vertices(scene.vertices)
    c.refit_geometry()
    return c


def test_option_round_trip_and_symbols(vhr):
    c = lib.Context(64, 64, host_only=True)
    try:
        assert c.get_option(KEY) == 0 and c.object_motion_statistics() == dict(active=0, differing_records=0, motion_launches=0)
        c.set_option(KEY, 1)
        assert c.get_option(KEY) == 1 and c.object_motion_statistics()["active"] == 0          # no tree yet: no arrays
        c.set_option(KEY, 0)
        assert c.get_option(KEY) == 0
        for bad in (2, -1):
            assert c.L.vhr_set_option(c.handle, KEY.encode(), bad) == INVALID_ARGUMENT and KEY in c.L.vhr_last_error(c.handle).decode()
        assert c.get_option(KEY) == 0
        assert KEY not in lib.option_table()
    finally:
        c.close()
    L = vhr.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vhr_amd.h")).read(), flags=re.S)
    for name in ("vhr_get_object_motion_statistics", "vhr_debug_triangle_records"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name) and name in lib.EXPORTS, name


def test_previous_is_the_last_state_bit_for_bit(vhr):
    """Tests 2, 3 and 4 of the issue: A takes the dirty path, B the whole-tree refit."""
    scene = soup(3, 2000, 8)
    a, b = _warm(_scene_ctx(scene, **{KEY: 1}), scene), _warm(_scene_ctx(scene, **{KEY: 1}), scene)
    try:
        for c in (a, b):
            omc.assert_settled(c, "after the warm-up refit, which rewrote every record with the same bits")
        omc.walk(scene, [(a, lambda c: c.refit_geometry_partial(force=True)), (b, lambda c: c.refit_geometry())], _fresh(scene))
        assert a.partial_refit_statistics()["partial_refits"] == len(omc.SEQUENCE)
    finally:
        a.close()
        b.close()


def test_a_rebuild_and_a_switch_off_and_on_reset_previous(vhr):
    scene = soup(3, 2000, 8)
    c = _warm(_scene_ctx(scene, **{KEY: 1}), scene)
    try:
        ups = cases.updates(scene)

        def move(name):
            cases.apply(c, ups[name])
            c.refit_geometry_partial(force=True)
            assert c.object_motion_statistics()["differing_records"] > 0
            assert not omc.same(c.triangle_records(), c.triangle_records(previous=True))
        move(omc.SEQUENCE[0])
        c.update_geometry(scene.vertices, scene.indices, scene.primitives)
        omc.assert_settled(c, "after a rebuild")
        _warm(c, scene)
        move(omc.SEQUENCE[1])
        cur = c.triangle_records()
        c.set_option(KEY, 0)
        assert c.object_motion_statistics() == dict(active=0, differing_records=0, motion_launches=0)
        n = C.c_uint32(0)
        assert c.L.vhr_debug_triangle_records(c.handle, 1, None, 0, C.byref(n)) == GRAPH and KEY in c.L.vhr_last_error(c.handle).decode()
        c.set_option(KEY, 1)
        omc.assert_settled(c, "after switching off and on")
        assert omc.same(c.triangle_records(), cur)
        move(omc.SEQUENCE[2])                                 # and the bookkeeping starts over
    finally:
        c.close()


def test_fingerprints_do_not_see_the_option(vhr):
    scene = soup(3, 2000, 8)
    on, off = _warm(_scene_ctx(scene, **{KEY: 1}), scene), _warm(_scene_ctx(scene), scene)
    try:
        ups = cases.updates(scene)
        for name in omc.SEQUENCE:
            for c in (on, off):
                cases.apply(c, ups[name])
                c.refit_geometry_partial(force=True)
            assert cases.state(on) == cases.state(off), name
            assert on.bvh_forms_fingerprint() == off.bvh_forms_fingerprint(), name
            assert on.refit_statistics() == off.refit_statistics() and on.partial_refit_statistics() == off.partial_refit_statistics(), name
        for c in (on, off):                                   # nothing pending: not counted by the refit statistics, option or not
            c.refit_geometry()
        assert cases.state(on) == cases.state(off) and on.refit_statistics() == off.refit_statistics()
        assert off.object_motion_statistics() == dict(active=0, differing_records=0, motion_launches=0)
    finally:
        on.close()
        off.close()


def test_triangle_records_refusals(vhr):
    scene = soup(1, 60, 3)
    c = lib.Context(64, 64, host_only=True)
    L = c.L
    err = lambda: L.vhr_last_error(c.handle).decode()
    n = C.c_uint32(7)
    try:
        assert L.vhr_debug_triangle_records(c.handle, 0, None, 0, C.byref(n)) == GRAPH and "no geometry" in err() and n.value == 0
        assert L.vhr_debug_triangle_records(c.handle, 0, None, 0, None) == INVALID_ARGUMENT
        assert L.vhr_debug_triangle_records(None, 0, None, 0, C.byref(n)) == INVALID_ARGUMENT
        assert L.vhr_get_object_motion_statistics(c.handle, None) == INVALID_ARGUMENT
        c.update_geometry(scene.vertices, scene.indices, scene.primitives)
        triangles = c.bvh_statistics()["triangles"]
        out = np.zeros((triangles, 9), np.float32)
        assert L.vhr_debug_triangle_records(c.handle, 2, out.ctypes.data, triangles, C.byref(n)) == INVALID_ARGUMENT
        assert L.vhr_debug_triangle_records(c.handle, 1, out.ctypes.data, triangles, C.byref(n)) == GRAPH and KEY in err()
        assert L.vhr_debug_triangle_records(c.handle, 0, out.ctypes.data, triangles - 1, C.byref(n)) == INVALID_ARGUMENT and n.value == triangles
        assert not out.any()
        assert L.vhr_debug_triangle_records(c.handle, 0, out.ctypes.data, triangles, C.byref(n)) == OK and n.value == triangles
        # flat order: triangle t of primitive p from the arrays, whatever the tree
        pr = scene.primitives[0]
        i = scene.indices[int(pr["index_offset"]):int(pr["index_offset"]) + 3].astype(np.int64) + int(pr["vertex_offset"])
        m = np.asarray(pr["transform"], np.float64).reshape(4, 4).T          # column-major 16 floats
        p = [m[:3, :3] @ scene.vertices["pos"][k].astype(np.float64) + m[:3, 3] for k in i]
        np.testing.assert_allclose(out[0], np.concatenate([p[0], p[1] - p[0], p[2] - p[0]]), rtol=1e-5, atol=1e-5)
    finally:
        c.close()
    pre = _scene_ctx(scenes.rotated(soup(22, 1500, 6), rot_y=0.6, rot_x=0.25), bvh_presplit=100, bvh_frame=0, **{KEY: 1})
    try:
        assert pre.bvh_presplit_level() >= 0
        assert pre.L.vhr_debug_triangle_records(pre.handle, 0, None, 0, C.byref(n)) == UNSUPPORTED and "bvh_presplit" in pre.L.vhr_last_error(pre.handle).decode()
    finally:
        pre.close()
