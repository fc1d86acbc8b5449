"""The judge of tests/tree_truth.py on the host builder's trees (host-only contexts, "bvh_builder" 0): every BVH the walkers read, as
vhr_debug_bvh_arrays hands it out, against exact geometry -- not against the library's own counters, which tests/tree_truth_cases.py only
compares with the judge's (T7).  First the judge itself: a tree written here byte by byte from the layouts' description must be clean, and
every planted defect must be caught by its rule, at the very step at which it becomes a defect."""
import ctypes as C
import struct
import types
from fractions import Fraction

import numpy as np
import pytest

from tests import tree_truth as tt
from tests import tree_truth_cases as cases
from vulkanhybridrenderer_amd import lib

F = np.float32
OK, INVALID_ARGUMENT, GRAPH = 0, -1, -5          # include/vhr_amd.h


def _ctx(scene, **options):
    c = lib.Context(64, 64, host_only=True)
    c.set_option("bvh_builder", 0)
    for k, v in options.items():
        c.set_option(k, v)
    c.update_geometry(scene.vertices, scene.indices, scene.primitives)
    return c


# ---------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------
def test_entry_point_checks_null_then_capacity_then_state(vhr):
    """(The refusal from inside a pass needs a graph that runs: tests/test_gpu_tree_truth.py.)"""
    L = vhr.load()
    scene = cases.one_leaf_scene()
    c = lib.Context(64, 64, host_only=True)
    try:
        header, counts = (C.c_uint32 * 24)(), (C.c_uint32 * 2)(7, 7)
        err = lambda: L.vhr_last_error(c.handle).decode()
        assert L.vhr_debug_bvh_arrays(None, header, None, None, None, None, None, 0, 0, counts) == INVALID_ARGUMENT
        assert L.vhr_debug_bvh_arrays(c.handle, None, None, None, None, None, None, 0, 0, counts) == INVALID_ARGUMENT and "must not be NULL" in err()
        assert L.vhr_debug_bvh_arrays(c.handle, header, None, None, None, None, None, 0, 0, None) == INVALID_ARGUMENT and "must not be NULL" in err()
        assert L.vhr_debug_bvh_arrays(c.handle, header, None, None, None, None, None, 0, 0, counts) == GRAPH and "no geometry" in err()
        assert list(counts) == [0, 0]
        c.update_geometry(scene.vertices, scene.indices, scene.primitives)
        assert L.vhr_debug_bvh_arrays(c.handle, header, None, None, None, None, None, 0, 0, counts) == INVALID_ARGUMENT and "room for 0 nodes" in err()
        assert list(counts) == [1, 1]
        bufs = [np.zeros(64, np.uint8) for _ in range(5)]
        ptrs = [b.ctypes.data for b in bufs]
        assert L.vhr_debug_bvh_arrays(c.handle, header, *ptrs, 1, 0, counts) == INVALID_ARGUMENT          # records: too small
        assert L.vhr_debug_bvh_arrays(c.handle, header, ptrs[0], None, *ptrs[2:], 1, 1, counts) == INVALID_ARGUMENT and "NULL array" in err()
        assert L.vhr_debug_bvh_arrays(c.handle, header, *ptrs, 1, 1, counts) == OK
        a = c.bvh_arrays()
        assert (a["node_count"], a["record_count"], a["depth"], a["frame_on"], a["frame_magnitude"]) == (1, 1, 0, False, 0.0)
        assert bytes(bufs[0]) == a["nodes"].tobytes() and bytes(bufs[4][:48]) == a["records"].tobytes()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------
# the decoder against the header's text: two triangles, one inner node, all four layouts written byte by byte
# ---------------------------------------------------------------------------------------------
def _hand_made():
    m = 2.0 ** -10                                    # every slot face this far outside its triangle's corners (all values dyadic: no rounding anywhere)
    node = struct.pack("<6f6f2i2i", -m, 1 + m, -m, 1 + m, -m, m,      2 - m, 3 + m, -m, 1 + m, -m, 1 + m,      ~((0 << 2) | 0), ~((1 << 2) | 0), 0, 0)
    node_ch = struct.pack("<6f3f3f2i2i", 0.5, 2.5, 0.5, 0.5, 0.0, 0.5,      0.5 + m, 0.5 + m, m,      0.5 + m, 0.5 + m, 0.5 + m,      -1, -5, 0, 0)
    # upper 16 bits of an fp32, rounded up: 0.5 + 2^-10 -> 0.5 (1 + 2^-7) = 0x3F01; 2^-10 = 0x3A80
    node48 = struct.pack("<6f3I2iI", 0.5, 2.5, 0.5, 0.5, 0.0, 0.5,      (0x3F01 << 16) | 0x3F01, (0x3A80 << 16) | 0x3F01, (0x3F01 << 16) | 0x3F01,      -1, -5, 0)
    # halves about the scene centre (1.5, 0.5, 0.5): -1 = 0xBC00, 1 = 0x3C00, -0.5 = 0xB800; 0.5 (1 + 2^-8) = 0x3804, 2^-9 = 0x1800
    node16 = struct.pack("<6H6H2i", 0xBC00, 0x3C00, 0, 0, 0xB800, 0,      0x3804, 0x3804, 0x3804, 0x3804, 0x1800, 0x3804,      -1, -5)
    records = struct.pack("<9f3I", 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0) + struct.pack("<9f3I", 2, 0, 0, 1, 0, 0, 0, 1, 1, 0, 1, 1)
    raw = lambda b, size: np.frombuffer(b, np.uint8).reshape(-1, size)
    arrays = dict(nodes=raw(node, 64), nodes_ch=raw(node_ch, 64), nodes48=raw(node48, 48), nodes16=raw(node16, 32), records=raw(records, 48),
                  centre=F([1.5, 0.5, 0.5]), frame=np.eye(3, dtype=F).reshape(9), frame_on=False, half_nodes=True, node_count=1, record_count=2, depth=1,
                  frame_magnitude=0.0)
    vertices = np.zeros(6, [("pos", "<f4", (3,))])
    vertices["pos"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [2, 1, 1]]
    primitives = np.zeros(1, [("transform", "<f4", (16,)), ("vertex_offset", "<u4"), ("index_offset", "<u4"), ("index_count", "<u4")])
    primitives["transform"][0] = np.eye(4, dtype=F).reshape(16)
    primitives["index_count"] = 6
    return arrays, types.SimpleNamespace(vertices=vertices, indices=np.arange(6, dtype=np.uint32), primitives=primitives)


def test_hand_made_tree_is_judged_clean_and_its_defects_are_not():
    arrays, scene = _hand_made()
    v = tt.judge(arrays, scene, leaf_triangles=1, statistics={"nodes": 1, "triangles": 2, "max_depth": 1})
    assert v.clean(), (v.failed(), v.where)
    assert v.faces == 12 and v.extreme_records == [0, 1]
    # margin 2^-10 under a pad of 1e-3 + 1e-5 max|x|: the smallest ratio at the x faces of the second box (pad 1e-3 + 3e-5), the largest at z of the first
    assert v.min_margin_over_pad == pytest.approx(2.0 ** -10 / (1e-3 + 1e-5 * 3.0), rel=1e-12) and v.max_margin_over_pad == pytest.approx(2.0 ** -10 / 1e-3, rel=1e-12)
    # the 32-byte form: 2^-10 to spare at magnitude |centre| + |c| + h = 1.5 + 1 + 0.501953125 on x
    assert v.half_spare_ulps == pytest.approx(2.0 ** -10 / (2.0 ** -23 * (1.5 + 1.0 + 0.501953125)), rel=1e-12)
    assert tt.sah_cost(arrays) == pytest.approx(((1 + 2 * 2.0 ** -10) ** 2 + 2 * (1 + 2 * 2.0 ** -10) * 2 * 2.0 ** -10 + 3 * (1 + 2 * 2.0 ** -10) ** 2) /
                                                (2 * (3 + 2 * 2.0 ** -10) * (1 + 2 * 2.0 ** -10) + (1 + 2 * 2.0 ** -10) ** 2), rel=1e-12)
    # the decoder reads each field where the header's text puts it: one changed field, one rule
    for form, field, index, value, rule in (("nodes", "box", (0, 1, 0), F(2.0 + 2.0 ** -10), "t3_margin"), ("nodes_ch", "h", (0, 1, 2), F(0.5), "t5_ch"),
                                            ("nodes48", "hp", (0, 1), (0x3A7F << 16) | 0x3F01, "t5_48"), ("nodes16", "h", (0, 2, 0), 0x13FF, "t5_16"),
                                            ("nodes16", "c", (0, 0, 1), 0x3C02, "t5_16"), ("nodes48", "child", (0, 1), -9, "t1_offsets"),
                                            ("records", "e2", (1, 2), F(1.0 + 2.0 ** -23), "t2_record"), ("records", "flat", (1,), 0, "t2_flat")):
        parts = tt.unpack(arrays)
        parts[form][field][index] = value
        bad = tt.judge(tt.repack(arrays, parts), scene, leaf_triangles=1)
        assert rule in bad.failed(), (form, field, bad.failed())


# ---------------------------------------------------------------------------------------------
# planted defects on the downloaded arrays of a clean soup tree
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup_tree(vhr):
    scene = cases.rt.soup_scene(1)
    c = _ctx(scene, bvh_frame=0)
    try:
        arrays = c.bvh_arrays()
    finally:
        c.close()
    assert tt.judge(arrays, scene).clean()
    return arrays, scene


def _verdict(soup_tree, parts):
    arrays, scene = soup_tree
    return tt.judge(tt.repack(arrays, parts), scene)


def _only(verdict, rule, where, beside=()):
    """`rule` flagged `where` and nothing else; the rules of `beside` may have flagged the same (node, child) slot, and no rule anything else."""
    failed = verdict.failed()
    assert verdict.where[rule] == [where], (rule, verdict.where[rule], failed)
    for other in failed:
        if other == rule:
            continue
        assert other in beside, (rule, failed, verdict.where[other][:4])
        assert all(tuple(w[:2]) == tuple(where[:2]) for w in verdict.where[other]), (other, verdict.where[other][:4])


def _fr(x):
    return Fraction(float(x))


def _leaf_slots(parts):
    """(node, child, first record, records) of every leaf."""
    out = []
    for k, nd in enumerate(parts["nodes"]):
        for w in range(2):
            link = int(nd["child"][w])
            if link < 0:
                out.append((k, w, (~link & 0xFFFFFFFF) >> 2, ((~link) & 3) + 1))
    return out


def _inner_links(parts):
    return [(k, w, int(nd["child"][w])) for k, nd in enumerate(parts["nodes"]) for w in range(2) if nd["child"][w] >= 0]


def test_a_face_one_step_inside_an_extreme_corner(soup_tree):
    parts = tt.unpack(soup_tree[0])
    rec = parts["records"]
    k, w, s, a = next((k, w, s, a) for k, w, s, n in _leaf_slots(parts) if n == 1 and k > 0 for a in range(3)
                      if rec["e1"][s, a] > 0 and rec["e2"][s, a] > 0)                       # v0 is the exact low extreme on axis a
    parts["nodes"]["box"][k, w, 2 * a] = rec["v0"][s, a]                                       # on the corner: margin 0 < rho
    on = _verdict(soup_tree, parts)
    parts["nodes"]["box"][k, w, 2 * a] = np.nextafter(rec["v0"][s, a], F(np.inf))             # one fp32 step inside it
    inside = _verdict(soup_tree, parts)
    for v in (on, inside):
        _only(v, "t3_margin", (k, w, a, 0))
    assert inside.min_margin_over_pad < 0 == on.min_margin_over_pad


@pytest.mark.parametrize("form", ["ch", "48", "16 extent", "16 centre"])
def test_a_form_one_step_short_of_its_slot(soup_tree, form):
    """The forms carry a few ulp to spare, so the defect is planted where it begins: the half extent (or the 32-byte centre) is moved step by step
    while the form still contains the slot in exact arithmetic (Fractions, here), then one step further.  The judge must flag exactly that step."""
    arrays, _ = soup_tree
    parts = tt.unpack(arrays)
    k, w, a = 3, 1, 1
    lo, hi = _fr(parts["nodes"]["box"][k, w, 2 * a]), _fr(parts["nodes"]["box"][k, w, 2 * a + 1])
    centre = _fr(arrays["centre"][a])
    half = lambda bits: _fr(np.array([bits], np.uint16).view(np.float16)[0])
    if form == "ch":
        c = _fr(parts["nodes_ch"]["c"][k, a, w])
        read = lambda: _fr(parts["nodes_ch"]["h"][k, w, a])
        def step():
            parts["nodes_ch"]["h"][k, w, a] = np.nextafter(parts["nodes_ch"]["h"][k, w, a], F(-np.inf))
        contains, rule = (lambda: c - read() <= lo and c + read() >= hi), "t5_ch"
    elif form == "48":
        c = _fr(parts["nodes48"]["c"][k, a, w])
        word, shift = divmod(3 * w + a, 2)
        shift = 16 * (1 - shift)
        read = lambda: _fr(np.array([((int(parts["nodes48"]["hp"][k, word]) >> shift) & 0xFFFF) << 16], np.uint32).view(F)[0])
        def step():
            parts["nodes48"]["hp"][k, word] -= np.uint32(1 << shift)
        contains, rule = (lambda: c - read() <= lo and c + read() >= hi), "t5_48"
    else:
        field = "h" if form == "16 extent" else "c"
        def step():
            parts["nodes16"][field][k, a, w] -= np.uint16(1)              # one half step: a smaller extent, or a centre nearer 0
        contains = lambda: (centre + half(parts["nodes16"]["c"][k, a, w]) - half(parts["nodes16"]["h"][k, a, w]) <= lo and
                            centre + half(parts["nodes16"]["c"][k, a, w]) + half(parts["nodes16"]["h"][k, a, w]) >= hi)
        rule = "t5_16"
    assert contains()
    steps = 0
    while contains():
        assert _verdict(soup_tree, parts).clean(), (form, steps)
        step()
        steps += 1
    assert 1 <= steps <= 64, (form, steps)
    _only(_verdict(soup_tree, parts), rule, (k, w, a))


def test_two_leaf_links_made_equal(soup_tree):
    parts = tt.unpack(soup_tree[0])
    (k0, w0, s0, n0), (k1, w1, s1, n1) = _leaf_slots(parts)[3], _leaf_slots(parts)[9]
    for form in ("nodes", "nodes_ch", "nodes48", "nodes16"):
        parts[form]["child"][k1, w1] = parts[form]["child"][k0, w0]
    v = _verdict(soup_tree, parts)
    assert sorted(v.where["t1_cover"]) == sorted(list(range(s0, s0 + n0)) + list(range(s1, s1 + n1)))          # those twice, these unreachable
    # (the slot now holds a box of other records, and its ancestors' boxes no longer fit what lies below them: T3 follows the topology)
    assert set(v.failed()) <= {"t1_cover", "t3_margin", "t3_tight"} and (k1, w1) in {x[:2] for x in v.where["t3_margin"]}, v.failed()


def test_a_link_to_an_ancestor(soup_tree):
    parts = tt.unpack(soup_tree[0])
    k, w, link = _inner_links(parts)[-1]
    for form, stride in (("nodes", 1), ("nodes_ch", 1), ("nodes48", 48), ("nodes16", 32)):
        parts[form]["child"][k, w] = 0
    v = _verdict(soup_tree, parts)
    assert (k, w) in v.where["t1_links"] and (link, -1) in v.where["t1_links"]                 # the cycle, and the node nothing reaches any more
    assert v.counts["t1_cover"] > 0
    # (the nodes that still hang on the tree hold boxes of records nothing reaches: T3's tightness follows the topology; T4 at the link itself)
    assert all(r.startswith("t1_") or r in ("t3_tight", "t4_child") for r in v.failed()) and {x[:2] for x in v.where["t4_child"]} <= {(k, w)}, v.failed()


def test_a_48_byte_link_to_another_index(soup_tree):
    parts = tt.unpack(soup_tree[0])
    k, w, link = _inner_links(parts)[2]
    parts["nodes48"]["child"][k, w] = (link + 1) * 48
    _only(_verdict(soup_tree, parts), "t1_offsets", (k, w))
    parts["nodes48"]["child"][k, w] = link                                                     # the index, where the byte offset belongs
    _only(_verdict(soup_tree, parts), "t1_offsets", (k, w))


def test_a_record_one_ulp_off(soup_tree):
    parts = tt.unpack(soup_tree[0])
    parts["records"]["e1"][17, 2] = np.nextafter(parts["records"]["e1"][17, 2], F(np.inf))
    _only(_verdict(soup_tree, parts), "t2_record", 17)


def test_a_slot_grown_by_ten_pads(soup_tree):
    """A bloated box (what a refit that only ever grows its boxes would leave): one face ten pads out, where the parent's slot still holds it,
    with derived forms widened to match -- contained everywhere, and caught by tightness alone."""
    arrays, _ = soup_tree
    parts = tt.unpack(arrays)
    nodes = parts["nodes"]
    parent = {link: (k, w) for k, w, link in _inner_links(parts)}
    for k, w, s, n in _leaf_slots(parts):
        if k == 0:
            continue
        pk, pw = parent[k]
        for a in range(3):
            pad = F(1e-3) + F(1e-5) * max(abs(nodes["box"][k, w, 2 * a]), abs(nodes["box"][k, w, 2 * a + 1]))
            grown = F(nodes["box"][k, w, 2 * a] - F(10) * pad)
            if grown > nodes["box"][pk, pw, 2 * a]:
                break
        else:
            continue
        break
    nodes["box"][k, w, 2 * a] = grown
    wider = F(11) * pad
    parts["nodes_ch"]["h"][k, w, a] += wider
    word, low = divmod(3 * w + a, 2)
    h48 = (np.array([parts["nodes_ch"]["h"][k, w, a]], F).view(np.uint32)[0] >> 16) + 1
    parts["nodes48"]["hp"][k, word] = (int(parts["nodes48"]["hp"][k, word]) & (0xFFFF0000 if low else 0x0000FFFF)) | (int(h48) << (0 if low else 16))
    h16 = np.array([parts["nodes16"]["h"][k, a, w]], np.uint16).view(np.float16)
    parts["nodes16"]["h"][k, a, w] = np.nextafter(np.float16(float(h16[0]) + float(wider)), np.float16(np.inf)).view(np.uint16)
    _only(_verdict(soup_tree, parts), "t3_tight", (k, w, a, 0))


# ---------------------------------------------------------------------------------------------
# clean verdicts on every kind of tree the host builder and the host refits make
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.build_cases()))
def test_built_trees_are_clean(vhr, name):
    make, options = cases.build_cases()[name]
    scene = make()
    c = _ctx(scene, **options)
    try:
        cases.check_built_case(c, scene, name, options, name)
    finally:
        c.close()


@pytest.mark.parametrize("name", cases.LIFECYCLES)
def test_refitted_and_rebuilt_trees_are_clean(vhr, name):
    scene = cases.lifecycle_scene(name)
    c = _ctx(scene)
    try:
        assert c.bvh_arrays()["frame_on"] == (name != "soup2")
        cases.run_lifecycle(c, scene, name)
    finally:
        c.close()


@pytest.mark.parametrize("name,how,keeps_frame", cases.FAR)
def test_the_frame_far_from_the_origin(vhr, name, how, keeps_frame):
    """A frame coordinate near 0 made of world coordinates of 2^14 and 2^17 m (the scene moved along the frame's third row), and the same scene
    2^10 times as large about the origin: rotate()'s rounding follows the WORLD magnitude, which 1e-3 + 1e-5 |frame coordinate| alone does not
    cover.  (soup1_rot x 2^10: the frame search's capped integer cost finds no frame at that size; that tree is judged on
    the world axes.)"""
    c = _ctx(cases.framed_scenes()[name]())
    try:
        cases.check_far(c, name, how, keeps_frame)
    finally:
        c.close()


@pytest.mark.parametrize("partial", [False, True])
def test_a_refit_that_leaves_the_frame_magnitude_fails_and_a_rebuild_recovers(vhr, partial):
    scene = cases.framed_scenes()["soup1_rot"]()
    c = _ctx(scene)
    try:
        assert c.bvh_arrays()["frame_magnitude"] == 16.0                   # the power of two at or above twice the largest |coordinate| (6.86)
        cases.check_leaving_the_magnitude(c, scene, partial)
    finally:
        c.close()
