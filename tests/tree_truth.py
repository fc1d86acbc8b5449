"""The judge of the trees (tests/test_tree_truth.py, tests/test_gpu_tree_truth.py).  TEST INFRASTRUCTURE, no tests here.

judge(arrays, scene, ...) takes the bytes vhr_debug_bvh_arrays hands out -- the four node forms and the leaf records as the walkers read them
-- and decides, against EXACT geometry, the one sentence everything the library answers rests on: a box only culls.  It decodes the layouts
from their description in csrc/vhr_internal.hpp's comments by itself and uses nothing of the library beyond those bytes: no bvh_math.hpp
function, no counter of the library, none of its Python modules.

Exactness.  Every fp32 and every half is a multiple of 2^-149, so every value that decides a verdict is a Python integer in units of 2^-149
(`_exact32`, `_exact16`), products of two of them integers in units of 2^-298; sums, products and comparisons of integers do not round.  The
thresholds (rho, the tightness bound) are binary64 numbers computed as written below and converted to the same integers exactly
(fractions.Fraction).  No case is filtered out, left undecided or skipped.  Floats appear only in what is REPORTED (margins, ratios, ulps).

The rules, one counter each (Verdict.counts; Verdict.where lists the (node, child) slots or record slots a rule flagged):
 T1 topology   t1_links    a link out of range, or a node reached twice from node 0 (a shared node or a cycle), or never
               t1_offsets  the centre / half-extent form's links differ from the (lo, hi) form's, or an inner link of the 48- / 32-byte form is
                           not index * 48 / index * 32, or a leaf link differs
               t1_leaf     a leaf link that names no 1 .. leaf_triangles records inside the record array
               t1_cover    a record slot that lies in no leaf or in several
               t1_depth    the depth (inner nodes on the longest path; 0 for a one-leaf scene) is not the reported one or exceeds 40
               t1_counts   node / record counts differ from the header's or the statistics'
               t1_absent   a one-leaf scene's absent child that is not inverted (lo > hi) / negative (h < 0) in some form
 T2 records    t2_record   a record that is not world_record(prim, tri) restated in numpy fp32, bit for bit
               t2_flat     a record whose flat index is not its triangle's
               t2_flats    a flat index that appears in no record (presplit: at least once; else exactly once)
 T3 slots      t3_margin   a slot face closer than rho to the extreme exact corner below it (or inside it)
               t3_tight    a slot face farther from it than the padding and the builder's own rounding explain (a stale or bloated box)
 T4 children   t4_child    a slot of an inner child outside the slot its parent holds for that child
 T5 forms      t5_ch / t5_48 / t5_16   c +- h, c +- upper-16 extent, centre + half(c) +- half(h) does not contain the fp32 slot, exactly
               t5_48_centre a 48-byte centre whose bits differ from the centre / half-extent form's
               t5_16_range  an inf, NaN or subnormal half (a zero centre is allowed) where the header says the walkers are on the 32-byte form
               t5_centre    the scene centre is not centre_of_root restated: per axis 0.5f * (lo + hi) over the root's slots that exist
 T6 presplit   t6_lattice  a point of the barycentric lattice (eighths, corners included) of a triangle that lies in the leaf slot of none of
                           its references (takes T3's place on a "bvh_presplit" tree: a reference's box is a clipped part of its triangle)

rho -- what the walker's own rounding may use up of a margin, from the operations as written.
 csrc/trace_device.hpp box_ray() rotates the origin: bo_i = fl(fl(fl(R_i0 o_0) + fl(R_i1 o_1)) + fl(R_i2 o_2)), five roundings, each relative
 2^-24 to a quantity that is at most sum_j |R_ij| |o_j| (1 + 2^-22) <= sqrt(3) W (1 + 2^-21) for a unit row and an origin inside the scene's
 world bounds, W = the largest |world coordinate| of the records' corners:
     rho_rotation = 5 sqrt(3) 2^-24 W (1 + 2^-20)         (0 on the world axes: nothing is rotated, W drops out)
 box_test() then computes fl(fl(face - bo) * inv) with inv = fl(1 / bd): the subtraction, the reciprocal and the product, plus the builder's
 fl(lo - pad) that made the face -- four roundings, taken relative to the frame coordinate x of the face as a slab test's padding
 traditionally is:
     rho_slab = 4 * 2^-24 |x|
 rho = rho_rotation + rho_slab.  NOT in rho, because they grow with the distance t a ray travels and not with where the scene lies: the
 rounding of the rotated DIRECTION (a displacement of at most t 5 sqrt(3) 2^-24) and the slab products' relative error on |face - bo| where
 that exceeds |x|.  A padding rule that wants to cover them for rays inside the scene needs another ~30 * 2^-24 W (t <= 2 sqrt(3) W).

Tightness.  A slot face is fl(b -+ fl(pad)) with b the fp32 extreme of the rotated (or plain) fp32 corners, so its distance from the EXACT
extreme is at most pad(x) + e_b + rounding, where e_b is the builder's own error: the corner sum fl(v0 + e) (2^-24 |coordinate|, i.e.
sqrt(3) 2^-24 W after a rotation) and rotate()'s five roundings (as above) -- e_b <= 6 sqrt(3) 2^-24 W (1 + 2^-20) in a frame, 2^-24 |x| on
the world axes -- and the rounding is the pad's own (2^-22 pad, fp32 constants and products) plus the subtraction's (2^-24 |x|, twice for
slack in |x| itself).  pad = 1e-3 + 1e-5 max(|lo|, |hi|) over the axis' two exact extents (the builders pad both faces of an axis alike) + in a
frame 2^-18 times the world magnitude in the arrays' header (include/vhr_amd.h, "bvh_frame").  t3_tight counts faces beyond that sum; the
verdict reports the largest and the smallest margin over the pad per tree."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
U = 2.0 ** -24
MAX_DEPTH = 40
LATTICE = 8
FRAME_PAD_FACTOR = 2.0 ** -18        # the frame padding per unit of the header's world magnitude (include/vhr_amd.h, "bvh_frame")

NODE = np.dtype([("box", "<f4", (2, 6)), ("child", "<i4", (2,)), ("pad", "<i4", (2,))])                                   # 64 bytes: (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z) twice
NODE_CH = np.dtype([("c", "<f4", (3, 2)), ("h", "<f4", (2, 3)), ("child", "<i4", (2,)), ("pad", "<i4", (2,))])            # c[axis][child], h[child][axis]
NODE48 = np.dtype([("c", "<f4", (3, 2)), ("hp", "<u4", (3,)), ("child", "<i4", (2,)), ("pad", "<i4")])                    # hp: (h0.x, h0.y) (h0.z, h1.x) (h1.y, h1.z), first in bits 31..16
NODE16 = np.dtype([("c", "<u2", (3, 2)), ("h", "<u2", (3, 2)), ("child", "<i4", (2,))])                                   # halves: c[axis][child], h[axis][child]
RECORD = np.dtype([("v0", "<f4", (3,)), ("e1", "<f4", (3,)), ("e2", "<f4", (3,)), ("prim", "<u4"), ("tri", "<u4"), ("flat", "<u4")])
assert (NODE.itemsize, NODE_CH.itemsize, NODE48.itemsize, NODE16.itemsize, RECORD.itemsize) == (64, 64, 48, 32, 48)

RULES = ("t1_links", "t1_offsets", "t1_leaf", "t1_cover", "t1_depth", "t1_counts", "t1_absent", "t2_record", "t2_flat", "t2_flats", "t3_margin", "t3_tight",
         "t4_child", "t5_ch", "t5_48", "t5_48_centre", "t5_16", "t5_16_range", "t5_centre", "t6_lattice")


# ---------------------------------------------------------------------------------------------
# exact values: Python integers in units of 2^-149 (object arrays)
# ---------------------------------------------------------------------------------------------
def _exact32(a):
    """fp32 array -> object array of integers, value * 2^149.  Finite values only (the caller has checked)."""
    bits = np.ascontiguousarray(a, F).view(np.uint32).astype(np.int64)
    e, m = (bits >> 23) & 255, bits & 0x7FFFFF
    mant = np.where(e == 0, m, m | 0x800000)
    shift = np.where(e == 0, 0, e - 1)
    out = mant.astype(object) * (2 ** shift.astype(object))
    return np.where(bits >> 31 != 0, -out, out)


def _exact16(h):
    """IEEE half bit patterns -> integers, value * 2^149.  Finite values only."""
    h = np.asarray(h).astype(np.int64)
    e, m = (h >> 10) & 31, h & 1023
    mant = np.where(e == 0, m, m | 1024)
    shift = np.where(e == 0, 0, e - 1)
    out = mant.astype(object) * (2 ** (shift + 125).astype(object))          # a half's unit is 2^-24 = 2^125 * 2^-149
    return np.where(h >> 15 != 0, -out, out)


def _units(x, power=149):
    """A binary64 threshold as an exact integer count of 2^-power, rounded up (a threshold only ever demands more for it)."""
    return int(math.ceil(Fraction(float(x)) * 2 ** power))


def _to_float(n, power=149):
    return float(Fraction(int(n), 2 ** power))


# ---------------------------------------------------------------------------------------------
# restatements (numpy fp32, one operation per rounding)
# ---------------------------------------------------------------------------------------------
def world_records(scene):
    """bvh_math::world_record of every triangle in flat order: transform * vec4(pos, 1), columns accumulated left to right; e1 = w1 - w0,
    e2 = w2 - w0.  -> (v0, e1, e2, prim, tri), fp32 (n, 3) each."""
    pr = scene.primitives
    counts = pr["index_count"].astype(np.int64) // 3
    prim = np.repeat(np.arange(len(counts)), counts)
    tri = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, np.int64)
    base = pr["index_offset"].astype(np.int64)[prim] + 3 * tri
    idx = np.asarray(scene.indices, np.uint32).astype(np.int64)
    pos = np.ascontiguousarray(scene.vertices["pos"], F)
    m = np.ascontiguousarray(pr["transform"], F).reshape(-1, 16)[prim]
    w = []
    for k in range(3):
        p = pos[pr["vertex_offset"].astype(np.int64)[prim] + idx[base + k]]
        w.append(np.stack([((m[:, r] * p[:, 0] + m[:, 4 + r] * p[:, 1]) + m[:, 8 + r] * p[:, 2]) + m[:, 12 + r] for r in range(3)], 1))
    assert w[0].dtype == F
    return w[0], w[1] - w[0], w[2] - w[0], prim.astype(np.uint32), tri.astype(np.uint32)


def centre_of_root(root_box):
    """bvh_math::centre_of_root on the root's (2, 6) slots: per axis 0.5f * (lo + hi) over the slots that exist on that axis, else 0."""
    out = np.zeros(3, F)
    for a in range(3):
        lo, hi = F(3.0e38), F(-3.0e38)
        for w in range(2):
            if root_box[w, 2 * a] <= root_box[w, 2 * a + 1]:
                lo, hi = min(lo, root_box[w, 2 * a]), max(hi, root_box[w, 2 * a + 1])
        out[a] = F(0.5) * F(lo + hi) if lo <= hi else F(0)
    return out


def sah_cost(arrays):
    """vhr_get_bvh_sah_cost's 'now' restated in binary64 from the downloaded slots: the sum over every child that exists of its slot's half area
    x (1 for an inner child, the record count for a leaf), over the half area of the root's slots together."""
    nodes = np.frombuffer(np.ascontiguousarray(arrays["nodes"]).tobytes(), NODE)
    b = nodes["box"].astype(np.float64)
    d = b[:, :, 1::2] - b[:, :, 0::2]
    area = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
    child = nodes["child"].astype(np.int64)
    weight = np.where(child >= 0, 1.0, ((~child) & 3) + 1.0)
    exists = np.ones(child.shape, bool)
    if len(nodes) == 1 and child[0, 0] == child[0, 1]:
        exists[0, 1] = False
    total = float((area * weight)[exists].sum())
    rb = b[0][exists[0]]
    lo, hi = rb[:, 0::2].min(0), rb[:, 1::2].max(0)
    e = hi - lo
    root = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
    return total / root if root > 0 else 0.0


# ---------------------------------------------------------------------------------------------
# the verdict
# ---------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self):
        self.counts = {r: 0 for r in RULES}
        self.where = {r: [] for r in RULES}
        self.min_margin_over_pad = math.inf       # T3: the smallest / largest (face to extreme exact corner) / pad(x), over the tree
        self.max_margin_over_pad = -math.inf
        self.min_margin_over_rho = math.inf
        self.half_spare_ulps = math.inf           # T5: the 32-byte form's smallest spare in fp32 ulps of |centre| + |c| + h
        self.extreme_records = []                 # record slots whose corners attain a slot extreme
        self.world_magnitude = 0.0
        self.faces = 0                            # slot faces judged by T3 (or lattice points by T6)

    def flag(self, rule, what):
        self.counts[rule] += 1
        self.where[rule].append(what)

    def failed(self):
        return {r: c for r, c in self.counts.items() if c}

    def clean(self):
        return not self.failed()

    def summary(self):
        return (f"margin/pad min {self.min_margin_over_pad:.4f} max {self.max_margin_over_pad:.4f}, margin/rho min {self.min_margin_over_rho:.2f}, "
                f"32-byte spare {self.half_spare_ulps:.1f} ulp, faces {self.faces}, failed {self.failed()}")


def decode(arrays):
    def as_(key, dt):
        return np.frombuffer(np.ascontiguousarray(arrays[key], np.uint8).tobytes(), dt)
    return as_("nodes", NODE), as_("nodes_ch", NODE_CH), as_("nodes48", NODE48), as_("nodes16", NODE16), as_("records", RECORD)


def unpack(arrays):
    """The five arrays as writable structured copies (the planted defects of tests/test_tree_truth.py are written into these)."""
    return {k: np.frombuffer(bytearray(np.ascontiguousarray(arrays[k], np.uint8).tobytes()), dt)
            for k, dt in (("nodes", NODE), ("nodes_ch", NODE_CH), ("nodes48", NODE48), ("nodes16", NODE16), ("records", RECORD))}


def repack(arrays, parts):
    """`arrays` with the five arrays taken from unpack()'s `parts`."""
    out = dict(arrays)
    for k, a in parts.items():
        out[k] = np.frombuffer(a.tobytes(), np.uint8).reshape(len(a), a.dtype.itemsize)
    return out


def _leaf(link):
    v = ~int(link) & 0xFFFFFFFF
    return v >> 2, (v & 3) + 1


def judge(arrays, scene, leaf_triangles=2, presplit=False, statistics=None):
    """arrays: Context.bvh_arrays() (or the same dict made by hand); scene: .vertices["pos"], .indices, .primitives["transform" / "vertex_offset" /
    "index_offset" / "index_count"]; statistics: bvh_statistics() (nodes, triangles = records, max_depth) or None."""
    V = Verdict()
    nodes, nch, n48, n16, rec = decode(arrays)
    n, m = len(nodes), len(rec)
    single = n == 1 and nodes["child"][0, 0] == nodes["child"][0, 1]
    frame_on = bool(arrays["frame_on"])
    if (n, m) != (arrays["node_count"], arrays["record_count"]) or len(nch) != n or len(n48) != n or len(n16) != n:
        V.flag("t1_counts", "header")
    if statistics is not None and (n, m, arrays["depth"]) != (statistics["nodes"], statistics["triangles"], statistics["max_depth"]):
        V.flag("t1_counts", "statistics")

    # ---- T1: one walk from node 0; a node is entered the first time only ----
    child = nodes["child"].astype(np.int64)
    visits = np.zeros(n, np.int64)
    cover = np.zeros(m, np.int64)
    owner = np.full((m, 2), -1, np.int64)            # the (node, child) whose leaf holds the record slot
    order, depth = [], 0
    visits[0] = 1
    stack = [(0, 1)]
    while stack:
        k, d = stack.pop()
        order.append(k)
        for w in range(2):
            if w == 1 and single:
                continue
            link = int(child[k, w])
            if link >= 0:
                if link >= n:
                    V.flag("t1_links", (k, w))
                    continue
                visits[link] += 1
                if visits[link] > 1:
                    V.flag("t1_links", (k, w))
                else:
                    stack.append((link, d + 1))
            else:
                depth = max(depth, d)
                first, count = _leaf(link)
                if count > leaf_triangles or first + count > m:
                    V.flag("t1_leaf", (k, w))
                    continue
                cover[first:first + count] += 1
                owner[first:first + count] = (k, w)
    for k in np.nonzero(visits == 0)[0]:
        V.flag("t1_links", (int(k), -1))
    for s in np.nonzero(cover != 1)[0]:
        V.flag("t1_cover", int(s))
    if single:
        depth = 0
    if depth != arrays["depth"] or depth > MAX_DEPTH:
        V.flag("t1_depth", (depth, arrays["depth"]))
    inner = child >= 0
    for form, stride in ((nch, 1), (n48, 48), (n16, 32)):
        want = np.where(inner, child * stride, child)
        for k, w in zip(*np.nonzero(form["child"].astype(np.int64) != want)):
            V.flag("t1_offsets", (int(k), int(w)))

    # ---- the values, exact ----
    box = nodes["box"]                                                   # (n, 2, 6)
    exists = np.ones((n, 2), bool)
    if single:
        exists[0, 1] = False
        half_h = n16["h"][0, :, 1]
        if not (np.all(box[0, 1, 0::2] > box[0, 1, 1::2]) and np.all(nch["h"][0, 1] < 0) and np.all(_upper16(n48["hp"][0])[3:] < 0) and np.all(half_h >> 15 != 0)):
            V.flag("t1_absent", (0, 1))
    finite = np.isfinite(box[exists]).all() and np.isfinite(rec["v0"]).all() and np.isfinite(rec["e1"]).all() and np.isfinite(rec["e2"]).all()
    if not finite:
        V.flag("t3_margin", "non-finite slot or record")
        return V
    xbox = _exact32(np.where(exists[:, :, None], box, F(0)))            # (n, 2, 6) integers

    # ---- T2: the records ----
    v0, e1, e2, prim, tri = world_records(scene)
    flat = rec["flat"].astype(np.int64)
    ok_flat = flat < len(v0)
    for s in np.nonzero(~ok_flat)[0]:
        V.flag("t2_flat", int(s))
    f = np.where(ok_flat, flat, 0)
    same = np.ones(m, bool)
    for got, want in ((rec["v0"], v0), (rec["e1"], e1), (rec["e2"], e2)):
        same &= (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want[f]).view(np.uint32)).all(1)
    for s in np.nonzero(ok_flat & ~same)[0]:
        V.flag("t2_record", int(s))
    for s in np.nonzero(ok_flat & ((rec["prim"] != prim[f]) | (rec["tri"] != tri[f])))[0]:
        V.flag("t2_flat", int(s))
    seen = np.bincount(flat[ok_flat], minlength=len(v0))
    for t in np.nonzero((seen == 0) if presplit else (seen != 1))[0]:
        V.flag("t2_flats", int(t))

    # ---- the exact corners of every record, in the tree's frame: integers in units of 2^-298 (2^-149 on the world axes, scaled up) ----
    x0, x1, x2 = _exact32(rec["v0"]), _exact32(rec["e1"]), _exact32(rec["e2"])
    corners = np.stack([x0, x0 + x1, x0 + x2], 1)                        # (m, 3 corners, 3 axes), exact
    W = max((_to_float(abs(c)) for c in (corners.min(), corners.max())), default=0.0) if m else 0.0
    V.world_magnitude = W
    if frame_on:
        R = _exact32(np.asarray(arrays["frame"], F).reshape(3, 3))
        fc = np.stack([sum(R[i, j] * corners[:, :, j] for j in range(3)) for i in range(3)], 2)       # (m, 3, 3) units 2^-298
    else:
        fc = corners * (2 ** 149)
    P = 298
    rec_lo, rec_hi = fc.min(1), fc.max(1)                                # (m, 3) per record
    sbox = xbox * (2 ** 149)                                             # the slots in the same units

    def rho_of(x):
        return (5.0 * math.sqrt(3.0) * U * W * (1.0 + 2.0 ** -20) if frame_on else 0.0) + 4.0 * U * abs(x)

    def pad_of(x):
        return 1e-3 + 1e-5 * abs(x) + float(arrays.get("frame_magnitude", 0.0)) * FRAME_PAD_FACTOR * (1.0 if frame_on else 0.0)

    def tight_of(x, pad):
        e_b = 6.0 * math.sqrt(3.0) * U * W * (1.0 + 2.0 ** -20) if frame_on else U * abs(x)
        return pad * (1.0 + 2.0 ** -22) + e_b + 2.0 * U * (abs(x) + pad)

    # ---- T3 (T6 on a presplit tree): bottom-up, every slot against the extreme exact corner of all records below it ----
    below = {}                                                           # (node, child) -> (lo[3], hi[3], argmin[3], argmax[3])
    for k in reversed(order):
        for w in range(2):
            if not exists[k, w]:
                continue
            link = int(child[k, w])
            if link >= 0:
                if link >= n or (link, 0) not in below:
                    continue
                parts = [below[(link, c)] for c in range(2) if (link, c) in below]
            else:
                first, count = _leaf(link)
                if count > leaf_triangles or first + count > m:
                    continue
                parts = [([rec_lo[s, a] for a in range(3)], [rec_hi[s, a] for a in range(3)], [s] * 3, [s] * 3) for s in range(first, first + count)]
            lo, hi, alo, ahi = list(parts[0][0]), list(parts[0][1]), list(parts[0][2]), list(parts[0][3])
            for p in parts[1:]:
                for a in range(3):
                    if p[0][a] < lo[a]:
                        lo[a], alo[a] = p[0][a], p[2][a]
                    if p[1][a] > hi[a]:
                        hi[a], ahi[a] = p[1][a], p[3][a]
            below[(k, w)] = (lo, hi, alo, ahi)
            if presplit:
                continue
            for a in range(3):
                for side, ext, face, who in ((0, lo[a], int(sbox[k, w, 2 * a]), alo[a]), (1, hi[a], int(sbox[k, w, 2 * a + 1]), ahi[a])):
                    margin = ext - face if side == 0 else face - ext
                    x = _to_float(ext, P)
                    rho, pad = rho_of(x), pad_of(max(abs(_to_float(lo[a], P)), abs(_to_float(hi[a], P))))
                    V.faces += 1
                    if margin < _units(rho, P):
                        V.flag("t3_margin", (k, w, a, side))
                    if margin > _units(tight_of(x, pad), P):
                        V.flag("t3_tight", (k, w, a, side))
                    mf = _to_float(margin, P)
                    V.min_margin_over_pad = min(V.min_margin_over_pad, mf / pad)
                    V.max_margin_over_pad = max(V.max_margin_over_pad, mf / pad)
                    V.min_margin_over_rho = min(V.min_margin_over_rho, mf / rho if rho > 0 else math.inf)
                    V.extreme_records.append(who)
    V.extreme_records = sorted(set(V.extreme_records))

    if presplit:
        _lattice(V, rec, owner, xbox, x0, x1, x2, cover)

    # ---- T4: an inner child's two slots inside the slot its parent holds for it ----
    for k in order:
        for w in range(2):
            link = int(child[k, w])
            if not exists[k, w] or link < 0 or link >= n:
                continue
            for c in range(2):
                if not exists[link, c]:
                    continue
                inside = all(xbox[link, c, 2 * a] >= xbox[k, w, 2 * a] and xbox[link, c, 2 * a + 1] <= xbox[k, w, 2 * a + 1] for a in range(3))
                if not inside:
                    V.flag("t4_child", (k, w, c))

    _forms(V, arrays, nodes, nch, n48, n16, xbox, exists)
    return V


def _upper16(hp):
    """The six half extents of a 48-byte node as fp32 (h0.x, h0.y, h0.z, h1.x, h1.y, h1.z): upper 16 bits of an fp32 pattern each."""
    hp = np.asarray(hp, np.uint32)
    w16 = np.stack([hp[..., 0] >> 16, hp[..., 0] & 0xFFFF, hp[..., 1] >> 16, hp[..., 1] & 0xFFFF, hp[..., 2] >> 16, hp[..., 2] & 0xFFFF], -1).astype(np.uint32)
    return (w16 << 16).view(F)


def _lattice(V, rec, owner, xbox, x0, x1, x2, cover):
    """T6: N * P = N v0 + i e1 + j e2 (exact) against N * slot, for the lattice i + j <= N of every triangle, in the leaf slots of its references."""
    N = LATTICE
    ij = [(i, j) for i in range(N + 1) for j in range(N + 1 - i)]
    by_flat = {}
    for s in range(len(rec)):
        if cover[s] == 1:
            by_flat.setdefault(int(rec["flat"][s]), []).append(s)
    for flat, slots in by_flat.items():
        s0 = slots[0]
        pts = ij if len(slots) > 1 else [(0, 0), (N, 0), (0, N)]
        boxes = [xbox[owner[s, 0], owner[s, 1]] * N for s in slots]
        for i, j in pts:
            p = [N * x0[s0, a] + i * x1[s0, a] + j * x2[s0, a] for a in range(3)]
            V.faces += 1
            if not any(all(b[2 * a] <= p[a] <= b[2 * a + 1] for a in range(3)) for b in boxes):
                V.flag("t6_lattice", (flat, i, j))


def _forms(V, arrays, nodes, nch, n48, n16, xbox, exists):
    """T5: the three derived forms against the fp32 slots, exactly."""
    n = len(nodes)
    centre = np.asarray(arrays["centre"], F)
    if not np.array_equal(centre.view(np.uint32), centre_of_root(nodes["box"][0]).view(np.uint32)):
        V.flag("t5_centre", tuple(float(c) for c in centre))
    lo, hi = xbox[:, :, 0::2], xbox[:, :, 1::2]                          # (n, 2 children, 3 axes)
    c_ch = np.transpose(nch["c"], (0, 2, 1))                             # -> (n, child, axis)
    h_ch = nch["h"]
    c_48 = np.transpose(n48["c"], (0, 2, 1))
    h_48 = _upper16(n48["hp"]).reshape(n, 2, 3)
    cb, hb = np.transpose(n16["c"], (0, 2, 1)).astype(np.int64), np.transpose(n16["h"], (0, 2, 1)).astype(np.int64)
    for k, w, a in zip(*np.nonzero(np.ascontiguousarray(c_48).view(np.uint32) != np.ascontiguousarray(c_ch).view(np.uint32))):
        V.flag("t5_48_centre", (int(k), int(w), int(a)))
    live = np.broadcast_to(exists[:, :, None], lo.shape)
    for name, c, h in (("t5_ch", c_ch, h_ch), ("t5_48", c_48, h_48)):
        good = np.isfinite(c) & np.isfinite(h)
        xc, xh = _exact32(np.where(good, c, F(0))), _exact32(np.where(good, h, F(0)))
        bad = live & (~good | (xc - xh > lo) | (xc + xh < hi))
        bad |= ~live & ~(h < 0)
        for k, w, a in zip(*np.nonzero(bad)):
            V.flag(name, (int(k), int(w), int(a)))
    ec, eh = (cb >> 10) & 31, (hb >> 10) & 31
    in_range = ~((ec == 31) | ((ec == 0) & (cb != 0)) | (eh == 31) | (eh == 0))
    if arrays["half_nodes"]:
        for k, w, a in zip(*np.nonzero(live & ~in_range)):
            V.flag("t5_16_range", (int(k), int(w), int(a)))
        good = (ec != 31) & (eh != 31)
        xcentre = _exact32(centre)
        xc = _exact16(np.where(good, cb, 0)) + xcentre[None, None, :]
        xh = _exact16(np.where(good, hb, 0))
        under, over = lo - (xc - xh), (xc + xh) - hi
        bad = live & (~good | (under < 0) | (over < 0))
        bad |= ~live & ~(hb >> 15 != 0)
        for k, w, a in zip(*np.nonzero(bad)):
            V.flag("t5_16", (int(k), int(w), int(a)))
        ok = live & good & ~bad
        if ok.any():
            spare = np.minimum(under, over)[ok]
            mag = (abs(xcentre)[None, None, :] + abs(xc - xcentre[None, None, :]) + xh)[ok]
            V.half_spare_ulps = min(float(Fraction(int(s) * 2 ** 23, int(g))) for s, g in zip(spare, mag) if g > 0)
