"""The binary64 truth vhr_closest_point_query's point / triangle function (csrc/closest_point.hpp) is held against, the error bound of its d2,
and the pair sets both the CPU test (tests/test_point_query_host.py: the host's copy against the truth) and the GPU test
(tests/test_gpu_point_query.py: the device's copy against the host's, bit for bit) run.

The truth works on the same fp32 records (p, v0, e1, e2 widened to binary64, every operation after that in binary64: 29 bits to spare) and finds
the nearest point of the closed triangle by exhaustion: the three vertices, the three edges as clamped segments, and the foot of the perpendicular
where it falls inside.  It also names the region of Ericson's classification (Real-Time Collision Detection 5.1.5) the nearest point lies in.

THE BOUND (DESIGN.md 4d derives it from the operations as written).  With u = 2^-24, A = |p - v0| and E = the longest edge (2-norms),
    |d2 - D^2| <= 24 u (A + E)^2
  - 13 u (A + E)^2: evaluating |(ap - u e1) - v e2|^2 at the candidate's own (u, v) -- ap = p - v0 rounded once, two products and two differences
    per axis (at most u (3 |ap| + 3 |e1| + 2 |e2|) per axis), |r| <= A + E, three squares and two sums (3 u relative).  Every candidate is a point OF
    the triangle, so this alone bounds how far d2 can lie BELOW the truth.
  - 10 u E (A + E) <= 10 u (A + E)^2: how far the best candidate's point can lie from the true nearest point, squared (the two errors are at right
    angles).  On an edge the clamped parameter is off by a few u: second order, nothing.  In the face the foot of the perpendicular is off by at most
    20 u E (A + E) / w (w = the triangle's smallest height: the rounded normal tilts by 4 u E / w, the two numerators are off by 8 u A E |n| each,
    n.n by 11 u E / w relative) -- or the face candidate is wrong or missing altogether, and then the nearest boundary point is at most the inradius
    <= w / 2 away.  The smaller of the two, squared, is at most their product: 10 u E (A + E), whatever w is -- a needle or a record without area
    included.
  - first order in u; the terms in u^2 are below 2^-20 of the bound."""
import numpy as np

U = 2.0 ** -24
BOUND_CONSTANT = 24.0
SCALES = (2.0 ** -10, 1.0, 2.0 ** 10)
REGIONS = ("face", "edge AB", "edge AC", "edge BC", "vertex A", "vertex B", "vertex C")


def split(pairs):
    p = np.asarray(pairs, np.float32).reshape(-1, 12).astype(np.float64)
    return p[:, 0:3], p[:, 3:6], p[:, 6:9], p[:, 9:12]


def bound(pairs):
    """24 u (A + E)^2 per pair, in binary64."""
    p, v0, e1, e2 = split(pairs)
    a = np.linalg.norm(p - v0, axis=1)
    e = np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(e2 - e1, axis=1))
    return BOUND_CONSTANT * U * (a + e) ** 2


def _segment(ap, d):
    """Nearest point of the segment {t d, 0 <= t <= 1} to ap: (squared distance, t)."""
    dd = np.einsum("ij,ij->i", d, d)
    t = np.where(dd > 0, np.einsum("ij,ij->i", ap, d) / np.where(dd > 0, dd, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    r = ap - t[:, None] * d
    return np.einsum("ij,ij->i", r, r), t


def truth(pairs):
    """-> (D2, u, v, region): the squared distance to the closed triangle, the barycentrics of a nearest point and the index into REGIONS of the
    region it lies in (face: strictly inside; an edge: strictly between its ends)."""
    p, v0, e1, e2 = split(pairs)
    ap = p - v0
    n = len(ap)
    with np.errstate(all="ignore"):
        d_ab, t_ab = _segment(ap, e1)
        d_ac, t_ac = _segment(ap, e2)
        d_bc, t_bc = _segment(ap - e1, e2 - e1)
        nrm = np.cross(e1, e2)
        nn = np.einsum("ij,ij->i", nrm, nrm)
        ok = nn > 0
        safe = np.where(ok, nn, 1.0)
        fu = np.einsum("ij,ij->i", np.cross(ap, e2), nrm) / safe
        fv = np.einsum("ij,ij->i", np.cross(e1, ap), nrm) / safe
        inside = ok & (fu > 0) & (fv > 0) & (fu + fv < 1)
        r = ap - fu[:, None] * e1 - fv[:, None] * e2
        d_face = np.where(inside, np.einsum("ij,ij->i", r, r), np.inf)
    d = np.stack([d_face, d_ab, d_ac, d_bc], axis=1)
    which = np.argmin(d, axis=1)
    D2 = d[np.arange(n), which]
    u = np.choose(which, [fu, t_ab, np.zeros(n), 1.0 - t_bc])
    v = np.choose(which, [fv, np.zeros(n), t_ac, t_bc])
    w = np.choose(which, [1.0 - fu - fv, 1.0 - t_ab, 1.0 - t_ac, np.zeros(n)])
    region = np.zeros(n, np.int64)                        # by the zeros among the barycentrics (w, u, v) of (A, B, C)
    region[(v == 0) & (u > 0) & (w > 0)] = 1
    region[(u == 0) & (v > 0) & (w > 0)] = 2
    region[(w == 0) & (u > 0) & (v > 0)] = 3
    region[(u == 0) & (v == 0)] = 4
    region[(v == 0) & (w == 0)] = 5
    region[(u == 0) & (w == 0)] = 6
    return D2, u, v, region


def inside_unit_triangle(u, v):
    """u, v >= 0 and u + v <= 1 in EXACT arithmetic, for fp32 u and v: 1 - x is exact in fp32 for x in [0.5, 1], two numbers below 0.5 sum to less than 1."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    one = np.float32(1.0)
    sum_ok = np.where(u >= 0.5, v <= one - u, np.where(v >= 0.5, u <= one - v, True))
    return np.isfinite(u) & np.isfinite(v) & (u >= 0) & (v >= 0) & (u <= 1) & (v <= 1) & sum_ok


def violations(pairs, out):
    """Per pair, true where (d2, u, v) = out breaks the contract: d2 farther than the bound from the truth, (u, v) outside the closed unit triangle,
    or the point (u, v) names not at the distance d2 claims (within the same bound).  For pairs of finite numbers."""
    out = np.asarray(out, np.float32).reshape(-1, 3)
    D2, _, _, _ = truth(pairs)
    b = bound(pairs)
    d2, u, v = out[:, 0].astype(np.float64), out[:, 1], out[:, 2]
    p, v0, e1, e2 = split(pairs)
    r = (p - v0) - u.astype(np.float64)[:, None] * e1 - v.astype(np.float64)[:, None] * e2
    at = np.einsum("ij,ij->i", r, r)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(d2 - D2) <= b) | ~inside_unit_triangle(u, v) | ~(np.abs(d2 - at) <= b)


def ratio(pairs, out):
    """The largest |d2 - D^2| / bound over the pairs whose bound is not 0."""
    out = np.asarray(out, np.float32).reshape(-1, 3)
    D2, _, _, _ = truth(pairs)
    b = bound(pairs)
    k = b > 0
    return float(np.max(np.abs(out[k, 0].astype(np.float64) - D2[k]) / b[k])) if k.any() else 0.0


# ---------------------------------------------------------------------------------------------
# the pair sets: (n, 12) float32 (p, v0, e1, e2) at scale 1; scaled() multiplies every number by a power of two
# ---------------------------------------------------------------------------------------------
def _pack(p, v0, e1, e2):
    return np.concatenate([p, v0, e1, e2], axis=1).astype(np.float32)


def _triangles(rng, n):
    v0 = rng.normal(size=(n, 3))
    size = 10.0 ** rng.uniform(-2, 0.5, size=(n, 1))
    return v0, rng.normal(size=(n, 3)) * size, rng.normal(size=(n, 3)) * size


def random_pairs(n=2500, seed=1):
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _triangles(rng, n)
    # half of the points around the triangle at its own scale (all seven regions), half anywhere
    bu, bv = rng.uniform(-0.7, 1.7, (n, 1)), rng.uniform(-0.7, 1.7, (n, 1))
    nrm = np.cross(e1, e2)
    near = v0 + bu * e1 + bv * e2 + nrm * rng.normal(size=(n, 1)) * 10.0 ** rng.uniform(-3, 0.5, (n, 1))
    p = np.where(rng.random((n, 1)) < 0.5, near, rng.normal(size=(n, 3)) * 2.0)
    return _pack(p, v0, e1, e2)


def boundary_pairs(n=1200, seed=2):
    """Points ON edges and vertices (as fp32 rounds them) and a hair off them."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = (x.astype(np.float32).astype(np.float64) for x in _triangles(rng, n))
    kind = rng.integers(0, 6, n)
    t = rng.random((n, 1))
    on = np.choose(kind[:, None], [v0, v0 + e1, v0 + e2, v0 + t * e1, v0 + t * e2, v0 + e1 + t * (e2 - e1)])
    off = rng.normal(size=(n, 3)) * rng.choice([0.0, 0.0, 1e-7, 1e-5, 1e-3], (n, 1))
    return _pack(on + off, v0, e1, e2)


def needle_pairs(n=1500, seed=3):
    """Needles (a height of 1e-1 .. 1e-8 of the length) and records without area: e2 a multiple of e1, one or both edges zero."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _triangles(rng, n)
    e1 = e1.astype(np.float32).astype(np.float64)
    s = rng.choice([0.5, 2.0, -1.0, 1.0, 0.25, 3.0], (n, 1))
    thin = 10.0 ** rng.uniform(-8, -1, (n, 1))
    kind = rng.integers(0, 6, n)[:, None]
    perp = np.cross(e1, rng.normal(size=(n, 3)))
    e2 = np.where(kind <= 2, s * e1 + thin * perp, np.where(kind == 3, s * e1, np.where(kind == 4, 0.0, e2)))
    e1 = np.where(kind == 5, 0.0, e1)
    both = rng.random((n, 1)) < 0.05
    e1, e2 = np.where(both, 0.0, e1), np.where(both, 0.0, e2)
    bu, bv = rng.uniform(-0.5, 1.5, (n, 1)), rng.uniform(-0.5, 1.5, (n, 1))
    p = v0 + bu * e1 + bv * e2 + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-6, 0.5, (n, 1))
    return _pack(p, v0, e1, e2)


def duplicate_pairs(n=500, seed=4):
    """Duplicated vertices: B == C, A == B, A == C, A == B == C."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _triangles(rng, n)
    kind = rng.integers(0, 4, n)[:, None]
    e2 = np.where(kind == 0, e1, np.where(kind >= 2, 0.0, e2))
    e1 = np.where((kind == 1) | (kind == 3), 0.0, e1)
    p = v0 + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-4, 0.5, (n, 1))
    return _pack(p, v0, e1, e2)


def plane_and_far_pairs(n=1000, seed=5):
    """Points in the triangle's plane (inside and around it) and points hundreds of edge lengths away."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _triangles(rng, n)
    bu, bv = rng.uniform(-0.5, 1.5, (n, 1)), rng.uniform(-0.5, 1.5, (n, 1))
    in_plane = v0 + bu * e1 + bv * e2
    far = v0 + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(1, 3, (n, 1))
    return _pack(np.where(rng.random((n, 1)) < 0.5, in_plane, far), v0, e1, e2)


def scaled(pairs, scale):
    return (np.asarray(pairs, np.float32) * np.float32(scale)).astype(np.float32)


def pair_sets():
    """name -> (n, 12) float32: the five sets at the three scales (about 20 000 pairs)."""
    base = dict(random=random_pairs(), boundary=boundary_pairs(), needle=needle_pairs(), duplicate=duplicate_pairs(), plane_far=plane_and_far_pairs())
    return {f"{name} x {scale:g}": scaled(pairs, scale) for name, pairs in base.items() for scale in SCALES}


def special_pairs():
    """Pairs with non-finite numbers and numbers whose products overflow: (pairs, rows whose POINT is not finite)."""
    rng = np.random.default_rng(6)
    base = random_pairs(96, seed=7)
    rows = []
    for i, bad in enumerate([np.nan, np.inf, -np.inf]):
        for c in range(3):
            r = base[3 * i + c].copy(); r[c] = bad; rows.append(r)
    n_point = len(rows)
    for i, bad in enumerate([np.nan, np.inf, -np.inf]):
        for c in range(3, 12):
            r = base[9 + 9 * i + (c - 3)].copy(); r[c] = bad; rows.append(r)
    for k in range(12):
        r = base[40 + k].copy(); r[3:] *= np.float32(1e30) if k % 2 else np.float32(1e19); rows.append(r)      # e . e overflows / almost
        r = base[60 + k].copy(); r[:3] = rng.normal(size=3) * 1e25; rows.append(r)
    return np.array(rows, np.float32), n_point
