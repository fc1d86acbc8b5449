"""Ray answers judged against exact arithmetic.  TEST INFRASTRUCTURE (tests/test_ray_truth.py, tests/test_gpu_ray_truth.py,
tests/test_closest_truth.py, tests/test_gpu_closest_truth.py, tools/ray_truth_scale.py, tools/audit_decision_vi.py).

The truth of a ray is what oracle/vhr_oracle.c's orc_ray_truth returns for it -- every triangle of the scene decided without rounding
(oracle/vhr_exact.h; the pairs its binary64 filter leaves open are settled here with tests/exact_rational.py, so no ray is ever left
out), no boxes involved -- reduced to the pairs that matter:

    X   the exact hits of the ray, each with its exact (t, u, v) and fp32 Moeller-Trumbore's forward error bounds (et, eu, ev);
    N   the exact misses inside the band: the exact (u, v, t) lies within those bounds of a decision border (margin <= 1), so an fp32
        evaluation of the formulas may call the pair a hit and nobody can blame it (class D, explained) -- and the numerators allow a
        hit at all (numerators_allow_a_hit: what keeps nearly collinear triangles from putting every ray of a scene into the band).

A pair is "explained" when its margin is <= 1.  The verdict on an answer (the device's or the oracle's):

    closest hit, answer (k, t, u, v):  k in X -> |t - xt| <= et, |u - xu| <= eu, |v - xv| <= ev;   k not in X -> k in N;
                                       every j in X with xt_j < xt_k - (et_j + et_k) is explained (else a nearer true hit was lost);
    closest hit, answer "miss":        every j in X is explained;
    closest hit, answer k alone:       the same without the clause on (t, u, v), and no j < k in X whose world record equals k's bit for bit
                                       (judge_closest_triangle: for images that name the triangle and carry no t, u, v);
    any hit, "occluded":               X or N is not empty;          any hit, "not occluded": every j in X is explained.

The bounds are derived, not tuned: k = 8 * 2^-24 (7 roundings to a numerator, the reciprocal and the product) times the permanents of
the polynomials, mt_error_bounds() below -- the one definition; orc_ray_truth restates it operation by operation and
tests/test_ray_truth.py holds the two equal.  None of this depends on a hierarchy: a box can only cull points outside it and a true hit
is never outside, so the verdict holds where bit-identity with the oracle is no longer the right contract (other units of length,
1000-fold mixed scales)."""
import dataclasses

import numpy as np

from tests import exact_rational
from vulkanhybridrenderer_amd import abi, scenes

EPS = 2.0 ** -24
K = 8 * EPS                                           # 7 roundings to a numerator + the reciprocal and the product
SCALES = (2.0 ** -10, 1.0, 2.0 ** 10)


def _pcross(a, b):
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _pdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mt_error_bounds(o, d, v0, e1, e2, tmin, tmax, xdet, xu, xv, xt):
    """fp32 Moeller-Trumbore's forward error bounds on (u, v, t) around the exact values, and the margin: how far, in units of those
    bounds, the exact (u, v, t) sits from the nearest decision border.  Arrays of pairs ((..., 3) vectors, (...) scalars), binary64
    throughout -> (eu, ev, et, margin).  An exact determinant of 0 has no bounds (inf) and margin 0."""
    o, d, v0, e1, e2 = (np.abs(np.asarray(x, np.float64)) for x in (o, d, v0, e1, e2))
    tmin, tmax, xdet, xu, xv, xt = (np.asarray(x, np.float64) for x in (tmin, tmax, xdet, xu, xv, xt))
    tv = o + v0
    ppv, pqv = _pcross(d, e2), _pcross(tv, e1)
    pdet, pun, pvn, ptn = _pdot(e1, ppv), _pdot(tv, ppv), _pdot(d, pqv), _pdot(e2, pqv)
    det = np.abs(xdet)
    with np.errstate(divide="ignore", invalid="ignore"):
        eu = K * (pun + np.abs(xu) * pdet) / det
        ev = K * (pvn + np.abs(xv) * pdet) / det
        et = K * (ptn + np.abs(xt) * pdet) / det
        margins = [np.abs(xu) / eu, np.abs(1 - xu) / eu, np.abs(xv) / ev, np.abs(1 - xu - xv) / (eu + ev + EPS), np.abs(xt - tmin) / et,
                   np.abs(tmax - xt) / et]
        margin = margins[0]
        for m in margins[1:]:
            margin = np.where(m < margin, m, margin)          # (python's min(): the first of equals, a leading NaN stays)
    zero = det == 0
    inf = np.float64(np.inf)
    return np.where(zero, inf, eu), np.where(zero, inf, ev), np.where(zero, inf, et), np.where(zero, 0.0, margin)


def numerators_allow_a_hit(o, d, v0, e1, e2):
    """A second necessary condition for an fp32 Moeller-Trumbore hit, on the numerators: the margin above divides by the exact
    determinant, so on a triangle whose determinant's own relative error reaches 1 (three nearly collinear vertices; a soup has dozens)
    its bounds are infinite and EVERY ray of the scene would have a pair "in the band" -- the verdict would excuse anything.  But an fp32
    hit needs 0 <= fl(u) <= 1 and 0 <= fl(v) <= 1, that is |fl(un)| <= |fl(det)| (1 + 3 eps) and the same for vn, and with
    |fl(x) - x| <= 8 eps P(x) for the three polynomials (7 roundings at most)
          |un| <= |det| + 2 K (P(un) + P(det)),     |vn| <= |det| + 2 K (P(vn) + P(det))                        (K = 8 eps; 2: slack)
    must hold for the exact values.  A pair that fails either cannot be an fp32 hit whatever its margin says; N is the band intersected
    with this.  The polynomials are evaluated in binary64 as in oracle/vhr_exact.h (error <= 64 * 2^-53 P, far below K P).
    -> (allowed, certainly an exact miss: |un| or |vn| exceeds |det| by more than binary64's own error)."""
    o, d, v0, e1, e2 = (np.asarray(x, np.float64) for x in (o, d, v0, e1, e2))
    tv, atv = o - v0, np.abs(o) + np.abs(v0)
    pv, qv = np.cross(d, e2), np.cross(tv, e1)
    ppv, pqv = _pcross(np.abs(d), np.abs(e2)), _pcross(atv, np.abs(e1))
    det, un, vn = np.abs(_pdot(e1, pv)), np.abs(_pdot(tv, pv)), np.abs(_pdot(d, qv))
    pdet, pun, pvn = _pdot(np.abs(e1), ppv), _pdot(atv, ppv), _pdot(np.abs(d), pqv)
    B = 64 * 2.0 ** -53
    with np.errstate(invalid="ignore"):
        allowed = ~((un > det + 2 * K * (pun + pdet) + B * (pun + pdet)) | (vn > det + 2 * K * (pvn + pdet) + B * (pvn + pdet)))
        certain = (un - B * pun > det + B * pdet) | (vn - B * pvn > det + B * pdet)
    return allowed, certain


def mt_error_margin(rec):
    """The margin of one audit record (oracle.binding.audit_record_dtype): <= 1 means inside the band where the rounding of the fp32
    evaluation decides."""
    return float(mt_error_bounds(rec["o"], rec["d"], rec["v0"], rec["e1"], rec["e2"], rec["tmin"], rec["tmax"], rec["xdet"], rec["xu"],
                                 rec["xv"], rec["xt"])[3])


# ---------------------------------------------------------------------------------------------
# scenes and rays in another unit of length
# ---------------------------------------------------------------------------------------------
def scaled_scene(scene, s):
    """Every length of the scene times s (a power of two: exact in fp32): vertex positions, the transforms' translations, the camera's
    position, near plane and dolly.  Rotations, normals and the light's direction are untouched."""
    s = np.float32(s)
    v, p = scene.vertices.copy(), scene.primitives.copy()
    v["pos"] *= s
    p["transform"][:, 12:15] *= s
    cam = dict(scene.camera)
    for k in ("position", "dolly"):
        cam[k] = tuple(float(c) * float(s) for c in cam[k])
    cam["znear"] = float(cam["znear"]) * float(s)
    if cam.get("world") is not None:
        w = np.array(cam["world"], np.float64)
        w[:3, 3] *= float(s)
        cam["world"] = w
    return dataclasses.replace(scene, vertices=v, primitives=p, camera=cam)


def scaled_rays(rays, s):
    """Origins, tmin and tmax times s; directions untouched."""
    r = np.array(rays, np.float32)
    r[:, 0:4] *= np.float32(s)
    r[:, 7] *= np.float32(s)
    return r


def scaled_trace_params(tp, s):
    tp = tp.copy()
    for k in ("ao_tmax", "normal_bias", "tmin", "tmax"):
        tp[k] = np.float32(tp[k]) * np.float32(s)
    return tp


def tiny_far(choices=(1e-3, 1.0, 1.0, 1.0, 1e3)):
    """tests/test_gpu_edge_cases.py::test_scene_far_from_the_origin_with_mixed_scales' scene -- coordinates around 12 345, vertices scaled
    at random -- with the 1000-fold mix that test had to leave out (the oracle's own BVH then differs from its brute force)."""
    rng = np.random.default_rng(9)
    tiny = scenes.tiny_scene()
    v = tiny.vertices.copy()
    centre = np.float32(12345.678)
    scale = rng.choice(np.array(choices, np.float32), size=(len(v), 1)).astype(np.float32)
    v["pos"] = v["pos"] * scale + centre
    cam = dict(tiny.camera)
    cam["position"] = tuple(float(c) + float(centre) for c in cam["position"])
    return dataclasses.replace(tiny, name="tiny_far", vertices=v, camera=cam)


def grazing_rays(tris, rng, n):
    """tests/test_gpu_ray_query.py::_grazing_rays on explicit world triangles ((m, 3, 3) float64): rays in or within 1e-7..1e-3 of the
    planes of the non-degenerate ones, through their interiors, edges and corners."""
    k = rng.integers(0, len(tris), n)
    v0, e1, e2 = tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]
    keep = np.linalg.norm(np.cross(e1, e2), axis=1) > 1e-6
    v0, e1, e2 = v0[keep], e1[keep], e2[keep]
    n = len(v0)
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    kind = rng.integers(0, 4, n)
    bu, bv = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = bu + bv > 1
    bu[flip], bv[flip] = 1 - bu[flip], 1 - bv[flip]
    bu[kind == 1] = 0.0
    bv[kind == 2] = 1.0 - bu[kind == 2]
    bu[kind == 3], bv[kind == 3] = 0.0, 0.0
    point = v0 + bu[:, None] * e1 + bv[:, None] * e2
    along = e1 * rng.normal(size=(n, 1)) + e2 * rng.normal(size=(n, 1))
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    d = along + rng.choice([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3], n)[:, None] * nrm
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = point - 10.0 ** rng.uniform(-2, 0.5, (n, 1)) * d
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3], rays[:, 7] = rng.choice([0.0, 1e-3], n), rng.choice([np.inf, 1e4], n)
    return rays


def flat_offsets(scene):
    """First flat triangle index of every primitive (flat order: primitive-major, triangle-minor)."""
    counts = scene.primitives["index_count"].astype(np.int64) // 3
    return np.concatenate([[0], np.cumsum(counts)[:-1]])


def flat_of_hits(scene, hits):
    """abi.ray_hit_dtype answers -> (hit bool[n], flat triangle index int64[n] (0 where the ray missed))."""
    hit = hits["geometry_index"] != abi.RAY_MISS
    g = np.where(hit, hits["geometry_index"], 0).astype(np.int64)
    off = flat_offsets(scene)
    flat = off[np.minimum(g, len(off) - 1)] + np.where(hit, hits["primitive_index"], 0).astype(np.int64)
    return hit, flat


# ---------------------------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------------------------
class Truth:
    """The pairs that matter of a batch of rays on oracle.binding.Scene `osc`, sorted by (ray, flat): ray, flat, hit (in X; else in N),
    exact t / u / v, bounds et / eu / ev, margin.  `undecided` counts the pairs python Fractions had to settle."""

    def __init__(self, ob, osc, rays, prim_masks=None, ray_masks=None, cull_mask=0xFF):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        offsets, pairs = ob.ray_truth(osc, rays, prim_masks, ray_masks, cull_mask)
        self.n, self.ntris = len(rays), int(osc.triangle_count)
        ray = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(offsets))
        tris, _ = osc.triangles()
        self.tris = tris                                   # (ntris, 3, 3) float32 world records (v0, e1, e2): judge_closest_triangle's ties
        keep = np.ones(len(pairs), bool)
        # exact misses and open pairs: could fp32 call them a hit at all?  (numerators_allow_a_hit)
        cand = np.nonzero(pairs["decision"] != 1)[0]
        r, tr = rays[ray[cand]], tris[pairs["flat"][cand]]
        allowed, certain_miss = numerators_allow_a_hit(r[:, 0:3], r[:, 4:7], tr[:, 0], tr[:, 1], tr[:, 2])
        is_open = pairs["decision"][cand] < 0
        settled_miss = is_open & certain_miss
        pairs["decision"][cand[settled_miss]] = 0
        keep[cand] = allowed & ~(settled_miss & ~(pairs["margin"][cand] <= 1))
        open_ = cand[is_open & ~certain_miss]
        self.undecided = len(open_)
        if len(open_):
            val = np.zeros((len(open_), 4))
            hit = np.zeros(len(open_), bool)
            for n_, i in enumerate(open_):
                r, tr = rays[ray[i]], tris[pairs["flat"][i]]
                hit[n_], q = exact_rational.ray_triangle(r[0:3], r[4:7], tr[0], tr[1], tr[2], r[3], r[7])
                val[n_] = [0.0, np.nan, np.nan, np.nan] if q is None else [float(x) for x in q]
            r, tr = rays[ray[open_]], tris[pairs["flat"][open_]]
            eu, ev, et, margin = mt_error_bounds(r[:, 0:3], r[:, 4:7], tr[:, 0], tr[:, 1], tr[:, 2], r[:, 3], r[:, 7], *val.T)
            pairs["decision"][open_] = hit
            for name, a in (("det", val[:, 0]), ("u", val[:, 1]), ("v", val[:, 2]), ("t", val[:, 3]), ("eu", eu), ("ev", ev), ("et", et), ("margin", margin)):
                pairs[name][open_] = a
            keep[open_] = hit | ((margin <= 1) & keep[open_])
        self.open_rays = np.bincount(ray[open_], minlength=self.n) > 0
        pairs, ray = pairs[keep], ray[keep]
        self.ray, self.flat, self.hit = ray, pairs["flat"].astype(np.int64), pairs["decision"] == 1
        self.t, self.u, self.v = pairs["t"], pairs["u"], pairs["v"]
        self.et, self.eu, self.ev, self.margin = pairs["et"], pairs["eu"], pairs["ev"], pairs["margin"]
        self.explained = self.margin <= 1
        self.key = self.ray * self.ntris + self.flat
        assert (np.diff(self.key) > 0).all()
        self.hits_per_ray = np.bincount(self.ray[self.hit], minlength=self.n)
        self.pairs_per_ray = np.bincount(self.ray, minlength=self.n)
        # rays with a band pair (a member of N, or an exact hit inside the band) or one python Fractions had to settle: where the
        # verdict may not bite
        self.band_rays = (np.bincount(self.ray[self.explained], minlength=self.n) > 0) | self.open_rays

    def find(self, flat, where):
        """Index of the pair (ray i, flat[i]) for the rays of `where`, and whether it exists."""
        q = np.arange(self.n, dtype=np.int64) * self.ntris + np.where(where, np.asarray(flat, np.int64), 0)
        if not len(self.key):
            return np.zeros(self.n, np.int64), np.zeros(self.n, bool)
        idx = np.minimum(np.searchsorted(self.key, q), len(self.key) - 1)
        return idx, where & (self.key[idx] == q) & (np.asarray(flat, np.int64) >= 0) & (np.asarray(flat, np.int64) < self.ntris)

    def closest(self):
        """The exact closest hit per ray: (hit bool[n], flat int64[n], t float64[n]); ties go to the smaller flat index."""
        hit = self.hits_per_ray > 0
        flat, t = np.zeros(self.n, np.int64), np.full(self.n, np.inf)
        order = np.lexsort((self.flat, self.t, self.ray))
        order = order[self.hit[order]]
        first = np.ones(len(order), bool)
        first[1:] = self.ray[order][1:] != self.ray[order][:-1]
        flat[self.ray[order][first]], t[self.ray[order][first]] = self.flat[order][first], self.t[order][first]
        return hit, flat, t


@dataclasses.dataclass
class Verdict:
    bad: np.ndarray                   # bool per ray
    reasons: dict                     # name -> ray indices
    explained_d: int = 0              # answers on a triangle of N (class D, explained)
    explained_lost: int = 0           # true hits the answer passed over that lie inside the band (class E / C, explained)
    ties: int = 0                     # judge_closest_triangle: answers in X that share their world record with another exact hit of the ray

    @property
    def violations(self):
        return int(self.bad.sum())

    def describe(self, limit=4):
        return "; ".join(f"{k}: {len(v)} rays, first {v[:limit].tolist()}" for k, v in self.reasons.items() if len(v)) or "clean"


def _over(truth, cond):
    return np.bincount(truth.ray[cond], minlength=truth.n) > 0


def judge_closest(truth, hit, flat, t, u, v):
    """The verdict on closest-hit answers: hit bool[n]; flat triangle index, t, u, v per ray (read where hit)."""
    T = truth
    hit = np.asarray(hit, bool)
    t, u, v = (np.asarray(x, np.float64) for x in (t, u, v))
    idx, found = T.find(flat, hit)
    unknown = hit & ~found                                           # neither an exact hit nor an exact miss inside the band
    in_x = found & T.hit[idx] if len(T.key) else found
    with np.errstate(invalid="ignore"):
        values = in_x & ~((np.abs(t - T.t[idx]) <= T.et[idx]) & (np.abs(u - T.u[idx]) <= T.eu[idx]) & (np.abs(v - T.v[idx]) <= T.ev[idx])) if len(T.key) else in_x
        xt_k, et_k = (np.where(found, T.t[idx], np.nan), np.where(found, T.et[idx], np.nan)) if len(T.key) else (np.full(T.n, np.nan),) * 2
        passed = T.hit & found[T.ray] & (T.t < xt_k[T.ray] - (T.et + et_k[T.ray]))       # true hits in front of the answer
    nearer = _over(T, passed & ~T.explained)
    lost = _over(T, T.hit & ~hit[T.ray] & ~T.explained)             # answer "miss" with an unexplained true hit
    reasons = {"hit on a triangle that is no exact hit and not in the band": np.nonzero(unknown)[0],
               "t, u or v beyond fp32's error bound": np.nonzero(values)[0], "a nearer true hit was lost": np.nonzero(nearer)[0],
               "miss, but a true hit exists": np.nonzero(lost)[0]}
    return Verdict(unknown | values | nearer | lost, reasons, int((found & ~in_x).sum()),
                   int((passed & T.explained).sum() + (T.hit & ~hit[T.ray] & T.explained).sum()))


def identical_records(world_tris):
    """(n, 3, 3) float32 world records -> int64[n]: the smallest flat index whose (v0, e1, e2) equals this one's bit for bit."""
    rec = np.ascontiguousarray(world_tris, np.float32).reshape(len(world_tris), 9).view(np.uint32)
    _, first, inverse = np.unique(rec, axis=0, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)].astype(np.int64)                # (np.unique's first occurrence is the smallest index)


def judge_closest_triangle(truth, hit, flat, world_tris=None):
    """The verdict on WHICH triangle a closest-hit answer names, for answers that carry no (t, u, v) (an image that encodes the triangle):
    judge_closest's clauses with the found pair's own exact values, so its clause on the values never fires, and one more --

        ties:  the answer k is in X and some j < k in X has a world record (v0, e1, e2) identical to k's bit for bit.

    Identical operands give identical (t, u, v) in fp32 and in binary64, in every walker, so "min t, then the smaller flat index" decides
    that case with no excuse: no band is consulted.  world_tris: (ntris, 3, 3) float32, default the truth's own scene."""
    T = truth
    hit, flat = np.asarray(hit, bool), np.asarray(flat, np.int64)
    idx, found = T.find(flat, hit)
    own = [np.where(found, x[idx], 0.0) if len(T.key) else np.zeros(T.n) for x in (T.t, T.u, T.v)]
    v = judge_closest(T, hit, flat, *own)
    assert not len(v.reasons["t, u or v beyond fp32's error bound"])
    del v.reasons["t, u or v beyond fp32's error bound"]
    same = identical_records(T.tris if world_tris is None else world_tris)
    in_x = found & T.hit[idx] if len(T.key) else found
    k = np.where(in_x, flat, -1)
    twin = T.hit & in_x[T.ray] & (same[T.flat] == same[np.maximum(k, 0)[T.ray]]) & (T.flat != k[T.ray])      # another exact hit, same operands
    tie = _over(T, twin & (T.flat < k[T.ray]))                                                             # ... that comes first
    v.reasons["tie not broken towards the smaller flat index"] = np.nonzero(tie)[0]
    v.bad = v.bad | tie
    v.ties = int(_over(T, twin).sum())
    return v


def judge_any(truth, occluded):
    """The verdict on terminate-on-first-hit answers: occluded bool[n]."""
    T = truth
    occluded = np.asarray(occluded, bool)
    spurious = occluded & (T.pairs_per_ray == 0)
    leak = _over(T, T.hit & ~occluded[T.ray] & ~T.explained)
    reasons = {"occluded, but no exact hit and nothing in the band": np.nonzero(spurious)[0],
               "not occluded, but a true hit exists": np.nonzero(leak)[0]}
    return Verdict(spurious | leak, reasons, int((occluded & (T.hits_per_ray == 0)).sum()), int((T.hit & ~occluded[T.ray] & T.explained).sum()))


def oracle_answers(osc, rays, use_bvh):
    """The CPU oracle's closest hit (hit, flat, t, u, v) and any-hit booleans, one ray at a time."""
    n = len(rays)
    hit, occ = np.zeros(n, bool), np.zeros(n, bool)
    flat, tuv = np.zeros(n, np.int64), np.zeros((n, 3), np.float32)
    _, prim = osc.triangles()
    first = np.searchsorted(prim, np.arange(int(prim.max()) + 1 if len(prim) else 0))
    for i, r in enumerate(rays):
        h = osc.closest(r[0:3], r[4:7], float(r[3]), float(r[7]), use_bvh=use_bvh)
        if h is not None:
            hit[i], tuv[i], flat[i] = True, h[0:3], first[h[3]] + h[4]
        occ[i] = osc.occluded(r[0:3], r[4:7], float(r[3]), float(r[7]), use_bvh=use_bvh)
    return (hit, flat, tuv[:, 0], tuv[:, 1], tuv[:, 2]), occ


# ---------------------------------------------------------------------------------------------
# the cases both test modules and tools/ray_truth_scale.py share
# ---------------------------------------------------------------------------------------------
SOUPS = ((1, 60, 3), (2, 400, 5), (3, 2000, 8))


def soup_scene(seed):
    from tests.test_gpu_fuzz import soup
    return soup(*[s for s in SOUPS if s[0] == seed][0])


def soup_rays(scene, seed, n=8000):
    """The random set: origins in the scene's box grown by 0.2, isotropic directions, tmin in {0, 2^-7}, tmax in {inf, 4, 16, 8192}."""
    from vulkanhybridrenderer_amd import ray_queries
    lo, hi = ray_queries.scene_bounds(scene)
    return ray_queries.random_rays(np.random.default_rng(100 + seed), n, lo, hi, margin=0.2, tmins=(0.0, 2.0 ** -7), tmaxs=(np.inf, 4.0, 16.0, 8192.0))


def soup_grazing(scene, n=1500):
    """The grazing set: what reaches the band and the binary64 launch."""
    from vulkanhybridrenderer_amd import ray_queries
    return grazing_rays(ray_queries.world_triangles(scene), np.random.default_rng(7), n)


def tiny_far_rays(far, n=1500):
    """On tiny_far: n rays aimed at points of its triangles, n random ones and n grazing ones."""
    from vulkanhybridrenderer_amd import ray_queries
    rng = np.random.default_rng(31)
    tris = ray_queries.world_triangles(far)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    k = rng.integers(0, len(tris), n)
    b = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = (tris[k] * b[:, :, None]).sum(1)
    centre = np.median(tris.reshape(-1, 3), axis=0)
    o = centre + rng.normal(size=(n, 3)) * 3.0
    aimed = np.zeros((n, 8), np.float32)
    d = target - o
    aimed[:, 0:3], aimed[:, 4:7], aimed[:, 7] = o, d / np.linalg.norm(d, axis=1, keepdims=True), np.inf
    random = ray_queries.random_rays(rng, n, lo, hi, margin=0.2, tmins=(0.0, 2.0 ** -7), tmaxs=(np.inf, 16.0, 8192.0))
    near = ray_queries.random_rays(rng, n, centre - 4.0, centre + 4.0, margin=0.2, tmins=(0.0, 2.0 ** -7), tmaxs=(np.inf, 16.0, 8192.0))
    return np.concatenate([aimed, random[: n // 2], near[: n - n // 2], grazing_rays(tris, rng, n)])
