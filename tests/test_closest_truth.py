"""tests/probe_scenes.py and tests/ray_truth.py's judge_closest_triangle on the CPU, with the oracle's own answers: the colour codes
survive the oracle's shading for every index, the oracle's mirror ray, stand-in G-buffer and raytraced path carry no violation at three
units of length, the ray logs have the shape the GPU tests rely on, the inputs reach what those tests are for (hits, ties, candidates
decided again in binary64, rays outside the band) and the verdict catches each kind of planted error -- the tie rule included."""
import numpy as np
import pytest

from tests import probe_scenes as ps
from tests import ray_truth as rt

W, H = ps.W, ps.H
HYBRID = [(name, scale) for name in ps.NAMES for scale in rt.SCALES]
RAYTRACED = [(name, scale) for name in ps.NAMES for scale in ps.RAYTRACED_SCALES]
NEARER, MISS, UNKNOWN, TIE = ("a nearer true hit was lost", "miss, but a true hit exists", "hit on a triangle that is no exact hit and not in the band",
                              "tie not broken towards the smaller flat index")


def _probes(oracle, name, scale):
    """what -> Probe, for every observable the case has at this scale."""
    out = {}
    if scale in rt.SCALES:
        c = ps.hybrid_case(oracle, name, scale)
        out["mirror"], out["G-buffer"] = c["mirror"], c["primary"]
    if scale in ps.RAYTRACED_SCALES:
        out["raytraced"] = ps.raytraced_case(oracle, name, scale)["primary"]
    return out


ALL = sorted(set(HYBRID) | set(RAYTRACED))


# --------------------------------------------------------------------------------------------- 1. round trip
def test_every_index_survives_the_oracles_shading(oracle):
    """A gallery of 2 018 triangles (soup 3's count: every digit in every channel), each 4 x 4 pixels of the image: the index the oracle's
    closest hit names for the logged ray is the index decoded from NORMALS.w, from reflection_hit.rchit's payload (a G-buffer with N = 0 at
    the near plane sends the mirror ray down the view ray) and from the raytraced path's image, and every index appears in each."""
    from vulkanhybridrenderer_amd import abi, camera
    n = 2018
    Wg, Hg = ps.gallery_size(n)
    for what in ("hybrid", "raytraced"):
        scene = ps.gallery(n, ps.MIRROR_LEVELS if what == "hybrid" else ps.RAYTRACED_LEVELS)
        osc = oracle.Scene(scene)
        pfd = camera.dolly_frames(scene, Wg, Hg, 2)[1]
        images = []
        if what == "hybrid":
            pfd["directional_light"]["intensity"][:3] = 0.0
            with oracle.Audit(ray_log=2 * Wg * Hg) as a:
                gbuf = osc.gbuffer(pfd, Wg, Hg)
            images.append(("NORMALS.w", oracle.RAY_KIND_PRIMARY, a.ray_log, lambda pix: ps.decode_ids(gbuf[0].reshape(-1, 4)[pix], gbuf[2].reshape(-1)[pix] != 0, n)))
            tp = abi.default_trace_params(shadow=False, ao_spp=0, reflections=True)
            with oracle.Audit(ray_log=2 * Wg * Hg) as b:
                refl = osc.raygen(pfd, tp, np.zeros((Hg, Wg, 4), np.uint16), np.ones((Hg, Wg), np.float32))[1]
            images.append(("mirror payload", oracle.RAY_KIND_MIRROR, b.ray_log, lambda pix: ps.decode_mirror(refl.reshape(-1, 4)[pix], n)))
        else:
            pfd["directional_light"]["color"][:3] = 0.0
            with oracle.Audit(ray_log=2 * Wg * Hg) as a:
                image, _ = osc.raytraced(pfd, Wg, Hg, False)
            images.append(("raytraced image", oracle.RAY_KIND_PRIMARY, a.ray_log, lambda pix: ps.decode_raytraced(image.reshape(-1, 4)[pix], n)))
        for name, kind, log, decode in images:
            pix, rays = ps.rays_of(log, kind, Wg * Hg)
            assert len(pix) == Wg * Hg
            hit, flat = decode(pix)
            (want_hit, want_flat, _, _, _), _ = rt.oracle_answers(osc, rays, True)
            assert np.array_equal(hit, want_hit) and np.array_equal(flat[hit], want_flat[hit]), name
            seen = np.bincount(flat[hit], minlength=n)
            assert (seen >= 4).all(), f"{name}: indices {np.nonzero(seen < 4)[0][:8].tolist()} reach fewer than 4 pixels"


# --------------------------------------------------------------------------------------------- 2. clean verdict
@pytest.mark.parametrize("name,scale", ALL)
def test_the_oracles_answers_carry_no_violation(oracle, name, scale):
    for what, p in _probes(oracle, name, scale).items():
        v = rt.judge_closest_triangle(p.truth, p.hit, p.flat)
        print(f"{name} x {scale}, {what}: {v.violations} violations of {len(p.rays)} rays, hit share {p.hit.mean():.3f}, ties {v.ties}, explained D {v.explained_d} / passed over {v.explained_lost}, escalated {p.escalated}")
        assert v.violations == 0, f"{name} x {scale}, {what}: {v.describe()}"
        # outside the band the answer IS the exact closest hit
        xhit, xflat, _ = p.truth.closest()
        clear = ~p.truth.band_rays
        assert np.array_equal(p.hit[clear], xhit[clear]) and np.array_equal(p.flat[clear & xhit], xflat[clear & xhit])


def test_the_oracles_answers_on_the_1000_fold_mix(oracle):
    c = ps.hybrid_case(oracle, "tiny_far", 1.0)
    for what in ("mirror", "primary"):
        p = c[what]
        v = rt.judge_closest_triangle(p.truth, p.hit, p.flat)
        assert v.violations == 0, f"tiny_far, {what}: {v.describe()}"
        assert p.hit.mean() > 0.5


# --------------------------------------------------------------------------------------------- 3. log shape
@pytest.mark.parametrize("name", ps.NAMES)
def test_the_ray_logs_of_the_gbuffer_and_the_raytraced_path(oracle, name):
    """One PRIMARY ray per pixel from orc_gbuffer; from orc_raytraced one per pixel and one SHADOW ray per primary hit, at the hit's
    pixel; pixels unique per kind; pixel and kind are reset after the loops."""
    c = ps.hybrid_case(oracle, name, 1.0)
    log = c["log_g"]
    assert (log["kind"] == oracle.RAY_KIND_PRIMARY).all() and np.array_equal(np.sort(log["pixel"]), np.arange(W * H))
    assert (log["tmin"] == 1.0).all()                                        # the near plane, in units of the unnormalised direction
    assert (c["log_m"]["kind"] == oracle.RAY_KIND_MIRROR).all() and np.array_equal(np.sort(c["log_m"]["pixel"]), np.nonzero(c["gbuf"][2].reshape(-1) != 0)[0])
    r = ps.raytraced_case(oracle, name, 1.0)
    log, p = r["log"], r["primary"]
    assert set(np.unique(log["kind"]).tolist()) == {oracle.RAY_KIND_PRIMARY, oracle.RAY_KIND_SHADOW}
    assert np.array_equal(np.sort(p.pix), np.arange(W * H))
    shadow = log[log["kind"] == oracle.RAY_KIND_SHADOW]
    assert np.array_equal(np.sort(shadow["pixel"]), np.sort(p.pix[p.hit])) and len(log) == W * H + int(p.hit.sum())
    assert (log["tmin"] == np.float32(0.1)).all() and (log["tmax"] == 10000.0).all()
    with oracle.Audit(ray_log=4) as a:
        c["osc"].closest(p.rays[0, 0:3], p.rays[0, 4:7], 0.0, 1e30)
    assert (a.ray_log["kind"] == oracle.RAY_KIND_OTHER).all() and (a.ray_log["pixel"] == 0xFFFFFFFF).all() and len(a.ray_log) == 1


# --------------------------------------------------------------------------------------------- 4. input conditions
@pytest.mark.parametrize("name,scale", ALL)
def test_the_inputs_reach_what_the_gpu_tests_are_for(oracle, name, scale):
    """What keeps tests/test_gpu_closest_truth.py from being vacuous: the rays hit, nearly all of them lie outside the band (where the
    verdict has no excuse to offer), at least 50 of them have a duplicate triangle in front, and at 2^10 the oracle's own walk meets
    candidates that contradict themselves."""
    for what, p in _probes(oracle, name, scale).items():
        T = p.truth
        if what == "mirror":
            assert p.hit.mean() >= 0.5
        else:
            assert p.hit.sum() >= 0.9 * W * H
        assert (~T.band_rays).mean() >= 0.99, (what, int(T.band_rays.sum()))
        ties = ps.front_ties(T)
        assert ties.sum() >= 50 and rt.judge_closest_triangle(T, p.hit, p.flat).ties >= 50, (what, int(ties.sum()))
        if scale == 2.0 ** 10:
            assert p.escalated > 0, what


# --------------------------------------------------------------------------------------------- 5. the judge bites
def _second_nearest(T):
    """Per ray the second exact hit in (t, flat) order, where it lies behind the first by more than both t bounds: pair index or -1."""
    order = np.lexsort((T.flat, T.t, T.ray))
    order = order[T.hit[order]]
    r = T.ray[order]
    first = np.ones(len(order), bool)
    first[1:] = r[1:] != r[:-1]
    i = np.nonzero(first)[0]
    i = i[i + 1 < len(order)]
    i = i[r[i + 1] == r[i]]
    a, b = order[i], order[i + 1]
    far = T.t[b] - T.t[a] > T.et[a] + T.et[b]
    out = np.full(T.n, -1)
    out[T.ray[a[far]]] = b[far]
    return out


def _larger_twin(T, flat, rays):
    """For each of `rays` (answer flat[ray], an exact hit): the smallest larger flat index among the ray's exact hits whose world record
    equals the answer's bit for bit, or -1."""
    same = rt.identical_records(T.tris)
    out = np.full(len(rays), -1)
    for n_, r in enumerate(rays):
        sel = T.hit & (T.ray == r) & (same[T.flat] == same[flat[r]]) & (T.flat > flat[r])
        if sel.any():
            out[n_] = T.flat[sel].min()
    return out


@pytest.mark.parametrize("name", ps.NAMES)
def test_planted_errors_are_caught(oracle, name):
    """The oracle's mirror-ray answers at scale 1, mutated four ways: every mutated ray outside the band is flagged, for the right
    reason, and no other ray is; and a payload half a level off does not decode."""
    p = ps.hybrid_case(oracle, name, 1.0)["mirror"]
    T = p.truth
    clear = ~T.band_rays
    rng = np.random.default_rng(11)

    def judged(rays, new_hit, new_flat, reason, at_least):
        rays = rays[clear[rays]]
        assert len(rays) >= at_least, (reason, len(rays))
        hit, flat = p.hit.copy(), p.flat.copy()
        hit[rays], flat[rays] = new_hit, new_flat[rays] if new_flat is not None else 0
        v = rt.judge_closest_triangle(T, hit, flat)
        if reason is not None:
            assert np.isin(rays, v.reasons[reason]).all(), f"{reason}: {int((~np.isin(rays, v.reasons[reason])).sum())} of {len(rays)} mutated rays are not flagged for it"
        assert v.bad[rays].all() and v.violations == len(rays), v.describe()
        return v

    second = _second_nearest(T)
    judged(np.nonzero(p.hit & (second >= 0))[0], True, np.where(second >= 0, T.flat[np.maximum(second, 0)], 0), NEARER, 500 if name == "soup 3" else 100)
    judged(np.nonzero(p.hit)[0], False, None, MISS, 2000)
    other = (p.flat + rng.integers(1, T.ntris, T.n)) % T.ntris               # any triangle but the answer
    v = judged(np.nonzero(p.hit)[0], True, other, None, 2000)
    assert len(v.reasons[UNKNOWN]) > 0.9 * v.violations                    # (a random triangle is rarely another exact hit of the ray)
    tied = np.nonzero(ps.front_ties(T) & p.hit)[0]
    twin = np.full(T.n, -1)
    twin[tied] = _larger_twin(T, p.flat, tied)
    assert (twin[tied] >= 0).all() and len(tied) >= 50                       # every front tie of a soup is a duplicate triangle
    v = judged(tied, True, twin, TIE, 50)
    assert v.violations == len(v.reasons[TIE])                               # ... and nothing but the tie clause sees it
    # the decoder: half a level is farther than a quarter from every level
    bits = ps.hybrid_case(oracle, name, 1.0)["reflections"].reshape(-1, 4)[p.pix[p.hit]][:64]
    assert ps.decode_mirror(bits)[0].all()
    moved = bits.view(np.float16).astype(np.float32)
    moved[5, 1] += np.float32(0.5 / 16 * ps.MIRROR_AMBIENT)
    with pytest.raises(ps.Undecodable):
        ps.decode_mirror(moved.astype(np.float16).view(np.uint16))


def test_the_decoders_refuse_what_is_off_the_table():
    flat = np.arange(2018)
    hit, back = ps.decode_mirror(ps.encode_mirror(flat), 2018)
    assert hit.all() and np.array_equal(back, flat)
    with pytest.raises(ps.Undecodable):                                      # beyond the scene
        ps.decode_mirror(ps.encode_mirror(flat), 2000)
    good = ps.encode_mirror(flat[:8]).view(np.float16).astype(np.float32)
    for channel, value in ((0, 15 / 16 * ps.MIRROR_AMBIENT), (2, 0.0), (1, np.nan), (3, 0.5)):     # digit 14, digit -1, NaN, a fractional alpha
        bad = good.copy()
        bad[3, channel] = value
        with pytest.raises(ps.Undecodable):
            ps.decode_mirror(bad.astype(np.float16).view(np.uint16))
    code = 5 * (ps.digits(flat) + 1)
    bgra = np.concatenate([code[:, ::-1], np.full((len(flat), 1), 255)], 1).astype(np.uint8)
    for delta in (-1, 0, 1):                                                  # one code value off still decodes, two do not
        hit, back = ps.decode_raytraced((bgra.astype(int) + [delta, delta, delta, 0]).astype(np.uint8), 2018)
        assert hit.all() and np.array_equal(back, flat)
    for delta in (-2, 2, 3):
        with pytest.raises(ps.Undecodable):
            ps.decode_raytraced((bgra[:4].astype(int) + [0, delta, 0, 0]).astype(np.uint8))
    miss = np.array([ps.RAYTRACED_MISS_BGRA], np.uint8)
    assert not ps.decode_raytraced(miss)[0].any()
    normals = np.zeros((4, 4), np.float16)
    normals[:, 2], normals[:, 3] = 1.0, [0, 7, 2017, 2047]
    assert np.array_equal(ps.decode_ids(normals.view(np.uint16))[1], [0, 7, 2017, 2047])
    for w in (0.5, -1.0, np.nan, 2048.0):
        normals[1, 3] = w
        with pytest.raises(ps.Undecodable):
            ps.decode_ids(normals.view(np.uint16), np.ones(4, bool))
    with pytest.raises(ps.Undecodable):
        ps.decode_ids(np.float16([[0, 0, 1, 300]]).view(np.uint16), count=298)
