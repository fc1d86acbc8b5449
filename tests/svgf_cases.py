"""Input families for the a-trous kernels (TEST INFRASTRUCTURE): each is a function (W, H, step, seed) -> (normals_bits, integrated_bits),
two (H, W, 4) uint16 images of fp16 bit patterns -- (nx, ny, nz, object id) and (shadow, AO, shadow variance, AO variance).

helpers.synthetic_svgf_inputs draws ids and normals per 16 x 16 block, so at step 8 85 % of the taps are rejected by id and at step 16 the
expected output IS the input.  Here a family's surfaces grow with the step: families a-e keep >= 40 % of the in-image taps alive and change
>= 90 % of the pixels at every step they are used with (tests/test_atrous_reference.py asserts it from the binary64 tap count), f walks
through the id conversions, g rejects every tap.  Luminance and variance are never negative: the output is then a positive-weighted mean of
non-negative values and nothing cancels, which is what the one-fp16-step bar of tests/test_gpu_atrous_parity.py rests on."""
import numpy as np


def _bits(a):
    return np.asarray(a, np.float32).astype(np.float16).view(np.uint16)


def _blocks(rng, W, H, block, draw):
    """`draw(shape)` per block of `block` x `block` pixels, repeated over the image."""
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    v = draw((by, bx))
    return np.repeat(np.repeat(v, block, 0), block, 1)[:H, :W]


def _block_size(step):
    return 8 * step + 8          # (>= 4 * step + 8: a tap 2 * step away stays in the centre's block three times out of four)


def _surfaces(rng, W, H, step, noise=0.05):
    """Ids and coarse normals constant over blocks, small per-pixel normal noise: (H, W, 4) float32."""
    block = _block_size(step)
    coarse = _blocks(rng, W, H, block, lambda s: rng.normal(size=s + (3,)).astype(np.float32))
    nrm = coarse / np.linalg.norm(coarse, axis=-1, keepdims=True) + noise * rng.normal(size=(H, W, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    ids = _blocks(rng, W, H, block, lambda s: rng.integers(0, 103, size=s)).astype(np.float32)
    return np.concatenate([nrm, ids[..., None]], -1)


def _integrated(lum_s, lum_a, var_s, var_a):
    return _bits(np.stack([lum_s, lum_a, var_s, var_a], -1))


def _quantised_luminance(rng, W, H):
    """What K3 feeds K4 on frame 0: shadow in {0, 1}, AO in {0, .5, 1}."""
    return (rng.random((H, W)) < 0.7).astype(np.float32), rng.integers(0, 3, size=(H, W)).astype(np.float32) * 0.5


def live_taps(W, H, step, seed):
    """a: block surfaces with normal noise, luminance uniform in [0, 1], variance 0.3 r^2."""
    rng = np.random.default_rng([seed, 1])
    n = _surfaces(rng, W, H, step)
    return _bits(n), _integrated(rng.random((H, W)), rng.random((H, W)), 0.3 * rng.random((H, W)) ** 2, 0.3 * rng.random((H, W)) ** 2)


def one_surface(W, H, step, seed):
    """b: one id, identical normals (0, 0, 1): every in-image tap is accepted and the normal weight is exactly 1."""
    rng = np.random.default_rng([seed, 2])
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = 1.0
    n[..., 3] = 7.0
    return _bits(n), _integrated(rng.random((H, W)), rng.random((H, W)), 0.3 * rng.random((H, W)) ** 2, 0.3 * rng.random((H, W)) ** 2)


def variance_range(W, H, step, seed):
    """c: as a, variances log-uniform over 1e-7 .. 1e2 per pixel (fp16 subnormals, below 6.1e-5, included)."""
    rng = np.random.default_rng([seed, 3])
    n = _surfaces(rng, W, H, step)
    var = lambda: 10.0 ** rng.uniform(-7.0, 2.0, size=(H, W))          # noqa: E731
    return _bits(n), _integrated(rng.random((H, W)), rng.random((H, W)), var(), var())


def zero_variance(W, H, step, seed):
    """c, all-zero variant: 1 / 1e-6 in the exponent, so only taps of exactly equal luminance survive -- quantised luminance gives some."""
    rng = np.random.default_rng([seed, 4])
    n = _surfaces(rng, W, H, step)
    s, a = _quantised_luminance(rng, W, H)
    z = np.zeros((H, W), np.float32)
    return _bits(n), _integrated(s, a, z, z)


def subnormal_variance(W, H, step, seed):
    """c, every variance an fp16 subnormal (2^-24 .. 6e-5, log-uniform): 1 / (4 sqrt(var) + 1e-6) lies between 30 and 1000 where a flush
    to zero would give 1e6.  Luminance within 0.01 of 0.25 (some forty fp16 values), so that these denominators leave live weights."""
    rng = np.random.default_rng([seed, 5])
    n = _surfaces(rng, W, H, step)
    var = lambda: np.maximum(2.0 ** -24, 10.0 ** rng.uniform(-7.2, np.log10(6e-5), size=(H, W)))          # noqa: E731
    lum = lambda: 0.25 + 0.01 * rng.random((H, W))          # noqa: E731
    out = _integrated(lum(), lum(), var(), var())
    assert ((out[..., 2:4] & 0x7c00) == 0).all() and (out[..., 2:4] != 0).all()
    return _bits(n), out


def quantised_luminance(W, H, step, seed):
    """d: as a with shadow in {0, 1} and AO in {0, .5, 1}: many taps have |l - l'| == 0 exactly."""
    rng = np.random.default_rng([seed, 6])
    n = _surfaces(rng, W, H, step)
    s, a = _quantised_luminance(rng, W, H)
    return _bits(n), _integrated(s, a, 0.3 * rng.random((H, W)) ** 2, 0.3 * rng.random((H, W)) ** 2)


def _longest_fp16(direction, seed):
    """Among fp16 roundings of unit vectors close to `direction`, the one whose length exceeds 1 by most."""
    cand = np.asarray(direction, np.float64) + 0.02 * np.random.default_rng(seed).normal(size=(4096, 3))
    cand = (cand / np.linalg.norm(cand, axis=-1, keepdims=True)).astype(np.float16)
    return cand[np.argmax((cand.astype(np.float64) ** 2).sum(-1))]


def normal_contract_border(W, H, step, seed):
    """e: one id; fp16-rounded unit vectors around (0.6, 0, 0.8), up to the border of K4's stated preconditions and not
    beyond (every |n| |n'| stays far below 2):
      * two repeated vectors whose fp16 rounding is LONGER than 1 (one near the bulk, one near the diagonal, where all three components
        can round up), so n.n' exceeds 1 -- by 2^-10.5 and 2^-10.4 -- wherever two of them meet;
      * exactly orthogonal pairs ((1,0,0), (0,1,0), (0,0,1): weight exactly 0) and antiparallel pairs ((0,0,1), (0,0,-1));
      * one component (of the bulk direction) or two (of +z) below 2^-13, fp16 subnormals (2^-20, 2^-24) among them."""
    rng = np.random.default_rng([seed, 7])
    base = np.array([0.6, 0.0, 0.8], np.float32)
    bulk = base + 0.06 * rng.normal(size=(H, W, 3)).astype(np.float32)
    bulk /= np.linalg.norm(bulk, axis=-1, keepdims=True)
    nrm = bulk.astype(np.float16)
    kind = rng.random((H, W))
    long_bulk, long_diag = _longest_fp16(base, 77), _longest_fp16(np.ones(3) / np.sqrt(3.0), 78)
    assert (long_bulk.astype(np.float64) ** 2).sum() > 1.0 + 2.0 ** -11 and (long_diag.astype(np.float64) ** 2).sum() > 1.0 + 2.0 ** -10.5
    nrm[kind < 0.08] = long_bulk
    nrm[(kind >= 0.08) & (kind < 0.095)] = long_diag
    tiny = np.array([2.0 ** -14, -2.0 ** -15, 2.0 ** -20, -2.0 ** -24], np.float32)
    one = np.stack([np.full((H, W), 0.6, np.float32), rng.choice(tiny, size=(H, W)), np.full((H, W), 0.8, np.float32)], -1).astype(np.float16)
    sel = (kind >= 0.095) & (kind < 0.175)
    nrm[sel] = one[sel]
    two = np.stack([rng.choice(tiny, size=(H, W)), rng.choice(tiny, size=(H, W)), np.ones((H, W), np.float32)], -1).astype(np.float16)
    sel = (kind >= 0.175) & (kind < 0.19)
    nrm[sel] = two[sel]
    axes = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, -1], [0, 0, 1], [0, 0, 1]], np.float16)
    a = axes[rng.integers(0, len(axes), size=(H, W))]
    sel = (kind >= 0.19) & (kind < 0.215)
    nrm[sel] = a[sel]
    n = np.concatenate([nrm.astype(np.float32), np.full((H, W, 1), 3.0, np.float32)], -1)
    return _bits(n), _integrated(rng.random((H, W)), rng.random((H, W)), 0.3 * rng.random((H, W)) ** 2, 0.3 * rng.random((H, W)) ** 2)


ODD_IDS = (-0.0, 0.0, -0.5, 0.7, 1.0, 1.9, 2049.0, 4097.0, float("nan"))     # (no inf: int(inf) is undefined in the oracle)


def odd_ids(W, H, step, seed):
    """f: the w channel drawn from ODD_IDS per block, a third of the pixels redrawn per pixel: int(w) truncates toward zero, -0 is 0,
    a NaN id is 0 (oracle decision viii), 2049 and 4097 are 2048 and 4096 as halves.  One smooth surface otherwise."""
    rng = np.random.default_rng([seed, 8])
    n = _surfaces(rng, W, H, step)
    n[..., :3] = np.array([0.0, 0.6, 0.8], np.float32) + 0.05 * rng.normal(size=(H, W, 3)).astype(np.float32)
    n[..., :3] /= np.linalg.norm(n[..., :3], axis=-1, keepdims=True)
    odd = np.array(ODD_IDS, np.float32)
    w = _blocks(rng, W, H, max(2, step + 1), lambda s: odd[rng.integers(0, len(odd), size=s)])
    per_pixel = odd[rng.integers(0, len(odd), size=(H, W))]
    w = np.where(rng.random((H, W)) < 0.33, per_pixel, w)
    n[..., 3] = w
    return _bits(n), _integrated(rng.random((H, W)), rng.random((H, W)), 0.3 * rng.random((H, W)) ** 2, 0.3 * rng.random((H, W)) ** 2)


def rejected_taps(W, H, step, seed):
    """g: every tap has another id than its centre -- id = (x / step mod 5) + 5 (y / step mod 5), and a tap is 1 or 2 steps away on
    at least one axis -- so the output must be the input, bit for bit.  Identical normals: only the id rejects."""
    rng = np.random.default_rng([seed, 9])
    ys, xs = np.mgrid[0:H, 0:W]
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = 1.0
    n[..., 3] = (xs // step) % 5 + 5 * ((ys // step) % 5)
    return _bits(n), _integrated(rng.random((H, W)), rng.random((H, W)), 0.3 * rng.random((H, W)) ** 2, 0.3 * rng.random((H, W)) ** 2)


# name -> (generator, non-vacuity class): "live" = the two conditions of families a-e; "some" = the all-zero variance variant (a live tap
# on >= 1 % of the pixels); "ids" = f (no condition); "none" = g (no live tap anywhere)
FAMILIES = {
    "a_live_taps": (live_taps, "live"),
    "b_one_surface": (one_surface, "live"),
    "c_variance_range": (variance_range, "live"),
    "c_zero_variance": (zero_variance, "some"),
    "c_subnormal_variance": (subnormal_variance, "live"),
    "d_quantised_luminance": (quantised_luminance, "live"),
    "e_normal_contract_border": (normal_contract_border, "live"),
    "f_odd_ids": (odd_ids, "ids"),
    "g_rejected_taps": (rejected_taps, "none"),
}

MIN_CHANGED_PIXELS = 0.90      # of all pixels: binary64 output differs from the input in channel 0 or 1
MIN_LIVE_TAPS = 0.40           # of all in-image taps: non-zero binary64 weight


def in_image_taps(W, H, step, display_size=None):
    """Per pixel, the number of the 24 taps that pass the shader's bounds test."""
    dw, dh = (W, H) if display_size is None else display_size
    ys, xs = np.mgrid[0:H, 0:W]
    count = np.zeros((H, W), np.int64)
    for y in range(-2, 3):
        for x in range(-2, 3):
            if x or y:
                sx, sy = xs + x * step, ys + y * step
                count += (sx >= 0) & (sx.astype(np.float32) < np.float32(dw)) & (sy >= 0) & (sy.astype(np.float32) < np.float32(dh))
    return count


def non_vacuity(kind, in_bits, f64_bits, live, W, H, step, display_size=None):
    """The condition on the INPUTS a family must meet, from atrous_f64's output and tap count; returns a message, or None if it is met."""
    per_pixel = in_image_taps(W, H, step, display_size)
    taps = per_pixel.sum()
    # "Of the pixels" = of those that have an in-image tap at all and lie inside display_size: every pixel at the sizes of
    # tests/test_atrous_reference.py (asserted there).  An image smaller than the step has pixels whose output is the input by
    # construction, and a pixel outside display_size has no variance tap (:28-29), so a zero variance, whatever the inputs are.
    dw, dh = (W, H) if display_size is None else display_size
    ys, xs = np.mgrid[0:H, 0:W]
    counted = (per_pixel > 0) & (xs.astype(np.float32) < np.float32(dw)) & (ys.astype(np.float32) < np.float32(dh))
    changed = float((f64_bits[..., 0:2] != in_bits[..., 0:2]).any(-1)[counted].mean()) if counted.any() else 0.0
    share = float(live.sum()) / float(2 * taps) if taps else 0.0
    if kind == "live":
        if taps == 0:
            return None                                    # (a one-pixel image and the like: nothing to be alive)
        if changed < MIN_CHANGED_PIXELS or share < MIN_LIVE_TAPS:
            return f"vacuous inputs: {changed:.3f} of the pixels change (>= {MIN_CHANGED_PIXELS}), {share:.3f} of the in-image taps are live (>= {MIN_LIVE_TAPS})"
    elif kind == "some":
        some = float((live > 0).any(-1).mean())
        if some < 0.01:
            return f"vacuous inputs: a live tap on {some:.4f} of the pixels (>= 0.01)"
    elif kind == "none":
        if live.any():
            return f"{int((live > 0).any(-1).sum())} pixels have a live tap"
    return None


def special_positions_equal(got_bits, ref_bits):
    """NaN positions identical (any payload) and inf positions identical, sign included."""
    g, r = np.asarray(got_bits, np.uint16), np.asarray(ref_bits, np.uint16)
    nan_g, nan_r = (g & 0x7fff) > 0x7c00, (r & 0x7fff) > 0x7c00
    inf_g, inf_r = (g & 0x7fff) == 0x7c00, (r & 0x7fff) == 0x7c00
    return np.array_equal(nan_g, nan_r) and np.array_equal(inf_g, inf_r) and np.array_equal(g[inf_g], r[inf_r])


def fp16_steps(got_bits, ref_bits):
    """(distance in fp16 steps, mask of the channels that are finite in the reference); -0 and +0 are the same value."""
    def key(x):
        x = np.asarray(x, np.uint16).astype(np.int32)
        return np.where(x & 0x8000, -(x & 0x7fff), x & 0x7fff)
    r = np.asarray(ref_bits, np.uint16)
    return np.abs(key(got_bits) - key(ref_bits)), (r & 0x7fff) < 0x7c00
