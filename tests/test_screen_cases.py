"""The case families of tests/screen_cases.py on the CPU: the oracle against the float64 restatement at the bars of
test_screen_space.py::test_oracle_matches_the_numpy_restatement, the blur against the exact mean, and the conditions that keep a family
from being vacuous -- asserted from float64, at the sizes that have room for them (screen_cases.ROOMY):
  * s2 / s3 / s4 / s5: every coordinate class the case is built for (numpy_restatement.ssao_sample_census) holds >= 64 samples, and >= 10 %
    of the texels lie strictly between 0 and 1;
  * r1: between 10 % and 90 % of the pixels find a reflection;
  * b2 / b3: the number of non-finite outputs is what the geometry predicts (none; the two 13x13 neighbourhoods clipped to the image).
A case for which the oracle alone misses a bar is to be redesigned; the bars stay.  tests/test_gpu_screen_cases.py holds the device to the
same bars on the same cases."""
import numpy as np
import pytest

from tests import numpy_restatement as nr
from tests import screen_cases as sc

KERNEL_SHAPES = [(k, W, H) for k in ("ssao", "blur", "ssr") for W, H in sc.SHAPES[k]]


def non_vacuity(c, ref):
    """A message if the case does not reach what it is built for, else None."""
    roomy = (c["W"], c["H"]) in sc.ROOMY
    if c["kernel"] == "ssao" and c.get("reach") and roomy:
        census = nr.ssao_sample_census(c["pfd"], c["depth"], c["radius"])
        for cls in c["reach"]:
            if census[cls] < 64:
                return f"{census[cls]} {cls} sample coordinates (>= 64): {census}"
        inside = float(((ref > 0.0) & (ref < 1.0)).mean())
        if inside < 0.10:
            return f"{inside:.3f} of the texels lie strictly between 0 and 1 (>= 0.10)"
    if c["kernel"] == "ssr" and c.get("finds") and roomy:
        share = float(ref[0].mean())
        if not 0.1 < share < 0.9:
            return f"found share {share:.3f} (0.1 .. 0.9)"
    if c["kernel"] == "blur" and "non_finite" in c:
        n = int((~np.isfinite(ref)).sum())
        if n != c["non_finite"]:
            return f"{n} non-finite outputs, the geometry predicts {c['non_finite']}"
        if "nan_set" in c and not (np.array_equal(np.isnan(ref), c["nan_set"]) and np.array_equal(np.isposinf(ref), c["inf_set"])):
            return "the NaN / inf sets are not the two neighbourhoods"
    return None


@pytest.mark.parametrize("kernel,W,H", KERNEL_SHAPES)
def test_oracle_meets_the_bars_on_every_case(oracle, kernel, W, H):
    fails = []
    for c in sc.cases(kernel, W, H):
        ref = sc.truth(c)
        msg = non_vacuity(c, ref)
        assert msg is None, f"{kernel} {c['name']} {W}x{H}: vacuous: {msg}"
        got = sc.oracle_image(oracle, c)
        f, worst = sc.judge_against_float64(c, got, ref)
        print(f"SCREEN_CASES {kernel} {c['name']} {W}x{H}: oracle worst difference from float64 {worst:.3g}")
        fails += f + sc.judge_case_properties(c, got)
        if kernel == "blur":                                  # the fp32 restatement in the shader's summation order: the same bits
            mine = nr.ssao_blur_f32(c["raw"], float(c["pfd"]["display_size"][0]), float(c["pfd"]["display_size"][1]))
            same = (nr.f2h(mine) == got[..., 0]) | (np.isnan(mine) & ((got[..., 0] & 0x7fff) > 0x7c00))
            if not same.all():
                fails.append(f"blur {c['name']} {W}x{H}: {int((~same).sum())} texels differ from ssao_blur_f32")
    assert not fails, "\n".join(fails)


def test_every_family_is_reached_somewhere():
    """The conditions above are skipped where an image has no room; each must have been asserted at one size at least."""
    seen = set()
    for kernel in ("ssao", "blur", "ssr"):
        for W, H in sc.SHAPES[kernel]:
            for c in sc.cases(kernel, W, H):
                if (c.get("reach") or c.get("finds")) and (W, H) in sc.ROOMY:
                    seen.add(c["name"])
                if "non_finite" in c:
                    seen.add(c["name"])
                if c.get("analytic"):
                    sky = c["sky"]
                    assert sc.footprint_all(~sky).any() and (not sky.any() or sc.footprint_all(sky).any()), (c["name"], W, H)
    assert {"s2_rough_near", "s3_planted_extremes", "s4_frame_0", "s4_frame_wraps", "s5_small_display", "r1_small_world",
            "b2_display_nan_beyond", "b2_display_inf_beyond", "b3_specials_inside"} <= seen


def test_s3_plants_keep_their_distances():
    for W, H in sc.ROOMY:
        d = sc.s3_planted_extremes(W, H)["depth"]
        patch, inf, nan = np.argwhere(d == np.float32(1e30)), np.argwhere(np.isinf(d)), np.argwhere(np.isnan(d))
        assert len(patch) == 3 * min(3, H) and len(inf) == 1 and len(nan) == 1 and (d == 0).sum() >= 6
        cheb = lambda a, b: np.abs(a[:, None] - b[None]).max(-1).min()      # noqa: E731
        assert cheb(patch, inf) >= 8 and cheb(patch, nan) >= 8 and cheb(inf, nan) >= 8


def test_the_frame_index_cases_wrap_and_collapse():
    """s4: on frame 0 every pixel's seed is 0; under BIG_FRAME_INDEX the product passes 2^32 on all but two pixels."""
    for W, H in sc.SCREEN_SHAPES:
        ys, xs = np.mgrid[0:H, 0:W]
        pixel = ys * H + xs
        assert ((pixel * sc.BIG_FRAME_INDEX >= 2 ** 32) == (pixel >= 2)).all() and (pixel >= 2).any()
        c = sc.s2_rough_field(W, H, frame_index=sc.BIG_FRAME_INDEX)
        assert int(c["pfd"]["frame_index"]) == sc.BIG_FRAME_INDEX
        assert int(sc.s2_rough_field(W, H, frame_index=0)["pfd"]["frame_index"]) == 0


def test_ssr_parameters_refuse_a_long_march():
    """No case may reach the device with a march of more than 250 steps: a zero step_size is a 2^31-trip loop in ssr.comp."""
    for bad in ((25.0, 0.0, 0.5, 10), (25.0, 1e-40, 0.5, 10), (25.0, -0.1, 0.5, 10), (25.0, float("nan"), 0.5, 10), (25.0, float("inf"), 0.5, 10),
                (25.2, 0.1, 0.5, 10), (float("inf"), 0.1, 0.5, 10)):
        with pytest.raises(AssertionError):
            sc.ssr_parameters(*bad)
    for kernel_shape in sc.SHAPES["ssr"]:
        for c in sc.ssr_cases(*kernel_shape):
            assert int(np.float32(c["params"][0]) / np.float32(c["params"][1])) <= sc.MAX_MARCH_STEPS


def test_blur_exact_known_values():
    """169 ones / 169 is 1; a 7x7 corner of ones is 49 / 169; a display limit removes taps, a NaN beyond it is never read."""
    raw = np.zeros((20, 30, 4), np.uint16)
    raw[..., 0] = 0x3c00
    e = nr.ssao_blur_exact(raw, 30.0, 20.0)
    assert e[10, 15] == 1.0 and e[0, 0] == 49.0 / 169.0
    raw[:, 12:, 0] = 0x7e00
    e = nr.ssao_blur_exact(raw, 11.5, 20.0)
    assert np.isfinite(e).all() and e[10, 29] == 0.0 and e[10, 12] == 6 * 13 / 169.0      # columns 6 .. 11 of 13 rows
