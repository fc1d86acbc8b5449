"""The oracle's a-trous filter (fp32, expf, seven squarings) against a binary64 evaluation of the same shader, on inputs whose taps are alive.

The oracle and numpy_restatement.atrous are both fp32 and share the operation order, so neither is a truth for the other beyond their
agreement; numpy_restatement.atrous_f64 is.  Every family of tests/svgf_cases.py, steps {1, 2, 3, 4, 8, 16, 32}, two image sizes and one
display size smaller than the image.  Bars: NaN / inf positions identical, every finite channel within ONE fp16 step of binary64, >= 99 % of
the finite channels identical (the fp32 restatement, measured on nine input sets of this kind at 203x117: 1 step at most, >= 0.9985
identical), family g (every tap rejected) exactly the input.  The same cases assert the families' non-vacuity conditions, which are
conditions on the inputs: no GPU is involved here."""
import numpy as np
import pytest

from tests import svgf_cases
from tests.helpers import simple_pfd
from tests.numpy_restatement import atrous_f64

STEPS = (1, 2, 3, 4, 8, 16, 32)
SIZES = ((203, 117), (333, 301))


def _check(oracle, name, W, H, step, display_size=None):
    gen, kind = svgf_cases.FAMILIES[name]
    normals, integ = gen(W, H, step, seed=1000 + step)
    assert (integ & 0x8000).sum() == 0, "luminance and variance must not be negative"
    pfd = simple_pfd(W, H)
    if display_size is not None:
        pfd["display_size"] = display_size
        pfd["display_size_inverse"] = [1.0 / display_size[0], 1.0 / display_size[1]]
    ref, live = atrous_f64(normals, integ, step, display_size)
    # ---- the inputs exercise the filter (a condition on the inputs, from binary64 alone) ----
    if display_size is None:
        assert (svgf_cases.in_image_taps(W, H, step) > 0).all()           # every pixel has a tap: "of the pixels" below means of all pixels
    msg = svgf_cases.non_vacuity(kind, integ, ref, live, W, H, step, display_size)
    assert msg is None, f"{name} {W}x{H} step {step}: {msg}"
    # ---- the oracle against binary64 ----
    got = oracle.svgf_atrous(pfd, normals, integ, step)
    assert svgf_cases.special_positions_equal(got, ref), f"{name} step {step}: NaN / inf positions differ"
    d, finite = svgf_cases.fp16_steps(got, ref)
    assert d[finite].max() <= 1, f"{name} step {step}: {d[finite].max()} fp16 steps from binary64 at {np.argwhere(finite & (d > 1))[:5].tolist()}"
    exact = float((d[finite] == 0).mean())
    assert exact >= 0.99, f"{name} step {step}: only {exact:.4f} of the finite channels identical to binary64"
    untouched = ~(live > 0).any(-1)
    assert np.array_equal(got[untouched], integ[untouched]), f"{name} step {step}: a pixel without a live tap is not its input"
    if kind == "none":
        assert np.array_equal(got, integ) and np.array_equal(ref, integ)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("name", sorted(svgf_cases.FAMILIES))
def test_oracle_atrous_against_binary64(oracle, name, step, W, H):
    _check(oracle, name, W, H, step)


@pytest.mark.parametrize("step", (2, 16))
def test_oracle_atrous_display_size_smaller_than_the_image(oracle, step):
    """(float)sx >= display_size skips the tap (:75-76): 150.5 keeps column 150 and drops 151; all 203 x 117 pixels are computed."""
    _check(oracle, "a_live_taps", 203, 117, step, display_size=(150.5, 90.0))


def test_family_e_reaches_the_border_of_the_normal_contract():
    """n.n' above 1, exactly 0, exactly -1, and components below 2^-13 (fp16 subnormals among them) all occur between a pixel and its taps."""
    normals, _ = svgf_cases.normal_contract_border(203, 117, 1, seed=1001)
    n = normals.view(np.float16).astype(np.float64)[..., :3]
    d = (n[:, 1:] * n[:, :-1]).sum(-1)
    assert d.max() > 1.0 + 2.0 ** -11 and d.max() <= 2.0 and (d == 0.0).any() and (d == -1.0).any()
    mag = np.abs(n)
    assert ((mag > 0) & (mag < 2.0 ** -13)).any() and ((mag > 0) & (mag < 2.0 ** -14)).any()
    assert (np.sqrt((n * n).sum(-1)) <= np.sqrt(2.0)).all()               # |n| |n'| <= 2


def test_binary64_restatement_agrees_with_the_fp32_one():
    """Two independent spellings of the shader (fp32 with seven squarings, binary64 with np.power): 1 fp16 step at most."""
    from tests.numpy_restatement import atrous
    normals, integ = svgf_cases.live_taps(97, 61, 2, seed=5)
    ref, _ = atrous_f64(normals, integ, 2)
    d, finite = svgf_cases.fp16_steps(atrous(normals, integ, 2), ref)
    assert finite.all() and d.max() <= 1 and (d == 0).mean() >= 0.99
