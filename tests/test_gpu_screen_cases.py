"""The screen-space kernels K6 / K7 / K8 (ssao_kernel, ssao_blur_kernel, ssr_kernel), one dispatch at a time, on the constructed cases of
tests/screen_cases.py -- every case of a kernel at every image size of its list, one graph (an upload pass, the kernel's pass, a sink) and one
context per size.

tests/test_screen_space.py compares the kernels with the oracle on rendered G-buffers; those never take ssao.comp's samples more than one
period out of the image, never reach the saturating float -> int conversion (oracle decision xiii), never put a display limit or a NaN next to
the blur's tile, and always cover the image with the dispatch.  Here the truth is the float64 restatement (numpy_restatement.ssao, ssr,
ssao_blur_exact); the oracle is the bit-level yardstick.  Bars per case:
  * against the oracle: the blur is bit-identical on every texel (a NaN equals a NaN: its payload is no part of the contract); ssao and ssr
    are bit-identical with the allowance of test_screen_space._bits_close, fewer than 0.1 % of the texels -- which on an image of fewer than
    1000 texels is no texel; NaN and inf positions identical everywhere;
  * against float64, the bars test_oracle_matches_the_numpy_restatement holds the ORACLE to, on the device's image: ssao within 2e-2 and
    within 2e-3 on all but 0.2 % of the texels; ssr's found mask equal on more than 99.8 %, median relative colour error below 1e-3 and
    above 2e-2 on fewer than 0.5 % of the jointly found channels, misses exactly zero; a share bar on an image of fewer than 1 / share
    texels admits no exception;
  * the blur within ONE fp16 step of the exact mean on every finite texel, NaN / inf sets equal to the truth's.  Derived, not measured: the
    inputs are non-negative, so the fp32 running sum of at most 169 terms carries a relative error of at most 168 * 2^-24, about 1e-5, far
    below the 2.4e-4 of half an fp16 step: it can move a result over one rounding boundary and no further;
  * s1: exactly 1.0 over the plane, exactly 0 over the sky; b4: +0.0 everywhere; r2 without a march step or with a thickness that admits
    nothing: the cleared texel everywhere;
  * partial dispatch: the upload pass writes 0x7bff into the output image; texels at or beyond 8 * groups still hold it afterwards, every
    texel before holds the kernel's answer.
ssao.comp is dispatched without push constants, as the reference does, so it runs with the radius the context starts with (0.75): no blur
dispatch precedes it in these graphs (the quirk of test_gpu_settings_and_the_radius_quirk).

Each case prints one SCREEN_CASES_TRUTH row (pytest -s): profiles/screen_cases_truth.txt is a run's rows."""
import numpy as np
import pytest

from tests import numpy_restatement as nr
from tests import screen_cases as sc
from tests.helpers import bits_equal_nan_aware
from tests.test_screen_space import _bits_close
from vulkanhybridrenderer_amd import abi, lib

pytestmark = pytest.mark.gpu

F4, D32, BGRA = abi.FORMAT_R16G16B16A16_SFLOAT, abi.FORMAT_D32_SFLOAT, abi.FORMAT_B8G8R8A8_UNORM
FILL = 0x7bff                                                               # 65504: what a texel no dispatch wrote still holds
OUTPUT = {"ssao": lib.SSAO_RAW, "blur": lib.SSAO, "ssr": lib.SSR}


class _Device:
    """One context and one graph per kernel and image size; run(case) is one ec.dispatch of the kernel with the case's group counts and
    push constants, after the upload pass has written the case's inputs and FILL into the output image."""

    def __init__(self, kernel, W, H):
        self.kernel, self.W, self.H = kernel, W, H
        self.case = None
        self.ctx = ctx = lib.Context(W, H)
        out = OUTPUT[kernel]
        if kernel == "ssao":
            ctx.add_graphics_pass("G-Buffer Pass", [], [lib.transient(lib.NORMALS, F4, 1, lib.ATTACHMENT_IMAGE), lib.transient(lib.DEPTH, D32, 3, lib.ATTACHMENT_IMAGE)], self._upload)
            ctx.add_compute_pass("SSAO Pass", [lib.transient(lib.NORMALS, F4, 0, lib.SAMPLED_IMAGE), lib.transient(lib.DEPTH, D32, 1, lib.SAMPLED_IMAGE)],
                                 [lib.transient(out, F4, 2)], [lib.SSAO_SHADER], 0, lambda ec: ec.dispatch(lib.SSAO_SHADER, *self.case["groups"], 1))
        elif kernel == "blur":
            ctx.add_graphics_pass("Raw Pass", [], [lib.transient(lib.SSAO_RAW, F4, 0, lib.ATTACHMENT_IMAGE)], self._upload)
            ctx.add_compute_pass("SSAO Blur Pass", [lib.transient(lib.SSAO_RAW, F4, 0)], [lib.transient(out, F4, 1)], [lib.SSAO_BLUR_SHADER], 4,
                                 lambda ec: ec.dispatch(lib.SSAO_BLUR_SHADER, *self.case["groups"], 1, np.float32([0.75])))
        else:
            ctx.add_graphics_pass("G-Buffer Pass", [], [lib.transient(lib.ALBEDO, BGRA, 0, lib.ATTACHMENT_IMAGE), lib.transient(lib.NORMALS, F4, 1, lib.ATTACHMENT_IMAGE),
                                                        lib.transient(lib.MOTION, F4, 2, lib.ATTACHMENT_IMAGE), lib.transient(lib.DEPTH, D32, 3, lib.ATTACHMENT_IMAGE)], self._upload)
            ctx.add_compute_pass("SSR Pass", [lib.transient(lib.ALBEDO, BGRA, 0, lib.SAMPLED_IMAGE), lib.transient(lib.NORMALS, F4, 1, lib.SAMPLED_IMAGE),
                                              lib.transient(lib.MOTION, F4, 2, lib.SAMPLED_IMAGE), lib.transient(lib.DEPTH, D32, 3, lib.SAMPLED_IMAGE)],
                                 [lib.transient(out, F4, 4)], [lib.SSR_SHADER], 16,
                                 lambda ec: ec.dispatch(lib.SSR_SHADER, *self.case["groups"], 1,
                                                        np.array([self.case["params"]], dtype=[("a", "f4"), ("b", "f4"), ("c", "f4"), ("d", "i4")])))
        ctx.add_graphics_pass("Sink", [lib.transient(out, F4, 5, lib.SAMPLED_IMAGE)], [lib.render_output(0)])
        ctx.build()

    def _upload(self, c):
        case = self.case
        if self.kernel == "blur":
            c.upload(lib.SSAO_RAW, case["raw"])
        else:
            c.upload(lib.NORMALS, case["normals"])
            c.upload(lib.DEPTH, case["depth"])
            if self.kernel == "ssr":
                c.upload(lib.ALBEDO, case["albedo"])
                c.upload(lib.MOTION, case["motion"])
        c.upload(OUTPUT[self.kernel], np.full((self.H, self.W, 4), FILL, np.uint16))

    def run(self, case):
        if case["kernel"] == "ssr":
            sc.ssr_parameters(*case["params"])              # no long march reaches the device
        self.case = case
        self.ctx.update_per_frame_ubo(0, case["pfd"])
        self.ctx.execute(0, 0)
        self.ctx.synchronize()
        return self.ctx.download(OUTPUT[self.kernel])

    def close(self):
        self.ctx.close()


def _special_positions_differ(got, want):
    nan_g, nan_w = (got & 0x7fff) > 0x7c00, (want & 0x7fff) > 0x7c00
    inf_g, inf_w = (got & 0x7fff) == 0x7c00, (want & 0x7fff) == 0x7c00
    return not (np.array_equal(nan_g, nan_w) and np.array_equal(inf_g, inf_w) and np.array_equal(got[inf_g], want[inf_w]))


def judge_against_oracle(c, got, want):
    """Returns (failures, the number of texels on which device and oracle differ)."""
    what = f"{c['kernel']} {c['name']} {c['W']}x{c['H']}"
    differ = int((~bits_equal_nan_aware(got, want).all(-1)).sum())
    fails = []
    if _special_positions_differ(got, want):
        fails.append(f"{what}: NaN / inf positions differ from the oracle's")
    if c["kernel"] == "blur" or got.shape[0] * got.shape[1] < 1000:
        if differ:
            fails.append(f"{what}: {differ} texels differ from the oracle")
    else:
        try:
            _bits_close(got, want, what)
        except AssertionError as e:
            fails.append(str(e))
    return fails, differ


def _run_cases(oracle, kernel, W, H):
    dev = _Device(kernel, W, H)
    fails = []
    try:
        for c in sc.cases(kernel, W, H):
            got = dev.run(c)
            gx, gy = c["groups"]
            ry, rx = min(H, 8 * gy), min(W, 8 * gx)
            outside = np.ones((H, W), bool)
            outside[:ry, :rx] = False
            what = f"{kernel} {c['name']} {W}x{H}"
            if not (got[outside] == FILL).all():
                bad = np.argwhere(outside & (got != FILL).any(-1))
                fails.append(f"{what}: {len(bad)} texels outside the dispatch were written, first (y, x) {bad[:6].tolist()}")
            if c["name"] == "partial_dispatch":
                assert outside.sum() > 0.1 * W * H
            if (got[:ry, :rx] == FILL).all(-1).any():                              # (no answer is four times 65504: ao <= 1, ssr's alpha is 0 or 1)
                fails.append(f"{what}: {int((got[:ry, :rx] == FILL).all(-1).sum())} texels inside the dispatch were not written")
            want, ref = sc.oracle_image(oracle, c), sc.truth(c)
            f_orc, differ = judge_against_oracle(c, got[:ry, :rx], want[:ry, :rx])
            f_dev, worst_dev = sc.judge_against_float64(c, got, ref, region=(ry, rx))
            _, worst_orc = sc.judge_against_float64(c, want, ref, region=(ry, rx))
            fails += f_orc + f_dev + sc.judge_case_properties(c, got, region=(ry, rx))
            census = nr.ssao_sample_census(c["pfd"], c["depth"], c["radius"]) if kernel == "ssao" else dict(wrapped=0, saturated=0, non_finite=0)
            print(f"SCREEN_CASES_TRUTH {kernel:5s} {c['name']:24s} {W:4d}x{H:<4d} {worst_orc:10.3g} {worst_dev:10.3g} {census['wrapped']:8d} {census['saturated']:6d} "
                  f"{census['non_finite']:6d} {differ:6d}")
    finally:
        dev.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("W,H", sc.SHAPES["ssao"])
def test_ssao_kernel_on_every_case(oracle, W, H):
    _run_cases(oracle, "ssao", W, H)


@pytest.mark.parametrize("W,H", sc.SHAPES["blur"])
def test_blur_kernel_on_every_case(oracle, W, H):
    _run_cases(oracle, "blur", W, H)


@pytest.mark.parametrize("W,H", sc.SHAPES["ssr"])
def test_ssr_kernel_on_every_case(oracle, W, H):
    _run_cases(oracle, "ssr", W, H)
