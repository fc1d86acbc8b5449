"""The a-trous kernels (K4), one dispatch at a time, against a binary64 evaluation of the shader on inputs whose taps are alive.

tests/test_gpu_svgf.py::test_atrous_single_dispatch compares with the fp32 oracle on inputs whose ids change every 16 pixels: at step 16 its
expected output is its input, no tile of its images is an interior tile, and 8-row tiles never run.  Here:
  * the truth is numpy_restatement.atrous_f64; the oracle is only the yardstick for how often fp32 may land on the neighbouring fp16 value;
  * the inputs are the families of tests/svgf_cases.py, whose surfaces grow with the step (non-vacuity asserted at the two large sizes);
  * three kernel forms: the literal kernel, the tile kernel with 4-row tiles and with 8-row tiles, steps {1, 2, 4, 8, 16}; steps {3, 32}
    take the literal kernel whatever the option says;
  * 333x301 has interior tiles (no bounds tests in the loads) for every step and both tile heights -- asserted from the tile formulas;
    203x117, 64x40 (one tile column, lane 63 on the image edge), 65x9 (one pixel in the second tile column), 1x5, 5x1, 20x20 at step 16.

Bars per case:
  * NaN positions and inf positions identical to binary64's;
  * every finite channel within ONE fp16 step of binary64.  Derived, not measured: a weight carries a relative error of about 1e-5 (128 *
    log2 of a 1-ulp v_log_f32, a 1-ulp v_exp_f32; kernels_svgf.hip), rcp and sqrt are 1-ulp fp32 instructions, and the output is a mean with
    positive weights of non-negative values, so its relative error stays about 1e-5, while half an fp16 step is 2.4e-4 relative at
    worst: such an error moves a result over one rounding boundary and no further;
  * the share of finite channels not identical to binary64 is at most the ORACLE's share on the same input plus 0.01 (the project's
    allowance for K4, min_exact = 0.99 in tests/test_gpu_svgf.py, now spent against an independent truth);
  * a pixel without a live tap in binary64 (taps outside the image, other ids, family g everywhere) is its input, bit for bit -- for
    family f this is the oracle's accept / reject decision on every odd id."""
import numpy as np
import pytest

from vulkanhybridrenderer_amd import lib
from tests import svgf_cases
from tests.helpers import GpuSvgfHarness, simple_pfd
from tests.numpy_restatement import atrous_f64

pytestmark = pytest.mark.gpu

FORMS = (("literal", 0, 1), ("tile_r4", 1, 1), ("tile_r8", 1, 0))          # name, atrous_variant, atrous_small_tiles
TILE_STEPS = (1, 2, 4, 8, 16)
LARGE = ((333, 301), (203, 117))
FILL = 0x7bff                                                               # 65504: what a pixel no dispatch wrote still holds


def interior_tiles(W, H, step, R):
    """svgf_atrous_tile_kernel's workgroup-uniform test, restated: tiles of 64 columns x R comb rows whose halo lies inside the image."""
    out = []
    for x0 in range(0, W, 64):
        for group in range((H + R * step - 1) // (R * step)):
            for phase in range(step):
                y0 = group * R * step + phase
                if x0 - 2 * step >= 0 and x0 + 64 + 2 * step <= W and y0 - 2 * step >= 0 and y0 + (R + 1) * step < H:
                    out.append((x0, y0))
    return out


def test_the_large_image_has_interior_tiles_for_every_step_and_tile_height():
    for step in TILE_STEPS:
        for R in (4, 8):
            assert interior_tiles(333, 301, step, R), (step, R)
    assert (64, 128) in interior_tiles(333, 301, 16, 8)
    assert not interior_tiles(128, 72, 1, 4) and not interior_tiles(203, 117, 16, 4)      # what the older test's images reach


class _Device:
    """One context per image size; each run() is one ec.dispatch of the a-trous shader from image a into image b."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.job = None
        self.h = GpuSvgfHarness(W, H, self._body)
        self.motion = np.zeros((H, W, 4), np.uint16)
        self.rt = np.zeros((H, W, 2), np.uint16)

    def _body(self, ec):
        step, gx, gy = self.job
        ec.dispatch(lib.ATROUS_SHADER, gx, gy, 1, self.h.push_constants(step))

    def run(self, form, normals, integ, step, groups=None, display_size=None):
        _, variant, small = form
        W, H, h = self.W, self.H, self.h
        h.ctx.set_option("atrous_variant", variant)
        h.ctx.set_option("atrous_small_tiles", small)
        pfd = simple_pfd(W, H)
        if display_size is not None:
            pfd["display_size"] = display_size
            pfd["display_size_inverse"] = [1.0 / display_size[0], 1.0 / display_size[1]]
        gx, gy = groups if groups is not None else ((W + 7) // 8, (H + 7) // 8)
        self.job = (step, gx, gy)
        h.ctx.upload(h.images["a"], integ)
        h.ctx.upload(h.images["b"], np.full((H, W, 4), FILL, np.uint16))
        h.run(pfd, (normals, self.motion, self.rt))
        return h.ctx.download(h.images["b"])

    def close(self):
        self.h.close()


class _Truth:
    """binary64 and the oracle on one input, computed once and shared by the kernel forms."""

    def __init__(self, oracle, name, W, H, step, display_size=None, seed=None):
        gen, self.kind = svgf_cases.FAMILIES[name]
        self.name, self.W, self.H, self.step, self.display_size = name, W, H, step, display_size
        self.normals, self.integ = gen(W, H, step, seed=2000 + step if seed is None else seed)
        self.ref, self.live = atrous_f64(self.normals, self.integ, step, display_size)
        pfd = simple_pfd(W, H)
        if display_size is not None:
            pfd["display_size"] = display_size
            pfd["display_size_inverse"] = [1.0 / display_size[0], 1.0 / display_size[1]]
        self.oracle_out = oracle.svgf_atrous(pfd, self.normals, self.integ, step)

    def vacuity(self):
        return svgf_cases.non_vacuity(self.kind, self.integ, self.ref, self.live, self.W, self.H, self.step, self.display_size)

    def judge(self, got, form_name, region=None):
        """The bars of the module docstring over `region` (rows, columns; default: the image).  Returns the failures as messages."""
        what = f"{self.name} {self.W}x{self.H} step {self.step} {form_name}"
        ry, rx = region if region is not None else (self.H, self.W)
        got, ref, orc = got[:ry, :rx], self.ref[:ry, :rx], self.oracle_out[:ry, :rx]
        integ, live = self.integ[:ry, :rx], self.live[:ry, :rx]
        fails = []
        if not svgf_cases.special_positions_equal(got, ref):
            fails.append(f"{what}: NaN / inf positions differ from binary64's")
        d, finite = svgf_cases.fp16_steps(got, ref)
        d_orc, _ = svgf_cases.fp16_steps(orc, ref)
        if not finite.any():
            return fails
        share, share_orc = float((d[finite] != 0).mean()), float((d_orc[finite] != 0).mean())
        print(f"ATROUS_PARITY {what}: max {int(d[finite].max())} steps, not identical {share:.5f}, oracle {share_orc:.5f}, oracle max {int(d_orc[finite].max())}")
        if d[finite].max() > 1:
            bad = np.argwhere(finite & (d > 1))
            fails.append(f"{what}: {int(d[finite].max())} fp16 steps from binary64 at {len(bad)} channels, first (y, x, channel) {bad[:6].tolist()}")
        if share > share_orc + 0.01:
            fails.append(f"{what}: {share:.5f} of the finite channels differ from binary64, the oracle's share is {share_orc:.5f}")
        untouched = ~(live > 0).any(-1)
        if not np.array_equal(got[untouched], integ[untouched]):
            bad = np.argwhere(untouched & (got != integ).any(-1))
            fails.append(f"{what}: {len(bad)} pixels without a live tap are not their input, first (y, x) {bad[:6].tolist()}")
        if self.kind == "none" and not np.array_equal(got, integ):
            fails.append(f"{what}: every tap is rejected, yet the output is not the input")
        return fails


@pytest.mark.parametrize("name", sorted(svgf_cases.FAMILIES))
@pytest.mark.parametrize("W,H", LARGE)
def test_atrous_forms_against_binary64(oracle, W, H, name):
    dev = _Device(W, H)
    fails = []
    try:
        for step in TILE_STEPS:
            truth = _Truth(oracle, name, W, H, step)
            msg = truth.vacuity()
            assert msg is None, f"{name} {W}x{H} step {step}: {msg}"
            for form in FORMS:
                fails += truth.judge(dev.run(form, truth.normals, truth.integ, step), form[0])
        if (W, H) == LARGE[1]:
            for step in (3, 32):                                            # no tile kernel of these steps: the literal one, under the tile option
                truth = _Truth(oracle, name, W, H, step)
                msg = truth.vacuity()
                assert msg is None, f"{name} {W}x{H} step {step}: {msg}"
                fails += truth.judge(dev.run(FORMS[2], truth.normals, truth.integ, step), "tile option, literal kernel")
    finally:
        dev.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["a_live_taps", "b_one_surface"])
@pytest.mark.parametrize("W,H,steps", [(64, 40, TILE_STEPS), (65, 9, TILE_STEPS), (1, 5, TILE_STEPS), (5, 1, TILE_STEPS), (20, 20, (16,))])
def test_atrous_forms_on_small_images(oracle, W, H, steps, name):
    """Addressing at the image's edges: every tile is a border tile, most taps of the larger steps lie outside the image (the families'
    non-vacuity conditions are conditions for the large sizes; here the live taps are whatever the image has room for)."""
    dev = _Device(W, H)
    fails = []
    try:
        for step in steps:
            truth = _Truth(oracle, name, W, H, step)
            for form in FORMS:
                fails += truth.judge(dev.run(form, truth.normals, truth.integ, step), form[0])
    finally:
        dev.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("step", [2, 16])
def test_partial_dispatch_leaves_the_other_pixels_alone(oracle, step):
    """A dispatch of fewer groups than the image has: pixels at x >= 8 * x_groups or y >= 8 * y_groups keep what the image held."""
    W, H = 203, 117
    gx, gy = W // 8 - 3, H // 8 - 2
    dev = _Device(W, H)
    fails = []
    try:
        truth = _Truth(oracle, "a_live_taps", W, H, step)
        for form in FORMS:
            got = dev.run(form, truth.normals, truth.integ, step, groups=(gx, gy))
            outside = np.ones((H, W), bool)
            outside[:8 * gy, :8 * gx] = False
            if not (got[outside] == FILL).all():
                bad = np.argwhere(outside & (got != FILL).any(-1))
                fails.append(f"step {step} {form[0]}: {len(bad)} pixels outside the dispatch were written, first (y, x) {bad[:6].tolist()}")
            fails += truth.judge(got, form[0] + " partial", region=(8 * gy, 8 * gx))
            assert (got[:8 * gy, :8 * gx] != FILL).any(-1).all()
    finally:
        dev.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("step", [2, 16])
def test_display_size_smaller_than_the_image(oracle, step):
    """display_size (150.5, 90.0) on a 203x117 image: taps at or beyond it are skipped ((float)sx >= display_size, :28-29 and :75-76), all W x H
    pixels are computed."""
    W, H = 203, 117
    dev = _Device(W, H)
    fails = []
    try:
        truth = _Truth(oracle, "a_live_taps", W, H, step, display_size=(150.5, 90.0))
        msg = truth.vacuity()
        assert msg is None, msg
        for form in FORMS:
            fails += truth.judge(dev.run(form, truth.normals, truth.integ, step, display_size=(150.5, 90.0)), form[0] + " display 150.5x90")
    finally:
        dev.close()
    assert not fails, "\n".join(fails)
