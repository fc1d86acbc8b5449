"""The case families of tests/composition_cases.py on the CPU:
  * the oracle (orc_composition, orc_raytraced_composition) against the float64 restatement: inside the envelope on every channel of every
    case but `highlight` -- which tests DELTA and EPS themselves, for the oracle rounds in fp32 as the device does -- and, against itself, a
    clean pass of judge_against_oracle; the envelope's width caps on every case of 500 pixels and more;
  * each family's census: what it is built to reach, it reaches (counted from float64);
  * the mutants: the float64 truth with one planted error, encoded, handed to both judges in place of a device image; the family that aims at the
    error must reject it, at every image size from 63 x 3 on, by the oracle rule and (outside `highlight`) by the envelope.
A case for which the oracle alone misses a bar is to be redesigned; DELTA, EPS and the caps stay.  tests/test_gpu_composition_cases.py holds the
device to the same judges on the same cases, and checks what vhr_standin_composition refuses (its validation follows the host-only refusal).

Each case prints one COMPOSITION_CASES_TRUTH row (pytest -s): profiles/composition_cases_truth.txt is a run's rows."""
import numpy as np
import pytest

from tests import composition_cases as cc
from tests import numpy_restatement as nr


def _each(W, H):
    for i, c in enumerate(cc.all_cases(W, H)):
        yield i, c, cc.truth_of(W, H, i)


row = cc.row


@pytest.mark.parametrize("W,H", cc.ALL_SHAPES)
def test_oracle_lies_inside_the_envelope_on_every_case(oracle, W, H):
    fails = []
    for _, c, ref in _each(W, H):
        got, lighting = cc.oracle_image(oracle, c)
        f_self, _ = cc.judge_against_oracle(c, got, got, lighting)
        f_env, width = cc.judge_against_float64(c, got, ref) if c["family"] != "highlight" else ([], -1)
        f_caps = cc.envelope_caps(c, ref)[0] if c["kernel"] == "composition" else []
        codes = ref[0] if c["kernel"] != "composition" else ref["codes"]
        differ = int((codes[..., :3] != got[..., :3]).sum())          # the oracle against the centre of the envelope, for the record
        print(row(c["kernel"], c, "".join(map(str, c.get("modes", "-"))), differ, width, cc.census(c, ref)))
        fails += f_self + f_env + f_caps + cc.judge_case_properties(c, got)
    assert not fails, "\n".join(fails)


def test_random_family_covers_every_mode_triple_and_both_formats():
    seen = {}
    for W, H in cc.SHAPES:
        for c in cc.random_cases(W, H):
            seen.setdefault(c["modes"], set()).add(c["shadow_ao"].shape[-1])
    assert set(seen) == set(cc.MODE_TRIPLES)
    for modes, formats in seen.items():
        assert formats == {2, 4} or not (modes[0] == 0 or modes[1] == 0), modes


def test_each_family_reaches_what_it_is_built_for():
    total = {}
    for W, H in cc.ALL_SHAPES:
        for _, c, ref in _each(W, H):
            n = cc.census(c, ref)
            roomy = W * H >= 189
            if c["family"] == "material_edges" and roomy:
                assert min(n.values()) >= 15, (c["name"], W, H, n)                      # both sides of both clamps, the exact-1 branch, NaN
            if c["name"] == "encode_sweep_ao" and c["full_sweep"]:
                assert n["codes_reached"] == 256 and n["linear_segment"] > 1000 and n["saturated"] > 1000 and n["stores_0_special"] >= 12, n
                ao = c["shadow_ao"][..., 1].reshape(-1)
                assert set(cc.SWEEP_AO.tolist()) <= set(ao.tolist())
            if c["family"] == "sky_and_zero_normal" and roomy:
                assert n["sky_pixels"] >= 63 and n["zero_normal_pixels"] >= 63 and n["surface_pixels"] >= 63, n
                P = cc.positions(c["pfd"], c["depth"])
                assert not np.isfinite(P[c["classes"] == 0]).all(-1).any()               # every sky pixel's P is inf or NaN
                assert (c["albedo"][c["classes"] == 0][:, :3] > 0).all()
            if c["family"] == "highlight":
                P, cam = cc.positions(c["pfd"], c["depth"]), nr._mat(c["pfd"], "camera_view_inverse")[:3, 3]
                V = (cam - P) / np.linalg.norm(cam - P, axis=-1, keepdims=True)
                Hh = (cc.TO_LIGHT + V) / np.linalg.norm(cc.TO_LIGHT + V, axis=-1, keepdims=True)
                assert np.abs(nr.h2f(c["normals"])[..., :3] - Hh).max() <= 2.0 ** -10
            if c["family"] in ("pcf_4096", "pcf_wrap"):
                for k, v in n.items():
                    total[(c["family"], k)] = total.get((c["family"], k), 0) + v
                total[(c["name"], "fully_lit")] = total.get((c["name"], "fully_lit"), 0) + n["fully_lit"]
                total[(c["name"], "fully_dark")] = total.get((c["name"], "fully_dark"), 0) + n["fully_dark"]
            if c["family"] == "raytraced" and c["name"] == "raytraced_bytes" and W * H >= 256:
                assert all(n[f"bytes_ch{k}"] == 256 for k in range(3)) and n["bytes_ch3"] == 4, n
    print("COMPOSITION_CASES_CENSUS " + " ".join(f"{a}.{b}={v}" for (a, b), v in sorted(total.items())))
    assert total[("pcf_4096", "partly_lit")] >= 500 and total[("pcf_4096", "undecided_taps")] >= 100 and total[("pcf_4096", "cleared_texel_taps")] >= 1000
    assert total[("pcf_4096_bias_band", "fully_lit")] >= 100 and total[("pcf_4096_bias_band", "fully_dark")] >= 100
    assert total[("pcf_wrap", "wrapped")] >= 1000 and total[("pcf_wrap", "saturated")] >= 1000 and total[("pcf_wrap", "non_finite")] >= 1000
    assert total[("pcf_wrap", "fully_lit")] >= 100 and total[("pcf_wrap", "fully_dark")] >= 100


def test_material_edges_branches_change_some_code():
    """The exact-1 branch and the two clamps each change the code of some pixel: without one of them the truth's image differs."""
    for W, H in cc.SHAPES[1:]:
        for i, c, ref in _each(W, H):
            if c["family"] != "material_edges":
                continue
            for mutant in ("metallic_branch_at_0.999", "roughness_floor_0", "metallic_unclamped"):
                assert (cc.truth(c, mutant)["codes"] != ref["codes"]).any(), (c["name"], W, H, mutant)


# mutant -> the cases that aim at it (family, a part of the name)
AIMED = {
    "ambient_times_shadow": ("random", "random_0"),
    "reflections_without_shadow": ("random", "random_0"),
    "metallic_branch_at_0.999": ("material_edges", ""),
    "roughness_floor_0": ("material_edges", ""),
    "metallic_unclamped": ("material_edges", ""),
    "red_blue_swapped": ("encode_sweep", "albedo"),
    "no_flip": ("random", ""),
    "pcf_bias_plus": ("pcf_4096", "bias_band"),
    "pcf_scale_2048": ("pcf_4096", "steps"),
    "pcf_clamp": ("pcf_wrap", "5x5_periods"),
    "linear_segment_to_0.04045": ("encode_sweep", "ao"),
    "rg16f_read_with_rgba_stride": ("random", "rg16f"),
}


@pytest.mark.parametrize("mutant", nr.COMPOSITION_MUTANTS)
def test_each_mutant_is_rejected_by_the_family_that_aims_at_it(oracle, mutant):
    assert set(AIMED) == set(nr.COMPOSITION_MUTANTS)
    family, part = AIMED[mutant]
    for W, H in cc.SHAPES[1:]:
        by_oracle = by_envelope = aimed = 0
        for _, c, ref in _each(W, H):
            if c["family"] != family or part not in c["name"]:
                continue
            if mutant == "reflections_without_shadow" and c["modes"][2] == 2:
                continue
            if mutant == "rg16f_read_with_rgba_stride" and not (c["modes"][0] == 0 or c["modes"][1] == 0):
                continue                                                           # a triple that never reads the image
            aimed += 1
            image = cc.truth(c, mutant)["codes"]
            want, lighting = cc.oracle_image(oracle, c)
            f_orc, differ = cc.judge_against_oracle(c, image, want, lighting)
            f_env, _ = cc.judge_against_float64(c, image, ref)
            by_oracle += bool(f_orc)
            by_envelope += bool(f_env)
            print(row(c["kernel"], c, "".join(map(str, c["modes"])), differ, -1, dict(rejected_by_oracle=bool(f_orc), rejected_by_envelope=bool(f_env)),
                      judged=f"mutant:{mutant}"))
        assert aimed and by_oracle == aimed and by_envelope == aimed, f"{mutant} at {W}x{H}: {aimed} cases aim at it, the oracle rule rejects {by_oracle}, the envelope {by_envelope}"


def test_the_judges_pass_the_truth_and_a_one_code_error_fails():
    """The float64 truth's own image passes the envelope; one code added to a channel with a one-code envelope fails it; one code off the oracle
    away from a rounding boundary fails the oracle rule."""
    c = [c for c in cc.all_cases(65, 5) if c["name"].startswith("random_010_rg16f")][0]
    ref = cc.truth(c)
    assert not cc.judge_against_float64(c, ref["codes"], ref)[0]
    narrow = np.argwhere((ref["code_lo"] == ref["code_hi"]) & (ref["code_hi"] < 255))
    assert len(narrow) > 900
    y, x, k = narrow[len(narrow) // 2]
    bad = ref["codes"].copy()
    bad[y, x, k] += 1
    assert cc.judge_against_float64(c, bad, ref)[0]
    bad = ref["codes"].copy()
    bad[0, 0, 3] = 254
    assert cc.judge_against_float64(c, bad, ref)[0]


def test_oracle_rule_allows_one_code_only_next_to_a_boundary(oracle):
    c = [c for c in cc.all_cases(65, 5) if c["name"].startswith("random_010_rg16f")][0]
    want, lighting = cc.oracle_image(oracle, c)
    v = cc.code_before_rounding(lighting)[..., ::-1]
    far = np.argwhere((np.abs(v - np.rint(v)) > 0.1) & (want[..., :3] < 255))
    y, x, k = far[0]
    bad = want.copy()
    bad[y, x, k] += 1
    assert cc.judge_against_oracle(c, bad, want, lighting)[0]
    lo, hi = 0.2, 0.3                                                          # a synthetic texel: lighting whose code value sits 2e-4 under 128
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cc.code_before_rounding(np.float32(mid)) < 128.0 - 2e-4 else (lo, mid)
    one = dict(c, W=1, H=1)
    lit = np.full((1, 1, 3), np.float32(lo))
    assert abs(float(cc.code_before_rounding(lit)[0, 0, 0]) - 128.0) < 1e-3
    img = np.array([[[127, 127, 127, 255]]], np.uint8)
    assert not cc.judge_against_oracle(one, img + np.uint8([1, 1, 1, 0]), img, lit)[0]
    assert cc.judge_against_oracle(one, img + np.uint8([2, 0, 0, 0]), img, lit)[0]


def test_binding_refuses_a_missing_reflections_image(oracle):
    """reflection_mode 0 / 1 without a reflections image: vhr_standin_composition refuses it (include/vhr_amd.h), and so does the oracle's binding;
    under reflection_mode 2 the image is never read."""
    c = dict([c for c in cc.all_cases(65, 5) if c["name"].startswith("random_010_rg16f")][0])
    c["reflections"] = None
    for rmode in (0, 1):
        c["modes"] = (0, 1, rmode)
        with pytest.raises(ValueError):
            cc.oracle_image(oracle, c)
    c["modes"] = (0, 1, 2)
    cc.oracle_image(oracle, c)
