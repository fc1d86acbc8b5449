"""composition_kernel and raytraced_composition_kernel, one launch at a time, on the constructed cases of tests/composition_cases.py -- every
case at every image size of its list, one context and one graph per size: an upload pass that writes the case's images and fills the output
storage image with the sentinel byte 0x5a (alpha included), and the "Composition Pass", whose callback calls standin_composition (or
standin_raytraced_composition) and whose RENDER_OUTPUT ends the graph.

tests/test_gpu_composition.py and tests/test_shadow_map.py compare the kernel with the oracle on rendered frames of 128 x 72 and 512 x 512,
by a share of the image.  Here, per case and per channel, no shares:
  * every texel was written: no sentinel is left, alpha is 255 (the raytraced path's: the input's alpha);
  * judge_against_oracle: equal to the oracle, or one code apart where the oracle's own value before truncation lies within 1e-3 of an integer
    (the device encodes with powf in fp32, the oracle with pow in binary64; kernels_standin.hip is built without contraction, so the lighting
    itself is meant to be the oracle's fp32 bit for bit);
  * judge_against_float64 (not for `highlight`): inside the envelope of the float64 restatement, DELTA and EPS derived in DESIGN.md section 4;
  * the case's exact properties: saturated pixels exactly 255, dark pixels exactly 0.
The 4096 x 4096 map of pcf_4096 is uploaded once per module, into device memory every context binds as its "Shadow Map".
test_standin_composition_refuses_bad_arguments is here, not in the CPU file: the entry point's validation follows its host-only refusal.

Each case prints one COMPOSITION_CASES_TRUTH row (pytest -s): profiles/composition_cases_truth.txt is a run's rows."""
import ctypes as C

import numpy as np
import pytest

from tests import composition_cases as cc
from vulkanhybridrenderer_amd import abi, lib

pytestmark = pytest.mark.gpu

F4, RG, D32, BGRA = abi.FORMAT_R16G16B16A16_SFLOAT, abi.FORMAT_R16G16_SFLOAT, abi.FORMAT_D32_SFLOAT, abi.FORMAT_B8G8R8A8_UNORM
SENTINEL = 0x5a
INVALID_ARGUMENT = -1                                     # VHR_ERROR_INVALID_ARGUMENT, include/vhr_amd.h
SA_RG, SA_RGBA = "Composition Cases Shadow and AO RG16F", "Composition Cases Shadow and AO RGBA16F"
SMALL_MAPS = {8: "Composition Cases Shadow Map 8", 5: "Composition Cases Shadow Map 5", 1: "Composition Cases Shadow Map 1"}
ODD_MAP = "Composition Cases Shadow Map 8 x 4"


@pytest.fixture(scope="module")
def big_map():
    """cc.map_4096() in device memory, uploaded once."""
    import torch
    t = torch.from_numpy(np.array(cc.map_4096())).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    yield t
    del t


class _Device:
    """One context and one graph per image size.  run(case) executes the graph once: the upload pass, then `body` -- by default the case's one
    standin_composition / standin_raytraced_composition call -- and returns the output storage image."""

    def __init__(self, W, H, big_map):
        self.W, self.H, self.case, self.body = W, H, None, None
        self.ctx = ctx = lib.Context(W, H)
        self.out = ctx.upload_new_storage_image(W, H, abi.FORMAT_B8G8R8A8_SRGB)
        images = [(lib.ALBEDO, BGRA, 0, 0), (lib.NORMALS, F4, 0, 0), (lib.MOTION, F4, 0, 0), (lib.DEPTH, D32, 0, 0), (SA_RG, RG, 0, 0), (SA_RGBA, F4, 0, 0),
                  (lib.REFLECTIONS, F4, 0, 0), (lib.SSAO, F4, 0, 0), (lib.RAYTRACED_OUTPUT, BGRA, 0, 0), (lib.SHADOW_MAP, D32, 4096, 4096), (ODD_MAP, D32, 8, 4)]
        images += [(name, D32, size, size) for size, name in SMALL_MAPS.items()]
        ctx.add_graphics_pass("Upload Pass", [], [lib.transient(n, f, i, lib.ATTACHMENT_IMAGE, w, h) for i, (n, f, w, h) in enumerate(images)], self._upload)
        ctx.add_graphics_pass("Composition Pass", [lib.transient(n, f, i, lib.SAMPLED_IMAGE, w, h) for i, (n, f, w, h) in enumerate(images)],
                              [lib.render_output(0)], lambda c: (self.body or self._compose)(c))
        ctx.build()
        ctx.bind_external_image(lib.SHADOW_MAP, big_map.data_ptr())

    def _upload(self, c):
        case = self.case
        if case["kernel"] == "raytraced_composition":
            c.upload(lib.RAYTRACED_OUTPUT, case["image"])
        else:
            c.upload(lib.ALBEDO, case["albedo"])
            c.upload(lib.NORMALS, case["normals"])
            c.upload(lib.MOTION, case["motion"])
            c.upload(lib.DEPTH, case["depth"])
            c.upload(SA_RGBA if case["shadow_ao"].shape[-1] == 4 else SA_RG, case["shadow_ao"])
            if case["reflections"] is not None:
                c.upload(lib.REFLECTIONS, case["reflections"])
            if case["ssao"] is not None:
                c.upload(lib.SSAO, case["ssao"])
            if case["shadow_map"] is not None and case["shadow_map"].shape[0] in SMALL_MAPS:
                c.upload(SMALL_MAPS[case["shadow_map"].shape[0]], case["shadow_map"])
        c.upload(self.out, np.full((self.H, self.W, 4), SENTINEL, np.uint8))

    def images_of(self, case):
        sm = case["shadow_map"]
        return dict(shadow_ao=SA_RGBA if case["shadow_ao"].shape[-1] == 4 else SA_RG, reflections=lib.REFLECTIONS if case["reflections"] is not None else None,
                    ssao=lib.SSAO if case["ssao"] is not None else None,
                    shadow_map=None if sm is None else SMALL_MAPS.get(sm.shape[0], lib.SHADOW_MAP))

    def _compose(self, c):
        case = self.case
        if case["kernel"] == "raytraced_composition":
            c.standin_raytraced_composition(self.out)
        else:
            c.standin_composition(self.out, *case["modes"], **self.images_of(case))

    def run(self, case, body=None):
        self.case, self.body = case, body
        self.ctx.update_per_frame_ubo(0, case["pfd"] if "pfd" in case else cc.make_pfd(self.W, self.H))
        try:
            self.ctx.execute(0, 0)
            self.ctx.synchronize()
        finally:
            self.body = None
        return self.ctx.download(self.out)

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("W,H", cc.ALL_SHAPES)
def test_composition_kernels_on_every_case(oracle, big_map, W, H):
    dev = _Device(W, H, big_map)
    fails = []
    try:
        for i, c in enumerate(cc.all_cases(W, H)):
            got = dev.run(c)
            what = f"{c['kernel']} {c['name']} {W}x{H}"
            ref = cc.truth_of(W, H, i)
            want, lighting = cc.oracle_image(oracle, c)
            unwritten = (got == SENTINEL).all(-1)                      # (no answer is 0x5a four times: alpha is 255, or one of 0, 1, 254, 255)
            if unwritten.any():
                fails.append(f"{what}: {int(unwritten.sum())} texels were not written, first (y, x) {np.argwhere(unwritten)[:6].tolist()}")
            f_orc, differ = cc.judge_against_oracle(c, got, want, lighting)
            f_env, width = cc.judge_against_float64(c, got, ref) if c["family"] != "highlight" else ([], -1)
            fails += f_orc + f_env + cc.judge_case_properties(c, got)
            print(cc.row(c["kernel"], c, "".join(map(str, c.get("modes", "-"))), differ, width, cc.census(c, ref), judged="device"))
    finally:
        dev.close()
    assert not fails, "\n".join(fails)


def test_standin_composition_refuses_bad_arguments(oracle, big_map):
    """What include/vhr_amd.h says vhr_standin_composition refuses -- extents that differ, wrong formats, a mode of 3 or -1, shadow_mode 1 without a
    square D32 map, ambient_occlusion_mode 1 without ssao, reflection_mode 0 / 1 without a reflections image -- is refused with
    VHR_ERROR_INVALID_ARGUMENT and nothing is launched: the output keeps the sentinel.  Under reflection_mode 2 a NULL reflections image is fine."""
    W, H = 65, 5
    c = [c for c in cc.all_cases(W, H) if c["name"] == "random_010_rg16f"][0]
    dev = _Device(W, H, big_map)

    def desc(shadow=0, ao=0, refl=2, albedo=lib.ALBEDO, normals=lib.NORMALS, shadow_ao=SA_RG, reflections=None, ssao=None, shadow_map=None):
        enc = lambda s: s.encode() if s else None      # noqa: E731
        return lib.CompositionDesc(shadow, ao, refl, enc(albedo), enc(normals), lib.MOTION.encode(), lib.DEPTH.encode(), enc(shadow_ao), enc(reflections),
                                   dev.out, enc(ssao), enc(shadow_map))

    bad = {
        "extents differ": desc(shadow_ao=SMALL_MAPS[8]),
        "albedo is no 4-byte image": desc(albedo=SA_RGBA),
        "normals are D32": desc(normals=lib.DEPTH),
        "shadow_ao is D32": desc(shadow_ao=lib.DEPTH),
        "shadow_mode 3": desc(shadow=3),
        "shadow_mode -1": desc(shadow=-1),
        "ambient_occlusion_mode 3": desc(ao=3),
        "reflection_mode 3": desc(refl=3),
        "reflection_mode -1": desc(refl=-1),
        "shadow_mode 1 without a map": desc(shadow=1),
        "shadow_mode 1 with a map that is not square": desc(shadow=1, shadow_map=ODD_MAP),
        "shadow_mode 1 with a map that is not D32": desc(shadow=1, shadow_map=lib.SSAO),
        "ambient_occlusion_mode 1 without ssao": desc(ao=1),
        "reflection_mode 0 without reflections": desc(refl=0),
        "reflection_mode 1 without reflections": desc(refl=1),
    }
    try:
        dev.run(c)                                                              # the case's images are in place, the output is written
        dev.ctx.upload(dev.out, np.full((H, W, 4), SENTINEL, np.uint8))
        results = {label: dev.ctx.L.vhr_standin_composition(dev.ctx.handle, 0, C.byref(d)) for label, d in bad.items()}
        dev.ctx.synchronize()
        assert results == {label: INVALID_ARGUMENT for label in bad}, results
        assert (dev.ctx.download(dev.out) == SENTINEL).all(), "a refused call wrote the output"
        fine = dict(c, modes=(0, 1, 2), reflections=None)                       # reflection_mode 2: NULL is what the header allows
        got = dev.run(fine)
        want, lighting = cc.oracle_image(oracle, fine)
        assert not cc.judge_against_oracle(fine, got, want, lighting)[0]
    finally:
        dev.close()
