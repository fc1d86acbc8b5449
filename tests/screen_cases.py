"""Input families for the screen-space kernels K6 / K7 / K8 (TEST INFRASTRUCTURE): ssao.comp, ssao_blur.comp and ssr.comp on G-buffers that
are written down, not rendered.  tests/test_screen_space.py runs the kernels on what the oracle rasterised from three scenes: images of 64x40
and more, display_size equal to the image, group counts that cover it, never frame 0, an SSAO radius below 0.27 uv.  Here:

  * a case is a dict: pfd (camera.FrameDriver, as test_screen_space._facing_plane), the input images, the kernel's parameters, the group
    counts and the display size; cases(kernel, W, H) yields every case of a kernel at one image size;
  * the sizes are chosen against the launch geometry -- 64x4 blocks (ssao, ssr), 64x16 tiles with a 6-texel halo (blur): narrower than a
    block or than the 13-tap window, exactly one block / tile, one texel more, several blocks;
  * SSAO: (s1) a plane facing the camera at depth 0.9 -- view z = -znear / 0.9, a radius of 6.75 uv, every sample wraps several periods and
    still lies in the plane: ao is 1.0 exactly, 0 where the four texels under a pixel are sky; (s2) random depth in [0.5, 0.9] under
    perturbed normals: the same wraps over varying texels; (s3) depths in [0.02, 0.05] with a 3x3 patch of 1e30 (sample coordinates beyond
    +-2^31 texels: the saturating conversion of oracle decision xiii), one +inf and one NaN texel (non-finite coordinates), a block of sky;
    (s4) s2 on frame 0 (every pixel draws from seed 0) and on a frame index whose product with the pixel index passes 2^32; (s5) a display
    smaller than the image;
  * blur: (b1) random values; (b2) a display smaller than the image with NaN, or +inf, in every texel at or beyond it; (b3) one NaN and one
    inf texel inside the display; (b4) all -0.0 and all +0.0;
  * SSR: (r1) a floor and a back wall, depth from the plane equations through camera_viewproj, constant normals per plane, varied
    roughness, metallic and albedo; (r2) r1 with no march step, no search step, a thickness that admits nothing, a coarse march; (r3) r1
    under a display smaller than the image;
  * partial dispatch: group counts that stop short of the image, at the largest size of each kernel.

What a family must reach is asserted from the float64 restatement (tests/test_screen_cases.py), at the sizes that have room for it.

No SSR case may ask for more than MAX_MARCH_STEPS march steps or carry a step size that is not a positive normal number: ssr.comp's loop
count is int(ray_distance / step_size), and a zero step would send a 2^31-trip loop to the device (ssr_parameters() refuses)."""
import numpy as np

from tests import numpy_restatement as nr
from vulkanhybridrenderer_amd import camera

ZNEAR = 0.1
SCREEN_SHAPES = ((1, 7), (13, 1), (5, 3), (64, 4), (65, 5), (150, 77))
BLUR_SHAPES = ((1, 1), (1, 20), (20, 1), (13, 13), (64, 16), (65, 17), (70, 23), (203, 117))
SMALL_DISPLAY = {(70, 23): (37.5, 11.0), (203, 117): (150.5, 90.0), (150, 77): (101.5, 60.0), (65, 5): (40.5, 4.0)}
PARTIAL = {(150, 77): (150 // 8 - 1, 77 // 8 - 1), (203, 117): (203 // 8 - 1, 117 // 8 - 1)}
ROOMY = ((64, 4), (65, 5), (150, 77), (70, 23))      # sizes at which s2 / s3 / r1 must meet their non-vacuity conditions
BIG_FRAME_INDEX = 0xfffffff1                          # times any pixel index >= 2 it passes 2^32
MAX_MARCH_STEPS = 250
SSR_DEFAULT = (25.0, 0.1, 0.5, 10)                    # hybrid_render_path.cpp:203-208


def _bits(a):
    return nr.f2h(np.asarray(a, np.float32))


def full_groups(W, H):
    return (W + 7) // 8, (H + 7) // 8


def make_pfd(W, H, frame_index=3, display_size=None):
    drv = camera.FrameDriver(W, H, 0.9, ZNEAR, camera.directional_light((0.0, -0.97, 0.35)))
    drv.frame_index = frame_index
    pfd = drv.next((0.0, 1.0, 0.0))
    if display_size is not None:
        pfd["display_size"] = display_size
        pfd["display_size_inverse"] = [np.float32(1.0) / np.float32(display_size[0]), np.float32(1.0) / np.float32(display_size[1])]
    return pfd


def toward_camera(pfd):
    return np.asarray(pfd["camera_view_inverse"], np.float32).reshape(4, 4).T[:3, 2]


def footprint_all(mask):
    """Per pixel (x, y): do the four texels its own bilinear fetch blends -- (x - 1, x) x (y - 1, y), wrapped -- all lie in `mask`."""
    return mask & np.roll(mask, 1, 0) & np.roll(mask, 1, 1) & np.roll(np.roll(mask, 1, 0), 1, 1)


# ---------------------------------------------------------------------------------------------------------
# SSAO
# ---------------------------------------------------------------------------------------------------------
def _ssao_case(name, W, H, normals, depth, frame_index=3, display_size=None, groups=None, **extra):
    return dict(name=name, kernel="ssao", W=W, H=H, pfd=make_pfd(W, H, frame_index, display_size), normals=normals, depth=depth.astype(np.float32),
                radius=0.75, groups=groups or full_groups(W, H), display_size=display_size, **extra)


def _plane_normals(W, H):
    n = np.zeros((H, W, 4), np.uint16)
    n[..., :3] = _bits(np.broadcast_to(toward_camera(make_pfd(W, H)), (H, W, 3)))
    return n


def sky_band(W, H):
    """A band of sky along the longer axis, two texels wide at least: from 5 texels on both a pixel over sky alone and one over the plane alone exist."""
    sky = np.zeros((H, W), bool)
    if W >= H:
        sky[:, :max(2, W // 4)] = True
    else:
        sky[:max(2, H // 4)] = True
    return sky


def s1_facing_plane(W, H, with_sky):
    depth = np.full((H, W), 0.9, np.float32)
    sky = sky_band(W, H) if with_sky else np.zeros((H, W), bool)
    depth[sky] = 0.0
    return _ssao_case("s1_plane_with_sky" if with_sky else "s1_plane", W, H, _plane_normals(W, H), depth, sky=sky, analytic=True)


def _rough_field(rng, W, H, lo, hi):
    n = toward_camera(make_pfd(W, H)) + 0.3 * rng.normal(size=(H, W, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normals = np.zeros((H, W, 4), np.uint16)
    normals[..., :3] = _bits(n)
    normals[..., 3] = _bits(rng.integers(0, 50, size=(H, W)))
    return normals, rng.uniform(lo, hi, size=(H, W)).astype(np.float32)


def s2_rough_field(W, H, frame_index=3, name="s2_rough_near", **kw):
    normals, depth = _rough_field(np.random.default_rng([W, H, 2]), W, H, 0.5, 0.9)
    return _ssao_case(name, W, H, normals, depth, frame_index, reach=("wrapped",), **kw)


def s3_planted_extremes(W, H):
    """The plants need room: a 3x3 patch, an inf and a NaN texel at least 8 texels (Chebyshev) from the patch and from each other, and a block
    of sky.  An image too small for that gets single texels where it has texels to give."""
    rng = np.random.default_rng([W, H, 3])
    normals, depth = _rough_field(rng, W, H, 0.02, 0.05)
    roomy = W >= 40
    if roomy:
        y0 = max(0, H // 2 - 1)
        depth[y0:y0 + 3, 4:7] = 1e30
        depth[min(H - 1, y0 + 1), 18] = np.inf
        depth[min(H - 1, y0 + 1), 30] = np.nan
        depth[:max(1, H // 3), W - 9:W - 3] = 0.0
    else:
        flat = depth.reshape(-1)
        n = flat.size
        flat[n // 2] = 1e30
        if n >= 5:
            flat[0], flat[n - 1] = np.inf, np.nan
        if n >= 9:
            flat[n // 4] = 0.0
    return _ssao_case("s3_planted_extremes", W, H, normals, depth, reach=("saturated", "non_finite") if roomy else ())


def ssao_cases(W, H):
    yield s1_facing_plane(W, H, False)
    yield s1_facing_plane(W, H, True)
    yield s2_rough_field(W, H)
    yield s3_planted_extremes(W, H)
    yield s2_rough_field(W, H, frame_index=0, name="s4_frame_0")
    yield s2_rough_field(W, H, frame_index=BIG_FRAME_INDEX, name="s4_frame_wraps")
    if (W, H) in SMALL_DISPLAY:
        yield s2_rough_field(W, H, name="s5_small_display", display_size=SMALL_DISPLAY[(W, H)])
    if (W, H) in PARTIAL:
        yield s2_rough_field(W, H, name="partial_dispatch", groups=PARTIAL[(W, H)])


# ---------------------------------------------------------------------------------------------------------
# blur
# ---------------------------------------------------------------------------------------------------------
def _blur_case(name, W, H, raw, display_size=None, groups=None, **extra):
    return dict(name=name, kernel="blur", W=W, H=H, pfd=make_pfd(W, H, 3, display_size), raw=raw, groups=groups or full_groups(W, H),
                display_size=display_size, **extra)


def _random_raw(W, H, salt):
    """All four channels random: the shader reads .x alone."""
    return _bits(np.random.default_rng([W, H, salt]).random((H, W, 4)))


def outside_display(W, H, display_size):
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs.astype(np.float32) >= np.float32(display_size[0])) | (ys.astype(np.float32) >= np.float32(display_size[1]))


def neighbourhood(W, H, x, y):
    """The pixels whose 13x13 window holds texel (x, y)."""
    ys, xs = np.mgrid[0:H, 0:W]
    return (np.abs(xs - x) <= 6) & (np.abs(ys - y) <= 6)


def blur_cases(W, H):
    yield _blur_case("b1_random", W, H, _random_raw(W, H, 11))
    if (W, H) in SMALL_DISPLAY:
        ds = SMALL_DISPLAY[(W, H)]
        for label, value in (("nan", 0x7e00), ("inf", 0x7c00)):
            raw = _random_raw(W, H, 12)
            raw[outside_display(W, H, ds)] = value
            yield _blur_case(f"b2_display_{label}_beyond", W, H, raw, display_size=ds, non_finite=0)
    raw = _random_raw(W, H, 13)
    nan_at, inf_at = (W // 4, H // 4), (W - 1 - W // 5, H - 1 - H // 5)           # (x, y)
    raw[nan_at[1], nan_at[0], 0] = 0x7e00
    nan_set = neighbourhood(W, H, *nan_at)
    inf_set = np.zeros((H, W), bool)
    if inf_at != nan_at:
        raw[inf_at[1], inf_at[0], 0] = 0x7c00
        inf_set = neighbourhood(W, H, *inf_at) & ~nan_set                          # inf + NaN is NaN
    yield _blur_case("b3_specials_inside", W, H, raw, nan_set=nan_set, inf_set=inf_set, non_finite=int(nan_set.sum() + inf_set.sum()))
    yield _blur_case("b4_minus_zero", W, H, np.full((H, W, 4), 0x8000, np.uint16), all_plus_zero=True)
    yield _blur_case("b4_plus_zero", W, H, np.zeros((H, W, 4), np.uint16), all_plus_zero=True)
    if (W, H) in PARTIAL:
        yield _blur_case("partial_dispatch", W, H, _random_raw(W, H, 14), groups=PARTIAL[(W, H)])


# ---------------------------------------------------------------------------------------------------------
# SSR
# ---------------------------------------------------------------------------------------------------------
def ssr_parameters(ray_distance, step_size, thickness, bsearch_steps):
    """The push constants of a case, refused unless the march is short: see the module docstring."""
    step = np.float32(step_size)
    assert np.isfinite(step) and step >= np.finfo(np.float32).tiny, f"step_size {step_size}: not a positive normal number"
    assert np.isfinite(np.float32(ray_distance)) and 0 <= int(np.float32(ray_distance) / step) <= MAX_MARCH_STEPS, (ray_distance, step_size)
    assert 0 <= int(bsearch_steps) <= 16
    return (float(ray_distance), float(step_size), float(thickness), int(bsearch_steps))


WALL_Z, WALL_TOP = -6.0, 2.5


def small_world(W, H):
    """A floor y = 0 (normal +y) and a back wall z = WALL_Z (normal +z) up to y = WALL_TOP, sky above, as the G-buffer of a camera at (0, 1, 0)
    looking down -z would hold them: depth is clip z / w of the point the ray through each texel centre meets."""
    pfd = make_pfd(W, H)
    VPinv = np.asarray(pfd["camera_viewproj_inverse"], np.float64).reshape(4, 4).T
    PV = np.asarray(pfd["camera_proj"], np.float64).reshape(4, 4).T @ np.asarray(pfd["camera_view"], np.float64).reshape(4, 4).T
    cam = np.asarray(pfd["camera_view_inverse"], np.float64).reshape(4, 4).T[:3, 3]
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * 2 - 1, np.ones((H, W)), np.ones((H, W))], -1) @ VPinv.T      # depth 1: the near plane
    d = ndc[..., :3] / ndc[..., 3:4] - cam
    with np.errstate(divide="ignore", invalid="ignore"):
        t_floor = np.where(d[..., 1] < 0, -cam[1] / d[..., 1], np.inf)
        t_wall = np.where(d[..., 2] < 0, (WALL_Z - cam[2]) / d[..., 2], np.inf)
    t_wall = np.where(cam[1] + t_wall * d[..., 1] <= WALL_TOP, t_wall, np.inf)
    t = np.minimum(t_floor, t_wall)
    hit = np.isfinite(t)
    p = cam + np.where(hit, t, 1.0)[..., None] * d
    clip = np.concatenate([p, np.ones((H, W, 1))], -1) @ PV.T
    depth = np.where(hit, clip[..., 2] / clip[..., 3], 0.0).astype(np.float32)
    on_floor = hit & (t_floor <= t_wall)
    n = np.zeros((H, W, 4), np.float32)
    n[on_floor, 1] = 1.0
    n[hit & ~on_floor, 2] = 1.0
    n[..., 3] = np.where(on_floor, 1.0, 2.0) * hit
    rng = np.random.default_rng([W, H, 21])
    motion = np.zeros((H, W, 4), np.float32)
    motion[..., 2] = rng.choice(np.float32([0.0, 0.3, 1.0]), size=(H, W))        # metallic
    motion[..., 3] = rng.uniform(0.0, 1.2, size=(H, W))                           # roughness, clamped to [0.04, 1] by the shader
    albedo = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    return pfd, albedo, _bits(n), _bits(motion), depth


def _ssr_case(name, W, H, params, display_size=None, groups=None, **extra):
    _, albedo, normals, motion, depth = small_world(W, H)
    return dict(name=name, kernel="ssr", W=W, H=H, pfd=make_pfd(W, H, 3, display_size), albedo=albedo, normals=normals, motion=motion, depth=depth,
                params=ssr_parameters(*params), groups=groups or full_groups(W, H), display_size=display_size, **extra)


def ssr_cases(W, H):
    yield _ssr_case("r1_small_world", W, H, SSR_DEFAULT, finds=True)
    yield _ssr_case("r2_no_march_step", W, H, (0.05, 0.1, 0.5, 10), all_zero=True)
    yield _ssr_case("r2_no_search_step", W, H, (25.0, 0.1, 0.5, 0))
    yield _ssr_case("r2_thickness_0.3", W, H, (25.0, 0.1, 0.3, 10), all_zero=True)
    yield _ssr_case("r2_thickness_0.25", W, H, (25.0, 0.1, 0.25, 10), all_zero=True)
    yield _ssr_case("r2_coarse_march", W, H, (8.0, 0.25, 1.5, 4))
    if (W, H) in SMALL_DISPLAY:
        yield _ssr_case("r3_small_display", W, H, SSR_DEFAULT, display_size=SMALL_DISPLAY[(W, H)])
    if (W, H) in PARTIAL:
        yield _ssr_case("partial_dispatch", W, H, SSR_DEFAULT, groups=PARTIAL[(W, H)])


def cases(kernel, W, H):
    return {"ssao": ssao_cases, "blur": blur_cases, "ssr": ssr_cases}[kernel](W, H)


SHAPES = {"ssao": SCREEN_SHAPES + ((70, 23),), "ssr": SCREEN_SHAPES, "blur": BLUR_SHAPES}


# ---------------------------------------------------------------------------------------------------------
# the truth and the oracle on a case, and the bars (tests/test_screen_cases.py on the oracle, tests/test_gpu_screen_cases.py on the device)
# ---------------------------------------------------------------------------------------------------------
def f16(a):
    return np.asarray(a, np.uint16).view(np.float16).astype(np.float32)


def oracle_image(oracle, c):
    if c["kernel"] == "ssao":
        return oracle.ssao(c["pfd"], c["normals"], c["depth"], radius=c["radius"])
    if c["kernel"] == "blur":
        return oracle.ssao_blur(c["pfd"], c["raw"])
    return oracle.ssr(c["pfd"], c["albedo"], c["normals"], c["motion"], c["depth"], *c["params"])


def truth(c):
    """float64: ssao -> (H, W) ao; blur -> (H, W) mean; ssr -> (found, lit)."""
    if c["kernel"] == "ssao":
        return nr.ssao(c["pfd"], c["normals"], c["depth"], c["radius"])
    if c["kernel"] == "blur":
        return nr.ssao_blur_exact(c["raw"], float(c["pfd"]["display_size"][0]), float(c["pfd"]["display_size"][1]))
    found, lit, _ = nr.ssr(c["pfd"], c["albedo"], c["normals"], c["motion"], c["depth"], *c["params"])
    return found, lit


def share_exceeds(mask, share):
    """A share bar `mask.mean() < share`; an image of fewer than 1 / share texels admits no exception."""
    return bool(mask.any()) if mask.size * share < 1.0 else bool(mask.mean() >= share)


def judge_against_float64(c, got_bits, ref, region=None):
    """The bars of test_oracle_matches_the_numpy_restatement on one image (the oracle's or the device's), over `region` (rows, columns).
    Returns (failures, the worst difference from float64)."""
    what = f"{c['kernel']} {c['name']} {c['W']}x{c['H']}"
    ry, rx = region if region is not None else (c["H"], c["W"])
    got = f16(got_bits)[:ry, :rx]
    fails = []
    if c["kernel"] == "ssao":
        ref = ref[:ry, :rx]
        if not np.isfinite(got).all():
            fails.append(f"{what}: {int((~np.isfinite(got)).sum())} non-finite channels")
        if not (got[..., :1] == got).all():
            fails.append(f"{what}: the four channels differ (decision xi)")
        d = np.abs(got[..., 0].astype(np.float64) - ref)
        worst = float(d.max())
        if not worst < 2e-2:
            fails.append(f"{what}: max |ao - float64| = {worst:.3g} (< 2e-2)")
        if share_exceeds(d > 2e-3, 2e-3):
            fails.append(f"{what}: {int((d > 2e-3).sum())} of {d.size} texels are more than 2e-3 from float64 (< 0.2 %)")
        return fails, worst
    if c["kernel"] == "blur":
        ref = ref[:ry, :rx]
        with np.errstate(over="ignore", invalid="ignore"):
            want = ref.astype(np.float16).view(np.uint16)                  # one rounding, float64 -> fp16
        g = np.asarray(got_bits, np.uint16)[:ry, :rx]
        if not (g[..., :1] == g).all():
            fails.append(f"{what}: the four channels differ (decision xi)")
        g = g[..., 0]
        nan_g, nan_r = (g & 0x7fff) > 0x7c00, np.isnan(ref)
        inf_g, inf_r = g == 0x7c00, np.isposinf(ref)
        if not (np.array_equal(nan_g, nan_r) and np.array_equal(inf_g, inf_r)) or (g == 0xfc00).any():
            fails.append(f"{what}: NaN / inf sets differ from float64's ({int(nan_g.sum())} / {int(inf_g.sum())} against {int(nan_r.sum())} / {int(inf_r.sum())})")
        finite = np.isfinite(ref)
        key = lambda x: np.where(x & 0x8000, -(x.astype(np.int32) & 0x7fff), x.astype(np.int32) & 0x7fff)      # noqa: E731
        steps = np.abs(key(g) - key(want))[finite]
        if steps.size and steps.max() > 1:
            fails.append(f"{what}: {int(steps.max())} fp16 steps from the exact mean on {int((steps > 1).sum())} texels")
        worst = float(np.abs(got[..., 0][finite].astype(np.float64) - ref[finite]).max()) if finite.any() else 0.0
        return fails, worst
    found, lit = ref[0][:ry, :rx], ref[1][:ry, :rx]
    got_found = got[..., 3] == 1.0
    if share_exceeds(got_found != found, 2e-3):
        fails.append(f"{what}: found mask differs from float64's on {int((got_found != found).sum())} of {found.size} texels (< 0.2 %)")
    if not (got[~got_found] == 0.0).all():
        fails.append(f"{what}: a miss is not the cleared texel")
    both = got_found & found
    worst = 0.0
    if both.any():
        rel = np.abs(got[..., :3] - lit)[both] / np.maximum(np.abs(lit[both]), 1e-2)
        worst = float(np.nanmax(rel)) if np.isfinite(rel).any() else float("nan")
        with np.errstate(invalid="ignore"):
            if not np.median(rel) < 1e-3:
                fails.append(f"{what}: median relative colour error {np.median(rel):.3g} (< 1e-3)")
            if share_exceeds(~(rel <= 2e-2), 5e-3):
                fails.append(f"{what}: {int((~(rel <= 2e-2)).sum())} of {rel.size} colour channels are more than 2e-2 from float64 (< 0.5 %)")
    return fails, worst


def judge_case_properties(c, got_bits, region=None):
    """What a case knows without any reference: s1's analytic values, b4's +0.0, r2's empty images."""
    what = f"{c['kernel']} {c['name']} {c['W']}x{c['H']}"
    ry, rx = region if region is not None else (c["H"], c["W"])
    g = np.asarray(got_bits, np.uint16)[:ry, :rx]
    fails = []
    if c.get("analytic"):
        sky = c["sky"]
        plane, empty = footprint_all(~sky)[:ry, :rx], footprint_all(sky)[:ry, :rx]
        if not (g[plane] == 0x3c00).all():
            fails.append(f"{what}: {int((g[plane] != 0x3c00).any(-1).sum())} pixels over the plane are not exactly 1.0")
        if not (g[empty] == 0).all():
            fails.append(f"{what}: {int((g[empty] != 0).any(-1).sum())} pixels over sky are not exactly 0")
    if c.get("all_plus_zero") or c.get("all_zero"):
        if g.any():
            fails.append(f"{what}: {int(g.any(-1).sum())} texels are not +0.0")
    return fails
