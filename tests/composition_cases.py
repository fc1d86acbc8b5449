"""Input families for the composition kernels (TEST INFRASTRUCTURE): composition_kernel (composition.frag:60-161) and
raytraced_composition_kernel (raytraced_render_path/composition.frag) on G-buffers that are written down, not rendered, after the pattern of
tests/screen_cases.py.  The rendered frames of tests/test_gpu_composition.py and tests/test_shadow_map.py are multiples of the 64 x 4 block,
are judged by a share of a whole image, and never reach a clamp, the exact-1 branch, a saturated or NaN store, a wrapped PCF tap or a
non-finite position.  Here:

  * a case is a dict: pfd, albedo (B8G8R8A8), normals / motion (RGBA16F bits), depth (D32), shadow_ao (RG16F (H, W, 2) or RGBA16F (H, W, 4)
    bits), reflections / ssao (RGBA16F bits or None), shadow_map (square D32 or None), modes (shadow, ambient occlusion, reflection);
    cases(W, H) yields every case of one image size;
  * SHAPES against the 64 x 4 block: one thread, a partial block in x, exactly one block, one texel more both ways, several blocks with
    partial ones on both edges.  encode_sweep's full sweep needs 17 413 pixels and has a size of its own (SWEEP_SHAPE);
  * the generator's limits, which DELTA and EPS are derived from ("composition cases"): camera at (0, 1, 0) looking down
    -z, yfov 0.9 at aspect 16 / 9 whatever the image's shape, view depth of every surface in [2, 4.5] m -- so the distance lies in [2, 6.4] m
    and |P| below 7.4 m -- and a light with L . V >= -0.5 on every pixel (|L + V| >= 1);
  * radiance inputs (shadow, ao, reflections, ssao) are non-negative except in encode_sweep's four special pixels.

The judges: judge_against_oracle (per channel: equal, or one code apart where the oracle's own value before truncation lies within 1e-3 of
an integer) and judge_against_float64 (per channel: inside the envelope of numpy_restatement.composition).  tests/test_composition_cases.py
holds the oracle and the mutants to them on the CPU, tests/test_gpu_composition_cases.py the device."""
import functools

import numpy as np

from tests import numpy_restatement as nr
from vulkanhybridrenderer_amd import abi, camera

ZNEAR = 0.1
SHAPES = ((1, 1), (63, 3), (64, 4), (65, 5), (130, 9))
SWEEP_SHAPE = (130, 134)                                  # 17 420 pixels: every finite fp16 value in [0, 4] and four specials
ALL_SHAPES = SHAPES + (SWEEP_SHAPE,)
DELTA = 2.0 ** -17                                        # what an fp32 evaluation may move H.V, N.L, N.H, N.V by: DESIGN.md section 4
EPS = 64 * 2.0 ** -24                                     # relative, on the lighting: the same place
CODE_SLACK = 1e-3                                         # powf against binary64 pow, in code units (tests/test_forward_raster_path.py)
TO_LIGHT = np.array([0.3, 0.8, 0.52]) / np.linalg.norm([0.3, 0.8, 0.52])
CAPPED_FROM = 500                                         # pixels from which a case must meet the envelope's width caps
UNCAPPED = ("highlight", "sky_and_zero_normal")
MODE_TRIPLES = [(s, a, r) for s in range(3) for a in range(3) for r in range(3)]
METALLIC_EDGES = (-1.0, 0.0, 0.999, 1.0, 1.001, 2.0, np.nan)
ROUGHNESS_EDGES = (-1.0, 0.0, 0.039, 0.04, 1.0, 3.0, np.nan)
REFLECTION_COLOUR = (0.8, 0.3, 0.1)


def _bits(a):
    return nr.f2h(np.asarray(a, np.float32))


def make_pfd(W, H, projview=None, intensity=3.0):
    light = camera.directional_light(-TO_LIGHT, intensity=intensity)
    if projview is not None:
        light["projview"] = abi.mat_to_glm(projview)
    drv = camera.FrameDriver(W, H, 0.9, ZNEAR, light, aspect=16.0 / 9.0)
    drv.frame_index = 3
    return drv.next((0.0, 1.0, 0.0))


def positions(pfd, depth):
    """float64 world positions of the texel centres, G-buffer orientation."""
    H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W]
    return nr._unproject(nr._mat(pfd, "camera_viewproj_inverse"), depth.astype(np.float64), (xs + 0.5) / W, (ys + 0.5) / H)


def check_limits(c):
    """The limits DELTA and EPS rest on, on every surface pixel of a case (sky pixels excepted)."""
    P = positions(c["pfd"], c["depth"])
    cam = nr._mat(c["pfd"], "camera_view_inverse")[:3, 3]
    surface = c["depth"] > 0
    if not surface.any():
        return
    d = np.linalg.norm(cam - P[surface], axis=-1)
    V = (cam - P[surface]) / d[:, None]
    assert np.linalg.norm(cam) <= 8 and np.linalg.norm(P[surface], axis=-1).max() <= 8 and d.min() >= 2, c["name"]
    assert (V @ TO_LIGHT).min() >= -0.5, c["name"]


def _depth(rng, W, H, lo=2.0, hi=4.5):
    return (ZNEAR / rng.uniform(lo, hi, size=(H, W))).astype(np.float32)                   # infinite reverse-Z projection: depth = znear / view depth


def _unit_normals(rng, W, H):
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    out = np.zeros((H, W, 4), np.uint16)
    out[..., :3] = _bits(n)
    out[..., 3] = _bits(rng.integers(0, 50, size=(H, W)))
    return out


def _facing_normals(rng, W, H):
    """Unit normals within about 25 degrees of +z, the direction of the camera: N.V and N.L stay above 0.3, where the lighting's slope in them is mild."""
    n = np.array([0.0, 0.0, 1.0]) + 0.25 * rng.normal(size=(H, W, 3)).clip(-1.5, 1.5)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    out = np.zeros((H, W, 4), np.uint16)
    out[..., :3] = _bits(n)
    out[..., 3] = _bits(rng.integers(0, 50, size=(H, W)))
    return out


def _motion(rng, W, H, metallic, roughness):
    m = np.zeros((H, W, 4), np.float32)
    m[..., :2] = rng.uniform(-0.01, 0.01, size=(H, W, 2))
    m[..., 2], m[..., 3] = metallic, roughness
    return _bits(m)


def _rgba16f(rgb, rng=None):
    """An RGBA16F image from (H, W, 3) or (H, W) values; the channels the shader does not read hold noise."""
    rgb = np.asarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    out = np.zeros((H, W, 4), np.float32) if rng is None else rng.uniform(0, 1, size=(H, W, 4)).astype(np.float32)
    if rgb.ndim == 2:
        out[..., 0] = rgb
    else:
        out[..., :3] = rgb
    return _bits(out)


def _shadow_ao(shadow, ao, rgba, rng=None):
    """RG16F (H, W, 2) or RGBA16F (H, W, 4) bits; under RGBA16F channels 2 and 3 hold what would betray a wrong stride (large values)."""
    H, W = np.shape(shadow)
    out = np.zeros((H, W, 4 if rgba else 2), np.float32)
    out[..., 0], out[..., 1] = shadow, ao
    if rgba:
        out[..., 2:] = 7.0 if rng is None else rng.uniform(5.0, 9.0, size=(H, W, 2))
    return _bits(out)


def two_level_map():
    """An 8 x 8 shadow map of two constant halves: a PCF tap blends only within half a texel of the two seams."""
    m = np.full((8, 8), 0.05, np.float32)
    m[:, 4:] = 0.6
    return m


def _case(name, family, W, H, modes, pfd, albedo, normals, motion, depth, shadow_ao, reflections=None, ssao=None, shadow_map=None, **extra):
    c = dict(name=name, family=family, kernel="composition", W=W, H=H, modes=tuple(modes), pfd=pfd, albedo=albedo, normals=normals, motion=motion,
             depth=depth, shadow_ao=shadow_ao, reflections=reflections, ssao=ssao, shadow_map=shadow_map, **extra)
    check_limits(c)
    return c


# ---------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------
def random_cases(W, H):
    """All 27 mode triples over the five shapes: shape k takes the triples k, k + 5, ...; a triple that reads shadow_ao runs under both formats."""
    k = SHAPES.index((W, H))
    for t, modes in enumerate(MODE_TRIPLES):
        if t % len(SHAPES) != k:
            continue
        reads = modes[0] == 0 or modes[1] == 0
        for rgba in ((False, True) if reads else (t % 2 == 1,)):
            rng = np.random.default_rng([W, H, 31, t])
            metallic = rng.choice(np.float32([0, 0.25, 0.5, 0.9, 1]), size=(H, W))
            roughness = rng.choice(np.float32([0, 0.04, 0.1, 0.3, 0.5, 1]), size=(H, W))
            # shadow_mode 1: the visible volume over two and a half periods of the two-level map, at a light depth between its levels
            projview = light_onto_plane((0.5, 0.5), (20.0, 12.0), 0.3, size=8) if modes[0] == 1 else None
            yield _case(f"random_{modes[0]}{modes[1]}{modes[2]}_{'rgba16f' if rgba else 'rg16f'}", "random", W, H, modes, make_pfd(W, H, projview),
                        rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8), _unit_normals(rng, W, H), _motion(rng, W, H, metallic, roughness),
                        _depth(rng, W, H), _shadow_ao(rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W)), rgba, rng),
                        reflections=_rgba16f(rng.uniform(0, 1, (H, W, 3)), rng) if modes[2] != 2 else None,
                        ssao=_rgba16f(rng.uniform(0, 1, (H, W)), rng) if modes[1] == 1 else None,
                        shadow_map=two_level_map() if modes[0] == 1 else None)


SWEEP_AO = np.concatenate([np.arange(0, 0x4400 + 1, dtype=np.uint16), np.uint16([0xbc00, 0x8000, 0x7c00, 0x7e00])])   # [0, 4], -1, -0.0, +inf, NaN


def encode_sweep_cases(W, H):
    """Modes (0, 0, 2) with shadow 0 under white albedo: the lighting is ao * PI_INVERSE.  At SWEEP_SHAPE ao takes every value of SWEEP_AO once (the
    rest of the image repeats the sweep's end); a smaller image takes an evenly strided part of it, the four specials included.  The second
    image: ao 3.140625 under albedo bytes 1, 2, 3, ... (a different byte in every channel)."""
    rng = np.random.default_rng([W, H, 32])
    n = W * H
    if n >= len(SWEEP_AO):
        ao = np.concatenate([SWEEP_AO, np.full(n - len(SWEEP_AO), 0x4400, np.uint16)])
    elif n > 4:
        ao = np.concatenate([SWEEP_AO[np.linspace(0, len(SWEEP_AO) - 5, n - 4).astype(np.int64)], SWEEP_AO[-4:]])
    else:
        ao = SWEEP_AO[[9000]]
    sa = np.zeros((H, W, 2), np.uint16)
    sa[..., 1] = ao.reshape(H, W)
    white = np.full((H, W, 4), 255, np.uint8)
    common = dict(pfd=make_pfd(W, H), normals=_unit_normals(rng, W, H), motion=_motion(rng, W, H, 0.5, 0.5), depth=_depth(rng, W, H))
    yield _case("encode_sweep_ao", "encode_sweep", W, H, (0, 0, 2), albedo=white, shadow_ao=sa, full_sweep=n >= len(SWEEP_AO), **common)
    if (W, H) != SWEEP_SHAPE:
        idx = np.arange(n).reshape(H, W)
        albedo = np.stack([idx % 255 + 1, (idx + 85) % 255 + 1, (idx + 170) % 255 + 1, idx % 256], -1).astype(np.uint8)
        yield _case("encode_sweep_albedo", "encode_sweep", W, H, (0, 0, 2), albedo=albedo,
                    shadow_ao=_shadow_ao(np.zeros((H, W)), np.full((H, W), 3.140625), False), **common)


def material_edges_cases(W, H):
    """Every (metallic, roughness) pair of the two edge lists, pixel i takes pair i mod 49, under reflection_mode 0 and 1 with a constant
    non-grey reflections image."""
    idx = np.arange(W * H).reshape(H, W)
    metallic = np.float32(METALLIC_EDGES)[idx % 7]
    roughness = np.float32(ROUGHNESS_EDGES)[(idx // 7) % 7]
    for rmode in (0, 1):
        rng = np.random.default_rng([W, H, 33, rmode])
        yield _case(f"material_edges_r{rmode}", "material_edges", W, H, (0, 0, rmode), make_pfd(W, H),
                    rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8), _unit_normals(rng, W, H), _motion(rng, W, H, metallic, roughness),
                    _depth(rng, W, H), _shadow_ao(rng.uniform(0.5, 1, (H, W)), rng.uniform(0, 1, (H, W)), bool(rmode), rng),
                    reflections=_rgba16f(np.broadcast_to(np.float32(REFLECTION_COLOUR), (H, W, 3))))


def pixel_classes(W, H):
    """sky_and_zero_normal: 0 sky (depth 0, P non-finite), 1 N = 0 on a surface, 2 an ordinary surface -- by row, by column on a one-row image."""
    ys, xs = np.mgrid[0:H, 0:W]
    return (ys if H >= 3 else xs) % 3


def sky_and_zero_normal_cases(W, H):
    cls = pixel_classes(W, H)
    for modes in ((0, 0, 0), (2, 2, 1), (1, 1, 0), (1, 2, 2)):
        rng = np.random.default_rng([W, H, 34, *modes])
        projview = light_onto_plane((0.5, 0.5), (20.0, 12.0), 0.3, size=8) if modes[0] == 1 else None
        depth = _depth(rng, W, H)
        depth[cls == 0] = 0.0
        normals = _unit_normals(rng, W, H)
        normals[cls == 1, :3] = 0
        normals[(cls == 0) & (np.arange(W)[None, :] % 2 == 0), :3] = 0                      # the G-buffer clears a sky texel's normal; every other one keeps a unit normal
        albedo = rng.integers(1, 256, size=(H, W, 4), dtype=np.uint8)
        metallic = rng.choice(np.float32([0, 0.5, 1]), size=(H, W))
        yield _case(f"sky_and_zero_normal_{modes[0]}{modes[1]}{modes[2]}", "sky_and_zero_normal", W, H, modes, make_pfd(W, H, projview), albedo, normals,
                    _motion(rng, W, H, metallic, rng.uniform(0.04, 1, (H, W))), depth,
                    _shadow_ao(rng.uniform(0.25, 1, (H, W)), rng.uniform(0.25, 1, (H, W)), True, rng),
                    reflections=_rgba16f(rng.uniform(0.25, 1, (H, W, 3)), rng) if modes[2] != 2 else None,
                    ssao=_rgba16f(rng.uniform(0.25, 1, (H, W)), rng) if modes[1] == 1 else None,
                    shadow_map=two_level_map() if modes[0] == 1 else None, classes=cls)


def highlight_cases(W, H):
    """N is the fp16 rounding of H (within 2^-10 of it), roughness in [0.04, 0.1], modes (0, 2, 2) with shadow 1, 2^-8 or 2^-12 by pixel: the GGX
    peak, saturated or scaled back into range.  f = nh^2 (a^2 - 1) + 1 cancels here: the family is judged against the oracle alone."""
    rng = np.random.default_rng([W, H, 35])
    pfd = make_pfd(W, H)
    depth = _depth(rng, W, H)
    P = positions(pfd, depth)
    cam = nr._mat(pfd, "camera_view_inverse")[:3, 3]
    V = (cam - P) / np.linalg.norm(cam - P, axis=-1, keepdims=True)
    Hh = (TO_LIGHT + V) / np.linalg.norm(TO_LIGHT + V, axis=-1, keepdims=True)
    normals = np.zeros((H, W, 4), np.uint16)
    normals[..., :3] = _bits(Hh)
    shadow = np.float32([1.0, 2.0 ** -8, 2.0 ** -12])[np.arange(W * H).reshape(H, W) % 3]
    yield _case("highlight", "highlight", W, H, (0, 2, 2), pfd, rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8), normals,
                _motion(rng, W, H, rng.choice(np.float32([0, 0.5, 1]), size=(H, W)), rng.uniform(0.04, 0.1, (H, W))), depth,
                _shadow_ao(shadow, np.ones((H, W)), False))


PLANE_DEPTH = 3.0                                         # view depth of the plane the PCF families look at
HALF_WIDTH, HALF_HEIGHT = PLANE_DEPTH * np.tan(0.45) * 16.0 / 9.0, PLANE_DEPTH * np.tan(0.45)


@functools.lru_cache(maxsize=None)
def map_4096():
    """4096 x 4096, made in numpy: cleared texels (0) in rows below 256; depth 0.3 above row 2048 and 0.6 from it on (a step along a texel row),
    raised by 0.2 from column 2048 on (a step along a texel column); a 0.3 / 0.6 checkerboard from column 3072 on."""
    m = np.full((4096, 4096), 0.3, np.float32)
    m[2048:] = 0.6
    m[:, 2048:3072] += np.float32(0.2)
    ys, xs = np.mgrid[0:4096, 3072:4096]
    m[:, 3072:] = np.where((xs + ys) % 2 == 0, np.float32(0.3), np.float32(0.6))
    m[:256] = 0.0
    m.setflags(write=False)
    return m


def light_onto_plane(centre_uv, texels, sz, size=4096, z_gain=0.0):
    """A directional_light.projview (math matrix) that lays the camera-facing plane at view depth PLANE_DEPTH over `texels` (x, y) texels of a
    map of `size`, centred on the uv `centre_uv`, at light depth sz (+ z_gain per metre of world z off the plane)."""
    m = np.zeros((4, 4))
    m[0, 0] = (texels[0] / size) / HALF_WIDTH                    # ndc = 2 uv - 1: the plane's half width maps onto texels / 2 texels of uv
    m[0, 3] = 2.0 * centre_uv[0] - 1.0
    m[1, 1] = (texels[1] / size) / HALF_HEIGHT
    m[1, 3] = 2.0 * centre_uv[1] - 1.0 - m[1, 1] * 1.0           # the camera stands at y = 1
    m[2, 2] = z_gain
    m[2, 3] = sz + z_gain * PLANE_DEPTH
    m[3, 3] = 1.0
    return m


def _plane_case(name, family, W, H, projview, shadow_map, rng, depth=None, **extra):
    depth = np.full((H, W), ZNEAR / PLANE_DEPTH, np.float32) if depth is None else depth
    # modes (1, 0, 2): the shadow comes from the map -- shadow_ao's first channel holds a value that would show if it were read -- under a random ao
    return _case(name, family, W, H, (1, 0, 2), make_pfd(W, H, projview), rng.integers(64, 256, size=(H, W, 4), dtype=np.uint8),
                 _facing_normals(rng, W, H), _motion(rng, W, H, 0.25, 0.5), depth,
                 _shadow_ao(np.full((H, W), 0.123), rng.uniform(0.3, 1.0, (H, W)), bool(rng.integers(0, 2)), rng), shadow_map=shadow_map, **extra)


# The crossing of the two steps, off the texel corner by a phase under which no tap of the 130 x 9 image lands within fp32's coordinate resolution
# (2^-12 texels at u * 4096) of the place where its blend passes sz: the envelope caps need float64 to call all but one pixel of that image.  The
# smaller images and the checkerboard / knife-edge cases keep such taps (test_composition_cases.py counts them).
STEPS_CENTRE = (2048.29 / 4096.0, 2048.23 / 4096.0)


def pcf_4096_cases(W, H):
    rng = np.random.default_rng([W, H, 36])
    m = map_4096()
    # the plane spans 12 x 6 texels around a crossing of the two steps, at a light depth between the levels: a pixel's 16 taps fall on both sides
    yield _plane_case("pcf_4096_steps", "pcf_4096", W, H, light_onto_plane(STEPS_CENTRE, (12, 6), 0.45), m, rng)
    yield _plane_case("pcf_4096_cleared", "pcf_4096", W, H, light_onto_plane((0.25, 256.0 / 4096.0), (9, 7), 0.2), m, rng)
    # over the flat 0.3, at two view depths: sz is 0.3 - 1e-4 + 0.5e-4 (lit by half the bias) or 0.3 - 1e-4 - 0.5e-4 (dark by as much), far outside the undecided bound
    depth = (ZNEAR / (PLANE_DEPTH + np.where(rng.integers(0, 2, size=(H, W)) == 1, 0.05, -0.05))).astype(np.float32)
    yield _plane_case("pcf_4096_bias_band", "pcf_4096", W, H, light_onto_plane((0.25, 0.25), (30, 30), 0.3 - 1e-4, z_gain=-1e-3), m, rng, depth=depth)
    if W * H < CAPPED_FROM:
        # Cases float64 cannot call on most pixels, kept to the images below CAPPED_FROM pixels; the oracle rule holds them to the texel.  Over the
        # checkerboard every tap is a blend of 0.3 and 0.6 and the fp32 texel coordinate (2^-12 texels at u * 4096) decides which side of sz it falls.
        yield _plane_case("pcf_4096_checkerboard", "pcf_4096", W, H, light_onto_plane((0.875, 0.625), (10, 5), 0.45), m, rng)
        # over the flat 0.3: sz runs through 0.3 - 1e-4 by a few ulp per metre of world z, the view depth varies by 0.2 m
        depth = _depth(rng, W, H, PLANE_DEPTH - 0.1, PLANE_DEPTH + 0.1)
        sz = float(np.float32(0.3) - np.float32(1e-4))
        yield _plane_case("pcf_4096_knife_edge", "pcf_4096", W, H, light_onto_plane((0.25, 0.25), (30, 30), sz, z_gain=1e-6), m, rng, depth=depth)


WRAP_SALT = 37


def pcf_wrap_cases(W, H):
    """A 5 x 5 and a 1 x 1 map.  The light frustum covers a fraction of the plane, so the coordinates run over several periods on both sides of
    [0, 1]; every third column is sky (NaN and inf coordinates); under the `huge` projview u * W passes +-2^31."""
    rng = np.random.default_rng([W, H, WRAP_SALT])
    five = rng.uniform(0.2, 0.8, size=(5, 5)).astype(np.float32)
    one = np.float32([[0.45]])
    sky = (np.arange(W)[None, :] % 3 == 2) & np.ones((H, 1), bool)
    for label, sm in (("5x5", five), ("1x1", one)):
        size = sm.shape[0]
        for span, texels in (("periods", (7.3 * size, 5.1 * size)), ("huge", (3.0e10 * size, 2.0e10 * size))):
            if span == "huge" and size > 1 and W * H >= CAPPED_FROM:
                continue                 # float64 has no verdict on a tap whose coordinate fp32 resolves to thousands of texels: small images only
            depth = _depth(rng, W, H, PLANE_DEPTH - 0.1, PLANE_DEPTH + 0.1)            # sz runs over 0.45 +- 0.1: lit and dark pixels under the 1 x 1 map too
            depth[sky] = 0.0
            yield _plane_case(f"pcf_wrap_{label}_{span}", "pcf_wrap", W, H, light_onto_plane((0.5, 0.5), texels, 0.45, size=size, z_gain=1.0), sm, rng,
                              depth=depth)


def raytraced_cases(W, H):
    """raytraced_composition_kernel: every channel takes all 256 bytes (from 256 pixels on), out of step with one another; alpha 0, 1, 254, 255."""
    idx = np.arange(W * H).reshape(H, W)
    img = np.stack([idx % 256, (idx * 7 + 3) % 256, (255 - idx) % 256, np.uint8([0, 1, 254, 255])[idx % 4]], -1).astype(np.uint8)
    yield dict(name="raytraced_bytes", family="raytraced", kernel="raytraced_composition", W=W, H=H, image=img)
    rng = np.random.default_rng([W, H, 38])
    yield dict(name="raytraced_random", family="raytraced", kernel="raytraced_composition", W=W, H=H, image=rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8))


FAMILIES = (random_cases, encode_sweep_cases, material_edges_cases, sky_and_zero_normal_cases, highlight_cases, pcf_4096_cases, pcf_wrap_cases)


@functools.lru_cache(maxsize=None)
def all_cases(W, H):
    """cases(W, H) and raytraced_cases(W, H) as one tuple, built once: the tests share the arrays and leave them unchanged."""
    return tuple(cases(W, H)) + (tuple(raytraced_cases(W, H)) if (W, H) != SWEEP_SHAPE else ())


def cases(W, H):
    """Every composition_kernel case of one image size."""
    if (W, H) == SWEEP_SHAPE:
        yield from encode_sweep_cases(W, H)
        return
    for family in FAMILIES:
        yield from family(W, H)


# ---------------------------------------------------------------------------------------------------------
# the truth and the oracle on a case, and the judges
# ---------------------------------------------------------------------------------------------------------
def truth(c, mutant=None):
    if c["kernel"] == "raytraced_composition":
        return nr.raytraced_composition(c["image"])
    return nr.composition(c["pfd"], c["modes"], c["albedo"], c["normals"], c["motion"], c["depth"], c["shadow_ao"], c["reflections"], c["ssao"],
                          c["shadow_map"], mutant=mutant, delta=DELTA, eps=EPS, code_slack=CODE_SLACK)


@functools.lru_cache(maxsize=None)
def truth_of(W, H, i):
    """truth(all_cases(W, H)[i]), computed once and shared by the tests."""
    return truth(all_cases(W, H)[i])


def row(kernel, c, modes, differ, width, counts, judged="oracle"):
    """One COMPOSITION_CASES_TRUTH row: who was judged, kernel, case, shape, modes, channels that differ from the oracle (for the oracle's own rows:
    from the centre of the envelope), the worst envelope width in codes (-1: not judged against float64), the census."""
    return (f"COMPOSITION_CASES_TRUTH {judged:8s} {kernel:22s} {c['name']:34s} {c['W']:4d}x{c['H']:<4d} {modes:4s} {differ:6d} {width:4d} "
            + " ".join(f"{k}={v}" for k, v in counts.items()))


def oracle_image(oracle, c):
    """(texels (H, W, 4), the oracle's fp32 lighting before the store (H, W, 3) r g b), presented orientation."""
    if c["kernel"] == "raytraced_composition":
        return oracle.raytraced_composition(c["image"]), np.ascontiguousarray(c["image"][::-1, :, 2::-1].astype(np.float32) * np.float32(1.0 / 255.0))
    return oracle.composition(c["pfd"], c["modes"], c["albedo"], c["normals"], c["motion"], c["depth"], c["shadow_ao"], c["reflections"],
                              ssao=c["ssao"], shadow_map=c["shadow_map"], with_lighting=True)


def _what(c):
    return f"{c['kernel']} {c['name']} {c['W']}x{c['H']}"


def code_before_rounding(lighting):
    """e * 255 + 0.5 of the oracle's srgb8 (binary64 on the fp32 lighting); NaN where the store takes no encode (NaN, <= 0, >= 1)."""
    c = np.asarray(lighting, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (c > 0.0) & (c < 1.0)
        x = np.where(inside, c, 0.5)
        e = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    return np.where(inside, e * 255.0 + 0.5, np.nan)


def judge_against_oracle(c, got, want, want_lighting):
    """Per channel, no shares: got == oracle, or one code apart where the oracle's value before truncation lies within 1e-3 of an integer.  Alpha
    is 255 everywhere (the raytraced path's: the input's).  Returns (failures, the number of channels that differ from the oracle)."""
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    fails = []
    if got.shape != want.shape:
        return [f"{_what(c)}: shape {got.shape}, the oracle's is {want.shape}"], -1
    if not np.array_equal(got[..., 3], want[..., 3]):
        fails.append(f"{_what(c)}: alpha differs from {'the input' if c['kernel'] != 'composition' else '255'} on {int((got[..., 3] != want[..., 3]).sum())} texels")
    d = np.abs(got[..., :3].astype(np.int32) - want[..., :3].astype(np.int32))
    v = code_before_rounding(want_lighting)[..., ::-1]                                   # r g b -> b g r
    with np.errstate(invalid="ignore"):
        near = np.abs(v - np.rint(v)) <= CODE_SLACK
    bad = (d > 1) | ((d == 1) & ~near)
    if bad.any():
        at = np.argwhere(bad)[:4].tolist()
        fails.append(f"{_what(c)}: {int(bad.sum())} channels differ from the oracle beyond the rounding allowance, worst {int(d.max())} codes, first (y, x, bgr) {at}: "
                     f"got {[int(got[y, x, k]) for y, x, k in at]}, oracle {[int(want[y, x, k]) for y, x, k in at]}")
    return fails, int((d != 0).sum())


def share_exceeds(mask, share):
    """A share bar `mask.mean() <= share`; a set of fewer than 1 / share members admits no exception."""
    return bool(mask.any()) if mask.size * share < 1.0 else bool(mask.mean() > share)


def judge_against_float64(c, got, ref):
    """Per channel: code_lo <= got <= code_hi of the float64 envelope, alpha 255 (the raytraced path's: the input's).
    Returns (failures, the worst envelope width in codes)."""
    got = np.asarray(got, np.uint8)
    fails = []
    if c["kernel"] == "raytraced_composition":
        codes, lo, hi = ref
        if not np.array_equal(got[..., 3], codes[..., 3]):
            fails.append(f"{_what(c)}: alpha did not pass through on {int((got[..., 3] != codes[..., 3]).sum())} texels")
    else:
        lo, hi = ref["code_lo"], ref["code_hi"]
        if not (got[..., 3] == 255).all():
            fails.append(f"{_what(c)}: alpha is not 255 on {int((got[..., 3] != 255).sum())} texels")
    if got.shape[:2] != lo.shape[:2]:
        return fails + [f"{_what(c)}: shape {got.shape}"], -1
    outside = (got[..., :3] < lo) | (got[..., :3] > hi)
    if outside.any():
        at = np.argwhere(outside)[:4].tolist()
        fails.append(f"{_what(c)}: {int(outside.sum())} channels outside the float64 envelope, first (y, x, bgr) {at}: got {[int(got[y, x, k]) for y, x, k in at]}, "
                     f"envelope {[(int(lo[y, x, k]), int(hi[y, x, k])) for y, x, k in at]}")
    return fails, int((hi.astype(np.int32) - lo).max())


def envelope_caps(c, ref):
    """The caps on the envelope's width, per case of CAPPED_FROM pixels and more outside UNCAPPED: exactly one code on >= 99 % of the channels, more
    than two codes on <= 0.1 %.  Returns (failures, share with one code, share with more than two)."""
    width = ref["code_hi"].astype(np.int32) - ref["code_lo"] + 1
    one, wide = float((width == 1).mean()), float((width > 2).mean())
    fails = []
    if c["W"] * c["H"] >= CAPPED_FROM and c["family"] not in UNCAPPED:
        if one < 0.99:
            fails.append(f"{_what(c)}: the envelope admits exactly one code on {one:.4%} of the channels (>= 99 %)")
        if share_exceeds(width > 2, 1e-3):
            fails.append(f"{_what(c)}: the envelope admits more than two codes on {wide:.4%} of the channels (<= 0.1 %)")
    return fails, one, wide


def judge_case_properties(c, got):
    """What a case knows without a reference: saturated pixels exactly 255, dark pixels exactly 0."""
    got = np.asarray(got, np.uint8)
    fails = []
    if c["name"] == "encode_sweep_ao":
        ao = nr.h2f(c["shadow_ao"][..., 1])[::-1]
        with np.errstate(invalid="ignore"):
            bright, dark = ao >= 3.15, ~(ao > 0)                                           # ao / pi >= 1 from 3.1416 on; 0, -0.0, -1 and NaN store 0
        if not (got[bright][:, :3] == 255).all():
            fails.append(f"{_what(c)}: {int((got[bright][:, :3] != 255).any(-1).sum())} saturated pixels are not exactly 255")
        if not (got[dark][:, :3] == 0).all():
            fails.append(f"{_what(c)}: {int((got[dark][:, :3] != 0).any(-1).sum())} dark pixels (ao 0, -0.0, -1, NaN) are not exactly 0")
    return fails


def census(c, ref):
    """What a case reaches, from the float64 truth (as nr.ssao_sample_census reports the SSAO samples)."""
    out = {}
    if c["kernel"] != "composition":
        for k in range(4):
            out[f"bytes_ch{k}"] = len(np.unique(c["image"][..., k]))
        return out
    mr = nr.h2f(c["motion"])[..., 2:4]
    if c["family"] == "material_edges":
        m, r = mr[..., 0], mr[..., 1]
        with np.errstate(invalid="ignore"):
            out.update(metallic_below_0=int((m < 0).sum()), metallic_inside=int(((m > 0) & (m < 1)).sum()), metallic_exactly_1=int((m == 1).sum()),
                       metallic_above_1=int((m > 1).sum()), metallic_nan=int(np.isnan(m).sum()), roughness_below_floor=int((r < 0.04).sum()),
                       roughness_inside=int(((r >= 0.04) & (r <= 1)).sum()), roughness_above_1=int((r > 1).sum()), roughness_nan=int(np.isnan(r).sum()))
    if c["family"] == "encode_sweep":
        codes = ref["codes"][..., :3]
        with np.errstate(invalid="ignore"):
            out.update(codes_reached=len(np.unique(codes)), linear_segment=int(((ref["lighting"] > 0) & (ref["lighting"] <= 0.0031308)).sum()),
                       saturated=int((ref["lighting"] >= 1).sum()), stores_0_special=int((~(ref["lighting"] > 0)).sum()))
    if c["family"] == "sky_and_zero_normal":
        cls = c["classes"][::-1]
        for k, label in enumerate(("sky", "zero_normal", "surface")):
            sel = ref["lighting"][cls == k]
            out[f"{label}_pixels"] = int((cls == k).sum())
            out[f"{label}_non_finite"] = int((~np.isfinite(sel)).any(-1).sum())
    if ref.get("pcf") is not None:
        lit, und = ref["pcf"]["lit"], ref["pcf"]["undecided"]
        out.update(fully_lit=int((lit == 16).sum()), fully_dark=int((lit == 0).sum()), undecided_pixels=int((und > 0).sum()))
        out.update(partly_lit=int(((lit >= 1) & (lit <= 15)).sum()), undecided_taps=int(und.sum()), **ref["pcf"]["census"])
    return out
