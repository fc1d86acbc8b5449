"""Scenes whose ordinary images name the triangle a closest-hit kernel committed.  TEST INFRASTRUCTURE (tests/test_closest_truth.py,
tests/test_gpu_closest_truth.py).

per_triangle() splits every primitive of a scene into one primitive per triangle -- the parent's transform and vertex block,
index_offset + 3k, index_count 3 -- so the flat triangle index IS the primitive index, and gives primitive i a base colour that spells
i in base 14, one digit per channel, on a table of levels chosen for the image that will carry it:

    MIRROR_LEVELS      (d + 1) / 16                the mirror ray's fp16 payload: with the light's intensity 0, reflection_hit.rchit leaves
                                                   albedo * (0.2 / pi); fp16 keeps a level to 15 * 2^-12 = 0.0037 of the spacing
    RAYTRACED_LEVELS   5 (d + 1) pi / 255          the raytraced path's B8G8R8A8_UNORM image: with the light's colour 0, closesthit.rchit
                                                   leaves albedo / pi, which lands on the code values 5, 10, ..., 70

The stand-in G-buffer needs no colour: NORMALS.w is the primitive index, exact in fp16 up to 2 048.

A decoder RAISES (Undecodable) when a channel lies farther than a quarter of the level spacing from every level (raytraced: more than
one code value), when a digit is out of range or the index is beyond the scene: a shading error must surface as "undecodable", never
as another triangle."""
import dataclasses

import numpy as np

BASE = 14
MIRROR_LEVELS = (np.arange(BASE) + 1) / 16.0
RAYTRACED_LEVELS = 5.0 * (np.arange(BASE) + 1) * np.pi / 255.0
MIRROR_AMBIENT = 0.2 / np.pi                                  # reflection_hit.rchit:59, ambient_factor
RAYTRACED_MISS_BGRA = (51, 204, 77, 255)                      # miss.rmiss:7, (0.3, 0.8, 0.2, 1) through the UNORM store
MAX_IDS = 2048                                                # integers fp16 holds exactly


class Undecodable(ValueError):
    pass


def digits(index):
    """(n,) indices -> (n, 3) base-14 digits, least significant first."""
    index = np.asarray(index, np.int64)
    return np.stack([(index // BASE ** c) % BASE for c in range(3)], -1)


def per_triangle(scene, levels, ids=False):
    """`scene` with one primitive per triangle, flat order kept, primitive i coloured levels[digit_c(i)] per channel, alpha 1, metallic 0,
    roughness 1, no textures in use.  ids=True: the primitive index must also fit NORMALS.w (<= 2 048 primitives)."""
    P = scene.primitives
    counts = P["index_count"].astype(np.int64) // 3
    parent = np.repeat(np.arange(len(P)), counts)
    k = np.arange(len(parent)) - np.repeat(np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)
    prims = P[parent].copy()
    prims["index_offset"] = P["index_offset"][parent].astype(np.int64) + 3 * k
    prims["index_count"] = 3
    n = len(prims)
    assert n < BASE ** 3, f"{n} triangles do not fit three base-{BASE} digits"
    assert not ids or n <= MAX_IDS, f"{n} primitives: NORMALS.w is exact only up to {MAX_IDS}"
    m = prims["material"]
    m["base_color"][:, :3] = np.asarray(levels, np.float64)[digits(np.arange(n))]
    m["base_color"][:, 3] = 1.0
    m["metallic_factor"], m["roughness_factor"] = 0.0, 1.0
    for name in ("base_color_texture", "metallic_roughness_texture", "normal_map"):
        assert (m[name] == -1).all(), f"{name}: the colour code needs untextured primitives"
    assert (m["alpha_mask"] == 0).all()
    return dataclasses.replace(scene, primitives=prims)


def _flat_of_levels(level, bad, spacing_limit, count, what):
    """level: (n, 3) float64, a channel in units of the level spacing (digit d sits at d); bad: rows to leave alone (misses)."""
    d = np.rint(level)
    with np.errstate(invalid="ignore"):
        off = ~(np.abs(level - d) <= spacing_limit) | ~((d >= 0) & (d < BASE))          # (NaN: off)
    off = off.any(-1) & ~bad
    if off.any():
        raise Undecodable(f"{what}: {int(off.sum())} hits carry no level of the table, first rows {np.nonzero(off)[0][:4].tolist()}, levels {level[off][:2].tolist()}")
    d = np.where(bad[:, None], 0, np.nan_to_num(d)).astype(np.int64)
    flat = d[:, 0] + BASE * d[:, 1] + BASE * BASE * d[:, 2]
    if count is not None and (flat >= count).any():
        raise Undecodable(f"{what}: index {int(flat.max())} is beyond the scene's {count} triangles")
    return flat


def decode_mirror(bits, count=None):
    """REFLECTIONS texels ((n, 4) uint16, RGBA16F bits) of a per_triangle(.., MIRROR_LEVELS) scene lit with intensity 0 -> (hit, flat)."""
    v = np.asarray(bits, np.uint16).reshape(-1, 4).view(np.float16).astype(np.float64)
    alpha = v[:, 3]
    if not np.isin(alpha, (0.0, 1.0)).all():
        raise Undecodable(f"mirror payload: alpha is neither 0 nor 1 on {int((~np.isin(alpha, (0.0, 1.0))).sum())} texels")
    hit = alpha == 1.0
    return hit, _flat_of_levels(v[:, :3] / MIRROR_AMBIENT * 16.0 - 1.0, ~hit, 0.25, count, "mirror payload")


def decode_raytraced(bgra8, count=None):
    """RAYTRACED_OUTPUT texels ((n, 4) uint8, B8G8R8A8) of a per_triangle(.., RAYTRACED_LEVELS) scene lit with colour 0 -> (hit, flat)."""
    c = np.asarray(bgra8, np.uint8).reshape(-1, 4).astype(np.float64)
    if not (c[:, 3] == 255).all():
        raise Undecodable("raytraced image: alpha is not 1 everywhere")
    hit = ~(c == RAYTRACED_MISS_BGRA).all(-1)
    return hit, _flat_of_levels(c[:, [2, 1, 0]] / 5.0 - 1.0, ~hit, 1.0 / 5.0 + 1e-9, count, "raytraced image")


def decode_ids(normals_bits, covered=None, count=None):
    """NORMALS texels ((n, 4) uint16, RGBA16F bits) and coverage (DEPTH != 0; None: a normal that is not the clear value) -> (hit, flat):
    NORMALS.w is the primitive index."""
    n = np.asarray(normals_bits, np.uint16).reshape(-1, 4)
    w = n.view(np.float16).astype(np.float64)[:, 3]
    hit = np.asarray(covered, bool).reshape(-1) if covered is not None else ((n[:, :3] & 0x7fff) != 0).any(-1)
    bad = hit & ~((w == np.rint(w)) & (w >= 0) & (w < (MAX_IDS if count is None else count)))
    if bad.any():
        raise Undecodable(f"NORMALS.w: {int(bad.sum())} covered texels hold no primitive index, first {w[bad][:4].tolist()}")
    return hit, np.where(hit, np.nan_to_num(w), 0).astype(np.int64)


def encode_mirror(flat):
    """What decode_mirror reads for hits on `flat`, exactly: (n, 4) uint16."""
    rgb = np.float32(MIRROR_LEVELS.astype(np.float32)[digits(flat)] * np.float32(MIRROR_AMBIENT))
    return np.concatenate([rgb, np.ones((len(rgb), 1), np.float32)], 1).astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------------
# the cases tests/test_closest_truth.py and tests/test_gpu_closest_truth.py share: 96 x 64, frame 1 of the dolly
# ---------------------------------------------------------------------------------------------
W, H = 96, 64
NAMES = ("soup 2", "soup 3")
RAYTRACED_SCALES = (2.0 ** -4, 1.0, 2.0 ** 10)      # raygen.rgen:20 hard-codes tmin = 0.1: at 2^-10 the whole 6 mm scene lies in front of
                                                    # 0.1 m and every primary ray misses, so the smallest unit this path can be judged at is 2^-4
_CASES = {}


def base_scene(name, levels):
    from tests import ray_truth as rt
    kind, _, seed = name.partition(" ")
    return per_triangle(rt.tiny_far() if kind == "tiny_far" else rt.soup_scene(int(seed)), levels, ids=True)


def rays_of(log, kind, n_pixels):
    """The rays of one kind of an oracle ray log, one per pixel at most -> (pixel int64[n], rays (n, 8) float32)."""
    sel = log[log["kind"] == kind]
    assert len(np.unique(sel["pixel"])) == len(sel) and (sel["pixel"] < n_pixels).all()
    rays = np.zeros((len(sel), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = sel["o"], sel["tmin"], sel["d"], sel["tmax"]
    return sel["pixel"].astype(np.int64), rays


@dataclasses.dataclass
class Probe:
    """One kind of ray of one case: the pixels and rays the oracle logged, their truth, the oracle's own answer (hit, flat) per ray and
    how many candidates its walk decided again in binary64."""
    pix: np.ndarray
    rays: np.ndarray
    truth: object
    hit: np.ndarray
    flat: np.ndarray
    escalated: int


def hybrid_case(ob, name, scale):
    """`name` split per triangle with the mirror table, every length times `scale`: the oracle's G-buffer (PRIMARY rays, ids from NORMALS.w)
    and its mirror ray from that G-buffer (no shadow, no AO, light intensity 0).  Computed once and left unchanged.
    -> dict(scene, osc, pfd, gbuf, tp, reflections, log_g, log_m, primary: Probe, mirror: Probe)"""
    from tests import ray_truth as rt
    from vulkanhybridrenderer_amd import abi, camera
    key = ("hybrid", name, scale)
    if key not in _CASES:
        scene = rt.scaled_scene(base_scene(name, MIRROR_LEVELS), scale)
        n = len(scene.primitives)
        osc = ob.Scene(scene)
        pfd = camera.dolly_frames(scene, W, H, 2)[1]
        pfd["directional_light"]["intensity"][:3] = 0.0
        tp = rt.scaled_trace_params(abi.default_trace_params(shadow=False, ao_spp=0, reflections=True), scale)
        with ob.Audit(ray_log=4 * W * H) as g:
            gbuf = osc.gbuffer(pfd, W, H)
        with ob.Audit(ray_log=4 * W * H) as m:
            refl = osc.raygen(pfd, tp, gbuf[0], gbuf[2])[1]
        pix, rays = rays_of(g.ray_log, ob.RAY_KIND_PRIMARY, W * H)
        hit, flat = decode_ids(gbuf[0].reshape(-1, 4)[pix], gbuf[2].reshape(-1)[pix] != 0, n)
        primary = Probe(pix, rays, rt.Truth(ob, osc, rays), hit, flat, int(g.counts["escalated"]))
        pix, rays = rays_of(m.ray_log, ob.RAY_KIND_MIRROR, W * H)
        hit, flat = decode_mirror(refl.reshape(-1, 4)[pix], n)
        mirror = Probe(pix, rays, rt.Truth(ob, osc, rays), hit, flat, int(m.counts["escalated"]))
        _CASES[key] = dict(scene=scene, osc=osc, pfd=pfd, gbuf=gbuf, tp=tp, reflections=refl, log_g=g.ray_log, log_m=m.ray_log, primary=primary, mirror=mirror)
    return _CASES[key]


def raytraced_case(ob, name, scale):
    """`name` split per triangle with the raytraced table, every length times `scale`, light colour 0: the oracle's raytraced image.
    -> dict(scene, osc, pfd, image, log, primary: Probe)"""
    from tests import ray_truth as rt
    from vulkanhybridrenderer_amd import camera
    key = ("raytraced", name, scale)
    if key not in _CASES:
        scene = rt.scaled_scene(base_scene(name, RAYTRACED_LEVELS), scale)
        osc = ob.Scene(scene)
        pfd = camera.dolly_frames(scene, W, H, 2)[1]
        pfd["directional_light"]["color"][:3] = 0.0
        with ob.Audit(ray_log=4 * W * H) as a:
            image, _ = osc.raytraced(pfd, W, H, False)
        pix, rays = rays_of(a.ray_log, ob.RAY_KIND_PRIMARY, W * H)
        hit, flat = decode_raytraced(image.reshape(-1, 4)[pix], len(scene.primitives))
        _CASES[key] = dict(scene=scene, osc=osc, pfd=pfd, image=image, log=a.ray_log,
                           primary=Probe(pix, rays, rt.Truth(ob, osc, rays), hit, flat, int(a.counts["escalated"])))
    return _CASES[key]


def front_ties(truth):
    """Rays whose exact closest hit shares its exact t with another exact hit of the ray (the soups' duplicates) -> bool[n]."""
    order = np.lexsort((truth.flat, truth.t, truth.ray))
    order = order[truth.hit[order]]
    r, t = truth.ray[order], truth.t[order]
    first = np.ones(len(order), bool)
    first[1:] = r[1:] != r[:-1]
    i = np.nonzero(first)[0]
    i = i[i + 1 < len(order)]
    i = i[(r[i + 1] == r[i]) & (t[i + 1] == t[i])]
    tie = np.zeros(truth.n, bool)
    tie[r[i]] = True
    return tie


GALLERY_COLUMNS, GALLERY_PIXELS = 64, 4


def gallery(n, levels):
    """n triangles side by side in the plane z = 0, one per unit cell of a 64-column grid, seen head-on by a camera whose image gives
    every cell 4 x 4 pixels (gallery_size(n)): every index of the code reaches the image.  -> the per_triangle scene"""
    from vulkanhybridrenderer_amd import scenes
    from vulkanhybridrenderer_amd.camera import directional_light
    rows = -(-n // GALLERY_COLUMNS)
    i = np.arange(n)
    corner = np.stack([i % GALLERY_COLUMNS, i // GALLERY_COLUMNS, np.zeros(n)], -1).astype(np.float64)
    tri = corner[:, None, :] + np.array([[0.05, 0.05, 0.0], [0.95, 0.05, 0.0], [0.5, 0.95, 0.0]])
    pos = tri.reshape(-1, 3).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(pos), 1))
    b = scenes._Builder()
    b.add((pos, nrm, np.zeros((len(pos), 2), np.float32), np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)))
    distance = 40.0
    camera = dict(position=(GALLERY_COLUMNS / 2, rows / 2, distance), yaw=0.0, pitch=0.0, yfov=2 * np.arctan(rows / 2 / distance), znear=0.1,
                  aspect=GALLERY_COLUMNS / rows, dolly=(0.0, 0.0, 0.0))
    return per_triangle(b.finish("gallery", camera, directional_light((0.25, -0.9, 0.3))), levels, ids=True)


def gallery_size(n):
    return GALLERY_COLUMNS * GALLERY_PIXELS, -(-n // GALLERY_COLUMNS) * GALLERY_PIXELS
