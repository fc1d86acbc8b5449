"""The scene, masks, sub-scenes and rays of the ray cull mask tests (tests/test_ray_masks_host.py, tests/test_gpu_ray_masks.py).  No tests here.

The truth needs no new oracle: a ray of mask m on scene A must see, bit for bit, what the plain ray sees on the scene made of A's
primitives p with masks[p] & m != 0 (sub_scene), because results never depend on the tree.  The oracle's shadow channel does not
depend on ao_spp, its AO channel not on shadow_enable, its reflections on neither (asserted in the host tests), so a frame with three
different class masks has a composite truth: shadow from sub(shadow mask), AO from sub(AO mask), reflections from sub(reflection mask)."""
import numpy as np

from tests import alpha_scenes
from vulkanhybridrenderer_amd import abi, ray_queries, scenes
from vulkanhybridrenderer_amd.scenes import _Builder, box, plane, trs

W, H, FRAMES = 72, 56, 3
N_TINY = 5                                                        # tiny_scene()'s primitives come first, all at 0xFF
OCCLUDER_MASKS = [0x01, 0x02, 0x04, 0x03, 0x06, 0x05, 0x00]        # in the order the occluders are appended
SHADOW_MASK, AO_MASK, REFLECTION_MASK = 0x01, 0x02, 0x04
QUERY_MASKS = [0x01, 0x02, 0x04, 0x03, 0xFF, 0x00]
N_RANDOM, N_AIMED = 1000, 30                                      # random_rays' count, and rays aimed at every occluder


def scene():
    """tiny_scene() plus seven OPAQUE untextured occluders with the geometry of alpha_scenes._uniform's seven: 12 primitives, 396 triangles."""
    tiny = scenes.tiny_scene()
    b = _Builder()
    b.v, b.i, b.p = [tiny.vertices], [tiny.indices], list(tiny.primitives)
    b.nv, b.ni = len(tiny.vertices), len(tiny.indices)
    b.add(plane([2.3, 0.5, 3.2], [1.4, 0, 0], [0, 0, -1.4], 2, 2), base_color=(0.8, 0.3, 0.3, 1.0))              # a low quad over the floor's right front
    b.add(plane([2.0, 0.8, -3.4], [1.6, 0, 0], [0, 1.8, 0], 1, 1), base_color=(0.3, 0.8, 0.4, 1.0))             # upright in front of the back wall's right
    b.add(plane([0.4, 0.4, 3.6], [0.9, 0, 0], [0, 0, -0.9], 1, 1), base_color=(0.8, 0.8, 0.3, 1.0))             # a small quad over the floor's middle front
    b.add(plane([-3.8, 0.7, 3.6], [3.0, 0, 0], [0, 0, -2.6], 3, 2), base_color=(0.8, 0.3, 0.8, 1.0))            # a wide low quad over the floor's left front
    b.add(box((1.4, 0.5, 1.4), 2), transform=trs((1.2, 1.2, 2.2), rot_y=0.3), base_color=(0.9, 0.2, 0.7, 1.0))   # a box hovering in front of the sphere
    b.add(plane([-3.8, 0.3, -3.3], [3.4, 0, 0], [0, 3.6, 0], 2, 2), base_color=(0.1, 0.9, 0.9, 1.0))            # upright in front of the back wall's left
    b.add(plane([-2.2, 1.9, 1.6], [4.6, 0, 0], [0, 0, -3.6], 3, 3), base_color=(0.3, 0.3, 0.9, 1.0))            # a canopy between the light and the floor
    return b.finish("ray_masks_A", tiny.camera, tiny.light, [])


def masks(sc=None):
    """One byte per primitive of scene(): 0xFF for tiny's five, then OCCLUDER_MASKS."""
    return np.array([0xFF] * N_TINY + OCCLUDER_MASKS, np.uint8)


def sub_scene(sc, prim_masks, m):
    """(the scene made of sc's primitives p with prim_masks[p] & m != 0, their indices in sc): what a ray of mask m sees.  A hit's
    geometry_index j on the sub-scene is keep[j] on sc; primitive_index, t, u, v are the same."""
    keep = np.nonzero(np.asarray(prim_masks, np.uint8) & np.uint8(m & 0xFF))[0]
    return (alpha_scenes.subset(sc, keep) if len(keep) else None), keep          # mask 0 keeps nothing: no scene, every ray misses


def remap_hits(hits, keep):
    """Closest hits on a sub-scene with geometry_index in the full scene's numbering."""
    out = hits.copy()
    hit = out["geometry_index"] != abi.RAY_MISS
    out["geometry_index"][hit] = np.asarray(keep, np.uint32)[out["geometry_index"][hit]]
    return out


def triangle_ranges(sc):
    """first flat triangle of every primitive, plus the total (len = primitives + 1)"""
    return np.concatenate([[0], np.cumsum(sc.primitives["index_count"] // 3)]).astype(np.int64)


def rays(sc, first_occluder=N_TINY):
    """random_rays with the alpha test's parameters (seed 5, 1 000 rays), then N_AIMED rays aimed at the interior of every occluder's
    triangles from origins inside the scene's bounds (the small quad is met by none of the random ones).  1 210 rays: no multiple of 64."""
    lo, hi = ray_queries.scene_bounds(sc)
    rng = np.random.default_rng(5)
    out = [ray_queries.random_rays(rng, N_RANDOM, lo, hi, margin=0.2, tmins=(0.0, 0.01), tmaxs=(np.inf, 3.0, 20.0, 1e4))]
    tris = ray_queries.world_triangles(sc)
    first = triangle_ranges(sc)
    for p in range(first_occluder, len(sc.primitives)):
        k = rng.integers(first[p], first[p + 1], N_AIMED)
        bu, bv = rng.uniform(0.1, 0.9, N_AIMED), rng.uniform(0.1, 0.9, N_AIMED)
        flip = bu + bv > 1
        bu[flip], bv[flip] = 1 - bu[flip], 1 - bv[flip]
        target = tris[k, 0] + bu[:, None] * (tris[k, 1] - tris[k, 0]) + bv[:, None] * (tris[k, 2] - tris[k, 0])
        origin = rng.uniform(lo, hi, (N_AIMED, 3))
        d = target - origin
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = np.zeros((N_AIMED, 8), np.float32)
        r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7] = origin, d, 0.0, np.inf
        out.append(r)
    return np.concatenate(out)


def hit_bits_differ(a, b):
    """per ray: the two closest-hit records differ in some bit"""
    return (a.view(np.uint32).reshape(-1, 6) != b.view(np.uint32).reshape(-1, 6)).any(axis=1)
