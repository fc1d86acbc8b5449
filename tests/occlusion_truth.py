"""The truth of vhr_occlusion_query, restated from the oracle's own primitives and never from the library: ray (i, j) of a query point from
orc_seed_thread, orc_random01, orc_cosine_hemisphere and orc_onb, the product (c0 v.x + c1 v.y) + n v.z in np.float32 in onb_transform's order,
and occlusion by oracle.Scene.occluded one ray at a time (use_bvh=False on the small soups: a brute force over the triangles).

Query points are (n, 8) float32 rows: origin, tmin, axis, tmax (abi.ray_dtype read as the contract reads it)."""
import ctypes as C

import numpy as np

from oracle import binding as ob

ZERO_STATE = 0x9E3779B9          # what a state of 0 is replaced by
M32 = 0xFFFFFFFF


def seed_thread(x):
    return int(ob.lib().orc_seed_thread(x & M32))


def ray_index(i, j, samples):
    return (i * samples + j) & M32


def state_of(g, seed):
    """The generator's state for ray index g: seed_thread(g ^ seed_thread(seed)), 0 replaced."""
    return seed_thread(g ^ seed_thread(seed)) or ZERO_STATE


def direction(axis, state):
    """onb_transform(axis, cosine_hemisphere(random01(state), random01(state))) in float32, each operation rounded once."""
    L = ob.lib()
    st = C.c_uint32(state)
    r1 = L.orc_random01(C.byref(st))
    r2 = L.orc_random01(C.byref(st))
    v = np.zeros(3, np.float32)
    L.orc_cosine_hemisphere(r1, r2, v.ctypes.data_as(C.c_void_p))
    n = np.ascontiguousarray(axis, np.float32)
    M = np.zeros(9, np.float32)
    L.orc_onb(n.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p))
    c0, c1, c2 = M[0:3], M[3:6], M[6:9]
    with np.errstate(all="ignore"):
        return (c0 * v[0] + c1 * v[1]) + c2 * v[2]


def rays(points, samples, seed, first=0):
    """(n, samples, 8) float32: the rays of `points`, whose first is point number `first` of its call."""
    points = np.asarray(points, np.float32)
    out = np.empty((len(points), samples, 8), np.float32)
    out[:, :, 0:4] = points[:, None, 0:4]
    out[:, :, 7] = points[:, None, 7]
    for i, p in enumerate(points):
        for j in range(samples):
            out[i, j, 4:7] = direction(p[4:7], state_of(ray_index(first + i, j, samples), seed))
    return out


def masks_of_rays(osc, r, use_bvh=False):
    """uint64[n] from (n, samples, 8) rays: bit j of entry i = the oracle finds ray (i, j) occluded."""
    out = np.zeros(len(r), np.uint64)
    for i in range(len(r)):
        m = 0
        for j in range(r.shape[1]):
            q = r[i, j]
            if osc.occluded(q[0:3], q[4:7], float(q[3]), float(q[7]), use_bvh=use_bvh):
                m |= 1 << j
        out[i] = m
    return out


def masks(osc, points, samples, seed, use_bvh=False):
    """uint64[n]: bit j of entry i = the oracle finds ray (i, j) of `points` occluded."""
    return masks_of_rays(osc, rays(points, samples, seed), use_bvh)


def popcount(m):
    return int(sum(bin(int(x)).count("1") for x in np.asarray(m).reshape(-1)))


def invert_seed_thread(y):
    """The x with seed_thread(x) == y: the hash is a bijection, undone step by step."""
    def unxorshift(v, s):              # undo v ^= v >> s
        r = v
        k = s
        while k < 32:
            r = v ^ (r >> s)
            k += s
        return r & M32
    v = unxorshift(y & M32, 15)
    v = (v * pow(0x27d4eb2d, -1, 1 << 32)) & M32
    v = unxorshift(v, 4)
    v = (v * pow(9, -1, 1 << 32)) & M32
    # v = (x ^ 61) ^ (x >> 16): the high half of x is v's, the low half follows
    hi = v >> 16
    lo = (v ^ 61 ^ hi) & 0xFFFF
    x = (hi << 16) | lo
    assert seed_thread(x) == (y & M32)
    return x
