"""What the surface-point tests share (tests/test_surface_host.py, tests/test_gpu_surface.py, tools/surface_rate.py).  No tests here.

resolve() restates the contract of vhr_resolve_hits (include/vhr_amd.h) in numpy float32, one operation per rounding: the checks that leave a
hit unresolved, the record by the builders' world_record, position, geometric normal, uv, shading normal and -- with material=True -- the
gbuf.frag lines of the stand-in G-buffer (base colour, discard, normal map, metallic / roughness) on a restatement of the library's texture
fetch.  geometry64() is the geometry part in binary64, and position_bound() the bound the fp32 position keeps to it."""
import math

import numpy as np

from tests.helpers import _wrap          # wrap_coord: the address modes on integer texel coordinates
from vulkanhybridrenderer_amd import abi

F = np.float32
MISS = 0xFFFFFFFF
VALID, DEGENERATE, NO_SHADING_NORMAL, NORMAL_MAPPED, DISCARDED = (abi.SURFACE_VALID, abi.SURFACE_DEGENERATE, abi.SURFACE_NO_SHADING_NORMAL,
                                                                  abi.SURFACE_NORMAL_MAPPED, abi.SURFACE_DISCARDED)
FIELDS = ("position", "flags", "geometric_normal", "metallic", "shading_normal", "roughness", "base_color", "uv0", "uv1")
GEOMETRY_FIELDS = ("position", "flags", "geometric_normal", "shading_normal", "uv0", "uv1")

# the sRGB decode table of the texture fetch (context.cpp: binary64, rounded once)
SRGB_LUT = np.array([(i / 255.0) / 12.92 if i / 255.0 <= 0.04045 else math.pow((i / 255.0 + 0.055) / 1.055, 2.4) for i in range(256)], np.float64).astype(F)


def same_bits(a, b, fields=FIELDS):
    """Field by field, bit for bit (-0 is not +0, a NaN equals itself): the names of the fields that differ."""
    return [f for f in fields if not np.array_equal(np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32))]


def hits_of(prim, tri, u, v):
    h = np.zeros(len(prim), abi.ray_hit_dtype)
    h["geometry_index"], h["primitive_index"], h["u"], h["v"] = prim, tri, u, v
    return h


def triangle_ids(scene):
    """(primitive, triangle within it) of every triangle, flat order."""
    counts = scene.primitives["index_count"].astype(np.int64) // 3
    prim = np.repeat(np.arange(len(counts)), counts)
    tri = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, np.int64)
    return prim.astype(np.uint32), tri.astype(np.uint32)


def triangle_hits(scene, seed, per_triangle=2):
    """Every triangle at `per_triangle` random barycentrics inside it and at its three corners: ray_hit_dtype, triangle-major."""
    prim, tri = triangle_ids(scene)
    rng = np.random.default_rng(seed)
    n = len(prim)
    a, b = rng.random((n, per_triangle)), rng.random((n, per_triangle))
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    u = np.concatenate([a, np.tile([0.0, 1.0, 0.0], (n, 1))], 1).astype(F)
    v = np.concatenate([b, np.tile([0.0, 0.0, 1.0], (n, 1))], 1).astype(F)
    k = per_triangle + 3
    return hits_of(np.repeat(prim, k), np.repeat(tri, k), u.reshape(-1), v.reshape(-1))


def flips_of(scene):
    """The facing-flip byte per primitive by the header's rule: binary64 cofactors along the first row of the transform's upper 3 x 3."""
    m = scene.primitives["transform"].astype(np.float64).reshape(-1, 16)
    m00, m10, m20, m01, m11, m21, m02, m12, m22 = m[:, 0], m[:, 1], m[:, 2], m[:, 4], m[:, 5], m[:, 6], m[:, 8], m[:, 9], m[:, 10]
    det = (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20)
    return (det < 0).astype(np.uint8)


def normal_matrices(scene):
    """inverseTranspose(mat3(transform)) per primitive, 9 floats column-major: geometry.cpp's normal_matrix3, binary64, rounded once."""
    m = scene.primitives["transform"].astype(np.float64).reshape(-1, 16)
    a, b, c, d, e, f, g, h, i = m[:, 0], m[:, 4], m[:, 8], m[:, 1], m[:, 5], m[:, 9], m[:, 2], m[:, 6], m[:, 10]
    c00, c01, c02 = e * i - f * h, -(d * i - f * g), d * h - e * g
    c10, c11, c12 = -(b * i - c * h), a * i - c * g, -(a * h - b * g)
    c20, c21, c22 = b * f - c * e, -(a * f - c * d), a * e - b * d
    det = (a * c00 + b * c01) + c * c02
    with np.errstate(all="ignore"):
        inv = np.where(det != 0.0, 1.0 / det, 0.0)
    out = np.zeros((len(m), 9), np.float64)
    out[:, 0], out[:, 3], out[:, 6] = c00 * inv, c01 * inv, c02 * inv
    out[:, 1], out[:, 4], out[:, 7] = c10 * inv, c11 * inv, c12 * inv
    out[:, 2], out[:, 5], out[:, 8] = c20 * inv, c21 * inv, c22 * inv
    return out.astype(F)


def world_record(m, p0, p1, p2):
    """bvh_math::world_record on (n, 16) transforms and (n, 3) corners: transform * vec4(pos, 1), columns left to right; e1 = w1 - w0, e2 = w2 - w0."""
    def point(p):
        return np.stack([((m[:, r] * p[:, 0] + m[:, 4 + r] * p[:, 1]) + m[:, 8 + r] * p[:, 2]) + m[:, 12 + r] for r in range(3)], 1)
    w0, w1, w2 = point(p0), point(p1), point(p2)
    assert w0.dtype == F
    return w0, w1 - w0, w2 - w0


def _addressable(scene, hits):
    """The hits the contract resolves (every check that comes before a gather)."""
    g, t, u, v = hits["geometry_index"].astype(np.int64), hits["primitive_index"].astype(np.int64), hits["u"], hits["v"]
    n_prims = len(scene.primitives)
    ok = (g != MISS) & (t != MISS) & (g < n_prims) & np.isfinite(u) & np.isfinite(v)
    tris = np.zeros(len(hits), np.int64)
    tris[ok] = scene.primitives["index_count"][g[ok]].astype(np.int64) // 3
    return ok & (t < tris)


def _corners(scene, g, t):
    pr = scene.primitives[g]
    base = pr["index_offset"].astype(np.int64) + 3 * t
    vo = pr["vertex_offset"].astype(np.int64)
    idx = np.asarray(scene.indices, np.uint32)
    return pr, [scene.vertices[vo + idx[base + k]] for k in range(3)]


def _interp(a, b, c, bx, by, bz):
    """a * bx + b * by + c * bz, the products summed left to right (trace_device.hpp: interpolate); (n, k) attributes, (n,) weights."""
    return (a * bx[:, None] + b * by[:, None]) + c * bz[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize3(a):
    """device_math.hpp: a * (1 / sqrtf(a . a))"""
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(_dot(a, a))
        return a * inv[:, None]


def _world_normal(M, N):
    """surface_world_normal: normalize(M N), or (0, False) where the squared length is not a positive finite number."""
    with np.errstate(all="ignore"):
        x = (M[:, 0] * N[:, 0] + M[:, 3] * N[:, 1]) + M[:, 6] * N[:, 2]
        y = (M[:, 1] * N[:, 0] + M[:, 4] * N[:, 1]) + M[:, 7] * N[:, 2]
        z = (M[:, 2] * N[:, 0] + M[:, 5] * N[:, 1]) + M[:, 8] * N[:, 2]
        d = (x * x + y * y) + z * z
        ok = (d > 0) & (d < np.inf)
        inv = F(1.0) / np.sqrt(np.where(ok, d, F(1.0)))
        out = np.stack([x * inv, y * inv, z * inv], 1)
    out[~ok] = 0
    assert out.dtype == F
    return out, ok


# ---- the texture fetch (trace_device.hpp: wrap_coord, fetch_texel, sample_texture) ----
def _to_int(x):
    """float -> int as the device converts: saturating, NaN -> 0"""
    return np.where(np.isnan(x), 0, np.clip(x.astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def _fetch(tex, x, y):
    p = np.asarray(tex["rgba8"], np.uint8)[y, x]
    out = np.zeros((len(x), 4), F)
    if tex["format"] == abi.FORMAT_R8G8B8A8_SRGB:
        out[:, :3] = SRGB_LUT[p[:, :3]]
    else:
        out[:, :3] = p[:, :3].astype(F) * F(1.0 / 255.0)
    out[:, 3] = p[:, 3].astype(F) * F(1.0 / 255.0)
    return out


def sample_texture(scene, idx, u, v):
    """sample_texture per hit: idx int (n,), uv float32 (n,) -> (n, 4) float32; an index outside the textures reads (0, 0, 0, 0)."""
    out = np.zeros((len(idx), 4), F)
    for k in np.unique(idx):
        if k < 0 or k >= len(scene.textures):
            continue
        tex = scene.textures[int(k)]
        sel = np.nonzero(idx == k)[0]
        H, W = np.asarray(tex["rgba8"]).shape[:2]
        x, y = u[sel] * F(W), v[sel] * F(H)
        au, av = tex["address_u"], tex["address_v"]
        if tex["mag"] == abi.FILTER_NEAREST:
            out[sel] = _fetch(tex, _wrap(_to_int(np.floor(x)), W, au), _wrap(_to_int(np.floor(y)), H, av))
            continue
        x, y = x - F(0.5), y - F(0.5)
        fx0, fy0 = np.floor(x), np.floor(y)
        fx, fy = (x - fx0)[:, None], (y - fy0)[:, None]
        x0, x1 = _wrap(_to_int(fx0), W, au), _wrap(_to_int(fx0) + 1, W, au)
        y0, y1 = _wrap(_to_int(fy0), H, av), _wrap(_to_int(fy0) + 1, H, av)
        a, b, c, d = _fetch(tex, x0, y0), _fetch(tex, x1, y0), _fetch(tex, x0, y1), _fetch(tex, x1, y1)
        one = F(1.0)
        out[sel] = (a * (one - fx) + b * fx) * (one - fy) + (c * (one - fx) + d * fx) * fy
    assert out.dtype == F
    return out


# ---- the contract ----
def resolve(scene, hits, material=False, flips=None):
    """vhr_resolve_hits restated: abi.surface_point_dtype per hit.  flips: the primitives' facing-flip bytes (default: by the transforms)."""
    hits = np.asarray(hits)
    out = np.zeros(len(hits), abi.surface_point_dtype)
    sel = np.nonzero(_addressable(scene, hits))[0]
    if not len(sel):
        return out
    g, t = hits["geometry_index"][sel].astype(np.int64), hits["primitive_index"][sel].astype(np.int64)
    u, v = hits["u"][sel].astype(F), hits["v"][sel].astype(F)
    flips = flips_of(scene) if flips is None else np.asarray(flips, np.uint8)
    pr, (a, b, c) = _corners(scene, g, t)
    flags = np.full(len(sel), VALID, np.uint32)
    with np.errstate(all="ignore"):
        v0, e1, e2 = world_record(pr["transform"].astype(F), a["pos"], b["pos"], c["pos"])
        position = (v0 + u[:, None] * e1) + v[:, None] * e2
        n = _cross(e1, e2)
        n = np.where((flips[g] != 0)[:, None], -n, n)
        nn = _dot(n, n)
        fine = (nn > 0) & (nn < np.inf)
        gn = n / np.sqrt(np.where(fine, nn, F(1.0)))[:, None]
        gn[~fine] = 0
        flags[~fine] |= DEGENERATE
        bx, by, bz = F(1.0) - u - v, u, v
        uv0, uv1 = _interp(a["uv0"], b["uv0"], c["uv0"], bx, by, bz), _interp(a["uv1"], b["uv1"], c["uv1"], bx, by, bz)
        normal = _interp(a["normal"], b["normal"], c["normal"], bx, by, bz)
        M = normal_matrices(scene)[g]
        N = normal
        base_color, metallic, roughness = np.zeros((len(sel), 4), F), np.zeros(len(sel), F), np.zeros(len(sel), F)
        if material:
            mat = pr["material"]
            base_color = mat["base_color"].astype(F).copy()                                              # gbuf.frag:19-26
            tex = mat["base_color_texture"].astype(np.int64)
            k = tex != -1
            base_color[k] = sample_texture(scene, tex[k], uv0[k, 0], uv0[k, 1])
            alpha = base_color[:, 3]
            flags[((mat["alpha_mask"] == 1) & (alpha < mat["alpha_cutoff"])) | (alpha == 0)] |= DISCARDED      # :27-32
            k = mat["normal_map"] >= 0                                                                    # :35-41
            if k.any():
                tx = sample_texture(scene, mat["normal_map"][k].astype(np.int64), uv0[k, 0], uv0[k, 1])
                tsn = _normalize3(tx[:, :3] * F(2.0) - F(1.0))
                tg = _interp(a["tangent"][k], b["tangent"][k], c["tangent"][k], bx[k], by[k], bz[k])
                T, nk = tg[:, :3], normal[k]
                bitangent = _cross(tsn, T) * tg[:, 3:4]                                                   # sic
                tangent = _normalize3(T - nk * _dot(T, nk)[:, None])
                N = normal.copy()
                N[k] = (tangent * tsn[:, 0:1] + bitangent * tsn[:, 1:2]) + nk * tsn[:, 2:3]
                flags[k] |= NORMAL_MAPPED
            metallic, roughness = mat["metallic_factor"].astype(F).copy(), mat["roughness_factor"].astype(F).copy()   # :50-56
            tex = mat["metallic_roughness_texture"].astype(np.int64)
            k = tex != -1
            if k.any():
                mr = sample_texture(scene, tex[k], uv0[k, 0], uv0[k, 1])
                metallic[k] *= mr[:, 1]
                roughness[k] *= mr[:, 2]
        sn, ok = _world_normal(M, N)                                                                      # :43
        flags[~ok] |= NO_SHADING_NORMAL
    for arr in (position, gn, uv0, uv1, sn, base_color, metallic, roughness):
        assert arr.dtype == F
    o = out[sel]
    o["position"], o["flags"], o["geometric_normal"], o["shading_normal"], o["uv0"], o["uv1"] = position, flags, gn, sn, uv0, uv1
    o["base_color"], o["metallic"], o["roughness"] = base_color, metallic, roughness
    out[sel] = o
    return out


def records(scene, hits):
    """(resolved mask, v0, e1, e2 float32 (n, 3) each): the fp32 leaf records of the hits' triangles (zero where a hit is not resolved)."""
    hits = np.asarray(hits)
    ok = _addressable(scene, hits)
    sel = np.nonzero(ok)[0]
    rec = [np.zeros((len(hits), 3), F) for _ in range(3)]
    if len(sel):
        pr, (a, b, c) = _corners(scene, hits["geometry_index"][sel].astype(np.int64), hits["primitive_index"][sel].astype(np.int64))
        with np.errstate(all="ignore"):
            for dst, src in zip(rec, world_record(pr["transform"].astype(F), a["pos"], b["pos"], c["pos"])):
                dst[sel] = src
    return (ok, *rec)


def geometry64(scene, hits, flips=None):
    """The geometry part in binary64 on the fp32 record: (resolved mask, position (n, 3), unit geometric normal (n, 3), |e1 x e2| (n,))."""
    ok, v0, e1, e2 = records(scene, hits)
    v0, e1, e2 = v0.astype(np.float64), e1.astype(np.float64), e2.astype(np.float64)
    u, v = np.asarray(hits["u"], np.float64)[:, None], np.asarray(hits["v"], np.float64)[:, None]
    flips = flips_of(scene) if flips is None else np.asarray(flips, np.uint8)
    with np.errstate(all="ignore"):
        position = (v0 + u * e1) + v * e2
        n = np.cross(e1, e2)
        g = np.where(ok, hits["geometry_index"], 0).astype(np.int64)
        n = np.where((flips[g] != 0)[:, None], -n, n)
        length = np.linalg.norm(n, axis=1)
        unit = n / np.where(length > 0, length, 1.0)[:, None]
    return ok, position, unit, length


def position_bound(scene, hits):
    """Per component: what |position - the binary64 value of (v0 + u e1) + v e2| may be.  Four fp32 roundings -- u e1, the sum with
    v0, v e2, the last sum -- each at most 2^-24 of its own result: 2^-24 (|u e1| + |v0 + u e1| + |v e2| + |P|), times 1 + 2^-20 for the second-
    order terms, plus 2^-148 for results in the subnormal range, where a rounding is absolute (2^-150 each)."""
    ok, v0, e1, e2 = records(scene, hits)
    v0, e1, e2 = v0.astype(np.float64), e1.astype(np.float64), e2.astype(np.float64)
    u, v = np.asarray(hits["u"], np.float64)[:, None], np.asarray(hits["v"], np.float64)[:, None]
    with np.errstate(all="ignore"):
        s = np.abs(u * e1) + np.abs(v0 + u * e1) + np.abs(v * e2) + np.abs((v0 + u * e1) + v * e2)
    return 2.0 ** -24 * s * (1 + 2.0 ** -20) + 2.0 ** -148


def position_violations(scene, hits, points):
    """bool (n,): resolved hits whose fp32 position leaves the bound around the binary64 value."""
    ok, truth, _, _ = geometry64(scene, hits)
    err = np.abs(np.asarray(points["position"], np.float64) - truth)
    return ok & ~(err <= position_bound(scene, hits)).all(1)
