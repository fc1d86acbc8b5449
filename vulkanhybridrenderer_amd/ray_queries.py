"""Ray batches for vhr_ray_query (Context.ray_query / ray_query_device): the rays the reference's RayqueryRenderPath traces, random
rays, and the world-space triangles of a scene to aim rays at.  Rays are (n, 8) float32 rows: origin, tmin, direction, tmax
(abi.ray_dtype)."""
import numpy as np

from . import abi

# rayquery_render_path/default.frag:36-45: rayQueryInitializeEXT(rq, TLAS, gl_RayFlagsTerminateOnFirstHitEXT, 0xFF, in_pos, 0.1, light_dir, 10000.0)
RAYQUERY_SHADOW_TMIN = 0.1
RAYQUERY_SHADOW_TMAX = 10000.0


def world_positions(pfd, depth, xs, ys):
    """The world-space position of pixels (xs, ys) of a depth image (glsl_common.h:118-122, get_world_space_position), float32."""
    H, W = depth.shape
    m = np.asarray(pfd["camera_viewproj_inverse"], np.float64).reshape(4, 4).T
    d = np.asarray(depth, np.float32)[ys, xs].astype(np.float64)
    ndc = np.stack([(xs + 0.5) / W * 2.0 - 1.0, (ys + 0.5) / H * 2.0 - 1.0, d, np.ones_like(d)], axis=0)
    r = m @ ndc
    return (r[:3] / r[3]).T.astype(np.float32)


def rayquery_shadow_rays(pfd, depth, xs=None, ys=None):
    """The rayquery path's shadow rays (default.frag:36-45) from the covered pixels among (xs, ys) -- every pixel if None -- in
    pixel order: origin in_pos (the fragment's world position, here from the stand-in G-buffer's depth), tmin 0.1, direction
    -light.direction, tmax 10000.  Returns (rays (n, 8) float32, flat pixel indices (n,))."""
    H, W = depth.shape
    if xs is None:
        ys, xs = np.divmod(np.arange(W * H), W)
    xs, ys = np.asarray(xs).reshape(-1), np.asarray(ys).reshape(-1)
    covered = np.asarray(depth)[ys, xs] != 0.0
    xs, ys = xs[covered], ys[covered]
    rays = np.empty((len(xs), 8), np.float32)
    rays[:, 0:3] = world_positions(pfd, depth, xs, ys)
    rays[:, 3] = RAYQUERY_SHADOW_TMIN
    rays[:, 4:7] = -np.asarray(pfd["directional_light"]["direction"][:3], np.float32)
    rays[:, 7] = RAYQUERY_SHADOW_TMAX
    return rays, ys * W + xs


def scene_bounds(scene):
    """(lo, hi) of the scene's world-space vertices."""
    tris = world_triangles(scene)
    return tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)


def world_triangles(scene):
    """(n, 3, 3) float64: every triangle in world space, in flat (primitive-major) order."""
    out = []
    for p in scene.primitives:
        T = abi.glm_to_mat(p["transform"])
        io, ic, vo = int(p["index_offset"]), int(p["index_count"]), int(p["vertex_offset"])
        pos = scene.vertices["pos"][scene.indices[io:io + ic].astype(np.int64) + vo].astype(np.float64)
        out.append((pos @ T[:3, :3].T + T[:3, 3]).reshape(-1, 3, 3))
    return np.concatenate(out)


def random_rays(rng, n, lo, hi, margin=0.25, tmins=(0.0,), tmaxs=(np.inf,)):
    """n rays with origins uniform in the box [lo, hi] grown by `margin` of its extent on every side, isotropic directions, tmin and
    tmax drawn from the given choices."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(lo - margin * ext, hi + margin * ext, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3] = rng.choice(np.asarray(tmins, np.float32), n)
    rays[:, 7] = rng.choice(np.asarray(tmaxs, np.float32), n)
    return rays


def occlusion_points(surface_points, bias=0.1, tmin=0.01, tmax=5.0):
    """Query points for Context.occlusion_query from abi.surface_point_dtype records (Context.resolve_hits): origin = position + bias *
    geometric normal (fp32, the product rounded before the sum), axis = the geometric normal, [tmin, tmax] for every ray of the point.  The
    defaults are abi.default_trace_params()' normal_bias, tmin and ao_tmax.  Records that were not resolved (flags == 0) give points whose rays
    can hit nothing (tmax = -1).  Returns (n, 8) float32."""
    sp = np.asarray(surface_points)
    n = np.asarray(sp["geometric_normal"], np.float32)
    pts = np.empty((len(sp), 8), np.float32)
    pts[:, 0:3] = np.asarray(sp["position"], np.float32) + np.float32(bias) * n
    pts[:, 3] = tmin
    pts[:, 4:7] = n
    pts[:, 7] = np.where(sp["flags"] & abi.SURFACE_VALID, np.float32(tmax), np.float32(-1.0))
    return pts
