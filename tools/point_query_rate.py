"""What closest-point queries cost: 2^20 queries of vhr_closest_point_query on sponza_proc and bistro_proc -- points sampled on the surfaces
(uniformly over the triangles' area) and lifted 1 cm along the normal, and points uniform in the scene's bounds; nearest surface and
VHR_POINT_QUERY_ANY_WITHIN; max_distance +inf and 1 m -- one JSON line per case with the library's source fingerprint: queries per second,
point / triangle evaluations per query (vhr_get_point_query_statistics) and the share of the queries that found something.  The yardstick is
vhr_ray_query's closest hit at the same count of random rays on the same scene, in the same process.  The points come in the order they were
drawn: neighbouring lanes of a wave are nowhere near each other in the scene.  It fixes no target.

  python tools/point_query_rate.py [--count 1048576] [--reps 10] [--scenes sponza_proc,bistro_proc] [--out profiles/point_query_rate.jsonl]
"""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, timed  # noqa: E402
from vulkanhybridrenderer_amd import lib, ray_queries, scenes  # noqa: E402


def surface_points(rng, tris, n, lift):
    """n points uniform over the triangles' area, `lift` along the triangle's normal"""
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    nrm = np.cross(e1, e2)
    area = np.linalg.norm(nrm, axis=1)
    keep = area > 0
    k = rng.choice(np.nonzero(keep)[0], n, p=area[keep] / area[keep].sum())
    u, v = rng.random((n, 1)), rng.random((n, 1))
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    return tris[k, 0] + u * e1[k] + v * e2[k] + lift * nrm[k] / area[k, None]


def measure(name, args, rec):
    import torch
    scene = getattr(scenes, name)()
    count = args.count
    rng = np.random.default_rng(23)
    tris = ray_queries.world_triangles(scene)
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    sets = dict(surface_1cm=surface_points(rng, tris, count, 0.01), uniform_in_bounds=rng.uniform(lo, hi, (count, 3)))
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        stream = torch.cuda.current_stream()
        common = dict(scene=name, triangles=scene.triangle_count, count=count, reps=args.reps)
        # the yardstick: closest-hit ray queries
        rays = ray_queries.random_rays(np.random.default_rng(11), count, lo, hi, margin=0.1, tmins=(0.0,), tmaxs=(np.inf,))
        d_rays = torch.from_numpy(rays).cuda()
        hits = torch.zeros((count, 6), dtype=torch.int32, device="cuda")
        ms = timed(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count, hits.data_ptr()), args.reps, 3)
        rec.emit(dict(common, what="ray_query_closest_hit", ms=ms, mqueries_s=count / ms / 1e3))
        for set_name, points in sets.items():
            for max_distance in (float("inf"), 1.0):
                q = np.empty((count, 4), np.float32)
                q[:, 0:3], q[:, 3] = points, max_distance
                d_q = torch.from_numpy(q).cuda()
                for any_within in (False, True):
                    out = torch.zeros(count if any_within else (count, 6), dtype=torch.uint8 if any_within else torch.int32, device="cuda")
                    ms = timed(torch, stream, lambda: ctx.closest_point_query_device(d_q.data_ptr(), count, out.data_ptr(), any_within=any_within), args.reps, 3)
                    s = ctx.point_query_statistics()
                    assert s[0] == count and s[3] == 0, s
                    rec.emit(dict(common, what="closest_point_query", points=set_name, max_distance="inf" if np.isinf(max_distance) else max_distance, any_within=any_within, ms=ms,
                                  mqueries_s=count / ms / 1e3, evaluations_per_query=s[2] / count, found_share=s[1] / count))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_query_rate.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("point_query_rate: no GPU (this measurement has no CPU fallback)")
    rec = Records(args.out, date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint())
    for name in args.scenes.split(","):
        measure(name, args, rec)


if __name__ == "__main__":
    main()
