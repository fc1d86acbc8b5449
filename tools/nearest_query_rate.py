"""What k-nearest queries cost: 2^20 queries of vhr_nearest_points_query on sponza_proc and bistro_proc -- the point sets of
tools/point_query_rate.py (points on the surfaces lifted 1 cm along the normal, and points uniform in the scene's bounds, in the order they were
drawn); max_distance +inf and 1 m; k = 1, 4 and 16 -- one JSON line per case with the library's source fingerprint: queries per second, point /
triangle evaluations per query and entries per query (vhr_get_nearest_query_statistics).  The yardsticks run on the same sets in the same
process: vhr_closest_point_query (nearest surface) per set and max_distance, and vhr_ray_query's closest hit at the same count of random rays.
Every case is timed `--rounds` times (the mean of `--reps` each time), so a record carries the spread a ratio has to be read against.  It fixes
no target.

  python tools/nearest_query_rate.py [--count 1048576] [--reps 10] [--rounds 3] [--scenes sponza_proc,bistro_proc] [--out profiles/nearest_query_rate.jsonl]
"""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from point_query_rate import surface_points  # noqa: E402
from rate_common import Records, timed  # noqa: E402
from vulkanhybridrenderer_amd import abi, lib, ray_queries, scenes  # noqa: E402


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

        def rounds(body):
            ms = [timed(torch, stream, body, args.reps, 3) for _ in range(args.rounds)]
            return dict(ms=float(np.mean(ms)), ms_rounds=ms, mqueries_s=count / float(np.mean(ms)) / 1e3)

        # the yardsticks: closest-hit ray queries, and below the closest-point query on each set
        rays = ray_queries.random_rays(np.random.default_rng(11), count, lo, hi, margin=0.1, tmins=(0.0,), tmaxs=(np.inf,))
        d_rays = torch.from_numpy(rays).cuda()
        hits = torch.zeros((count, 6), dtype=torch.int32, device="cuda")
        rec.emit(dict(common, what="ray_query_closest_hit", **rounds(lambda: ctx.ray_query_device(d_rays.data_ptr(), count, hits.data_ptr()))))
        out = torch.zeros((count, abi.NEAREST_MAX_K, 6), dtype=torch.int32, device="cuda")
        for set_name, points in sets.items():
            for max_distance in (float("inf"), 1.0):
                q = np.empty((count, 4), np.float32)
                q[:, 0:3], q[:, 3] = points, max_distance
                d_q = torch.from_numpy(q).cuda()
                case = dict(common, points=set_name, max_distance="inf" if np.isinf(max_distance) else max_distance)
                t = rounds(lambda: ctx.closest_point_query_device(d_q.data_ptr(), count, out.data_ptr()))
                s = ctx.point_query_statistics()
                assert s[0] == count and s[3] == 0, s
                rec.emit(dict(case, what="closest_point_query", evaluations_per_query=s[2] / count, entries_per_query=s[1] / count, **t))
                for k in (1, 4, 16):
                    t = rounds(lambda: ctx.nearest_points_query_device(d_q.data_ptr(), count, k, out.data_ptr()))
                    s = ctx.nearest_query_statistics()
                    assert s[0] == count and s[3] == 0, s
                    rec.emit(dict(case, what="nearest_points_query", k=k, evaluations_per_query=s[2] / count, entries_per_query=s[1] / count, **t))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_query_rate.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nearest_query_rate: no GPU (this measurement has no CPU fallback)")
    rec = Records(args.out, date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint())
    for name in args.scenes.split(","):
        measure(name, args, rec)


if __name__ == "__main__":
    main()
