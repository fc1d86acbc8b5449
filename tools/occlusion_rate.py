"""What the fused occlusion query costs beside its parts: 2^18 surface points on sponza_proc and bistro_proc -- the closest hits of a 512 x 512
image's primary rays through vhr_resolve_hits, origin = position + 0.1 x geometric normal, tmin 0.01, tmax 5 (vhr_default_trace_params' normal_bias,
tmin and ao_tmax) -- in primary-ray order and shuffled, samples = 1, 4, 16, 64.  The yardstick, in the same process: vhr_ray_query with
VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT on the very same rays, which vhr_debug_occlusion_rays materialises; only the query is timed, neither the
materialising nor the reduction of its bytes is charged to it.  HIP events, the mean of 10 calls, each case three times; one JSON line per case
with both sets of times and their ratio, and the library's source fingerprint.  The masks are checked against the yardstick's bytes on the way.
It fixes no ratio; the expectation to confirm or refute is that the fused call is no slower at any `samples`.

  python tools/occlusion_rate.py [--side 512] [--reps 10] [--library other/libvhr_amd.so] [--out profiles/occlusion_rate.jsonl]
"""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, timed  # noqa: E402
from surface_rate import primary_rays  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, ray_queries, scenes  # noqa: E402

SEED = 2026


def surface_points(ctx, torch, rays):
    """The query points of the closest hits of `rays`, in their order, and how many of them lie on a surface."""
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_hits = torch.zeros((n, 6), dtype=torch.int32, device="cuda")
    d_sp = torch.zeros((n, 20), dtype=torch.int32, device="cuda")
    ctx.ray_query_device(d_rays.data_ptr(), n, d_hits.data_ptr())
    ctx.resolve_hits_device(d_hits.data_ptr(), n, d_sp.data_ptr())
    sp = d_sp.cpu().numpy().view(abi.surface_point_dtype).reshape(-1)
    tp = abi.default_trace_params()
    return ray_queries.occlusion_points(sp, float(tp["normal_bias"]), float(tp["tmin"]), float(tp["ao_tmax"])), int(((sp["flags"] & abi.SURFACE_VALID) != 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--scenes", nargs="*", default=["sponza_proc", "bistro_proc"])
    ap.add_argument("--library", default=None, help="measure another build of the library (a scratch build, say)")
    ap.add_argument("--label", default="", help="a word about that build for the records")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_rate.jsonl"))
    args = ap.parse_args()
    if args.library:
        lib.LIB_PATH = os.path.abspath(args.library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("occlusion_rate: no GPU (this measurement has no CPU fallback)")
    rec = Records(args.out, date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint(), build=args.label)
    count = args.side * args.side
    for name in args.scenes:
        scene = getattr(scenes, name)()
        ctx = lib.Context(64, 64)
        try:
            ctx.upload_scene(scene)
            stream = torch.cuda.current_stream()
            ordered, on_surface = surface_points(ctx, torch, primary_rays(camera.dolly_frames(scene, args.side, args.side, 2)[1], args.side))
            for order, pts in (("primary", ordered), ("shuffled", ordered[np.random.default_rng(11).permutation(count)])):
                d_pts = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
                d_masks = torch.zeros(count, dtype=torch.int64, device="cuda")
                for samples in args.samples:
                    rays = ctx.debug_occlusion_rays(pts, samples, SEED)
                    d_rays = torch.from_numpy(rays.reshape(-1, 8)).cuda()
                    del rays
                    d_occ = torch.zeros(count * samples, dtype=torch.uint8, device="cuda")
                    fused = [timed(torch, stream, lambda: ctx.occlusion_query_device(d_pts.data_ptr(), count, samples, d_masks.data_ptr(), SEED), args.reps, 3)
                             for _ in range(args.repeats)]
                    stats = ctx.occlusion_statistics()
                    query = [timed(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count * samples, d_occ.data_ptr(), any_hit=True), args.reps, 3)
                             for _ in range(args.repeats)]
                    qstats = ctx.ray_query_statistics()
                    weights = torch.tensor([1 << j if j < 63 else -(1 << 63) for j in range(samples)], dtype=torch.int64, device="cuda")
                    want = (d_occ.reshape(count, samples).to(torch.int64) * weights).sum(dim=1)
                    assert torch.equal(want, d_masks), f"{name} {order} samples {samples}: the masks are not the ray query's bits"
                    assert stats[0] == count and stats[1] == qstats[1] and stats[3] == 0, (stats, qstats)
                    f, q = float(np.mean(fused)), float(np.mean(query))
                    rec.emit(dict(what="occlusion_query", scene=name, order=order, samples=samples, points=count, on_surface=on_surface,
                                  rays=count * samples, occluded=stats[1], points_redone=stats[2], rays_redone_by_ray_query=qstats[2],
                                  triangles=scene.triangle_count, reps=args.reps, fused_ms=fused, ray_query_ms=query, fused_ms_mean=f, ray_query_ms_mean=q,
                                  fused_over_ray_query=f / q, fused_mrays_s=count * samples / f / 1e3, ray_query_mrays_s=count * samples / q / 1e3))
                    del d_rays, d_occ
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
