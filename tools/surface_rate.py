"""What resolving hits costs: 2^20 closest-hit results on sponza_proc through vhr_resolve_hits, in primary-ray order (neighbouring hits share
triangles) and shuffled, geometry only and with VHR_SURFACE_MATERIAL, timed in one run with HIP events, one JSON line per case with the library's
source fingerprint.  Beside each rate stands the time of the vhr_ray_query that produced the hits (the same rays in the same order) and the least
time the bytes moved would take at the HBM peak: 24 B read and 80 B written per hit, and -- counted once per hit, as if no cache held them -- the
gathered primitive (120 B, its normal matrix 36 B and flip byte), three indices (12 B) and three vertices without their tangents (3 x 40 B).
It fixes no target; the expectation to confirm or refute is that a resolve costs a small fraction of the query that found the hits.

  python tools/surface_rate.py [--side 1024] [--reps 20] [--scene sponza_proc] [--out profiles/surface_rate.jsonl]
"""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, scenes  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E, specification
STREAM_BYTES = 24 + 80
GATHER_BYTES = 120 + 36 + 1 + 12 + 3 * 40


def primary_rays(pfd, side):
    """The stand-in G-buffer's primary rays of a side x side image, pixel order: from the camera through the pixel centre's point on the near plane."""
    ys, xs = np.divmod(np.arange(side * side), side)
    m = np.asarray(pfd["camera_viewproj_inverse"], np.float64).reshape(4, 4).T
    ndc = np.stack([(xs + 0.5) / side * 2 - 1, (ys + 0.5) / side * 2 - 1, np.ones(side * side), np.ones(side * side)])
    r = m @ ndc
    cam = np.asarray(pfd["camera_view_inverse"], np.float64).reshape(4, 4).T[:3, 3]
    rays = np.zeros((side * side, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = cam, 1.0, (r[:3] / r[3]).T - cam, 3.0e38
    return rays


def event_times(torch, stream, body, reps, warmup=3):
    """Milliseconds of each of `reps` calls of body() between HIP events on `stream`, after `warmup` untimed calls."""
    for _ in range(warmup):
        body()
    torch.cuda.synchronize()
    start = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    stop = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    with torch.cuda.stream(stream):
        for i in range(reps):
            start[i].record(stream)
            body()
            stop[i].record(stream)
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in zip(start, stop)])


def spread(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="sponza_proc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_rate.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("surface_rate: no GPU (this measurement has no CPU fallback)")
    rec = Records(args.out, date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint())
    scene = getattr(scenes, args.scene)()
    count = args.side * args.side
    ordered = primary_rays(camera.dolly_frames(scene, args.side, args.side, 2)[1], args.side)
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        stream = torch.cuda.current_stream()
        for order, rays in (("primary", ordered), ("shuffled", ordered[np.random.default_rng(11).permutation(count)])):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
            d_hits = torch.zeros((count, 6), dtype=torch.int32, device="cuda")
            d_out = torch.zeros((count, 20), dtype=torch.int32, device="cuda")
            query = event_times(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count, d_hits.data_ptr()), args.reps)
            hits = int((d_hits[:, 3] != -1).sum().item())
            for material in (False, True):
                ms = event_times(torch, stream, lambda: ctx.resolve_hits_device(d_hits.data_ptr(), count, d_out.data_ptr(), material=material), args.reps)
                stats = ctx.surface_statistics()
                assert stats[0] == count and stats[1] == hits and stats[3] == int(material), stats
                med = float(np.median(ms))
                rec.emit(dict(what="resolve_hits", scene=args.scene, order=order, material=material, hits=count, resolved=hits, discarded=stats[2],
                              triangles=scene.triangle_count, reps=args.reps, mhits_s=count / med / 1e3, **spread(ms),
                              query_ms_median=float(np.median(query)), query_ms_min=float(query.min()), query_ms_max=float(query.max()),
                              resolve_over_query=med / float(np.median(query)),
                              hbm_bound_ms_stream=count * STREAM_BYTES / HBM_PEAK_BYTES_PER_S * 1e3,
                              hbm_bound_ms_with_gathers=(count * STREAM_BYTES + hits * GATHER_BYTES) / HBM_PEAK_BYTES_PER_S * 1e3))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
