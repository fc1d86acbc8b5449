"""vhr_rebuild_geometry against vhr_update_geometry and vhr_refit_geometry on sponza_proc and bistro_proc at full size (one GPU process), one
JSON line per measurement, the library's source fingerprint in each.

Per scene, after one build, one refit and one rebuild that are not timed (the first calls load code objects and make the refit's plan):
  "rebuild": median over --reps of the host wall time of vhr_rebuild_geometry after a vhr_update_vertices of every vertex (perf_counter around
             the call; vhr_get_build_times beside it), against two baselines in the same process: vhr_update_geometry with the same arrays
             (wall time of the call, which validates on the host and uploads again) and vhr_refit_geometry after the same update, in its
             steady state; the first refit of a new tree, which also makes the refit's plan, is timed apart.  A second series with
             "object_motion_vectors" 1 adds the gather and the scatter of the previous records.
  "trees":   after a large displacement (every vertex above 1 m pushed along x by a wave of 1 m; a third of the primitives rotated by 30
             degrees about y), vhr_get_bvh_sah_cost and the any-hit launch of a hybrid frame at 1080p (kernel kind "raygen", bench.py's
             workload) on three trees over the same arrays: refitted, rebuilt in place, and a fresh vhr_update_geometry.  The rebuilt and the
             fresh tree are the same arrays bit for bit (tests/test_gpu_rebuild.py), so their two figures show the spread between launches.

Measured on an MI355X (profiles/rebuild_rate.jsonl; medians of 12; two earlier runs on other machines in brackets):
  sponza_proc (257 536 triangles): rebuild 11.3 ms [9.7, 10.0] (11.7 with "object_motion_vectors" 1) = 0.96 x vhr_update_geometry (11.7 ms)
    [0.92, 0.93] = 36 x the steady-state refit (0.32 ms) [33, 33]; the new tree's first refit 1.26 ms.  Displaced: SAH cost 94.6 refitted /
    43.9 rebuilt / 43.9 fresh, any-hit launch 1.321 / 0.418 / 0.419 ms.
  bistro_proc (2 910 880 triangles): rebuild 24.6 ms [23.0, 23.6] (25.5) = 0.80 x vhr_update_geometry (30.9 ms) [0.79, 0.77] = 22 x the refit
    (1.14 ms) [21, 20]; the new tree's first refit 12.9 ms.  Displaced: SAH cost 479.6 / 31.9 / 31.9, any-hit launch 6.307 / 0.318 / 0.317 ms.

  python tools/rebuild_rate.py [--reps 12] [--frames 20] [--out profiles/rebuild_rate.jsonl] [--scenes sponza_proc,bistro_proc]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records  # noqa: E402
from refit_rate import Frames, median, rotated_third, wave  # noqa: E402
from vulkanhybridrenderer_amd import lib, scenes  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def measure(name, scene, args, emit):
    W, H = 1920, 1080
    ctx = lib.Context(W, H)
    base = dict(scene=name, triangles=scene.triangle_count, fingerprint=lib.source_fingerprint())
    try:
        ctx.upload_scene(scene)                      # first calls: code objects, the refit's plan, the rebuild's passes
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
        ctx.update_vertices(scene.vertices)
        ctx.rebuild_geometry()
        st = ctx.bvh_statistics()
        base.update(nodes=int(st["nodes"]), depth=int(st["max_depth"]))
        for motion in (0, 1):
            ctx.set_option("object_motion_vectors", motion)
            rebuild, build0, transfer, first_refit, refit, update = [], [], [], [], [], []
            for _ in range(args.reps):
                ctx.update_vertices(scene.vertices)
                rebuild.append(timed(ctx.rebuild_geometry))
                b = ctx.build_times_ms()
                build0.append(b[0])
                transfer.append(b[1])
                ctx.update_vertices(scene.vertices)
                first_refit.append(timed(ctx.refit_geometry))      # the first refit of a new tree also makes the refit's plan
            for _ in range(args.reps):                              # ... the ones after it do not
                ctx.update_vertices(scene.vertices)
                refit.append(timed(ctx.refit_geometry))
            for _ in range(args.reps):
                update.append(timed(lambda: ctx.update_geometry(scene.vertices, scene.indices, scene.primitives)))
            ctx.update_vertices(scene.vertices)
            ctx.rebuild_geometry()
            rs = ctx.rebuild_statistics()
            emit(dict(base, what="rebuild", reps=args.reps, object_motion_vectors=motion, rebuild_wall_ms_median=median(rebuild), rebuild_wall_ms_min=float(min(rebuild)),
                      rebuild_wall_ms_max=float(max(rebuild)), build_times0_ms_median=median(build0), build_times1_ms_median=median(transfer),
                      update_geometry_wall_ms_median=median(update), refit_wall_ms_median=median(refit), first_refit_after_rebuild_wall_ms_median=median(first_refit),
                      rebuild_over_update_geometry=median(rebuild) / median(update), rebuild_over_refit=median(rebuild) / median(refit),
                      fetched_for_the_host_builder=rs[1], builder_used=ctx.bvh_builder_used()))
        ctx.set_option("object_motion_vectors", 0)
        # ---- three trees over the same displaced arrays
        frames = Frames(ctx, scene, W, H, args.frames)
        v = wave(scene, 1.0)
        t = rotated_third(scene, 30.0)
        prims = scene.primitives.copy()
        prims["transform"] = t.reshape(prims["transform"].shape)
        ctx.update_geometry(scene.vertices, scene.indices, scene.primitives)       # the tree of the scene at rest
        ctx.update_vertices(v)
        ctx.update_primitive_transforms(t)
        ctx.refit_geometry()
        out = dict(base, what="trees", displacement="wave 1 m + a third of the primitives rotated by 30 degrees", frames=args.frames)
        out["sah_cost_at_rest"], out["sah_cost_refitted"] = ctx.bvh_sah_cost()
        out["any_hit_ms_refitted"] = frames.run()[1]
        ctx.rebuild_geometry()
        out["sah_cost_rebuilt"] = ctx.bvh_sah_cost()[1]
        out["any_hit_ms_rebuilt"] = frames.run()[1]
        rebuilt_fingerprint = ctx.bvh_fingerprint()
        ctx.update_geometry(v, scene.indices, prims)
        out["sah_cost_fresh"] = ctx.bvh_sah_cost()[1]
        out["any_hit_ms_fresh"] = frames.run()[1]
        out["rebuilt_equals_fresh"] = bool(rebuilt_fingerprint == ctx.bvh_fingerprint())
        out["any_hit_refitted_over_rebuilt"] = out["any_hit_ms_refitted"] / out["any_hit_ms_rebuilt"]
        out["any_hit_rebuilt_over_fresh"] = out["any_hit_ms_rebuilt"] / out["any_hit_ms_fresh"]
        emit(out)
        frames.path.destroy()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rebuild_rate: no GPU (this measurement has no CPU fallback)")
    emit = Records(args.out).emit
    for name in args.scenes.split(","):
        scene = scenes.bistro_proc(texture_size=64) if name == "bistro_proc" else getattr(scenes, name)()      # (full-size geometry; small texels: nothing timed here samples them)
        measure(name, scene, args, emit)


if __name__ == "__main__":
    main()
