"""vhr_refit_geometry_partial(VHR_REFIT_FORCE_PARTIAL) against vhr_refit_geometry on sponza_proc and bistro_proc at full size, one JSON line
per measurement, the library's source fingerprint in each.  Meant to run as one GPU process per scene, each under its own time limit, the second
appending to the first's file:
  timeout -k 10 300 python tools/partial_refit_rate.py --scenes sponza_proc --out profiles/partial_refit_rate.jsonl
  timeout -k 10 500 python tools/partial_refit_rate.py --scenes bistro_proc --out profiles/partial_refit_rate.jsonl --append
(several --scenes in one call run in one process).

Per scene and dirty share (about 0.1 %, 1 %, 10 % and 50 % of the vertices, and 20 %, 30 % and 40 % to bracket the crossover): a contiguous vertex range that starts where a primitive's block
starts in the middle of the scene and covers the primitives behind it (the last one possibly in part) is displaced, back and forth, by
vhr_update_vertices of that range only.  In the same process and from the same arrays, medians over --reps after one untimed call each:
  "partial": host wall time of vhr_refit_geometry_partial(FORCE_PARTIAL) (perf_counter around the call); in a second series, with timing bit
             12 set, the device time of the mark + leaf pass, the upward pass and forms + checks; the dirty counts.
  "whole":   the same for vhr_refit_geometry after the same update.
  ratio = partial wall / whole wall; remainder = wall - the three stage times: the two host round trips and the launch overhead.
The yardstick is the whole-tree refit measured beside it, never an absolute time.

  python tools/partial_refit_rate.py [--reps 12] [--out profiles/partial_refit_rate.jsonl] [--append] [--scenes sponza_proc,bistro_proc]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records  # noqa: E402
from vulkanhybridrenderer_amd import lib, scenes  # noqa: E402

SHARES = (0.001, 0.01, 0.1, 0.2, 0.3, 0.4, 0.5)


def median(x):
    return float(np.median(np.asarray(x, np.float64)))


def dirty_range(scene, share):
    """[first, end) of about share x the vertices, starting at the block of the primitive where the middle of the vertex buffer lies (moved down
    if the range would not fit behind it); and the primitives whose blocks it touches."""
    n = len(scene.vertices)
    count = max(3, int(round(share * n)))
    starts = np.sort(np.unique(scene.primitives["vertex_offset"].astype(np.int64)))
    first = int(starts[np.searchsorted(starts, min(n // 2, n - count), side="right") - 1])
    first = min(first, n - count)
    end = first + count
    touched = int(np.count_nonzero((starts < end) & (np.append(starts[1:], n) > first)))
    return first, end, touched


def series(ctx, refit, blocks, first, reps):
    """wall times (ms) of refit() after update_vertices of the alternating blocks; one untimed call first; then the stage times in a second series."""
    wall, split = [], []
    for timing in (False, True):
        ctx.set_kernel_timing(False, refit=timing)
        for i in range(reps + 1):
            ctx.update_vertices(blocks[i & 1], first_vertex=first)
            t0 = time.perf_counter()
            refit()
            dt = (time.perf_counter() - t0) * 1e3
            if i == 0:
                continue
            if timing:
                split.append(ctx.refit_times_ms()[1:])
            else:
                wall.append(dt)
    ctx.set_kernel_timing(False)
    leaf, up, forms = (median([s[k] for s in split]) for k in range(3))
    w = median(wall)
    return dict(wall_ms_median=w, wall_ms_min=float(min(wall)), wall_ms_max=float(max(wall)), leaf_pass_ms=leaf, upward_pass_ms=up, forms_and_checks_ms=forms,
                remainder_ms=w - (leaf + up + forms))


def measure(name, scene, args, emit):
    ctx = lib.Context(64, 64)
    base = dict(scene=name, triangles=scene.triangle_count, vertices=len(scene.vertices), fingerprint=lib.source_fingerprint(), reps=args.reps)
    try:
        ctx.upload_scene(scene)                      # first calls: code objects, the refit's plan and the per-node boxes
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
        st = ctx.bvh_statistics()
        base.update(nodes=int(st["nodes"]), depth=int(st["max_depth"]))
        for share in SHARES:
            first, end, touched = dirty_range(scene, share)
            moved = scene.vertices[first:end].copy()
            moved["pos"][:, 1] += np.float32(0.05)
            blocks = (moved, scene.vertices[first:end])
            rec = dict(base, share_asked=share, share=(end - first) / len(scene.vertices), first_vertex=first, vertex_count=end - first, primitives_touched=touched)
            partial = series(ctx, lambda: ctx.refit_geometry_partial(force=True), blocks, first, args.reps)
            ps, rs = ctx.partial_refit_statistics(), ctx.refit_statistics()
            assert ps["ran_as"] == 0, ps
            emit(dict(rec, what="partial", **partial, dirty_records=ps["dirty_records"], dirty_nodes=ps["dirty_nodes"], forms_rewritten=ps["forms_rewritten"],
                      centre_moved=ps["centre_moved"], upward_launches=rs["upward_launches"], records_outside=rs["records_outside"],
                      children_outside=rs["children_outside"]))
            whole = series(ctx, ctx.refit_geometry, blocks, first, args.reps)
            emit(dict(rec, what="whole", **whole, upward_launches=ctx.refit_statistics()["upward_launches"]))
            emit(dict(rec, what="ratio", partial_over_whole=partial["wall_ms_median"] / whole["wall_ms_median"], partial_wins=bool(partial["wall_ms_median"] < whole["wall_ms_median"]),
                      partial_remainder_share=partial["remainder_ms"] / partial["wall_ms_median"]))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the records --out already holds (one process per scene)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("partial_refit_rate: no GPU (this measurement has no CPU fallback)")
    kept = open(args.out).read() if args.append and args.out and os.path.exists(args.out) else ""
    records = Records(args.out)
    if kept and records.out:
        records.out.write(kept)
    for name in args.scenes.split(","):
        scene = scenes.bistro_proc(texture_size=64) if name == "bistro_proc" else getattr(scenes, name)()      # (full-size geometry; small texels: nothing timed here samples them)
        measure(name, scene, args, records.emit)


if __name__ == "__main__":
    main()
