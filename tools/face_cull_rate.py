"""What ray face culling costs: 2^20 random ray queries on sponza_proc and bistro_proc, closest hit and terminate-on-first-hit, through
vhr_ray_query_faces with face_cull NONE / BACK / FRONT against vhr_ray_query_masked on the plain kernels, timed in one run, one JSON line
per case with the library's source fingerprint.  It fixes no target.

With a cull mode the answers differ from the plain ones (a culled ray walks on to the next surface, or to the end of the tree), so a ratio
compares two workloads, not two codes on one; face_cull NONE in closest-hit mode is the same workload on the face instantiation (it reports
the hit kind), and in any-hit mode it IS the plain launch.  The plain series is measured three times; its min..max is the spread a ratio has to
leave to mean anything.

  python tools/face_cull_rate.py [--rays 1048576] [--reps 10] [--scenes sponza_proc,bistro_proc] [--out profiles/face_cull_rate.jsonl]
"""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, timed  # noqa: E402
from vulkanhybridrenderer_amd import abi, lib, ray_queries, scenes  # noqa: E402

MODES = (("none", abi.FACE_CULL_NONE), ("back", abi.FACE_CULL_BACK), ("front", abi.FACE_CULL_FRONT))


def measure(name, args, rec):
    import torch
    scene = getattr(scenes, name)()
    count = args.rays
    lo, hi = ray_queries.scene_bounds(scene)
    rays = ray_queries.random_rays(np.random.default_rng(11), count, lo, hi, margin=0.1, tmins=(0.0,), tmaxs=(np.inf,))
    ctx = lib.Context(64, 64)
    try:
        ctx.upload_scene(scene)
        d_rays = torch.from_numpy(rays).cuda()
        stream = torch.cuda.current_stream()
        for any_hit in (False, True):
            out = torch.zeros(count if any_hit else (count, 6), dtype=torch.uint8 if any_hit else torch.int32, device="cuda")

            def hits():
                torch.cuda.synchronize()
                return int(out.to(torch.bool).sum().item()) if any_hit else int((out[:, 3] != -1).sum().item())

            plain = [timed(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count, out.data_ptr(), any_hit=any_hit, cull_mask=0xFF), args.reps, 3)
                     for _ in range(3)]
            assert ctx.face_cull_statistics()[1] == 0 and ctx.ray_mask_statistics()[2] == 0
            r = dict(what="face_cull_query", scene=name, rays=count, any_hit=any_hit, primitives=len(scene.primitives), triangles=scene.triangle_count,
                     flipped_primitives=ctx.face_cull_statistics()[0], plain_ms_min=min(plain), plain_ms_max=max(plain), plain_hits=hits(),
                     plain_mrays_s=count / float(np.median(plain)) / 1e3)
            for key, mode in MODES:
                ms = timed(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count, out.data_ptr(), any_hit=any_hit, face_cull=mode), args.reps, 3)
                ran = ctx.face_cull_statistics()[1]
                assert ran == (0 if any_hit and mode == abi.FACE_CULL_NONE else 1), (key, any_hit, ran)
                r.update({f"{key}_ms": ms, f"{key}_over_plain": ms / float(np.median(plain)), f"{key}_mrays_s": count / ms / 1e3, f"{key}_hits": hits(),
                          f"{key}_face_instantiation": ran})
            rec.emit(r)
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_cull_rate.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("face_cull_rate: no GPU (this measurement has no CPU fallback)")
    rec = Records(args.out, date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint())
    for name in args.scenes.split(","):
        measure(name, args, rec)


if __name__ == "__main__":
    main()
