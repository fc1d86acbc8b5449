"""How decision (vi) behaves when the unit of length changes: the scenes of tests/test_gpu_ray_truth.py -- the three soups with their
random rays, soup 3 with its grazing rays, and the hybrid path's shadow / AO / mirror rays on tiny_scene and the turned sponza_proc --
with every length times 2^-10, 1 and 2^10, for the CPU oracle and for the device, one JSON line per (scene, rays, scale) APPENDED to
profiles/ray_truth_scale.jsonl.  The exact hit sets are the same at every scale (tests/test_ray_truth.py); what changes is how much of
the work the absolute constants (box padding 1e-3 + 1e-5 |x|, the "contradicts itself" tolerance 5e-4 + 5e-6 |x|) do.

Per record:
  oracle   a brute-force audit session (every triangle, exact arithmetic): pairs A / B / C / D under the rule in force, E, pairs sent to
           binary64; and the verdict of tests/ray_truth.py on its answers: violations, explained class-D answers, explained true hits
           passed over
  device   the same verdict on the device's answers; rays (queries) or pixels (hybrid path) decided again in binary64; and the device's
           decision (vhr_debug_ray_triangle) on the oracle's class B / C / D / E pairs: A' = exact hits accepted, B' = exact misses
           rejected, D' = exact misses accepted, E' = exact hits rejected

  python tools/ray_truth_scale.py [--no-device] [--out profiles/ray_truth_scale.jsonl]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import binding as ob  # noqa: E402
from tests import ray_truth as rt  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, scenes  # noqa: E402

W, H = 96, 64
KINDS = {ob.RAY_KIND_SHADOW: "shadow", ob.RAY_KIND_AO: "AO", ob.RAY_KIND_MIRROR: "mirror"}


def verdict_fields(prefix, *verdicts):
    return {f"{prefix}_violations": sum(v.violations for v in verdicts), f"{prefix}_explained_d": sum(v.explained_d for v in verdicts),
            f"{prefix}_explained_true_hits_passed_over": sum(v.explained_lost for v in verdicts)}


def audit_fields(a):
    c = a.counts
    A, B, C, D = (int(x) for x in c["cls"][3])
    return dict(oracle_pairs=int(c["pairs"]), oracle_exact_hits=int(c["exact_hits"]), oracle_A=A, oracle_B=B, oracle_C=C, oracle_D=D,
                oracle_E=int(c["mt_miss_exact_hit"]), oracle_pairs_to_binary64=int(c["escalated"]), oracle_pairs_undecided_in_binary64=int(c["undecided"]),
                oracle_records_dropped=int(c["records_dropped"]))


def device_on_records(ctx, records):
    """The device's decision on the oracle's class B / C / D / E pairs."""
    recs = records[np.isin(records["cls"], (b"B", b"C", b"D", b"E"))]
    if not len(recs):
        return dict(device_A_on_records=0, device_B_on_records=0, device_D_on_records=0, device_E_on_records=0)
    pairs = np.concatenate([recs["o"], recs["d"], recs["v0"], recs["e1"], recs["e2"], recs["tmin"][:, None], recs["tmax"][:, None]], axis=1).astype(np.float32)
    accepted, _ = ctx.ray_triangle(pairs)
    exact = recs["exact"] == 1
    return dict(device_A_on_records=int((accepted & exact).sum()), device_B_on_records=int((~accepted & ~exact).sum()),
                device_D_on_records=int((accepted & ~exact).sum()), device_E_on_records=int((~accepted & exact).sum()))


def queries(emit, device):
    for seed, _, _ in rt.SOUPS:
        base = rt.soup_scene(seed)
        sets = [("random", rt.soup_rays(base, seed))] + ([("grazing", rt.soup_grazing(base))] if seed == 3 else [])
        for scale in rt.SCALES:
            scene = rt.scaled_scene(base, scale)
            osc = ob.Scene(scene)
            ctx = None
            if device:
                ctx = lib.Context(64, 64)
                ctx.upload_scene(scene)
            try:
                for name, rays in sets:
                    rays = rt.scaled_rays(rays, scale)
                    truth = rt.Truth(ob, osc, rays)
                    with ob.Audit(brute_force=True, max_records=400000) as a:
                        closest, occ = rt.oracle_answers(osc, rays, use_bvh=False)
                    r = dict(what="ray_truth_scale", path="ray queries", scene=base.name, rays=name, scale=scale, n_rays=len(rays), triangles=int(osc.triangle_count),
                             exact_hit_pairs=int(truth.hit.sum()), band_rays=int(truth.band_rays.sum()), oracle_hit_share=float(occ.mean()))
                    r.update(audit_fields(a))
                    r.update(verdict_fields("oracle", rt.judge_closest(truth, *closest), rt.judge_any(truth, occ)))
                    if ctx is not None:
                        hits = ctx.ray_query(rays)
                        s_closest = ctx.ray_query_statistics()
                        docc = ctx.ray_query(rays, any_hit=True)
                        s_any = ctx.ray_query_statistics()
                        hit, flat = rt.flat_of_hits(scene, hits)
                        r.update(verdict_fields("device", rt.judge_closest(truth, hit, flat, hits["t"], hits["u"], hits["v"]), rt.judge_any(truth, docc)))
                        r.update(device_rays_to_binary64_closest=s_closest[2], device_rays_to_binary64_any_hit=s_any[2], device_hit_share=float(docc.mean()),
                                 device_answers_equal_the_oracle=bool(np.array_equal(docc, occ) and np.array_equal(hit, closest[0]) and np.array_equal(flat[hit], closest[1][hit])
                                                                      and np.array_equal(hits["t"][hit], closest[2][hit])))
                        r.update(device_on_records(ctx, a.records))
                    emit(r)
            finally:
                if ctx is not None:
                    ctx.close()


def hybrid(emit, device):
    from tests.helpers import GpuHybrid, f16
    makers = {"tiny_scene": scenes.tiny_scene, "sponza_proc_rot": lambda: scenes.rotated(scenes.sponza_proc(0.15), rot_y=0.6, rot_x=0.25)}
    for name, maker in makers.items():
        for scale in rt.SCALES:
            scene = rt.scaled_scene(maker(), scale)
            osc = ob.Scene(scene)
            pfd = camera.dolly_frames(scene, W, H, 2)[1]
            gbuf = osc.gbuffer(pfd, W, H)
            tps = {"visibility": rt.scaled_trace_params(abi.default_trace_params(shadow=True, ao_spp=1, reflections=False), scale),
                   "mirror": rt.scaled_trace_params(abi.default_trace_params(shadow=False, ao_spp=0, reflections=True), scale)}
            g = GpuHybrid(scene, W, H, denoise=False, trace_params=tps["visibility"]) if device else None
            try:
                for frame, tp in tps.items():
                    with ob.Audit(brute_force=True, max_records=400000, ray_log=4 * W * H) as a:
                        sa, refl, _, _ = osc.raygen(pfd, tp, gbuf[0], gbuf[2], use_bvh=False)
                    oracle_images = dict(vis=f16(sa).reshape(W * H, 2), alpha=f16(refl).reshape(W * H, 4)[:, 3])
                    device_images = None
                    again = None
                    if g is not None:
                        g.ctx.set_trace_params(tp)
                        g.ctx.set_ray_statistics(True)
                        g.frame(pfd, gbuf)
                        again = g.ctx.binary64_statistics()
                        device_images = dict(vis=f16(g.ctx.download(lib.RAYTRACED)).reshape(W * H, 2), alpha=f16(g.ctx.download(lib.REFLECTIONS)).reshape(W * H, 4)[:, 3])
                    r = dict(what="ray_truth_scale", path="hybrid", scene=name, rays=frame, scale=scale, width=W, height=H, n_rays=len(a.ray_log), triangles=int(osc.triangle_count))
                    r.update(audit_fields(a))
                    verdicts = {"oracle": [], "device": []}
                    band = hits = 0
                    for kind in KINDS:
                        sel = a.ray_log[a.ray_log["kind"] == kind]
                        if not len(sel):
                            continue
                        rays = np.zeros((len(sel), 8), np.float32)
                        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = sel["o"], sel["tmin"], sel["d"], sel["tmax"]
                        truth = rt.Truth(ob, osc, rays)
                        band, hits = band + int(truth.band_rays.sum()), hits + int(truth.hit.sum())
                        for side, images in (("oracle", oracle_images), ("device", device_images)):
                            if images is not None:
                                occluded = images["alpha"][sel["pixel"]] == 1.0 if kind == ob.RAY_KIND_MIRROR else images["vis"][sel["pixel"], kind] == 0.0
                                verdicts[side].append(rt.judge_any(truth, occluded))
                    r.update(exact_hit_pairs=hits, band_rays=band)
                    r.update(verdict_fields("oracle", *verdicts["oracle"]))
                    if g is not None:
                        r.update(verdict_fields("device", *verdicts["device"]))
                        r.update(device_pixels_again_in_binary64=again["pixels_again"], device_mirror_pixels_again_in_binary64=again["mirror_pixels_again"],
                                 device_images_equal_the_oracle=bool(np.array_equal(device_images["vis"], oracle_images["vis"]) and np.array_equal(device_images["alpha"], oracle_images["alpha"])))
                        r.update(device_on_records(g.ctx, a.records))
                    emit(r)
            finally:
                if g is not None:
                    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-device", action="store_true", help="the oracle's half only (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_truth_scale.jsonl"))
    args = ap.parse_args()
    device = not args.no_device
    if device:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("ray_truth_scale: no GPU (--no-device measures the oracle's half alone)")
    common = dict(date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint(), device=device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        def emit(rec):
            line = json.dumps(dict(rec, **common))
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        queries(emit, device)
        hybrid(emit, device)


if __name__ == "__main__":
    main()
