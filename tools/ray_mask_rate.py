"""What ray cull masks cost: the hybrid path's shadow / AO launch and its mirror-ray launch on sponza_proc and bistro_proc at 1080p with
primitive masks and class masks that act, against the same context with every class mask at 255 (the plain kernels), one JSON line
per case with the library's source fingerprint.  It fixes no target; the comparator is the existing alpha route.

Class masks while on: shadow 0x01, AO 0x02, reflection 0x04.  Settings (primitive masks; every other primitive stays 0xFF):
  a  one far, tiny primitive at 0x08 (hidden from every class): what running the filtering instantiation costs at all
  b  10 % of the primitives at 0x06 (hidden from shadow rays only)          c  30 % likewise
  d  10 % of the primitives at 0x08 (hidden from all three classes)         e  30 % likewise
The 10 % / 30 % sets are the primitives scenes.alpha_masked(scene, percent) turns into cut-outs, so that the comparator -- that scene
with "alpha_test_rays" 1, in a context of its own in the same process -- hides (half of) the same geometry through the costlier rule.
The off series is measured three times; its min..max is the spread a ratio has to leave to mean anything.  With masks on the images
differ from those with them off (rays pass where a primitive is hidden), so a ratio compares two workloads, not two codes on one.

Then 2^20 random ray queries on the setting-e masks: vhr_ray_query against vhr_ray_query_masked with cull mask 0x01, closest and any hit.

  python tools/ray_mask_rate.py [--frames 30] [--warmup 5] [--scenes sponza_proc,bistro_proc] [--out profiles/ray_mask_rate.jsonl]
"""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, kernel_timing, timed  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, ray_queries, scenes  # noqa: E402

W, H = 1920, 1080
CLASS_MASKS = dict(shadow_ray_mask=0x01, ao_ray_mask=0x02, reflection_ray_mask=0x04)
SHADOW_ONLY, ALL_CLASSES = 0x06, 0x08


def launches(ctx, pfds, warmup):
    """(shadow / AO launch ms, mirror-ray launch ms) per frame, each kind timed in a pass of its own over the frames"""
    def frames(which):
        for pfd in which:
            ctx.update_per_frame_ubo(0, pfd)
            ctx.execute(0, 0)
    frames(pfds[:warmup])
    ctx.synchronize()
    out = []
    for kind in ("raygen", "reflection"):
        with kernel_timing(ctx, kind) as t:
            frames(pfds)
        out.append(t.ms / max(1, t.launches))
    return out


def hybrid(scene):
    ctx = lib.Context(W, H)
    ctx.upload_scene(scene)
    ctx.set_trace_params(abi.default_trace_params(shadow=True, ao_spp=2, reflections=True))
    path = lib.HybridRenderPath(ctx, shadow_mode=0, ambient_occlusion_mode=0, reflection_mode=0, denoise=False, atrous_steps=5,
                                gbuffer_pass=lambda c: c.standin_gbuffer(0))
    path.build()
    return ctx, path


def spread_set(n, percent):
    count = int(round(n * percent / 100.0))
    return np.unique((np.arange(count) * n) // count)                   # scenes.alpha_masked's choice


def far_tiny_primitive(scene):
    """the primitive with the fewest triangles; among those, the one farthest from the scene's centre"""
    tris = ray_queries.world_triangles(scene)
    first = np.concatenate([[0], np.cumsum(scene.primitives["index_count"] // 3)]).astype(np.int64)
    centre = tris.reshape(-1, 3).mean(axis=0)
    counts = np.diff(first)
    few = np.nonzero(counts == counts[counts > 0].min())[0]
    dist = [np.linalg.norm(tris[first[p]:first[p + 1]].reshape(-1, 3).mean(axis=0) - centre) for p in few]
    return int(few[int(np.argmax(dist))])


def measure(name, args, rec):
    import torch
    scene = getattr(scenes, name)()
    n = len(scene.primitives)
    pfds = camera.dolly_frames(scene, W, H, args.frames)
    settings = [("a", [far_tiny_primitive(scene)], ALL_CLASSES, 0), ("b", spread_set(n, 10), SHADOW_ONLY, 10), ("c", spread_set(n, 30), SHADOW_ONLY, 30),
                ("d", spread_set(n, 10), ALL_CLASSES, 10), ("e", spread_set(n, 30), ALL_CLASSES, 30)]
    # the comparator first, each in a context of its own: the alpha route on the same sets
    alpha_ms = {}
    for percent in (10, 30):
        ctx, path = hybrid(scenes.alpha_masked(scene, percent))
        try:
            ctx.set_option("alpha_test_rays", 1)
            alpha_ms[percent] = launches(ctx, pfds, args.warmup)
            assert ctx.alpha_launches() == 2
        finally:
            path.destroy()
            ctx.close()
    ctx, path = hybrid(scene)
    try:
        def series(on):
            for k, v in CLASS_MASKS.items():
                ctx.set_option(k, v if on else 255)
            ms = launches(ctx, pfds, args.warmup)
            return ms, ctx.ray_mask_statistics()[1]
        for key, hidden, value, percent in settings:
            masks = np.full(n, 0xFF, np.uint8)
            masks[np.asarray(hidden, np.int64)] = value
            ctx.set_primitive_masks(masks)
            off = []
            for _ in range(3):
                ms, ran = series(False)
                assert ran == 0, ran
                off.append(ms)
            on, ran = series(True)
            assert ran == (1 if value == SHADOW_ONLY else 2), ran
            off = np.array(off)
            r = dict(what="ray_masks", scene=name, width=W, height=H, setting=key, hidden_primitives=len(hidden), primitives=n,
                     hidden_from="shadow rays" if value == SHADOW_ONLY else "all classes", triangles=scene.triangle_count, frames=args.frames,
                     mask_launches_per_frame=ran, shadow_ao_ms_off_min=float(off[:, 0].min()), shadow_ao_ms_off_max=float(off[:, 0].max()),
                     shadow_ao_ms_on=on[0], shadow_ao_on_over_off=on[0] / float(np.median(off[:, 0])),
                     mirror_ms_off_min=float(off[:, 1].min()), mirror_ms_off_max=float(off[:, 1].max()), mirror_ms_on=on[1],
                     mirror_on_over_off=on[1] / float(np.median(off[:, 1])))
            if percent:
                r.update(alpha_route_shadow_ao_ms=alpha_ms[percent][0], alpha_route_mirror_ms=alpha_ms[percent][1])
            rec.emit(r)
        # queries, on the setting-e masks
        count = 1 << 20
        lo, hi = ray_queries.scene_bounds(scene)
        rays = ray_queries.random_rays(np.random.default_rng(11), count, lo, hi, margin=0.1, tmins=(0.0,), tmaxs=(np.inf,))
        d_rays = torch.from_numpy(rays).cuda()
        stream = torch.cuda.current_stream()
        for any_hit in (False, True):
            out = torch.zeros(count if any_hit else (count, 6), dtype=torch.uint8 if any_hit else torch.int32, device="cuda")
            plain = timed(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count, out.data_ptr(), any_hit=any_hit), 10, 3)
            assert ctx.ray_mask_statistics()[2] == 0
            masked = timed(torch, stream, lambda: ctx.ray_query_device(d_rays.data_ptr(), count, out.data_ptr(), any_hit=any_hit, cull_mask=0x01), 10, 3)
            assert ctx.ray_mask_statistics()[2] == 1
            rec.emit(dict(what="ray_masks_query", scene=name, rays=count, any_hit=any_hit, hidden_primitives=len(settings[-1][1]), primitives=n,
                          plain_ms=plain, masked_ms=masked, masked_over_plain=masked / plain, plain_mrays_s=count / plain / 1e3, masked_mrays_s=count / masked / 1e3))
    finally:
        path.destroy()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_mask_rate.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ray_mask_rate: no GPU (this measurement has no CPU fallback)")
    rec = Records(args.out, date=datetime.date.today().isoformat(), fingerprint=lib.source_fingerprint())
    for name in args.scenes.split(","):
        measure(name, args, rec)


if __name__ == "__main__":
    main()
