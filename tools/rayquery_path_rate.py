"""The rayquery render path's "Forward Pass" on sponza_proc at 1920 x 1080, frame 1 of its camera path, against the two other ways to the
same rays (one GPU process, after --warmup repetitions of each):

  (a) the Forward Pass: RayqueryRenderPath with vhr_standin_rayquery_forward as its body (rayquery_forward_queue_kernel: primary ray +
      inline query per 16x8 tile and wave) -- kernel timing kind "rayquery_forward" and HIP events around the graph's execute;
  (b) the composed route: vhr_standin_gbuffer, then vhr_ray_query (any hit) on ray_queries.rayquery_shadow_rays of that G-buffer's
      depth, all on the device -- HIP events around the two calls, and the ray query's own kernel timing kind;
  (c) the raytraced path's Raytracing Pass (the same work: one primary ray + one shadow ray per covered pixel) -- kernel timing kind
      "raygen" (its launch) and HIP events around the graph's execute.

One JSON line per measure, the library's source fingerprint in each.

  python tools/rayquery_path_rate.py [--reps 30] [--warmup 5] [--out profiles/rayquery_path_rate_sponza_proc_1080p.jsonl]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, kernel_timing, timed  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, ray_queries, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    W, H = args.width, args.height
    scene = scenes.sponza_proc()
    pfd = camera.dolly_frames(scene, W, H, 2)[1]
    emit = Records(args.out, scene="sponza_proc", width=W, height=H, frame=1, reps=args.reps, fingerprint=lib.source_fingerprint()).emit

    def kernel_ms(ctx, kind, body):
        with kernel_timing(ctx, kind) as t:
            for _ in range(args.reps):
                body()
        return t.ms / args.reps, t.launches / args.reps

    stream = torch.cuda.Stream()
    res = {}

    # (a) the Forward Pass
    ctx = lib.Context(W, H, stream=stream.cuda_stream)
    ctx.upload_scene(scene)
    present = ctx.upload_new_storage_image(W, H, abi.FORMAT_B8G8R8A8_SRGB)
    path = lib.RayqueryRenderPath(ctx, forward_pass=lambda c: c.standin_rayquery_forward(present))
    path.build()
    ctx.update_per_frame_ubo(0, pfd)
    try:
        run = lambda: ctx.execute(0, 0)      # noqa: E731
        wall = timed(torch, stream, run, args.reps, args.warmup)
        kms, launches = kernel_ms(ctx, "rayquery_forward", run)
        ctx.set_ray_statistics(True)
        run()
        st = ctx.ray_statistics()
        ctx.set_ray_statistics(False)
        res["a"] = kms
        emit(dict(measure="(a) Forward Pass (rayquery_forward_queue_kernel)", kernel_ms=kms, launches_per_frame=launches, wall_ms=wall,
                  rays=st["unique_rays"], queries=st["covered_pixels"], stack_overflows=st["stack_overflows"],
                  ns_per_ray_kernel=kms * 1e6 / st["unique_rays"]))
    finally:
        path.destroy()
        ctx.close()

    # (b) the composed route: G-buffer stand-in + vhr_ray_query on its shadow rays
    ctx = lib.Context(W, H, stream=stream.cuda_stream)
    ctx.upload_scene(scene)
    gpath = lib.HybridRenderPath(ctx, gbuffer_pass=lambda c: c.standin_gbuffer(0))
    gpath.build()
    ctx.update_per_frame_ubo(0, pfd)
    try:
        ctx.execute(0, 0)
        ctx.synchronize()
        depth = ctx.download(lib.DEPTH)
        rays, _ = ray_queries.rayquery_shadow_rays(pfd, depth)
        n = len(rays)
        rays_d = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda")
        out_d = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def composed():
            ctx.standin_gbuffer(0)
            ctx.ray_query_device(rays_d.data_ptr(), n, out_d.data_ptr(), any_hit=True)
        wall = timed(torch, stream, composed, args.reps, args.warmup)
        qms, qlaunches = kernel_ms(ctx, "ray_query", composed)
        res["b"] = wall
        emit(dict(measure="(b) vhr_standin_gbuffer + vhr_ray_query any hit on rayquery_shadow_rays", wall_ms=wall, ray_query_kernel_ms=qms,
                  ray_query_launches=qlaunches, rays=W * H + n, queries=n))
    finally:
        gpath.destroy()
        ctx.close()

    # (c) the raytraced path's Raytracing Pass
    ctx = lib.Context(W, H, stream=stream.cuda_stream)
    ctx.upload_scene(scene)
    rpath = lib.RaytracedRenderPath(ctx)
    rpath.build()
    ctx.update_per_frame_ubo(0, pfd)
    try:
        run = lambda: ctx.execute(0, 0)      # noqa: E731
        wall = timed(torch, stream, run, args.reps, args.warmup)
        kms, launches = kernel_ms(ctx, "raygen", run)
        ctx.set_ray_statistics(True)
        run()
        st = ctx.ray_statistics()
        res["c"] = kms
        emit(dict(measure="(c) raytraced path Raytracing Pass (raytraced_queue_kernel)", kernel_ms=kms, launches_per_frame=launches, wall_ms=wall,
                  rays=st["unique_rays"], queries=st["covered_pixels"], ns_per_ray_kernel=kms * 1e6 / st["unique_rays"]))
    finally:
        rpath.destroy()
        ctx.close()

    emit(dict(measure="ratios", a_over_b=res["a"] / res["b"], a_over_c=res["a"] / res["c"],
              target_a_below_b=res["a"] < res["b"], target_a_within_1_15_c=res["a"] <= 1.15 * res["c"]))


if __name__ == "__main__":
    main()
