"""The forward raster path's "Forward Pass" stand-in (vhr_standin_forward_raster) at 1920 x 1080, frame 1 of each scene's camera path: for
sponza_proc and bistro_proc, with and without MSAA (S = 8 / 1 sample rays per pixel), both kernels (variant_standin_forward_raster 1 = the work
queue, 0 = the literal one pixel per thread).  One GPU process, --warmup untimed frames before each measure.  Per measure: kernel
milliseconds (kernel timing kind "forward_raster"), wall milliseconds (HIP events around the graph's execute; the path's Depth Prepass
has no body here, so the Forward Pass is all the frame does), sample rays per second of the kernel, and fragments shaded per covered
pixel (the `fragments` probe, from one extra frame).  Then the ratios the feature was aimed at.  One JSON line per measure, the library's
source fingerprint in each.

  python tools/forward_raster_rate.py [--reps 20] [--warmup 3] [--out profiles/forward_raster_rate_1080p.jsonl]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, kernel_timing, timed  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, scenes  # noqa: E402

MSAA = "Forward Pass_MSAA"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="sponza_proc,bistro_proc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    W, H = args.width, args.height
    stream = torch.cuda.Stream()
    res = {}
    emit = Records(args.out, width=W, height=H, frame=1, reps=args.reps, fingerprint=lib.source_fingerprint()).emit

    for scene_name in args.scenes.split(","):
        scene = getattr(scenes, scene_name)()
        pfd = camera.dolly_frames(scene, W, H, 2)[1]
        for msaa in (1, 0):
            S = 8 if msaa else 1
            ctx = lib.Context(W, H, stream=stream.cuda_stream)
            ctx.upload_scene(scene)
            present = ctx.upload_new_storage_image(W, H, abi.FORMAT_B8G8R8A8_SRGB)
            frags = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
            probe = {"on": False}

            def body(c):
                c.standin_forward_raster(present, msaa=MSAA if msaa else None, fragments_ptr=frags.data_ptr() if probe["on"] else 0)
            path = lib.ForwardRasterRenderPath(ctx, forward_pass=body, enable_msaa=msaa)
            path.build()
            ctx.update_per_frame_ubo(0, pfd)
            try:
                run = lambda: ctx.execute(0, 0)      # noqa: E731
                for variant in (1, 0):
                    ctx.set_option("variant_standin_forward_raster", variant)
                    wall = timed(torch, stream, run, args.reps, args.warmup)
                    with kernel_timing(ctx, "forward_raster") as t:
                        for _ in range(args.reps):
                            run()
                    kms = t.ms / args.reps
                    ctx.set_ray_statistics(True)
                    probe["on"] = True
                    run()
                    ctx.synchronize()
                    st = ctx.ray_statistics()
                    ctx.set_ray_statistics(False)
                    probe["on"] = False
                    f = frags.cpu().numpy()
                    covered = f > 0
                    res[(scene_name, S, variant)] = kms
                    emit(dict(scene=scene_name, samples=S, kernel="forward_raster_queue_kernel" if variant else "forward_raster_kernel",
                              kernel_ms=kms, launches_per_frame=t.launches / args.reps, wall_ms=wall, sample_rays=st["unique_rays"],
                              sample_rays_per_s=st["unique_rays"] / (kms * 1e-3), stack_overflows=st["stack_overflows"],
                              covered_pixels=int(covered.sum()), fragments_per_covered_pixel=float(f[covered].mean()) if covered.any() else 0.0))
            finally:
                path.destroy()
                ctx.close()
        q8, q1, l8 = res[(scene_name, 8, 1)], res[(scene_name, 1, 1)], res[(scene_name, 8, 0)]
        emit(dict(scene=scene_name, measure="targets", queue_s8_ms=q8, target_s8_ms=1.85, s8_within_target=q8 <= 1.85, queue_over_literal_s8=q8 / l8,
                  queue_faster_than_literal=q8 < l8, s8_over_s1=q8 / q1, s8_over_s1_within_5=q8 / q1 <= 5.0))


if __name__ == "__main__":
    main()
