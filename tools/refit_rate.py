"""vhr_refit_geometry against vhr_update_geometry on sponza_proc and bistro_proc at full size (one GPU process), one JSON line per
measurement, the library's source fingerprint in each.

Per scene, after one build and one refit that are not timed (the first calls load code objects and make the refit's plan):
  "refit":   median over --reps of the host wall time of vhr_refit_geometry (perf_counter around the call, and the library's own figure,
             vhr_get_refit_times out[0]) after a vhr_update_vertices of every vertex; in a second series, with timing bit 12 set, the device
             time of the leaf pass, the upward pass and forms + checks (event pairs around the kernels).  The leaf pass's bytes per second:
             per record 16 B read of its (prim, tri, flat) word, 3 indices, 3 whole 56 B vertices (the gather touches their lines), 48 B
             written -- against the copy ceiling this project has measured on the part (5.5 TB/s).
  "rebuild": in the same process, the same arrays through vhr_update_geometry: wall time of the call and vhr_get_build_times out[0].
             condition_met = refit wall (median) <= a quarter of build_times[0] (median).
  "frame":   one hybrid frame at 1080p as bench.py runs it (shadow + 2 AO rays, SVGF, stand-in G-buffer): wall per frame and the any-hit
             launch (kernel kind "raygen"); refit wall over frame wall.
  "curve":   the any-hit launch and the SAH cost after a refit versus after a rebuild from the same arrays, for every vertex above 1 m pushed
             along x by a wave of growing amplitude, and for a third of the primitives rotated about y (about the scene's origin) by growing angles.

  python tools/refit_rate.py [--reps 12] [--frames 20] [--out profiles/refit_rate.jsonl] [--scenes sponza_proc,bistro_proc]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rate_common import Records, kernel_timing  # noqa: E402
from vulkanhybridrenderer_amd import abi, camera, lib, scenes  # noqa: E402

COPY_CEILING_TBS = 5.5


class Frames:
    """The hybrid path on a context, bench.py's workload: stand-in G-buffer, shadow + 2 AO rays, SVGF; no mirror ray."""

    def __init__(self, ctx, scene, W, H, n):
        self.ctx = ctx
        ctx.set_trace_params(abi.default_trace_params(shadow=True, ao_spp=2, reflections=False))
        self.path = lib.HybridRenderPath(ctx, shadow_mode=0, ambient_occlusion_mode=0, reflection_mode=2, denoise=True, atrous_steps=5,
                                         gbuffer_pass=lambda c: c.standin_gbuffer(0))
        self.path.build()
        self.pfds = camera.dolly_frames(scene, W, H, n)

    def run(self, warmup=3):
        """(wall ms per frame, any-hit launch ms per frame)"""
        ctx = self.ctx
        for pfd in self.pfds[:warmup]:
            ctx.update_per_frame_ubo(0, pfd)
            ctx.execute(0, 0)
        ctx.synchronize()
        t0 = time.perf_counter()
        for pfd in self.pfds:
            ctx.update_per_frame_ubo(0, pfd)
            ctx.execute(0, 0)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / len(self.pfds)
        with kernel_timing(ctx, "raygen") as t:
            for pfd in self.pfds:
                ctx.update_per_frame_ubo(0, pfd)
                ctx.execute(0, 0)
        return wall, t.ms / max(1, t.launches)


def wave(scene, amplitude):
    v = scene.vertices.copy()
    p = v["pos"]
    up = p[:, 1] > 1.0
    p[up, 0] += (amplitude * np.sin(3.0 * p[up, 1] + 2.0 * p[up, 2])).astype(np.float32)
    return v


def rotated_third(scene, degrees):
    t = np.ascontiguousarray(scene.primitives["transform"], np.float32).reshape(-1, 16).copy()
    r = scenes.trs(rot_y=np.radians(degrees))
    for p in range(0, len(t), 3):
        t[p] = abi.mat_to_glm(r @ abi.glm_to_mat(t[p]))
    return t


def median(x):
    return float(np.median(np.asarray(x, np.float64)))


def measure(name, scene, args, emit):
    W, H = 1920, 1080
    ctx = lib.Context(W, H)
    base = dict(scene=name, triangles=scene.triangle_count, fingerprint=lib.source_fingerprint())
    try:
        ctx.upload_scene(scene)                      # first calls: code objects, the refit's plan
        ctx.update_vertices(scene.vertices)
        ctx.refit_geometry()
        st = ctx.bvh_statistics()
        base.update(nodes=int(st["nodes"]), depth=int(st["max_depth"]))
        # ---- the refit
        wall, own = [], []
        for _ in range(args.reps):
            ctx.update_vertices(scene.vertices)
            t0 = time.perf_counter()
            ctx.refit_geometry()
            wall.append((time.perf_counter() - t0) * 1e3)
            own.append(ctx.refit_times_ms()[0])
        ctx.set_kernel_timing(False, refit=True)
        split = []
        for _ in range(args.reps):
            ctx.update_vertices(scene.vertices)
            ctx.refit_geometry()
            split.append(ctx.refit_times_ms()[1:])
        ctx.set_kernel_timing(False)
        leaf, up, forms = (median([s[i] for s in split]) for i in range(3))
        rs = ctx.refit_statistics()
        n = scene.triangle_count
        leaf_bytes = n * (16 + 12 + 3 * 56 + 48)
        refit_wall = median(wall)
        emit(dict(base, what="refit", reps=args.reps, wall_ms_median=refit_wall, wall_ms_min=float(min(wall)), wall_ms_max=float(max(wall)),
                  wall_ms_library=median(own), leaf_pass_ms=leaf, upward_pass_ms=up, forms_and_checks_ms=forms, upward_launches=rs["upward_launches"],
                  leaf_pass_bytes=leaf_bytes, leaf_pass_tb_per_s=leaf_bytes / (leaf * 1e-3) / 1e12 if leaf > 0 else None,
                  copy_ceiling_tb_per_s=COPY_CEILING_TBS, records_outside=rs["records_outside"], children_outside=rs["children_outside"]))
        # ---- the rebuild, same process, same arrays
        bwall, build = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ctx.update_geometry(scene.vertices, scene.indices, scene.primitives)
            bwall.append((time.perf_counter() - t0) * 1e3)
            build.append(ctx.build_times_ms()[0])
        build_ms = median(build)
        emit(dict(base, what="rebuild", reps=args.reps, update_geometry_wall_ms_median=median(bwall), build_times0_ms_median=build_ms,
                  refit_wall_over_build=refit_wall / build_ms, condition="refit wall <= build_times[0] / 4", condition_met=bool(refit_wall <= build_ms / 4)))
        # ---- one frame
        frames = Frames(ctx, scene, W, H, args.frames)
        frame_ms, anyhit_ms = frames.run()
        emit(dict(base, what="frame", frames=args.frames, frame_wall_ms=frame_ms, any_hit_launch_ms=anyhit_ms, refit_wall_over_frame=refit_wall / frame_ms))
        # ---- the degradation curve
        for kind, values in (("wave_amplitude_m", (0.0, 0.05, 0.2, 0.5, 1.0, 2.0)), ("third_rotated_deg", (2.0, 10.0, 30.0, 90.0))):
            for value in values:
                v = wave(scene, value) if kind == "wave_amplitude_m" else scene.vertices
                t = rotated_third(scene, value) if kind == "third_rotated_deg" else np.ascontiguousarray(scene.primitives["transform"], np.float32).reshape(-1, 16)
                prims = scene.primitives.copy()
                prims["transform"] = t.reshape(prims["transform"].shape)
                ctx.update_geometry(scene.vertices, scene.indices, scene.primitives)       # the tree of the scene at rest
                ctx.update_vertices(v)
                ctx.update_primitive_transforms(t)
                ctx.refit_geometry()
                cost = ctx.bvh_sah_cost()
                _, refit_anyhit = frames.run()
                ctx.update_geometry(v, scene.indices, prims)
                rebuilt_cost = ctx.bvh_sah_cost()[1]
                _, rebuilt_anyhit = frames.run()
                emit(dict(base, what="curve", kind=kind, value=value, sah_cost_built=cost[0], sah_cost_refitted=cost[1], sah_cost_rebuilt=rebuilt_cost,
                          sah_ratio_refit_over_rebuilt=cost[1] / rebuilt_cost, any_hit_ms_refitted=refit_anyhit, any_hit_ms_rebuilt=rebuilt_anyhit,
                          any_hit_ratio=refit_anyhit / rebuilt_anyhit))
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
        raise SystemExit("refit_rate: no GPU (this measurement has no CPU fallback)")
    emit = Records(args.out).emit
    for name in args.scenes.split(","):
        scene = scenes.bistro_proc(texture_size=64) if name == "bistro_proc" else getattr(scenes, name)()      # (full-size geometry; small texels: nothing timed here samples them)
        measure(name, scene, args, emit)


if __name__ == "__main__":
    main()
