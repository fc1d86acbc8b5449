"""ctypes binding of libvhr_amd.so (the C ABI declared in include/vhr_amd.h).

The shared library is the product; this module only marshals numpy arrays and Python callbacks across the
boundary, mirroring the reference's class names (ResourceManager / RenderGraph / execution contexts:
/root/reference/src/rendering_backend/resource_manager.h:16-78, src/render_graph/render_graph.h:5-60,
compute_execution_context.h:7-43, raytracing_execution_context.h:4-20).  There is no CPU fallback: if the
library is missing or no HIP device exists, calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvhr_amd.so")

# every symbol include/vhr_amd.h declares (tests/test_abi.py checks the .so exports each of them)
EXPORTS = [
    "vhr_create", "vhr_destroy", "vhr_resize", "vhr_last_error", "vhr_synchronize", "vhr_version", "vhr_abi_struct_sizes",
    "vhr_default_trace_params", "vhr_update_geometry", "vhr_upload_texture_from_data", "vhr_upload_new_storage_image",
    "vhr_destroy_storage_image", "vhr_update_per_frame_ubo", "vhr_set_trace_params", "vhr_graph_destroy_resources",
    "vhr_graph_add_graphics_pass", "vhr_graph_add_raytracing_pass", "vhr_graph_add_compute_pass", "vhr_graph_build",
    "vhr_graph_execute", "vhr_graph_gather_performance_statistics", "vhr_graph_get_pass_time_ms",
    "vhr_graph_get_execution_order", "vhr_graph_contains_image", "vhr_graph_get_image_format",
    "vhr_graph_set_pass_epilogue", "vhr_graph_bind_external_image", "vhr_trace_rays", "vhr_compute_get_display_size",
    "vhr_compute_dispatch", "vhr_compute_blit_image_storage_to_transient", "vhr_compute_blit_image_transient_to_storage",
    "vhr_compute_blit_image_storage_to_storage", "vhr_hybrid_create", "vhr_hybrid_destroy", "vhr_hybrid_build",
    "vhr_hybrid_rebuild", "vhr_hybrid_get_push_constants", "vhr_hybrid_last_error", "vhr_hybrid_state_size", "vhr_hybrid_save_state",
    "vhr_hybrid_load_state", "vhr_get_last_per_frame_ubo", "vhr_get_display_size",
    "vhr_get_transient_image", "vhr_get_storage_image", "vhr_upload_transient_image", "vhr_download_transient_image",
    "vhr_upload_storage_image", "vhr_download_storage_image", "vhr_standin_gbuffer", "vhr_standin_gbuffer_with_albedo", "vhr_standin_composition", "vhr_standin_shadow_map", "vhr_set_strip", "vhr_set_tile",
    "vhr_standin_raytraced_composition", "vhr_raytraced_create", "vhr_raytraced_destroy", "vhr_raytraced_build", "vhr_raytraced_rebuild",
    "vhr_raytraced_last_error", "vhr_standin_rayquery_forward", "vhr_rayquery_create", "vhr_rayquery_destroy", "vhr_rayquery_build",
    "vhr_rayquery_rebuild", "vhr_rayquery_last_error", "vhr_standin_forward_raster", "vhr_forward_raster_create", "vhr_forward_raster_destroy",
    "vhr_forward_raster_build", "vhr_forward_raster_rebuild", "vhr_forward_raster_last_error", "vhr_get_transient_image_samples",
    "vhr_set_ray_statistics", "vhr_get_ray_statistics", "vhr_get_bvh_statistics", "vhr_get_current_stream", "vhr_get_bvh_builder", "vhr_get_bvh_presplit_level", "vhr_get_bvh_frame", "vhr_get_bvh_form_checks", "vhr_get_bvh_fingerprint", "vhr_get_bvh_tree_fingerprint", "vhr_get_bvh_forms_fingerprint", "vhr_set_kernel_timing",
    "vhr_get_kernel_time", "vhr_set_option", "vhr_get_option", "vhr_option_count", "vhr_option_info", "vhr_get_traversal_statistics", "vhr_source_fingerprint", "vhr_debug_wave_lifetimes", "vhr_get_reflection_statistics", "vhr_get_binary64_statistics", "vhr_debug_ray_triangle", "vhr_get_traversal_cycles", "vhr_get_drain_statistics", "vhr_get_build_times", "vhr_atrous_overlap", "vhr_atrous_output_extent", "vhr_strip_plan_make",
    "vhr_strip_plan_exchanges", "vhr_tile_grid_choose", "vhr_tile_plan_make", "vhr_tile_plan_make_weighted", "vhr_get_tile_cost_map", "vhr_tile_plan_exchanges", "vhr_tile_plan_replan", "vhr_comm_replan", "vhr_comm_get_unique_id", "vhr_comm_use_library", "vhr_comm_library", "vhr_comm_create", "vhr_comm_create_tiled", "vhr_comm_destroy", "vhr_comm_last_error", "vhr_comm_exchange_raytraced",
    "vhr_comm_start_frame_exchanges", "vhr_comm_finish_frame_exchanges",
    "vhr_calibration_stream_read", "vhr_ray_query", "vhr_get_ray_query_statistics", "vhr_ray_query_struct_layout",
    "vhr_update_vertices", "vhr_update_primitive_transforms", "vhr_refit_geometry", "vhr_get_refit_statistics", "vhr_get_refit_times",
    "vhr_get_bvh_sah_cost", "vhr_refit_geometry_partial", "vhr_get_partial_refit_statistics",
    "vhr_get_object_motion_statistics", "vhr_debug_triangle_records", "vhr_debug_bvh_arrays",
    "vhr_set_primitive_masks", "vhr_get_primitive_masks", "vhr_ray_query_masked", "vhr_get_ray_mask_statistics",
    "vhr_closest_point_query", "vhr_get_point_query_statistics", "vhr_debug_point_triangle",
    "vhr_nearest_points_query", "vhr_get_nearest_query_statistics",
    "vhr_rebuild_geometry", "vhr_get_rebuild_statistics",
    "vhr_ray_query_faces", "vhr_get_primitive_facing_flips", "vhr_get_face_cull_statistics", "vhr_debug_ray_facing",
    "vhr_resolve_hits", "vhr_get_surface_statistics", "vhr_surface_point_layout",
    "vhr_occlusion_query", "vhr_get_occlusion_statistics", "vhr_debug_occlusion_rays",
]

PATH_PREFIXES = ("hybrid", "raytraced", "rayquery", "forward_raster")      # vhr_<prefix>_{create,destroy,build,rebuild,last_error}


class VhrError(RuntimeError):
    pass


class CreateInfo(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32), ("stream", C.c_void_p),
                ("flags", C.c_uint32)]


class TransientImage(C.Structure):
    _fields_ = [("type", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_int32),
                ("binding", C.c_uint32), ("clear_value", C.c_float * 4), ("multisampled", C.c_int32)]


class TransientResource(C.Structure):
    _fields_ = [("type", C.c_int32), ("name", C.c_char_p), ("image", TransientImage)]


class HitShader(C.Structure):
    _fields_ = [("closest_hit", C.c_char_p), ("any_hit", C.c_char_p)]


class RaytracingPipelineDescription(C.Structure):
    _fields_ = [("name", C.c_char_p), ("raygen_shader", C.c_char_p), ("miss_shaders", C.POINTER(C.c_char_p)),
                ("miss_shader_count", C.c_uint32), ("hit_shaders", C.POINTER(HitShader)), ("hit_shader_count", C.c_uint32)]


class ComputePipelineDescription(C.Structure):
    _fields_ = [("kernels", C.POINTER(C.c_char_p)), ("kernel_count", C.c_uint32), ("push_constant_size", C.c_uint32)]


class ImageInfo(C.Structure):
    _fields_ = [("device_ptr", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_int32),
                ("bytes_per_pixel", C.c_uint32)]


class CompositionDesc(C.Structure):
    _fields_ = [("shadow_mode", C.c_int32), ("ambient_occlusion_mode", C.c_int32), ("reflection_mode", C.c_int32),
                ("albedo_image", C.c_char_p), ("normals_image", C.c_char_p), ("motion_image", C.c_char_p), ("depth_image", C.c_char_p),
                ("shadow_ao_image", C.c_char_p), ("reflections_image", C.c_char_p), ("output_storage_image", C.c_int32),
                ("ssao_image", C.c_char_p), ("shadow_map_image", C.c_char_p)]


class RayqueryForwardDesc(C.Structure):
    """vhr_rayquery_forward_desc (include/vhr_amd.h); the three probes are device pointers (None = not written)."""
    _fields_ = [("output_storage_image", C.c_int32), ("depth_image", C.c_char_p), ("primary_hits", C.c_void_p), ("positions", C.c_void_p),
                ("shadowed", C.c_void_p)]


class ForwardRasterDesc(C.Structure):
    """vhr_forward_raster_desc (include/vhr_amd.h); the two probes are device pointers (None = not written)."""
    _fields_ = [("output_storage_image", C.c_int32), ("depth_image", C.c_char_p), ("msaa_image", C.c_char_p), ("sample_hits", C.c_void_p),
                ("fragments", C.c_void_p)]


class StripPlanC(C.Structure):
    """vhr_strip_plan (include/vhr_amd.h): the C planner's row strip, field for field tiling.StripPlan."""
    _fields_ = [("rank", C.c_uint32), ("world", C.c_uint32), ("height", C.c_uint32), ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
                ("overlap", C.c_uint32), ("halo", C.c_uint32)]


class RowExchangeC(C.Structure):
    _fields_ = [("peer", C.c_int32), ("send_begin", C.c_uint32), ("send_end", C.c_uint32), ("recv_begin", C.c_uint32), ("recv_end", C.c_uint32)]


class TilePlanC(C.Structure):
    """vhr_tile_plan (include/vhr_amd.h): the C planner's screen tile, field for field tiling.TilePlan."""
    _fields_ = [(n, C.c_uint32) for n in ("rank", "world", "width", "height", "grid_rows", "grid_cols", "col_begin", "col_end", "row_begin", "row_end",
                                          "overlap", "halo_rows", "halo_cols")] + [("col_cut", C.c_uint32 * 17), ("row_cut", (C.c_uint32 * 17) * 16)]      # VHR_TILE_MAX_GRID = 16


class RectC(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("x1", C.c_uint32), ("y0", C.c_uint32), ("y1", C.c_uint32)]


class RectExchangeC(C.Structure):
    _fields_ = [("peer", C.c_int32), ("send", RectC), ("recv", RectC)]


class HybridSettings(C.Structure):
    _fields_ = [("shadow_mode", C.c_int32), ("ambient_occlusion_mode", C.c_int32), ("reflection_mode", C.c_int32),
                ("denoise_shadow_and_ao", C.c_int32), ("atrous_steps", C.c_int32)]


EXTERNAL_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
RAYTRACING_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
COMPUTE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)

_lib = None


def option_table():
    """vhr_option_info for every option of the library's table: {name: (default, min, max)}."""
    L = load()
    out = {}
    for i in range(L.vhr_option_count()):
        name, d, lo, hi = C.c_char_p(), C.c_int32(), C.c_int32(), C.c_int32()
        if L.vhr_option_info(i, C.byref(name), C.byref(d), C.byref(lo), C.byref(hi)) != 0:
            raise VhrError(f"vhr_option_info({i})")
        out[name.value.decode()] = (int(d.value), int(lo.value), int(hi.value))
    return out


def source_fingerprint():
    """vhr_source_fingerprint(): the hash of the sources the loaded library was built from."""
    return load().vhr_source_fingerprint().decode()


def load():
    """Load libvhr_amd.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VhrError(f"{LIB_PATH} is missing: build it with `make -C vulkanhybridrenderer_amd/csrc` "
                       "(there is no CPU or pure-Python fallback)")
    # One HIP runtime (and one RCCL) per process.  PyTorch's wheel bundles its own libamdhip64 / librccl; libvhr_amd.so links
    # the ROCm installation's.  The loader merges them by soname only when torch's copies are loaded FIRST -- the other way round
    # the process ends up with two HIP runtimes, of which the second finds no device (measured: ncclCommInitRank fails with "no
    # ROCm-capable device", and the process aborts at exit).  torch is this package's plumbing for device memory and
    # torch.distributed anyway, so it goes first whenever it is installed; a C / C++ host without torch has one runtime by itself.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
    L.vhr_create.argtypes = [C.POINTER(CreateInfo), C.POINTER(vp)]
    L.vhr_destroy.argtypes = [vp]
    L.vhr_destroy.restype = None
    L.vhr_last_error.argtypes = [vp]
    L.vhr_last_error.restype = C.c_char_p
    L.vhr_synchronize.argtypes = [vp]
    L.vhr_resize.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.vhr_version.restype = C.c_char_p
    L.vhr_abi_struct_sizes.argtypes = [C.POINTER(u32)]
    L.vhr_default_trace_params.argtypes = [vp]
    L.vhr_default_trace_params.restype = None
    L.vhr_update_geometry.argtypes = [vp, vp, u32, vp, u32, vp, u32]
    L.vhr_upload_texture_from_data.argtypes = [vp, u32, u32, vp, i32, vp]
    L.vhr_upload_new_storage_image.argtypes = [vp, u32, u32, i32]
    L.vhr_destroy_storage_image.argtypes = [vp, i32]
    L.vhr_update_per_frame_ubo.argtypes = [vp, u32, vp]
    L.vhr_set_trace_params.argtypes = [vp, vp]
    L.vhr_graph_destroy_resources.argtypes = [vp]
    L.vhr_graph_add_graphics_pass.argtypes = [vp, C.c_char_p, C.POINTER(TransientResource), u32,
                                              C.POINTER(TransientResource), u32, EXTERNAL_CB, vp]
    L.vhr_graph_add_raytracing_pass.argtypes = [vp, C.c_char_p, C.POINTER(TransientResource), u32,
                                                C.POINTER(TransientResource), u32,
                                                C.POINTER(RaytracingPipelineDescription), RAYTRACING_CB, vp]
    L.vhr_graph_add_compute_pass.argtypes = [vp, C.c_char_p, C.POINTER(TransientResource), u32,
                                             C.POINTER(TransientResource), u32, C.POINTER(ComputePipelineDescription),
                                             COMPUTE_CB, vp]
    L.vhr_graph_build.argtypes = [vp]
    L.vhr_graph_execute.argtypes = [vp, u32, u32]
    L.vhr_graph_gather_performance_statistics.argtypes = [vp]
    L.vhr_graph_get_pass_time_ms.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vhr_graph_get_execution_order.argtypes = [vp, C.c_char_p, u32]
    L.vhr_graph_contains_image.argtypes = [vp, C.c_char_p]
    L.vhr_graph_get_image_format.argtypes = [vp, C.c_char_p]
    L.vhr_graph_set_pass_epilogue.argtypes = [vp, C.c_char_p, EXTERNAL_CB, vp]
    L.vhr_graph_bind_external_image.argtypes = [vp, C.c_char_p, vp]
    L.vhr_trace_rays.argtypes = [vp, u32, u32]
    L.vhr_compute_get_display_size.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.vhr_compute_dispatch.argtypes = [vp, C.c_char_p, u32, u32, u32, vp, u32]
    L.vhr_compute_blit_image_storage_to_transient.argtypes = [vp, i32, C.c_char_p]
    L.vhr_compute_blit_image_transient_to_storage.argtypes = [vp, C.c_char_p, i32]
    L.vhr_compute_blit_image_storage_to_storage.argtypes = [vp, i32, i32]
    for prefix in PATH_PREFIXES:         # what every render path's C entry points share (csrc/path_handle.hpp); create / rebuild differ and follow
        getattr(L, f"vhr_{prefix}_destroy").argtypes = [vp]
        getattr(L, f"vhr_{prefix}_destroy").restype = None
        getattr(L, f"vhr_{prefix}_build").argtypes = [vp]
        getattr(L, f"vhr_{prefix}_last_error").argtypes = [vp]
        getattr(L, f"vhr_{prefix}_last_error").restype = C.c_char_p
    L.vhr_hybrid_create.argtypes = [vp, C.POINTER(HybridSettings), EXTERNAL_CB, vp, EXTERNAL_CB, vp, C.POINTER(vp)]
    L.vhr_hybrid_rebuild.argtypes = [vp, C.POINTER(HybridSettings)]
    L.vhr_hybrid_get_push_constants.argtypes = [vp, vp]
    L.vhr_hybrid_state_size.argtypes = [vp, C.POINTER(u64)]
    L.vhr_hybrid_save_state.argtypes = [vp, vp, u64]
    L.vhr_hybrid_load_state.argtypes = [vp, vp, u64, vp]
    L.vhr_get_last_per_frame_ubo.argtypes = [vp, vp]
    L.vhr_get_display_size.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.vhr_get_transient_image.argtypes = [vp, C.c_char_p, C.POINTER(ImageInfo)]
    L.vhr_get_storage_image.argtypes = [vp, i32, C.POINTER(ImageInfo)]
    L.vhr_upload_transient_image.argtypes = [vp, C.c_char_p, vp, u64]
    L.vhr_download_transient_image.argtypes = [vp, C.c_char_p, vp, u64]
    L.vhr_upload_storage_image.argtypes = [vp, i32, vp, u64]
    L.vhr_download_storage_image.argtypes = [vp, i32, vp, u64]
    L.vhr_standin_gbuffer.argtypes = [vp, u32, C.c_char_p, C.c_char_p, C.c_char_p]
    L.vhr_standin_gbuffer_with_albedo.argtypes = [vp, u32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    L.vhr_standin_composition.argtypes = [vp, u32, C.POINTER(CompositionDesc)]
    L.vhr_standin_raytraced_composition.argtypes = [vp, C.c_char_p, i32]
    L.vhr_standin_shadow_map.argtypes = [vp, u32, C.c_char_p]
    L.vhr_raytraced_create.argtypes = [vp, i32, EXTERNAL_CB, vp, C.POINTER(vp)]
    L.vhr_raytraced_rebuild.argtypes = [vp, i32]
    L.vhr_standin_rayquery_forward.argtypes = [vp, u32, C.POINTER(RayqueryForwardDesc)]
    L.vhr_rayquery_create.argtypes = [vp, EXTERNAL_CB, vp, C.POINTER(vp)]
    L.vhr_rayquery_rebuild.argtypes = [vp]
    L.vhr_standin_forward_raster.argtypes = [vp, u32, C.POINTER(ForwardRasterDesc)]
    L.vhr_forward_raster_create.argtypes = [vp, EXTERNAL_CB, vp, EXTERNAL_CB, vp, i32, C.POINTER(vp)]
    L.vhr_forward_raster_rebuild.argtypes = [vp, i32]
    L.vhr_get_transient_image_samples.argtypes = [vp, C.c_char_p, C.POINTER(u32)]
    L.vhr_set_strip.argtypes = [vp, u32, u32, u32, u32]
    L.vhr_set_tile.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32]
    L.vhr_set_ray_statistics.argtypes = [vp, i32]
    L.vhr_get_ray_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_bvh_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_bvh_form_checks.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_current_stream.argtypes = [vp, C.POINTER(C.c_void_p)]
    L.vhr_get_bvh_builder.argtypes = [vp, C.POINTER(i32)]
    L.vhr_get_bvh_presplit_level.argtypes = [vp, C.POINTER(i32)]
    L.vhr_get_bvh_frame.argtypes = [vp, C.POINTER(C.c_float)]
    L.vhr_get_bvh_fingerprint.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_bvh_tree_fingerprint.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_bvh_forms_fingerprint.argtypes = [vp, C.POINTER(u64)]
    L.vhr_set_option.argtypes = [vp, C.c_char_p, i32]
    L.vhr_get_traversal_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_traversal_cycles.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_reflection_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_binary64_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_debug_ray_triangle.argtypes = [vp, C.c_void_p, u32, C.c_void_p, C.c_void_p]
    L.vhr_debug_wave_lifetimes.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(u32)]
    L.vhr_source_fingerprint.restype = C.c_char_p
    L.vhr_source_fingerprint.argtypes = []
    L.vhr_get_drain_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i32)]
    L.vhr_option_count.restype = i32
    L.vhr_option_count.argtypes = []
    L.vhr_option_info.argtypes = [i32, C.POINTER(C.c_char_p), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.vhr_get_build_times.argtypes = [vp, C.POINTER(C.c_double)]
    L.vhr_atrous_overlap.restype = u32
    L.vhr_atrous_overlap.argtypes = [u32]
    L.vhr_atrous_output_extent.restype = u32
    L.vhr_atrous_output_extent.argtypes = [u32, u32]
    L.vhr_strip_plan_make.argtypes = [u32, u32, u32, u32, u32, C.POINTER(StripPlanC)]
    L.vhr_strip_plan_exchanges.argtypes = [C.POINTER(StripPlanC), u32, C.POINTER(RowExchangeC)]
    L.vhr_tile_grid_choose.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.vhr_tile_plan_make.argtypes = [u32, u32, u32, u32, u32, u32, u32, u32, u32, C.POINTER(TilePlanC)]
    L.vhr_tile_plan_make_weighted.argtypes = [u32, u32, u32, u32, u32, u32, u32, u32, u32, vp, u32, u32, u32, C.POINTER(TilePlanC)]
    L.vhr_tile_plan_exchanges.argtypes = [C.POINTER(TilePlanC), u32, u32, C.POINTER(RectExchangeC), u32]
    L.vhr_tile_plan_replan.argtypes = [C.POINTER(TilePlanC), C.POINTER(TilePlanC), C.POINTER(RectExchangeC), u32]
    L.vhr_comm_create_tiled.argtypes = [vp, C.POINTER(TilePlanC), C.c_char_p, C.POINTER(vp)]
    L.vhr_get_tile_cost_map.argtypes = [vp, vp, u32, u32]
    L.vhr_comm_use_library.argtypes = [C.c_char_p]
    L.vhr_comm_library.restype = C.c_char_p
    L.vhr_comm_get_unique_id.argtypes = [C.c_char_p]
    L.vhr_comm_create.argtypes = [vp, C.POINTER(StripPlanC), C.c_char_p, C.POINTER(vp)]
    L.vhr_comm_destroy.argtypes = [vp]
    L.vhr_comm_destroy.restype = None
    L.vhr_comm_last_error.argtypes = [vp]
    L.vhr_comm_last_error.restype = C.c_char_p
    L.vhr_comm_exchange_raytraced.argtypes = [vp, C.c_char_p]
    L.vhr_comm_start_frame_exchanges.argtypes = [vp, i32, i32, C.c_char_p, i32, vp]
    L.vhr_comm_finish_frame_exchanges.argtypes = [vp]
    L.vhr_comm_replan.argtypes = [vp, C.POINTER(TilePlanC), i32, i32, i32]
    L.vhr_calibration_stream_read.argtypes = [vp, i32, u32]
    L.vhr_ray_query.argtypes = [vp, vp, u32, u32, vp]
    L.vhr_ray_query_masked.argtypes = [vp, vp, u32, u32, u32, vp, vp]
    L.vhr_ray_query_faces.argtypes = [vp, vp, u32, u32, u32, vp, u32, vp]
    L.vhr_get_primitive_facing_flips.argtypes = [vp, u32, u32, vp]
    L.vhr_get_face_cull_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_debug_ray_facing.argtypes = [vp, C.c_void_p, C.c_void_p, u32, C.c_void_p]
    L.vhr_set_primitive_masks.argtypes = [vp, u32, u32, vp]
    L.vhr_get_primitive_masks.argtypes = [vp, u32, u32, vp]
    L.vhr_get_ray_mask_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_ray_query_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_ray_query_struct_layout.argtypes = [C.POINTER(u32)]
    L.vhr_closest_point_query.argtypes = [vp, vp, u32, u32, u32, vp]
    L.vhr_get_point_query_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_nearest_points_query.argtypes = [vp, vp, u32, u32, u32, u32, vp]
    L.vhr_get_nearest_query_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_debug_point_triangle.argtypes = [vp, C.c_void_p, u32, C.c_void_p]
    L.vhr_resolve_hits.argtypes = [vp, vp, u32, u32, vp]
    L.vhr_get_surface_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_occlusion_query.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp]
    L.vhr_get_occlusion_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_debug_occlusion_rays.argtypes = [vp, vp, u32, u32, u32, vp]
    L.vhr_surface_point_layout.argtypes = [C.POINTER(u32)]
    L.vhr_update_vertices.argtypes = [vp, u32, u32, vp, u32]
    L.vhr_update_primitive_transforms.argtypes = [vp, u32, u32, vp]
    L.vhr_refit_geometry.argtypes = [vp]
    L.vhr_get_refit_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_refit_times.argtypes = [vp, C.POINTER(C.c_double)]
    L.vhr_get_bvh_sah_cost.argtypes = [vp, C.POINTER(C.c_double)]
    L.vhr_refit_geometry_partial.argtypes = [vp, u32]
    L.vhr_get_partial_refit_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_get_object_motion_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_rebuild_geometry.argtypes = [vp, u32]
    L.vhr_get_rebuild_statistics.argtypes = [vp, C.POINTER(u64)]
    L.vhr_debug_triangle_records.argtypes = [vp, i32, C.c_void_p, u32, C.POINTER(u32)]
    L.vhr_debug_bvh_arrays.argtypes = [vp, C.POINTER(u32)] + [C.c_void_p] * 5 + [u32, u32, C.POINTER(u32)]
    L.vhr_set_kernel_timing.argtypes = [vp, i32]
    L.vhr_get_kernel_time.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(u64), i32]
    _lib = L
    return L


# image / resource names of the hybrid path (hybrid_render_path.cpp:16-19,104-111,265-273)
NORMALS = "World Space Normals and Object IDs"
MOTION = "Motion Vectors and Metallic Roughness"
DEPTH = "Depth"
RAYTRACED = "Raytraced Shadows and Ambient Occlusion"
REFLECTIONS = "Raytraced Reflections"
DENOISED = "Denoised Raytraced Shadows and Ambient Occlusion"
ALBEDO = "Albedo"
SVGF_SHADER = "hybrid_render_path/svgf.comp"
ATROUS_SHADER = "hybrid_render_path/svgf_atrous_filter.comp"
RAYTRACED_OUTPUT = "RaytracedOutput"        # raytraced_render_path.cpp:15
SHADOW_MAP = "Shadow Map"                           # hybrid_render_path.cpp:62
SSAO_RAW = "Screen Space Ambient Occlusion Raw"     # hybrid_render_path.cpp:149
SSAO = "Screen Space Ambient Occlusion"             # :176
SSR = "Screen Space Reflections"                    # :219
SSAO_SHADER = "hybrid_render_path/ssao.comp"
SSAO_BLUR_SHADER = "hybrid_render_path/ssao_blur.comp"
SSR_SHADER = "hybrid_render_path/ssr.comp"

ATTACHMENT_IMAGE, SAMPLED_IMAGE, STORAGE_IMAGE = 0, 1, 2
UPDATE_DEVICE_MEMORY = 2          # vhr_update_vertices: VHR_UPDATE_DEVICE_MEMORY
REFIT_FORCE_PARTIAL = 1           # vhr_refit_geometry_partial: VHR_REFIT_FORCE_PARTIAL


def transient(name, fmt, binding, kind=STORAGE_IMAGE, width=0, height=0, clear=(0, 0, 0, 0)):
    """VkUtils::CreateTransient{Attachment,Sampled,Storage}Image (vulkan_utils.h:363-453)."""
    r = TransientResource()
    r.type = 0
    r.name = name.encode()
    r.image.type = kind
    r.image.width, r.image.height = width, height
    r.image.format = fmt
    r.image.binding = binding
    r.image.clear_value = (C.c_float * 4)(*clear)
    return r


def render_output(binding=0):
    return transient("RENDER_OUTPUT", 0, binding, ATTACHMENT_IMAGE)


_NP_FORMATS = {abi.FORMAT_R16G16B16A16_SFLOAT: (np.uint16, 4), abi.FORMAT_R16G16_SFLOAT: (np.uint16, 2),
               abi.FORMAT_D32_SFLOAT: (np.float32, 1), abi.FORMAT_B8G8R8A8_UNORM: (np.uint8, 4),
               abi.FORMAT_R8G8B8A8_UNORM: (np.uint8, 4), abi.FORMAT_R8G8B8A8_SRGB: (np.uint8, 4),
               abi.FORMAT_B8G8R8A8_SRGB: (np.uint8, 4)}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """vhr_context: device + ResourceManager + RenderGraph state for one GPU."""

    def __init__(self, width, height, device=0, stream=None, host_only=False, internal_stream=False):
        """stream: a hipStream_t handle used as given (None / 0 = the device's default stream)."""
        self.L = load()
        self.handle = C.c_void_p()
        info = CreateInfo(device, width, height, stream, (1 if host_only else 0) | (2 if internal_stream else 0))
        rc = self.L.vhr_create(C.byref(info), C.byref(self.handle))
        if rc < 0:
            self.handle = None
            raise VhrError("vhr_create: " + self.L.vhr_last_error(None).decode())
        self.width, self.height = width, height
        self._keep = []        # callbacks and strings the C side points at
        self._callback_error = None

    def close(self):
        if getattr(self, "handle", None):
            self.L.vhr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what):
        if rc < 0:
            raise VhrError(f"{what}: {self.L.vhr_last_error(self.handle).decode()}")
        return rc

    def _read(self, name, n, what=None, ctype=C.c_uint64):
        """The `n` uint64 (or `ctype`) values vhr_get_<name> fills in, as a list; `what` labels a failure (default: name)."""
        out = (ctype * n)()
        self.check(getattr(self.L, "vhr_get_" + name)(self.handle, out), what or name)
        return list(out)

    def synchronize(self):
        self.check(self.L.vhr_synchronize(self.handle), "synchronize")

    def display_size(self):
        w, h = C.c_uint32(), C.c_uint32()
        self.check(self.L.vhr_get_display_size(self.handle, C.byref(w), C.byref(h)), "display_size")
        return int(w.value), int(h.value)

    def resize(self, width, height):
        """VulkanContext::Resize (renderer.cpp:113-118): the new display extent; the graph and the storage pool's images are released, geometry, the
        acceleration structure, textures and options stay.  Follow with the render path's build()."""
        self.check(self.L.vhr_resize(self.handle, int(width), int(height)), "resize")
        self.width, self.height = int(width), int(height)

    # ---- ResourceManager ----
    def update_geometry(self, vertices, indices, primitives):
        v = np.ascontiguousarray(vertices)
        i = np.ascontiguousarray(indices, np.uint32)
        p = np.ascontiguousarray(primitives)
        assert v.dtype == abi.vertex_dtype and p.dtype == abi.primitive_dtype
        self.check(self.L.vhr_update_geometry(self.handle, _p(v), len(v), _p(i), len(i), _p(p), len(p)), "UpdateGeometry")
        self._primitive_count = len(p)

    # ---- refit: geometry that moves without a rebuild ----
    def update_vertices(self, vertices, first_vertex=0):
        """vhr_update_vertices from a host array (abi.vertex_dtype): overwrites vertices [first_vertex, first_vertex + len).  Follow with refit_geometry()."""
        v = np.ascontiguousarray(vertices)
        assert v.dtype == abi.vertex_dtype
        self.check(self.L.vhr_update_vertices(self.handle, int(first_vertex), len(v), _p(v) if len(v) else None, 0), "update_vertices")

    def update_vertices_device(self, vertices_ptr, count, first_vertex=0):
        """vhr_update_vertices from device memory (e.g. a torch tensor's data_ptr()): `count` vhr_vertex records, copied on the context's stream."""
        self.check(self.L.vhr_update_vertices(self.handle, int(first_vertex), int(count), vertices_ptr or None, UPDATE_DEVICE_MEMORY), "update_vertices_device")

    def update_primitive_transforms(self, transforms, first_primitive=0):
        """vhr_update_primitive_transforms: (n, 16) float32, the layout of vhr_primitive::transform (scene.primitives["transform"])."""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
        self.check(self.L.vhr_update_primitive_transforms(self.handle, int(first_primitive), len(t), _p(t) if len(t) else None), "update_primitive_transforms")

    # ---- ray cull masks: per-primitive visibility for rays and ray queries ----
    def set_primitive_masks(self, masks, first_primitive=0):
        """vhr_set_primitive_masks: uint8 per primitive from first_primitive on (0xFF after update_geometry).  A candidate hit on primitive p
        does not exist for a ray of mask m iff (masks[p] & m) == 0.  No refit is needed; takes effect at the next launch."""
        m = np.ascontiguousarray(masks, np.uint8).reshape(-1)
        self.check(self.L.vhr_set_primitive_masks(self.handle, int(first_primitive), len(m), _p(m) if len(m) else None), "set_primitive_masks")

    def primitive_masks(self, first_primitive=0, count=None):
        """vhr_get_primitive_masks: the masks of `count` primitives from first_primitive on (default: all that follow) as uint8."""
        n = getattr(self, "_primitive_count", 0) - int(first_primitive) if count is None else int(count)
        out = np.zeros(max(n, 0), np.uint8)
        self.check(self.L.vhr_get_primitive_masks(self.handle, int(first_primitive), len(out), _p(out) if len(out) else None), "primitive_masks")
        return out

    def ray_mask_statistics(self):
        """[primitives whose mask is not 0xFF, launches of the last trace_rays that ran a mask instantiation (0..2), 1 if the last ray
        query ran one, 0]."""
        return self._read("ray_mask_statistics", 4)

    # ---- ray face culling: the primitives' facing flips (the query itself: ray_query(face_cull=...)) ----
    def primitive_facing_flips(self, first_primitive=0, count=None):
        """vhr_get_primitive_facing_flips: uint8 per primitive from first_primitive on (default: all that follow), 1 = the primitive's
        transform mirrors (a negative determinant of its upper 3 x 3), so its triangles' facing is the reverse of their world-space winding."""
        n = getattr(self, "_primitive_count", 0) - int(first_primitive) if count is None else int(count)
        out = np.zeros(max(n, 0), np.uint8)
        self.check(self.L.vhr_get_primitive_facing_flips(self.handle, int(first_primitive), len(out), _p(out) if len(out) else None), "primitive_facing_flips")
        return out

    def face_cull_statistics(self):
        """[primitives with flip = 1, 1 if the last ray query of any kind launched the face instantiation, 0, 0]."""
        return self._read("face_cull_statistics", 4)

    def debug_ray_facing(self, pairs, flips=None):
        """The facing function on explicit pairs: pairs = (n, 9) float32 (d, e1, e2), flips = uint8[n] or None (all 0) -> uint8[n],
        abi.HIT_KIND_FRONT_FACING or abi.HIT_KIND_BACK_FACING.  A device context runs the device's copy, a host-only context the host's."""
        pairs = np.ascontiguousarray(pairs, dtype=np.float32).reshape(-1, 9)
        n = len(pairs)
        f = None
        if flips is not None:
            f = np.ascontiguousarray(flips, np.uint8).reshape(-1)
            if len(f) != n:
                raise ValueError(f"debug_ray_facing: {len(f)} flips for {n} pairs")
        out = np.zeros(n, np.uint8)
        self.check(self.L.vhr_debug_ray_facing(self.handle, pairs.ctypes.data if n else None, f.ctypes.data if f is not None and n else None, n,
                                               out.ctypes.data if n else None), "debug_ray_facing")
        return out

    def refit_geometry(self):
        self.check(self.L.vhr_refit_geometry(self.handle), "refit_geometry")

    def refit_geometry_partial(self, force=False):
        """vhr_refit_geometry_partial: only the records the pending updates' ranges touch and their leaves' ancestors; the same arrays as
        refit_geometry().  force=True: the dirty path whatever the dirty share (the first refit after a build is whole-tree regardless)."""
        self.check(self.L.vhr_refit_geometry_partial(self.handle, REFIT_FORCE_PARTIAL if force else 0), "refit_geometry_partial")

    def rebuild_geometry(self, flags=0):
        """vhr_rebuild_geometry: a new tree, built with the options as they are set now, over the arrays the context holds -- pending updates
        included.  Masks, options, frame state and (with "object_motion_vectors") last frame's records are kept; nothing is re-uploaded."""
        self.check(self.L.vhr_rebuild_geometry(self.handle, int(flags)), "rebuild_geometry")

    def rebuild_statistics(self):
        """vhr_get_rebuild_statistics: (successful rebuilds since update_geometry, 1 if the last fetched the scene for the host builder,
        non-finite coordinates the last call met, records whose previous differs from current after it, 0, 0, 0, 0)."""
        return tuple(self._read("rebuild_statistics", 8))

    def partial_refit_statistics(self):
        return dict(zip(("partial_refits", "dirty_records", "dirty_nodes", "forms_rewritten", "ran_as", "centre_moved", "vertex_ranges", "primitive_ranges"),
                        self._read("partial_refit_statistics", 8)))

    def object_motion_statistics(self):
        """"object_motion_vectors": whether the previous records exist, how many differ from the current ones after the last successful refit,
        and the G-buffer launches that ran the motion instantiation since the context was created."""
        return dict(zip(("active", "differing_records", "motion_launches"), self._read("object_motion_statistics", 4)))

    def triangle_records(self, previous=False):
        """vhr_debug_triangle_records: (n, 9) float32, (v0, e1, e2) of every triangle in flat (primitive-major) order; previous=True: the
        records before the last refit ("object_motion_vectors" 1)."""
        n = C.c_uint32(0)
        rc = self.L.vhr_debug_triangle_records(self.handle, 1 if previous else 0, None, 0, C.byref(n))  # the count: "too small" unless the scene is empty
        if rc != -1 or n.value == 0:                      # a refusal (no geometry, a presplit tree, no previous records) surfaces here
            self.check(rc, "triangle_records")
        out = np.zeros((n.value, 9), np.float32)
        self.check(self.L.vhr_debug_triangle_records(self.handle, 1 if previous else 0, out.ctypes.data, n.value, C.byref(n)), "triangle_records")
        return out

    def bvh_arrays(self):
        """vhr_debug_bvh_arrays: the tree as the walkers read it -- the raw bytes of the four node forms ((n, 64), (n, 64), (n, 48), (n, 32)
        uint8) and of the leaf records in slot order ((m, 48) uint8), with the header's fields.  The library interprets none of it here."""
        counts, header = (C.c_uint32 * 2)(), (C.c_uint32 * 24)()
        rc = self.L.vhr_debug_bvh_arrays(self.handle, header, None, None, None, None, None, 0, 0, counts)      # the counts: "too small" while there is a tree
        if rc != -1 or counts[0] == 0:
            self.check(rc, "bvh_arrays")
        n, m = int(counts[0]), int(counts[1])
        out = {"nodes": np.zeros((n, 64), np.uint8), "nodes_ch": np.zeros((n, 64), np.uint8), "nodes48": np.zeros((n, 48), np.uint8),
               "nodes16": np.zeros((n, 32), np.uint8), "records": np.zeros((m, 48), np.uint8)}
        self.check(self.L.vhr_debug_bvh_arrays(self.handle, header, *[out[k].ctypes.data for k in ("nodes", "nodes_ch", "nodes48", "nodes16", "records")], n, m, counts),
                   "bvh_arrays")
        words = np.array(list(header), np.uint32)
        out.update(centre=words[0:3].view(np.float32).copy(), frame=words[3:12].view(np.float32).copy(), frame_on=bool(words[12]), half_nodes=bool(words[13]),
                   node_count=int(words[14]), record_count=int(words[15]), depth=int(words[16]), frame_magnitude=float(words[17:18].view(np.float32)[0]))
        return out

    def refit_statistics(self):
        return dict(zip(("refits", "records", "nodes", "records_outside", "children_outside", "non_finite", "half_nodes", "upward_launches"),
                        self._read("refit_statistics", 8)))

    def refit_times_ms(self):
        """(host wall time, leaf pass, upward pass, forms + checks) of the last refit; the device times need set_kernel_timing(False, refit=True)."""
        return tuple(self._read("refit_times", 4, ctype=C.c_double))

    def bvh_sah_cost(self):
        """(as built, now): the tree's surface-area cost, the number to watch when deciding to rebuild."""
        return tuple(self._read("bvh_sah_cost", 2, ctype=C.c_double))

    def upload_scene(self, scene):
        for t in scene.textures:
            self.upload_texture_from_data(t["rgba8"], t["format"], (t["mag"], t["min"], t["address_u"], t["address_v"]))
        self.update_geometry(scene.vertices, scene.indices, scene.primitives)

    def upload_texture_from_data(self, rgba8, fmt=abi.FORMAT_R8G8B8A8_UNORM, sampler=None):
        img = np.ascontiguousarray(rgba8, np.uint8)
        s = (C.c_int32 * 4)(*sampler) if sampler is not None else None
        return self.check(self.L.vhr_upload_texture_from_data(self.handle, img.shape[1], img.shape[0], _p(img), fmt, s),
                          "UploadTextureFromData")

    def upload_new_storage_image(self, width, height, fmt):
        r = self.L.vhr_upload_new_storage_image(self.handle, width, height, fmt)
        if r < -1:        # -1 = the reference's "pool exhausted" sentinel, returned as is; every failure is below it
            self.check(r, "UploadNewStorageImage")
        return r

    def destroy_storage_image(self, idx):
        self.check(self.L.vhr_destroy_storage_image(self.handle, idx), "DestroyStorageImage")

    def update_per_frame_ubo(self, resource_idx, pfd):
        a = np.ascontiguousarray(pfd)
        assert a.dtype == abi.per_frame_dtype
        self.check(self.L.vhr_update_per_frame_ubo(self.handle, resource_idx, _p(a)), "UpdatePerFrameUBO")

    def set_trace_params(self, tp):
        a = np.ascontiguousarray(tp)
        assert a.dtype == abi.trace_params_dtype
        self.check(self.L.vhr_set_trace_params(self.handle, _p(a)), "set_trace_params")

    def set_strip(self, row_begin, row_end, overlap=0, halo=None):
        halo = overlap if halo is None else halo
        self.check(self.L.vhr_set_strip(self.handle, row_begin, row_end, overlap, halo), "set_strip")

    def set_tile(self, col_begin, col_end, row_begin, row_end, overlap=0, halo_rows=None, halo_cols=None):
        halo_rows = overlap if halo_rows is None else halo_rows
        halo_cols = overlap if halo_cols is None else halo_cols
        self.check(self.L.vhr_set_tile(self.handle, col_begin, col_end, row_begin, row_end, overlap, halo_rows, halo_cols), "set_tile")

    # ---- RenderGraph ----
    def destroy_resources(self):
        self.check(self.L.vhr_graph_destroy_resources(self.handle), "DestroyResources")
        self._keep.clear()

    @staticmethod
    def _resources(lst):
        arr = (TransientResource * max(1, len(lst)))(*lst)
        return arr, len(lst)

    def add_graphics_pass(self, name, dependencies, outputs, callback=None):
        cb = EXTERNAL_CB(lambda user, ctx: self._guard(lambda: callback(self))) if callback else EXTERNAL_CB()
        d, nd = self._resources(dependencies)
        o, no = self._resources(outputs)
        self._keep += [cb, d, o, dependencies, outputs]
        self.check(self.L.vhr_graph_add_graphics_pass(self.handle, name.encode(), d, nd, o, no, cb, None), "AddGraphicsPass")

    def add_raytracing_pass(self, name, dependencies, outputs, callback, raygen="hybrid_render_path/raygen.rgen",
                            miss=("hybrid_render_path/miss.rmiss", "hybrid_render_path/reflection_miss.rmiss"),
                            closest_hit=("hybrid_render_path/reflection_hit.rchit",), pipeline_name="Raytrace Pipeline", any_hit=None):
        cb = RAYTRACING_CB(lambda user, exec_: self._guard(lambda: callback(RaytracingExecutionContext(self, exec_))))
        d, nd = self._resources(dependencies)
        o, no = self._resources(outputs)
        miss_arr = (C.c_char_p * len(miss))(*[m.encode() for m in miss])
        any_hit = any_hit or (None,) * len(closest_hit)
        hits = (HitShader * len(closest_hit))(*[HitShader(h.encode(), ah.encode() if ah else None) for h, ah in zip(closest_hit, any_hit)])
        desc = RaytracingPipelineDescription(pipeline_name.encode(), raygen.encode(), miss_arr, len(miss), hits, len(closest_hit))
        self._keep += [cb, d, o, dependencies, outputs, miss_arr, hits, desc]
        self.check(self.L.vhr_graph_add_raytracing_pass(self.handle, name.encode(), d, nd, o, no, C.byref(desc), cb, None),
                   "AddRaytracingPass")

    def add_compute_pass(self, name, dependencies, outputs, kernels, push_constant_size, callback):
        cb = COMPUTE_CB(lambda user, exec_: self._guard(lambda: callback(ComputeExecutionContext(self, exec_))))
        d, nd = self._resources(dependencies)
        o, no = self._resources(outputs)
        k = (C.c_char_p * len(kernels))(*[s.encode() for s in kernels])
        desc = ComputePipelineDescription(k, len(kernels), push_constant_size)
        self._keep += [cb, d, o, dependencies, outputs, k, desc]
        self.check(self.L.vhr_graph_add_compute_pass(self.handle, name.encode(), d, nd, o, no, C.byref(desc), cb, None),
                   "AddComputePass")

    def set_pass_epilogue(self, name, callback):
        cb = EXTERNAL_CB(lambda user, ctx: self._guard(lambda: callback(self))) if callback else EXTERNAL_CB()
        self._keep.append(cb)
        self.check(self.L.vhr_graph_set_pass_epilogue(self.handle, name.encode(), cb, None), "set_pass_epilogue")

    def build(self):
        self.check(self.L.vhr_graph_build(self.handle), "Build")

    def execute(self, resource_idx=0, image_idx=0):
        self._callback_error = None
        rc = self.L.vhr_graph_execute(self.handle, resource_idx, image_idx)
        if self._callback_error is not None:
            raise self._callback_error
        self.check(rc, "Execute")

    def gather_performance_statistics(self):
        self.check(self.L.vhr_graph_gather_performance_statistics(self.handle), "GatherPerformanceStatistics")

    def pass_time_ms(self, name):
        ema, last = C.c_double(), C.c_double()
        self.check(self.L.vhr_graph_get_pass_time_ms(self.handle, name.encode(), C.byref(ema), C.byref(last)), "pass_time_ms")
        return ema.value, last.value

    def execution_order(self):
        buf = C.create_string_buffer(4096)
        n = self.check(self.L.vhr_graph_get_execution_order(self.handle, buf, 4096), "execution_order")
        return buf.value.decode().split("\n") if n else []

    def contains_image(self, name):
        return bool(self.L.vhr_graph_contains_image(self.handle, name.encode()))

    def image_format(self, name):
        return self.L.vhr_graph_get_image_format(self.handle, name.encode())

    def bind_external_image(self, name, device_ptr):
        self.check(self.L.vhr_graph_bind_external_image(self.handle, name.encode(), device_ptr), "bind_external_image")

    # ---- harness access ----
    def transient_info(self, name):
        info = ImageInfo()
        self.check(self.L.vhr_get_transient_image(self.handle, name.encode(), C.byref(info)), "get_transient_image")
        return info

    def storage_info(self, idx):
        info = ImageInfo()
        self.check(self.L.vhr_get_storage_image(self.handle, idx, C.byref(info)), "get_storage_image")
        return info

    def transient_samples(self, name):
        """vhr_get_transient_image_samples: 1, or 8 for a multisampled transient image."""
        n = C.c_uint32()
        self.check(self.L.vhr_get_transient_image_samples(self.handle, name.encode(), C.byref(n)), "get_transient_image_samples")
        return int(n.value)

    @staticmethod
    def _host_array(info):
        """(H, W[, C]); a multisampled image (bytes_per_pixel covers all its samples) gets a samples axis: (H, W, S[, C])."""
        dt, ch = _NP_FORMATS[info.format]
        samples = info.bytes_per_pixel // (np.dtype(dt).itemsize * ch)
        shape = (info.height, info.width) + ((samples,) if samples > 1 else ()) + ((ch,) if ch > 1 else ())
        return np.zeros(shape, dt)

    def download(self, name_or_idx):
        if isinstance(name_or_idx, str):
            info = self.transient_info(name_or_idx)
            out = self._host_array(info)
            self.check(self.L.vhr_download_transient_image(self.handle, name_or_idx.encode(), _p(out), out.nbytes), "download")
        else:
            info = self.storage_info(name_or_idx)
            out = self._host_array(info)
            self.check(self.L.vhr_download_storage_image(self.handle, name_or_idx, _p(out), out.nbytes), "download")
        return out

    def upload(self, name_or_idx, array):
        a = np.ascontiguousarray(array)
        if isinstance(name_or_idx, str):
            self.check(self.L.vhr_upload_transient_image(self.handle, name_or_idx.encode(), _p(a), a.nbytes), "upload")
        else:
            self.check(self.L.vhr_upload_storage_image(self.handle, name_or_idx, _p(a), a.nbytes), "upload")

    def standin_gbuffer(self, resource_idx=0, normals=NORMALS, motion=MOTION, depth=DEPTH):
        self.check(self.L.vhr_standin_gbuffer(self.handle, resource_idx, normals.encode(), motion.encode(), depth.encode()),
                   "standin_gbuffer")

    def standin_gbuffer_with_albedo(self, resource_idx=0, albedo=ALBEDO, normals=NORMALS, motion=MOTION, depth=DEPTH):
        self.check(self.L.vhr_standin_gbuffer_with_albedo(self.handle, resource_idx, albedo.encode(), normals.encode(), motion.encode(),
                                                          depth.encode()), "standin_gbuffer_with_albedo")

    def standin_composition(self, output_storage_image, shadow_mode=0, ao_mode=0, reflection_mode=0, shadow_ao=DENOISED,
                            reflections=REFLECTIONS, resource_idx=0, ssao=None, shadow_map=None):
        """composition.frag stand-in.  ao_mode 1 reads `ssao` (default SSAO), reflection_mode 1 expects `reflections` = SSR."""
        if ao_mode == 1 and ssao is None:
            ssao = SSAO
        if shadow_mode == 1 and shadow_map is None:
            shadow_map = SHADOW_MAP
        d = CompositionDesc(shadow_mode, ao_mode, reflection_mode, ALBEDO.encode(), NORMALS.encode(), MOTION.encode(), DEPTH.encode(),
                            shadow_ao.encode(), reflections.encode() if reflections else None, output_storage_image,
                            ssao.encode() if ssao else None, shadow_map.encode() if shadow_map else None)
        self.check(self.L.vhr_standin_composition(self.handle, resource_idx, C.byref(d)), "standin_composition")

    def standin_shadow_map(self, resource_idx=0, shadow_map=SHADOW_MAP):
        self.check(self.L.vhr_standin_shadow_map(self.handle, resource_idx, shadow_map.encode()), "standin_shadow_map")

    def standin_raytraced_composition(self, output_storage_image, raytraced_output=RAYTRACED_OUTPUT):
        self.check(self.L.vhr_standin_raytraced_composition(self.handle, raytraced_output.encode(), output_storage_image),
                   "standin_raytraced_composition")

    def standin_rayquery_forward(self, output_storage_image, resource_idx=0, depth=DEPTH, primary_hits_ptr=0, positions_ptr=0, shadowed_ptr=0):
        """The rayquery path's "Forward Pass" stand-in (default.vert + default.frag with its inline shadow query): swapchain texels into
        the pool storage image, reverse-Z depth into `depth`.  The probes are device pointers (e.g. torch tensors' data_ptr(); 0 = not
        written), one entry per pixel in Depth's row order: abi.ray_hit_dtype, 4 float32 (in_pos, covered), uint8 (shadowed)."""
        d = RayqueryForwardDesc(output_storage_image, depth.encode(), primary_hits_ptr or None, positions_ptr or None, shadowed_ptr or None)
        self.check(self.L.vhr_standin_rayquery_forward(self.handle, resource_idx, C.byref(d)), "standin_rayquery_forward")

    def standin_forward_raster(self, output_storage_image, resource_idx=0, depth=DEPTH, msaa=None, sample_hits_ptr=0, fragments_ptr=0):
        """The forward raster path's "Forward Pass" stand-in (default.vert + forward_raster_render_path/default.frag, 8x MSAA when `depth` has 8
        samples): resolved swapchain texels into the pool storage image, reverse-Z depth per sample into `depth`, the shaded samples into
        `msaa` (the "Forward Pass_MSAA" image; None when `depth` has 1 sample).  The probes are device pointers (0 = not written):
        abi.ray_hit_dtype per sample (pixel-major, samples consecutive) and uint8 fragments shaded per pixel."""
        d = ForwardRasterDesc(output_storage_image, depth.encode(), msaa.encode() if msaa else None, sample_hits_ptr or None, fragments_ptr or None)
        self.check(self.L.vhr_standin_forward_raster(self.handle, resource_idx, C.byref(d)), "standin_forward_raster")

    def set_ray_statistics(self, enable):
        self.check(self.L.vhr_set_ray_statistics(self.handle, int(enable)), "set_ray_statistics")

    def ray_statistics(self):
        return dict(zip(("unique_rays", "reference_issued_rays", "covered_pixels", "stack_overflows"), self._read("ray_statistics", 4)))

    def calibration_stream_read(self, storage_image, bytes_per_lane):
        self.check(self.L.vhr_calibration_stream_read(self.handle, storage_image, bytes_per_lane), "calibration_stream_read")

    def traversal_statistics(self):
        d = dict(zip(("node_visits", "leaf_visits", "triangle_tests", "wave_iterations"), self._read("traversal_statistics", 4)))
        d["active_lane_utilisation"] = (d["node_visits"] + d["triangle_tests"]) / (64.0 * d["wave_iterations"]) if d["wave_iterations"] else 0.0
        return d

    def reflection_statistics(self):
        """The mirror-ray launch's counters (reflection_queue_kernel with statistics enabled)."""
        d = dict(zip(("rays", "second_bounce_rays", "node_visits", "leaf_visits", "triangle_tests", "wave_iterations", "refills", "waves", "cycles_total", "cycles_walk"),
                     self._read("reflection_statistics", 10)))
        d["active_lane_utilisation"] = (d["node_visits"] + d["triangle_tests"]) / (64.0 * d["wave_iterations"]) if d["wave_iterations"] else 0.0
        return d

    def ray_triangle(self, pairs):
        """Decision (vi) as the device computes it, on explicit pairs: pairs = (n, 17) float32 (o, d, v0, e1, e2, tmin, tmax) -> (hit (n,) bool, tuv (n, 3) float32)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.float32).reshape(-1, 17)
        hit = np.zeros(len(pairs), np.uint32)
        tuv = np.zeros((len(pairs), 3), np.float32)
        self.check(self.L.vhr_debug_ray_triangle(self.handle, pairs.ctypes.data, len(pairs), hit.ctypes.data, tuv.ctypes.data), "ray_triangle")
        return hit != 0, tuv

    def binary64_statistics(self):
        """Decision (vi)'s binary64 half in the queue kernels of the last vhr_trace_rays (statistics enabled): pixels the any-hit launch and the mirror
        ray's launch computed again by the per-pixel code."""
        return dict(zip(("pixels_again", "mirror_pixels_again"), self._read("binary64_statistics", 4)))

    def alpha_launches(self):
        """Launches of the last vhr_trace_rays that ran an "alpha_test_rays" instantiation (0 with the switch off, and on a scene none of
        whose primitives can discard): 1 = the shadow / AO launch, 2 = that and the mirror ray's."""
        return self._read("binary64_statistics", 4)[2]

    def wave_lifetimes(self, capacity=1 << 20):
        """Lifetimes (shader clock ticks) of the last ray-tracing launch's waves (what raygen_cost_order sorts by)."""
        out = np.zeros(capacity, dtype=np.uint32)
        n = C.c_uint32(0)
        self.check(self.L.vhr_debug_wave_lifetimes(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32)), capacity, C.byref(n)), "wave_lifetimes")
        return out[:n.value].copy()

    def tile_cost_map(self):
        """vhr_get_tile_cost_map: the last frame's wave lifetimes (any-hit + mirror-ray launch) per 8 x 8-pixel cell, (ceil(H / 8), ceil(W / 8)) uint32."""
        rows, cols = (self.height + 7) // 8, (self.width + 7) // 8
        out = np.zeros((rows, cols), np.uint32)
        self.check(self.L.vhr_get_tile_cost_map(self.handle, out.ctypes.data_as(C.c_void_p), cols, rows), "tile_cost_map")
        return out

    def traversal_cycles(self):
        return dict(zip(("total", "setup", "refill", "nodes", "leaves", "refills", "waves", "drain_iterations"), self._read("traversal_cycles", 8)))

    def bvh_form_checks(self):
        """Host-side self-check of the last build: (boxes checked, CH violations, 48-byte-node violations, compact-node violations)."""
        return tuple(self._read("bvh_form_checks", 4))

    def bvh_frame(self):
        """Option "bvh_frame": the frame the current tree's boxes are in, a 3 x 3 array (row i = axis i in world coordinates; the identity = the world axes)."""
        return np.array(self._read("bvh_frame", 9, "get_bvh_frame", C.c_float), np.float32).reshape(3, 3)

    def bvh_presplit_level(self):
        """Option "bvh_presplit": the grid level the current tree's references were split on, -1 = one reference per triangle."""
        return self._read("bvh_presplit_level", 1, "get_bvh_presplit_level", C.c_int32)[0]

    def bvh_builder_used(self):
        """Which builder made the current tree: 1 = the device's (option "bvh_builder" 1, the default), 0 = the host's."""
        return self._read("bvh_builder", 1, "get_bvh_builder", C.c_int32)[0]

    def bvh_fingerprint(self):
        return self._read("bvh_fingerprint", 1)[0]

    def bvh_tree_fingerprint(self):
        """A hash of the tree, not of its arrays: equal for the host's and the device's build of a scene."""
        return self._read("bvh_tree_fingerprint", 1)[0]

    def bvh_forms_fingerprint(self):
        """(hash of the scene centre and the derived node forms as they stand, the same after the host derives them again from the
        (lo, hi) nodes): equal for any tree, whichever builder made or refitted it."""
        return tuple(self._read("bvh_forms_fingerprint", 2))

    def build_times_ms(self):
        """K0: (host BVH build, upload of scene + tree) of the last upload_scene, milliseconds."""
        return tuple(self._read("build_times", 2, ctype=C.c_double))

    def drain_statistics(self):
        return dict(zip(("cut_entries", "drain_trips_le4", "drain_trips_le8", "drain_trips_le16"), self._read("drain_statistics", 4)))

    def get_option(self, key):
        out = C.c_int32()
        self.check(self.L.vhr_get_option(self.handle, key.encode(), C.byref(out)), f"get_option({key})")
        return int(out.value)

    def bvh_statistics(self):
        return dict(zip(("nodes", "triangles", "max_depth", "node_bytes", "triangle_bytes"), self._read("bvh_statistics", 5)))

    KERNEL_KINDS = {"raygen": 0, "svgf_temporal": 1, "svgf_atrous": 2, "blit": 3, "reflection": 4, "ssao": 5, "ssao_blur": 6, "ssr": 7, "svgf_atrous_async": 8,
                    "ray_query": 9, "rayquery_forward": 10, "forward_raster": 11}
    REFIT_TIMING_BIT = 12          # a bit of vhr_set_kernel_timing's mask only (set_kernel_timing(..., refit=True)); the times come from refit_times_ms()

    @staticmethod
    def _aligned_zeros(n, dtype):
        """n zeroed records of `dtype` that start at a 16-byte boundary."""
        raw = np.zeros(n * dtype.itemsize + 16, np.uint8)
        start = -raw.ctypes.data % 16
        return raw[start:start + n * dtype.itemsize].view(dtype)

    @staticmethod
    def _records_array(a, dtype, columns, who):
        """(n, columns) float32 or a 1-D array of `dtype` -> a C-contiguous, 16-byte-aligned array of `dtype`; `who` = the names the errors
        use: (method, records, dtype)."""
        who, what, name = who
        a = np.asarray(a)
        if a.dtype == dtype:
            if a.ndim != 1:
                raise ValueError(f"{who}: a {name} array must be 1-D, got shape {a.shape}")
        elif a.dtype == np.float32:
            if a.ndim != 2 or a.shape[1] != columns:
                raise ValueError(f"{who}: float32 {what} must have shape (n, {columns}), got {a.shape}")
            a = np.ascontiguousarray(a).view(dtype).reshape(-1)
        else:
            raise TypeError(f"{who}: {what} must be float32 (n, {columns}) or abi.{name}, got {a.dtype}")
        if not a.flags.c_contiguous or a.ctypes.data % 16:       # the entry points want 16-byte-aligned records: copy into an aligned buffer
            aligned = Context._aligned_zeros(len(a), dtype)
            aligned[:] = a
            a = aligned
        return a

    @staticmethod
    def _rays_array(rays):
        """(n, 8) float32 (origin, tmin, direction, tmax) or abi.ray_dtype -> a C-contiguous, 16-byte-aligned ray_dtype array."""
        return Context._records_array(rays, abi.ray_dtype, 8, ("ray_query", "rays", "ray_dtype"))

    def ray_query(self, rays, any_hit=False, alpha_test=False, cull_mask=None, ray_masks=None, face_cull=None):
        """vhr_ray_query on host arrays: rays (n, 8) float32 or abi.ray_dtype.  Returns abi.ray_hit_dtype[n] (closest hit; a miss has
        geometry_index = primitive_index = abi.RAY_MISS) or, with any_hit, bool[n] (occluded).  alpha_test: a candidate hit the G-buffer
        pass would discard (alpha mask, alpha 0) does not exist for the ray.  cull_mask (0..255) and / or ray_masks (uint8[n]):
        vhr_ray_query_masked -- ray i's mask is cull_mask (default 0xFF) & ray_masks[i], and a candidate on a primitive whose mask shares no
        bit with it does not exist for the ray; with both left at None this is vhr_ray_query itself.  face_cull (abi.FACE_CULL_NONE / BACK /
        FRONT): vhr_ray_query_faces -- a candidate on a triangle facing away from (BACK) or towards (FRONT) the ray does not exist for it, and
        a closest hit's `reserved` is its hit kind (abi.HIT_KIND_*), NONE included; None keeps the entry points above."""
        r = self._rays_array(rays)
        n = len(r)
        out = np.zeros(n, np.uint8) if any_hit else np.zeros(n, abi.ray_hit_dtype)
        flags = abi.RAY_QUERY_HOST_MEMORY | (abi.RAY_QUERY_TERMINATE_ON_FIRST_HIT if any_hit else 0) | (abi.RAY_QUERY_ALPHA_TEST if alpha_test else 0)
        if cull_mask is None and ray_masks is None and face_cull is None:
            self.check(self.L.vhr_ray_query(self.handle, r.ctypes.data if n else None, n, flags, out.ctypes.data if n else None), "ray_query")
            return out.astype(bool) if any_hit else out
        rm = None
        if ray_masks is not None:
            rm = np.ascontiguousarray(ray_masks, np.uint8).reshape(-1)
            if len(rm) != n:
                raise ValueError(f"ray_query: {len(rm)} ray masks for {n} rays")
        if face_cull is not None:
            self.check(self.L.vhr_ray_query_faces(self.handle, r.ctypes.data if n else None, n, flags, 0xFF if cull_mask is None else int(cull_mask),
                                                  rm.ctypes.data if rm is not None and n else None, int(face_cull), out.ctypes.data if n else None), "ray_query")
        else:
            self.check(self.L.vhr_ray_query_masked(self.handle, r.ctypes.data if n else None, n, flags, 0xFF if cull_mask is None else int(cull_mask),
                                                   rm.ctypes.data if rm is not None and n else None, out.ctypes.data if n else None), "ray_query")
        return out.astype(bool) if any_hit else out

    def ray_query_device(self, rays_ptr, count, results_ptr, any_hit=False, alpha_test=False, cull_mask=None, ray_masks_ptr=0, face_cull=None):
        """vhr_ray_query on device memory (e.g. torch tensors' data_ptr()): `count` vhr_ray records at rays_ptr (16-byte aligned), results
        (vhr_ray_hit, or one uint8 per ray with any_hit) at results_ptr.  Enqueued on current_stream(); returns without synchronising.
        cull_mask and / or ray_masks_ptr (device memory, one uint8 per ray): vhr_ray_query_masked, as in ray_query(); face_cull:
        vhr_ray_query_faces, likewise."""
        flags = (abi.RAY_QUERY_TERMINATE_ON_FIRST_HIT if any_hit else 0) | (abi.RAY_QUERY_ALPHA_TEST if alpha_test else 0)
        if face_cull is not None:
            self.check(self.L.vhr_ray_query_faces(self.handle, rays_ptr or None, int(count), flags, 0xFF if cull_mask is None else int(cull_mask),
                                                  ray_masks_ptr or None, int(face_cull), results_ptr or None), "ray_query_device")
        elif cull_mask is None and not ray_masks_ptr:
            self.check(self.L.vhr_ray_query(self.handle, rays_ptr or None, int(count), flags, results_ptr or None), "ray_query_device")
        else:
            self.check(self.L.vhr_ray_query_masked(self.handle, rays_ptr or None, int(count), flags, 0xFF if cull_mask is None else int(cull_mask),
                                                   ray_masks_ptr or None, results_ptr or None), "ray_query_device")

    def ray_query_statistics(self):
        """The last ray query: [rays, rays with a hit, rays decided again in binary64, waves whose stack overflowed (must be 0)]."""
        return self._read("ray_query_statistics", 4)

    @staticmethod
    def _points_array(points):
        """(n, 4) float32 (point, max_distance) or abi.point_query_dtype -> a C-contiguous, 16-byte-aligned point_query_dtype array."""
        return Context._records_array(points, abi.point_query_dtype, 4, ("closest_point_query", "points", "point_query_dtype"))

    def closest_point_query(self, points, any_within=False, cull_mask=None):
        """vhr_closest_point_query on host arrays: points (n, 4) float32 (point, max_distance) or abi.point_query_dtype.  Returns
        abi.ray_hit_dtype[n] -- t = the distance to the nearest surface within max_distance, (u, v) the barycentrics of the nearest point,
        geometry_index = primitive_index = abi.RAY_MISS where there is none -- or, with any_within, bool[n].  cull_mask (0..255, default
        0xFF): a triangle on a primitive whose mask shares no bit with it does not exist for the query."""
        p = self._points_array(points)
        n = len(p)
        out = np.zeros(n, np.uint8) if any_within else np.zeros(n, abi.ray_hit_dtype)
        flags = abi.POINT_QUERY_HOST_MEMORY | (abi.POINT_QUERY_ANY_WITHIN if any_within else 0)
        self.check(self.L.vhr_closest_point_query(self.handle, p.ctypes.data if n else None, n, flags, 0xFF if cull_mask is None else int(cull_mask),
                                                  out.ctypes.data if n else None), "closest_point_query")
        return out.astype(bool) if any_within else out

    def closest_point_query_device(self, points_ptr, count, results_ptr, any_within=False, cull_mask=None):
        """vhr_closest_point_query on device memory (e.g. torch tensors' data_ptr()): `count` vhr_point_query records at points_ptr (16-byte
        aligned), results (vhr_ray_hit, or one uint8 per query with any_within) at results_ptr.  Enqueued on current_stream(); returns
        without synchronising."""
        flags = abi.POINT_QUERY_ANY_WITHIN if any_within else 0
        self.check(self.L.vhr_closest_point_query(self.handle, points_ptr or None, int(count), flags, 0xFF if cull_mask is None else int(cull_mask),
                                                  results_ptr or None), "closest_point_query_device")

    def point_query_statistics(self):
        """The last closest-point query: [queries, queries that found something, point / triangle evaluations, waves whose stack overflowed (must be 0)]."""
        return self._read("point_query_statistics", 4)

    def nearest_points_query(self, points, k, cull_mask=None):
        """vhr_nearest_points_query on host arrays: points as in closest_point_query(), 1 <= k <= abi.NEAREST_MAX_K.  Returns abi.ray_hit_dtype of
        shape (n, k): row q holds query q's candidates ordered by (distance, flat triangle index), every triangle at most once, then records with
        geometry_index = primitive_index = abi.RAY_MISS.  k == 1 is closest_point_query(), bit for bit."""
        p = self._points_array(points)
        n, k = len(p), int(k)
        out = np.zeros((n, max(k, 0)), abi.ray_hit_dtype)
        self.check(self.L.vhr_nearest_points_query(self.handle, p.ctypes.data if n else None, n, k, abi.POINT_QUERY_HOST_MEMORY, 0xFF if cull_mask is None else int(cull_mask),
                                                   out.ctypes.data if n else None), "nearest_points_query")
        return out

    def nearest_points_query_device(self, points_ptr, count, k, results_ptr, cull_mask=None):
        """vhr_nearest_points_query on device memory (e.g. torch tensors' data_ptr()): `count` vhr_point_query records at points_ptr (16-byte
        aligned), count * k vhr_ray_hit records at results_ptr.  Enqueued on current_stream(); returns without synchronising."""
        self.check(self.L.vhr_nearest_points_query(self.handle, points_ptr or None, int(count), int(k), 0, 0xFF if cull_mask is None else int(cull_mask),
                                                   results_ptr or None), "nearest_points_query_device")

    def nearest_query_statistics(self):
        """The last nearest-points query: [queries, entries returned over all queries, point / triangle evaluations of the walks, waves whose stack
        overflowed (must be 0)]."""
        return self._read("nearest_query_statistics", 4)

    def resolve_hits(self, hits, material=False):
        """vhr_resolve_hits on host arrays: hits = abi.ray_hit_dtype[n], as ray_query() and closest_point_query() return them (only u, v,
        geometry_index and primitive_index are read).  Returns abi.surface_point_dtype[n], 16-byte aligned: position, geometric normal (unit, on
        the triangle's front side), shading normal, uv0 / uv1 and, with material, base_color / metallic / roughness and the normal map's
        perturbation as the G-buffer pass evaluates them; flags = abi.SURFACE_* result bits, 0 (and an all-zero record) for a hit that was
        not resolved -- a miss, an index outside the scene, barycentrics that are no numbers.  A host-only context answers without material."""
        h = np.ascontiguousarray(hits, dtype=abi.ray_hit_dtype).reshape(-1)
        n = len(h)
        out = self._aligned_zeros(n, abi.surface_point_dtype)
        flags = abi.SURFACE_HOST_MEMORY | (abi.SURFACE_MATERIAL if material else 0)
        self.check(self.L.vhr_resolve_hits(self.handle, h.ctypes.data if n else None, n, flags, out.ctypes.data if n else None), "resolve_hits")
        return out

    def resolve_hits_device(self, hits_ptr, count, out_ptr, material=False):
        """vhr_resolve_hits on device memory (e.g. torch tensors' data_ptr()): `count` vhr_ray_hit records at hits_ptr (4-byte aligned),
        vhr_surface_point records (80 bytes each) at out_ptr (16-byte aligned).  Enqueued on current_stream(); returns without synchronising."""
        self.check(self.L.vhr_resolve_hits(self.handle, hits_ptr or None, int(count), abi.SURFACE_MATERIAL if material else 0, out_ptr or None), "resolve_hits_device")

    def surface_statistics(self):
        """The last resolve_hits: [hits, records with SURFACE_VALID, records with SURFACE_DISCARDED, 1 if the material instantiation ran]."""
        return self._read("surface_statistics", 4)

    @staticmethod
    def _occlusion_points_array(points):
        """(n, 8) float32 (origin, tmin, axis, tmax) or abi.ray_dtype -> a C-contiguous, 16-byte-aligned ray_dtype array."""
        return Context._records_array(points, abi.ray_dtype, 8, ("occlusion_query", "points", "ray_dtype"))

    def occlusion_query(self, points, samples, seed=0, cull_mask=None):
        """vhr_occlusion_query on host arrays: points (n, 8) float32 or abi.ray_dtype, read as (origin, tmin, axis, tmax); 1 <= samples <=
        abi.OCCLUSION_MAX_SAMPLES cosine-distributed any-hit rays around each axis.  Returns uint64[n]: bit j of entry i = ray (i, j) is
        occluded, bits from `samples` up are 0 (AO = 1 - popcount / samples).  cull_mask (0..255, default 0xFF) as in ray_query()."""
        p = self._occlusion_points_array(points)
        n = len(p)
        out = np.zeros(n, np.uint64)
        self.check(self.L.vhr_occlusion_query(self.handle, p.ctypes.data if n else None, n, int(samples), int(seed) & 0xFFFFFFFF, abi.OCCLUSION_HOST_MEMORY,
                                              0xFF if cull_mask is None else int(cull_mask), out.ctypes.data if n else None), "occlusion_query")
        return out

    def occlusion_query_device(self, points_ptr, count, samples, occluded_ptr, seed=0, cull_mask=None):
        """vhr_occlusion_query on device memory (e.g. torch tensors' data_ptr()): `count` query points at points_ptr (16-byte aligned), one
        uint64 mask per point at occluded_ptr (8-byte aligned).  Enqueued on current_stream(); returns without synchronising."""
        self.check(self.L.vhr_occlusion_query(self.handle, points_ptr or None, int(count), int(samples), int(seed) & 0xFFFFFFFF, 0,
                                              0xFF if cull_mask is None else int(cull_mask), occluded_ptr or None), "occlusion_query_device")

    def occlusion_statistics(self):
        """The last occlusion query: [points, occluded rays over all points, points computed again in binary64, waves whose stack overflowed
        (must be 0)]."""
        return self._read("occlusion_statistics", 4)

    def debug_occlusion_rays(self, points, samples, seed=0):
        """The rays occlusion_query() walks: points as there -> (n, samples, 8) float32 (origin, tmin, direction, tmax), ray (i, j) at [i, j].  A
        device context runs the device's copy of the generator, a host-only context the host's."""
        p = self._occlusion_points_array(points)
        n, samples = len(p), int(samples)
        out = self._aligned_zeros(n * max(samples, 0), abi.ray_dtype)
        self.check(self.L.vhr_debug_occlusion_rays(self.handle, p.ctypes.data if n else None, n, samples, int(seed) & 0xFFFFFFFF, out.ctypes.data if n else None), "debug_occlusion_rays")
        return out.view(np.float32).reshape(n, max(samples, 0), 8)

    def debug_point_triangle(self, pairs):
        """The query's point / triangle function on explicit pairs: pairs = (n, 12) float32 (p, v0, e1, e2) -> (n, 3) float32 (d2, u, v).  A device
        context runs the device's copy, a host-only context the host's."""
        pairs = np.ascontiguousarray(pairs, dtype=np.float32).reshape(-1, 12)
        out = np.zeros((len(pairs), 3), np.float32)
        n = len(pairs)
        self.check(self.L.vhr_debug_point_triangle(self.handle, pairs.ctypes.data if n else None, n, out.ctypes.data if n else None), "debug_point_triangle")
        return out

    def current_stream(self):
        """hipStream_t (as an int) the library is enqueueing on right now: inside a pass callback, the stream that pass is ordered on."""
        out = C.c_void_p()
        self.check(self.L.vhr_get_current_stream(self.handle, C.byref(out)), "get_current_stream")
        return int(out.value or 0)

    def set_option(self, key, value):
        self.check(self.L.vhr_set_option(self.handle, key.encode(), int(value)), "set_option")

    def set_kernel_timing(self, kinds, refit=False):
        """kinds: True (all), False (off) or an iterable of kind names from KERNEL_KINDS.  refit=True: vhr_refit_geometry times its stages too (refit_times_ms)."""
        if kinds is True:
            mask = 0xFF
        elif not kinds:
            mask = 0
        else:
            mask = sum(1 << self.KERNEL_KINDS[k] for k in kinds)
        if refit:
            mask |= 1 << self.REFIT_TIMING_BIT
        self.check(self.L.vhr_set_kernel_timing(self.handle, mask), "set_kernel_timing")

    def kernel_time(self, kind, reset=False):
        """(total_ms, launches) of a kernel kind, measured with HIP events on the context stream."""
        ms, n = C.c_double(), C.c_uint64()
        self.check(self.L.vhr_get_kernel_time(self.handle, self.KERNEL_KINDS[kind], C.byref(ms), C.byref(n), int(reset)), "kernel_time")
        return ms.value, n.value

    def _guard(self, fn):
        """Run a Python pass body; park exceptions (they must not unwind through C) for execute() to re-raise."""
        try:
            fn()
        except Exception as e:   # noqa: BLE001
            self._callback_error = e


class RaytracingExecutionContext:
    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def trace_rays(self, width, height):
        self.ctx.check(self.ctx.L.vhr_trace_rays(self.handle, width, height), "TraceRays")


class ComputeExecutionContext:
    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def get_display_size(self):
        w, h = C.c_uint32(), C.c_uint32()
        self.ctx.check(self.ctx.L.vhr_compute_get_display_size(self.handle, C.byref(w), C.byref(h)), "GetDisplaySize")
        return w.value, h.value

    def dispatch(self, shader, x_groups, y_groups, z_groups, push_constants=None):
        if push_constants is None:
            rc = self.ctx.L.vhr_compute_dispatch(self.handle, shader.encode(), x_groups, y_groups, z_groups, None, 0)
        else:
            a = np.ascontiguousarray(push_constants)
            rc = self.ctx.L.vhr_compute_dispatch(self.handle, shader.encode(), x_groups, y_groups, z_groups, _p(a), a.nbytes)
        self.ctx.check(rc, "Dispatch")

    def blit_image_storage_to_transient(self, src, dst):
        self.ctx.check(self.ctx.L.vhr_compute_blit_image_storage_to_transient(self.handle, src, dst.encode()), "BlitImageStorageToTransient")

    def blit_image_transient_to_storage(self, src, dst):
        self.ctx.check(self.ctx.L.vhr_compute_blit_image_transient_to_storage(self.handle, src.encode(), dst), "BlitImageTransientToStorage")

    def blit_image_storage_to_storage(self, src, dst):
        self.ctx.check(self.ctx.L.vhr_compute_blit_image_storage_to_storage(self.handle, src, dst), "BlitImageStorageToStorage")


class _RenderPath:
    """What the four vhr_<PREFIX>_* bindings share: the handle, its error text, build and destroy.  A binding is named like its C++
    class: errors quote that name."""
    PREFIX = None

    def __init__(self, ctx):
        self.ctx, self.handle, self._callbacks = ctx, C.c_void_p(), []

    def _create(self, *args):
        self.ctx.check(self._fn("create")(self.ctx.handle, *args, C.byref(self.handle)), f"vhr_{self.PREFIX}_create")

    def _callback(self, body):
        """An optional Python pass body `body(ctx)` as the C callback and its user pointer.  ctypes callbacks must outlive the handle: kept here."""
        ctx = self.ctx
        cb = EXTERNAL_CB(lambda user, c: ctx._guard(lambda: body(ctx))) if body else EXTERNAL_CB()
        self._callbacks.append(cb)
        return cb, None

    def _fn(self, name):
        return getattr(self.ctx.L, f"vhr_{self.PREFIX}_{name}")

    def _check(self, rc, what):
        if rc < 0:
            raise VhrError(f"{what}: {self._fn('last_error')(self.handle).decode()}")

    def build(self):
        self._check(self._fn("build")(self.handle), f"{type(self).__name__}::Build")

    def _rebuild(self, *args):
        self._check(self._fn("rebuild")(self.handle, *args), f"{type(self).__name__}::Rebuild")

    def destroy(self):
        if self.handle:
            self._fn("destroy")(self.handle)
            self.handle = None


class HybridRenderPath(_RenderPath):
    """vhr_hybrid_*: the C++ re-host of HybridRenderPath (csrc/hybrid_render_path.cpp)."""
    PREFIX = "hybrid"

    def __init__(self, ctx, shadow_mode=0, ambient_occlusion_mode=2, reflection_mode=2, denoise=False, atrous_steps=5,
                 gbuffer_pass=None, composition_pass=None):
        super().__init__(ctx)
        self.settings = HybridSettings(shadow_mode, ambient_occlusion_mode, reflection_mode, int(denoise), atrous_steps)
        self._create(C.byref(self.settings), *self._callback(gbuffer_pass), *self._callback(composition_pass))

    def rebuild(self, **changes):
        for k, v in changes.items():
            setattr(self.settings, k, int(v))
        self._rebuild(C.byref(self.settings))

    def push_constants(self):
        pc = np.zeros((), abi.svgf_push_constants_dtype)
        self.ctx.check(self.ctx.L.vhr_hybrid_get_push_constants(self.handle, _p(pc)), "get_push_constants")
        return pc

    def save_state(self):
        """vhr_hybrid_save_state: the path's cross-frame state (five SVGF images + the last frame's PerFrameData) as a uint8 array."""
        n = C.c_uint64()
        self._check(self.ctx.L.vhr_hybrid_state_size(self.handle, C.byref(n)), "vhr_hybrid_state_size")
        blob = np.empty(int(n.value), np.uint8)
        self._check(self.ctx.L.vhr_hybrid_save_state(self.handle, _p(blob), n.value), "vhr_hybrid_save_state")
        return blob

    def load_state(self, blob):
        """vhr_hybrid_load_state; returns the PerFrameData of the frame the blob was saved behind."""
        blob = np.ascontiguousarray(blob, np.uint8)
        last = np.zeros((), abi.per_frame_dtype)
        self._check(self.ctx.L.vhr_hybrid_load_state(self.handle, _p(blob), blob.size, _p(last)), "vhr_hybrid_load_state")
        return last


class RaytracedRenderPath(_RenderPath):
    """vhr_raytraced_*: the C++ re-host of RaytracedRenderPath (csrc/raytraced_render_path.cpp)."""
    PREFIX = "raytraced"

    def __init__(self, ctx, use_anyhit_shader=False, composition_pass=None):
        super().__init__(ctx)
        self.use_anyhit_shader = bool(use_anyhit_shader)
        self._create(int(self.use_anyhit_shader), *self._callback(composition_pass))

    def rebuild(self, use_anyhit_shader):
        self.use_anyhit_shader = bool(use_anyhit_shader)
        self._rebuild(int(self.use_anyhit_shader))


class RayqueryRenderPath(_RenderPath):
    """vhr_rayquery_*: the C++ re-host of RayqueryRenderPath (csrc/rayquery_render_path.cpp): one external "Forward Pass" whose body
    (`forward_pass(ctx)`, e.g. calling Context.standin_rayquery_forward) is the integrator's."""
    PREFIX = "rayquery"

    def __init__(self, ctx, forward_pass=None):
        super().__init__(ctx)
        self._create(*self._callback(forward_pass))

    def rebuild(self):
        self._rebuild()


class ForwardRasterRenderPath(_RenderPath):
    """vhr_forward_raster_*: the C++ re-host of ForwardRasterRenderPath (csrc/forward_raster_render_path.cpp): the external passes "Depth
    Prepass" (`depth_prepass(ctx)`, e.g. calling Context.standin_shadow_map) and "Forward Pass" (`forward_pass(ctx)`, e.g. calling
    Context.standin_forward_raster), their bodies the integrator's; `enable_msaa` makes RENDER_OUTPUT and "Depth" 8-sample images."""
    PREFIX = "forward_raster"

    def __init__(self, ctx, depth_prepass=None, forward_pass=None, enable_msaa=1):
        super().__init__(ctx)
        self.enable_msaa = int(enable_msaa)
        self._create(*self._callback(depth_prepass), *self._callback(forward_pass), self.enable_msaa)

    def rebuild(self, enable_msaa=None):
        """The ImGui radio button (forward_raster_render_path.cpp:99-111): set enable_msaa (None = keep it), then Rebuild()."""
        if enable_msaa is not None:
            self.enable_msaa = int(enable_msaa)
        self._rebuild(self.enable_msaa)


def strip_plan(height, world, rank, max_motion_rows, atrous_steps=5):
    """vhr_strip_plan_make: the C planner (csrc/comm.cpp).  None when the strips are thinner than the history halo."""
    p = StripPlanC()
    rc = load().vhr_strip_plan_make(height, world, rank, max_motion_rows, atrous_steps, C.byref(p))
    if rc == -4:                      # VHR_ERROR_OUT_OF_SLOTS
        return None
    if rc != 0:
        raise VhrError(f"vhr_strip_plan_make: {rc}")
    return p


def strip_plan_exchanges(plan, n_rows):
    out = (RowExchangeC * 2)()
    n = load().vhr_strip_plan_exchanges(C.byref(plan), n_rows, out)
    return [(out[i].peer, (out[i].send_begin, out[i].send_end), (out[i].recv_begin, out[i].recv_end)) for i in range(n)]


def tile_grid(width, height, world, overlap):
    """vhr_tile_grid_choose: (grid_rows, grid_cols) of the C planner."""
    r, c = C.c_uint32(), C.c_uint32()
    rc = load().vhr_tile_grid_choose(width, height, world, overlap, C.byref(r), C.byref(c))
    if rc != 0:
        raise VhrError(f"vhr_tile_grid_choose: {rc}")
    return int(r.value), int(c.value)


def tile_plan(width, height, world, rank, grid_rows=0, grid_cols=0, max_motion_rows=0, max_motion_cols=0, atrous_steps=5, cost=None, cost_cell=8):
    """vhr_tile_plan_make / _make_weighted: the C planner (csrc/comm.cpp).  None when a tile is thinner than its history halo.  cost: a 2-D uint32
    array, one value per cost_cell x cost_cell pixel block -- the grid is cut at equal cost."""
    p = TilePlanC()
    if cost is None:
        rc = load().vhr_tile_plan_make(width, height, world, rank, grid_rows, grid_cols, max_motion_rows, max_motion_cols, atrous_steps, C.byref(p))
    else:
        cm = np.ascontiguousarray(cost, np.uint32)
        rc = load().vhr_tile_plan_make_weighted(width, height, world, rank, grid_rows, grid_cols, max_motion_rows, max_motion_cols, atrous_steps,
                                                cm.ctypes.data_as(C.c_void_p), cm.shape[1], cm.shape[0], cost_cell, C.byref(p))
    if rc == -4:                      # VHR_ERROR_OUT_OF_SLOTS
        return None
    if rc != 0:
        raise VhrError(f"vhr_tile_plan_make: {rc}")
    return p


def tile_plan_exchanges(plan, halo_rows, halo_cols):
    out = (RectExchangeC * 64)()
    n = load().vhr_tile_plan_exchanges(C.byref(plan), halo_rows, halo_cols, out, 64)
    if n < 0:
        raise VhrError(f"vhr_tile_plan_exchanges: {n}")
    rect = lambda r: (r.x0, r.x1, r.y0, r.y1)
    return [(out[i].peer, rect(out[i].send), rect(out[i].recv)) for i in range(n)]


def tile_plan_replan(old, new):
    """vhr_tile_plan_replan: [(peer, send rect, recv rect)] that carry the cross-frame SVGF state from `old`'s rectangles to `new`'s (tiling.replan_transfers)."""
    out = (RectExchangeC * 256)()
    n = load().vhr_tile_plan_replan(C.byref(old), C.byref(new), out, 256)
    if n < 0:
        raise VhrError(f"vhr_tile_plan_replan: {n}")
    rect = lambda r: (r.x0, r.x1, r.y0, r.y1)   # noqa: E731
    return [(out[i].peer, rect(out[i].send), rect(out[i].recv)) for i in range(n)]


def comm_use_library(path):
    """vhr_comm_use_library: the RCCL library csrc/comm.cpp loads (before the process's first vhr_comm_* call); None = the default resolution."""
    rc = load().vhr_comm_use_library(path.encode() if path else None)
    if rc != 0:
        raise VhrError(f"vhr_comm_use_library: {rc} (the RCCL entry points are already bound)")


def comm_library():
    """vhr_comm_library: the file the RCCL entry points came from, or the reason they could not be resolved."""
    return load().vhr_comm_library().decode()


def comm_use_library_from_environment():
    """Test and bench tooling: VHR_RCCL_LIBRARY=<path> (tests/rccl_shim's stand-in, a site's own build) is honoured HERE, by the host program's explicit call
    -- the library itself reads no environment variable.  Returns the path or None."""
    path = os.environ.get("VHR_RCCL_LIBRARY") or None
    if path:
        comm_use_library(path)
    return path


class Comm:
    """vhr_comm_*: the strip / tile exchanges inside the library (RCCL).  One per context and process."""

    def __init__(self, ctx, plan, unique_id):
        self.ctx = ctx
        self.handle = C.c_void_p()
        if isinstance(plan, TilePlanC):
            ctx.check(ctx.L.vhr_comm_create_tiled(ctx.handle, C.byref(plan), unique_id, C.byref(self.handle)), "vhr_comm_create_tiled")
        else:
            ctx.check(ctx.L.vhr_comm_create(ctx.handle, C.byref(plan), unique_id, C.byref(self.handle)), "vhr_comm_create")

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = load().vhr_comm_get_unique_id(buf)
        if rc != 0:
            raise VhrError(f"vhr_comm_get_unique_id: {rc} (RCCL not available?)")
        return buf.raw

    def _check(self, rc, what):
        if rc != 0:
            raise VhrError(f"{what}: {self.ctx.L.vhr_comm_last_error(self.handle).decode()}")

    def exchange_raytraced(self, image=RAYTRACED):
        self._check(self.ctx.L.vhr_comm_exchange_raytraced(self.handle, image.encode()), "vhr_comm_exchange_raytraced")

    def start_frame_exchanges(self, history, moments, denoised=None, root=0, gathered_frame_ptr=None):
        self._check(self.ctx.L.vhr_comm_start_frame_exchanges(self.handle, history, moments, denoised.encode() if denoised else None, root,
                                                              gathered_frame_ptr), "vhr_comm_start_frame_exchanges")

    def finish_frame_exchanges(self):
        self._check(self.ctx.L.vhr_comm_finish_frame_exchanges(self.handle), "vhr_comm_finish_frame_exchanges")

    def replan(self, new_plan, history, moments, prev_normals):
        """vhr_comm_replan: the communicator and the context take `new_plan` (a TilePlanC), the three cross-frame storage images follow their pixels."""
        self._check(self.ctx.L.vhr_comm_replan(self.handle, C.byref(new_plan), int(history), int(moments), int(prev_normals)), "vhr_comm_replan")

    def destroy(self):
        if self.handle:
            self.ctx.L.vhr_comm_destroy(self.handle)
            self.handle = None
