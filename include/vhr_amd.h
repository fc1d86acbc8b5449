/*
 * vhr_amd.h -- C ABI of libvhr_amd.so: the MI355X-native (HIP / gfx950) implementation of the
 * ray-traced shadow / AO / mirror-reflection pass and the SVGF denoiser of
 * RMichelsen/VulkanHybridRenderer, behind the reference's render-graph pass API.
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * repository root).  All functions return 0 on success and a negative code on failure unless noted;
 * vhr_last_error() returns the message.  The reference has no error returns (VK_CHECK asserts,
 * vulkan_common.h:4-7); pool exhaustion returns -1 like resource_manager.cpp:847-848,876-877.
 *
 * Threading and streams: like the reference (renderer.cpp:184-235) one host thread drives one context.  Everything a frame PUBLISHES is
 * issued in order on the context's stream (the one given at creation, or an internal one with VHR_CREATE_INTERNAL_STREAM): after
 * vhr_graph_execute returns, work the caller enqueues on that stream sees every image the graph's passes declare as outputs.  Two things
 * leave that stream, all owned and joined by the library:
 *   - "svgf_async_unread" (default 1): a compute pass's a-trous dispatch whose output nothing reads (the reference's fifth iteration,
 *     hybrid_render_path.cpp:299-328) runs on a library-owned SIDE stream beside whatever the context's stream does next; the context's
 *     stream waits for it before the next compute pass, before storage-image uploads / downloads / vhr_get_storage_image and in
 *     vhr_synchronize.  A caller that reads that dispatch's storage image itself on the context's stream must call vhr_synchronize first
 *     or set the option to 0 (every dispatch in recorded order on the one stream).
 *   - "reflection_async" (default 1): the mirror ray's launch runs on a second library-owned stream behind the shadow / AO launch, beside the
 *     SVGF pass; the context's stream waits for it before a pass epilogue (not with value 2), before the frame's next external pass, at the
 *     end of vhr_graph_execute (so the sentence above holds for the Reflections image too), before image uploads, before downloads of and
 *     vhr_get_transient_image on the Reflections image, in vhr_get_current_stream (not with value 2: a caller who asks for the stream is
 *     about to enqueue kernels of its own, which may read Reflections or rewrite the G-buffer the launch reads) and in vhr_synchronize.
 *     With value 2 (the multi-GPU harness) a caller's own kernels that touch Reflections or the G-buffer inside a frame must call
 *     vhr_get_transient_image on Reflections (or vhr_synchronize) first.
 *   - "frames_in_flight" 2 / 3 (opt-in): the front of a frame (up to its last ray-tracing pass) runs on a second stream; vhr_get_current_stream
 *     tells an external pass which stream to enqueue on.
 * Pass time stamps ("pass_timestamps", vhr_graph_gather_performance_statistics) cover what the CONTEXT'S stream executes between a pass's
 * first kernel and the next kernel behind it: "Raytrace Pass" covers the shadow / AO launch (+ the mirror ray's with "reflection_async" 0);
 * with the side stream on, "SVGF Denoise Pass" covers 1 temporal + 4 a-trous dispatches + the
 * blits where the reference's vkCmdWriteTimestamp pair covers five a-trous dispatches (render_graph.cpp:167-182); with "svgf_async_unread" 0
 * it covers all five.  In mode 1 the END of a pass is stored by the next LIBRARY kernel on the stream, so GPU work an external (graphics)
 * pass's callback enqueues on the stream right behind a library pass is charged to that pass; mode 2 closes the pass in front of every such
 * callback and at the end of vhr_graph_execute (a one-thread kernel, +6 us each).
 * One context per GPU / per process for multi-GPU (screen tiles, vhr_set_tile; row strips, vhr_set_strip).
 */
#ifndef VHR_AMD_H
#define VHR_AMD_H

#include "vhr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vhr_context vhr_context;
typedef struct vhr_raytracing_execution_context vhr_raytracing_execution_context;
typedef struct vhr_compute_execution_context vhr_compute_execution_context;

enum {
    VHR_OK = 0,
    VHR_ERROR_INVALID_ARGUMENT = -1,
    VHR_ERROR_DEVICE = -2,
    VHR_ERROR_NOT_FOUND = -3,
    VHR_ERROR_OUT_OF_SLOTS = -4,
    VHR_ERROR_GRAPH = -5,
    VHR_ERROR_NO_DEVICE = -6,
    VHR_ERROR_UNSUPPORTED = -7      /* what the index-returning calls use for invalid arguments: their -1 is the reference's "exhausted" sentinel */
};

/* ---------------------------------------------------------------------------------------------
 * Context (replaces VulkanContext + the device half of ResourceManager:
 * src/rendering_backend/vulkan_context.cpp:44-89, resource_manager.cpp:15-70)
 * ------------------------------------------------------------------------------------------- */
/* vhr_create_info.flags */
enum {
    /* Pass registry / execution order / SanityCheck only: no HIP call is made, nothing can be uploaded,
     * executed or downloaded.  Lets the host-side graph logic be checked on a machine without a GPU. */
    VHR_CREATE_HOST_ONLY = 1,
    /* Ignore vhr_create_info.stream and create an internal (non-blocking) HIP stream. */
    VHR_CREATE_INTERNAL_STREAM = 2
};

typedef struct vhr_create_info {
    int32_t  device;          /* HIP device ordinal */
    uint32_t width;           /* display ("swapchain") size: context.swapchain.extent */
    uint32_t height;
    void    *stream;          /* hipStream_t to issue all work on, used as given (NULL = the default stream) */
    uint32_t flags;           /* 0 or VHR_CREATE_* bits */
} vhr_create_info;

int  vhr_create(const vhr_create_info *info, vhr_context **out);
void vhr_destroy(vhr_context *ctx);
/* VulkanContext::Resize (vulkan_context.cpp:118-120), the first half of the reference's one recovery route -- renderer.cpp:113-118,146-154:
 * `context->Resize(); active_render_path->Build();` when the swapchain is out of date.  The display extent changes; what was sized by the old one
 * is released: the graph (transient images, pass registry: RenderPath::Build would destroy it first anyway, render_path.cpp:14-20) and every image
 * of the storage pool (the render path's SVGF history, which its RegisterPath allocates again).  Geometry, the acceleration structure (K0 is NOT
 * rebuilt: vhr_get_build_times keeps its values), textures, options, trace parameters and kernel timers stay; the screen tile (vhr_set_tile) is the
 * whole image again.  Then the path registers and builds at the new extent: vhr_hybrid_build / vhr_raytraced_build (which read the extent from
 * the context) or RenderPath::Build() behind DeviceContext::Resize() (vhr_render_graph.hpp).  Frames after that equal a fresh context's bit for bit. */
int  vhr_resize(vhr_context *ctx, uint32_t width, uint32_t height);
const char *vhr_last_error(const vhr_context *ctx);   /* ctx may be NULL: error of the last failed vhr_create */
int  vhr_synchronize(vhr_context *ctx);               /* hipStreamSynchronize on the context stream */
/* The HIP stream (hipStream_t) the library is enqueueing on right now.  Outside vhr_graph_execute that is the stream given to
 * vhr_create.  Inside a pass or epilogue callback it is the stream that pass is ordered on: with "frames_in_flight" > 1 the passes up to
 * the last ray-tracing pass run on a second, library-owned stream, and an external graphics pass (the G-buffer producer) MUST enqueue its
 * work there -- or make that stream wait for its own -- for the Raytrace Pass to see a complete G-buffer (render_graph.cpp:722-796 orders
 * the same hand-over with image barriers).  The call also makes the stream wait for a held-back ray-tracing launch ("fuse_temporal") and for
 * the mirror ray's pending launch ("reflection_async" 1): whatever the caller enqueues behind it sees the frame's images as the single-stream
 * schedule would leave them. */
int  vhr_get_current_stream(vhr_context *ctx, void **stream);
const char *vhr_version(void);
int  vhr_abi_struct_sizes(uint32_t out[8]);            /* vertex, material, primitive, light, per-frame, push constants, trace params, 0 */
void vhr_default_trace_params(vhr_trace_params *out); /* raygen.rgen:29-65 constants */

/* ---------------------------------------------------------------------------------------------
 * ResourceManager (src/rendering_backend/resource_manager.h:16-78)
 * ------------------------------------------------------------------------------------------- */
/* UpdateGeometry (resource_manager.h:34, .cpp:291-360) + UpdateBLAS (.cpp:593-701) + UpdateTLAS
 * (.cpp:703-801): uploads the flat vertex / index / primitive arrays and builds the acceleration
 * structure -- here a host-built binned-SAH BVH2 over the world-space (transform-baked), two-sided,
 * all-opaque triangle soup.  gl_GeometryIndexEXT == primitive index, gl_PrimitiveID == triangle index
 * within the primitive.  On a VHR_CREATE_HOST_ONLY context the arrays are validated and the tree is built and checked
 * (vhr_get_bvh_statistics, vhr_get_bvh_form_checks, vhr_get_build_times), nothing is uploaded. */
int vhr_update_geometry(vhr_context *ctx, const vhr_vertex *vertices, uint32_t vertex_count,
                        const uint32_t *indices, uint32_t index_count,
                        const vhr_primitive *primitives, uint32_t primitive_count);
/* UploadTextureFromData (resource_manager.h:26, .cpp:152-196): RGBA8 texels, format
 * VHR_FORMAT_R8G8B8A8_{SRGB,UNORM}, sampler NULL = default sampler (LINEAR / REPEAT, .cpp:58-69).
 * Returns the bindless texture index (>= 0) or a negative error. */
int32_t vhr_upload_texture_from_data(vhr_context *ctx, uint32_t width, uint32_t height, const uint8_t *data,
                                     int32_t format, const vhr_sampler_info *sampler_info);
/* UploadNewStorageImage (resource_manager.h:28, .cpp:230-263): returns the first free slot index
 * (< 2048) of the bindless storage-image pool, or -1 when exhausted.  Contents are zero-initialised
 * (the reference leaves them undefined). */
int32_t vhr_upload_new_storage_image(vhr_context *ctx, uint32_t width, uint32_t height, int32_t format);
/* DestroyStorageImage (resource_manager.h:29, .cpp:265-269) */
int vhr_destroy_storage_image(vhr_context *ctx, int32_t id);
/* UpdatePerFrameUBO (resource_manager.h:35, .cpp:362-364); resource_idx < 3 (MAX_FRAMES_IN_FLIGHT) */
int vhr_update_per_frame_ubo(vhr_context *ctx, uint32_t resource_idx, const vhr_per_frame_data *per_frame_data);
/* extension: the constants raygen.rgen hard-codes */
int vhr_set_trace_params(vhr_context *ctx, const vhr_trace_params *params);

/* ---------------------------------------------------------------------------------------------
 * RenderGraph (src/render_graph/render_graph.h:10-21)
 * ------------------------------------------------------------------------------------------- */
typedef void (*vhr_external_pass_callback)(void *user, vhr_context *ctx);
typedef void (*vhr_raytracing_pass_callback)(void *user, vhr_raytracing_execution_context *exec);
typedef void (*vhr_compute_pass_callback)(void *user, vhr_compute_execution_context *exec);

/* DestroyResources (render_graph.h:8, .cpp:16-68): drops passes, pipelines and transient images */
int vhr_graph_destroy_resources(vhr_context *ctx);
/* AddGraphicsPass (render_graph.h:10-12, .cpp:70-85).  Raster passes (G-buffer, composition) stay with
 * the integrator: the callback runs at the pass's place in the execution order and is expected to
 * produce / consume the named transient images (through imported memory, vhr_graph_bind_external_image,
 * or vhr_upload_image).  `callback` may be NULL. */
int vhr_graph_add_graphics_pass(vhr_context *ctx, const char *render_pass_name,
                                const vhr_transient_resource *dependencies, uint32_t dependency_count,
                                const vhr_transient_resource *outputs, uint32_t output_count,
                                vhr_external_pass_callback callback, void *user);
/* AddRaytracingPass (render_graph.h:13-15, .cpp:87-101).  The shader names select HIP kernels:
 * raygen "hybrid_render_path/raygen.rgen", miss[0] "hybrid_render_path/miss.rmiss", miss[1]
 * "hybrid_render_path/reflection_miss.rmiss", hit[0].closest_hit
 * "hybrid_render_path/reflection_hit.rchit" (hybrid_render_path.cpp:112-124). */
int vhr_graph_add_raytracing_pass(vhr_context *ctx, const char *render_pass_name,
                                  const vhr_transient_resource *dependencies, uint32_t dependency_count,
                                  const vhr_transient_resource *outputs, uint32_t output_count,
                                  const vhr_raytracing_pipeline_description *pipeline,
                                  vhr_raytracing_pass_callback callback, void *user);
/* AddComputePass (render_graph.h:16-18, .cpp:103-116).  Known kernels:
 * "hybrid_render_path/svgf.comp", "hybrid_render_path/svgf_atrous_filter.comp" (SVGFPushConstants, 24 bytes), and the
 * screen-space alternatives of hybrid_render_path.cpp:138-243: "hybrid_render_path/ssao.comp" (bindings 0 normals, 1 depth,
 * 2 output; dispatched WITHOUT push constants, as the reference does although the shader reads SSAOPushConstants.radius --
 * the kernel uses the SSAOPushConstants last pushed on this context by any dispatch, 0.75 before the first),
 * "hybrid_render_path/ssao_blur.comp" (0 input, 1 output; SSAOPushConstants, 4 bytes, which the shader ignores) and
 * "hybrid_render_path/ssr.comp" (0 albedo, 1 normals, 2 motion / metallic-roughness, 3 depth, 4 output; SSRPushConstants,
 * 16 bytes).  Their inputs must be whole images (they sample anywhere on screen, REPEAT-wrapped); with row strips only the
 * owned output rows are computed (ssao.comp six more on either side for the blur).  A shader name is a
 * global key: registering it in two passes fails (render_graph.cpp:677). */
int vhr_graph_add_compute_pass(vhr_context *ctx, const char *render_pass_name,
                               const vhr_transient_resource *dependencies, uint32_t dependency_count,
                               const vhr_transient_resource *outputs, uint32_t output_count,
                               const vhr_compute_pipeline_description *pipeline,
                               vhr_compute_pass_callback callback, void *user);
/* Build (render_graph.h:20, .cpp:118-149): creates every named transient image, derives the execution
 * order by BFS from the single writer of "RENDER_OUTPUT" (.cpp:686-720) and runs SanityCheck
 * (.cpp:980-1021). */
int vhr_graph_build(vhr_context *ctx);
/* Execute (render_graph.h:21, .cpp:151-187): runs the pass callbacks in order on the context stream,
 * bracketing each pass with a pair of timing events (the reference's timestamp queries). */
int vhr_graph_execute(vhr_context *ctx, uint32_t resource_idx, uint32_t image_idx);
/* GatherPerformanceStatistics (render_graph.h:22, .cpp:189-201): blocks on the last Execute and folds
 * the per-pass times into the reference's EMA (0.95 * old + 0.05 * new). */
int vhr_graph_gather_performance_statistics(vhr_context *ctx);
/* pass_timestamps[name] (render_graph.cpp:199): EMA and last sample, milliseconds */
int vhr_graph_get_pass_time_ms(vhr_context *ctx, const char *render_pass_name, double *ema_ms, double *last_ms);
/* execution_order (render_graph.h:47): pass names joined by '\n' into buf; returns the pass count */
int vhr_graph_get_execution_order(vhr_context *ctx, char *buf, uint32_t buf_size);
/* ContainsImage / GetImageFormat (render_graph.h:25-26) */
int vhr_graph_contains_image(vhr_context *ctx, const char *image_name);
int32_t vhr_graph_get_image_format(vhr_context *ctx, const char *image_name);

/* extension (multi-GPU / interop hook): called right after the named pass's callback returns, on the
 * host thread, with the pass's work already enqueued on the context stream */
int vhr_graph_set_pass_epilogue(vhr_context *ctx, const char *render_pass_name,
                                vhr_external_pass_callback callback, void *user);
/* extension (interop): point a transient image at externally owned device memory of the same extent and
 * format (what VK_KHR_external_memory import would provide), 16-byte aligned.  NULL restores the context-owned memory. */
int vhr_graph_bind_external_image(vhr_context *ctx, const char *image_name, void *device_ptr);

/* ---------------------------------------------------------------------------------------------
 * RaytracingExecutionContext (src/render_graph/raytracing_execution_context.h:13)
 * ------------------------------------------------------------------------------------------- */
/* TraceRays(width, height) -> vkCmdTraceRaysKHR(w, h, 1) (raytracing_execution_context.cpp:4-13) */
int vhr_trace_rays(vhr_raytracing_execution_context *exec, uint32_t width, uint32_t height);

/* ---------------------------------------------------------------------------------------------
 * ComputeExecutionContext (src/render_graph/compute_execution_context.h:17-31)
 * ------------------------------------------------------------------------------------------- */
/* GetDisplaySize (:17) */
int vhr_compute_get_display_size(vhr_compute_execution_context *exec, uint32_t *width, uint32_t *height);
/* Dispatch (:18) and Dispatch<T> (:20-27): push constants are copied at call time (vkCmdPushConstants),
 * push_constants_size must equal the size declared at registration (assert at :23). */
int vhr_compute_dispatch(vhr_compute_execution_context *exec, const char *shader, uint32_t x_groups,
                         uint32_t y_groups, uint32_t z_groups, const void *push_constants,
                         uint32_t push_constants_size);
/* BlitImageStorageToTransient / TransientToStorage / StorageToStorage (:29-31, .cpp:31-176): same-extent
 * VK_FILTER_NEAREST blits == copies */
int vhr_compute_blit_image_storage_to_transient(vhr_compute_execution_context *exec, int32_t src, const char *dst);
int vhr_compute_blit_image_transient_to_storage(vhr_compute_execution_context *exec, const char *src, int32_t dst);
int vhr_compute_blit_image_storage_to_storage(vhr_compute_execution_context *exec, int32_t src, int32_t dst);

/* ---------------------------------------------------------------------------------------------
 * HybridRenderPath (src/render_paths/hybrid_render_path.{h,cpp}, render_path.{h,cpp}) re-hosted on the
 * API above; these entry points expose the C++ re-host (csrc/hybrid_render_path.cpp) to C callers.
 * ------------------------------------------------------------------------------------------- */
typedef struct vhr_hybrid_render_path vhr_hybrid_render_path;
typedef struct vhr_hybrid_settings {
    int32_t shadow_mode;             /* 0 raytraced, 1 rasterized, 2 off   (hybrid_render_path.h:4-8)  */
    int32_t ambient_occlusion_mode;  /* 0 raytraced, 1 ssao, 2 off        (hybrid_render_path.h:10-14) */
    int32_t reflection_mode;         /* 0 raytraced, 1 ssr, 2 off         (hybrid_render_path.h:16-20) */
    int32_t denoise_shadow_and_ao;   /* bool                              (hybrid_render_path.h:35)    */
    int32_t atrous_steps;            /* 5 in the reference (hybrid_render_path.cpp:299)               */
} vhr_hybrid_settings;
/* g-buffer / composition are external passes: callbacks may be NULL */
int  vhr_hybrid_create(vhr_context *ctx, const vhr_hybrid_settings *settings,
                       vhr_external_pass_callback gbuffer_pass, void *gbuffer_user,
                       vhr_external_pass_callback composition_pass, void *composition_user,
                       vhr_hybrid_render_path **out);
void vhr_hybrid_destroy(vhr_hybrid_render_path *path);      /* DeregisterPath + free */
int  vhr_hybrid_build(vhr_hybrid_render_path *path);        /* RenderPath::Build   (render_path.cpp:14-20) */
int  vhr_hybrid_rebuild(vhr_hybrid_render_path *path, const vhr_hybrid_settings *settings); /* Rebuild (:22-27) */
int  vhr_hybrid_get_push_constants(vhr_hybrid_render_path *path, vhr_svgf_push_constants *out);
const char *vhr_hybrid_last_error(vhr_hybrid_render_path *path);
/* Checkpoint / resume of the path's cross-frame state (the reference has none; its only state that survives a frame is
 * the five persistent SVGF storage images of hybrid_render_path.cpp:247-262, the previous frame's view / projection matrices and
 * frame_index, renderer.cpp:187-190,202).  The blob is host memory: a header (extent, formats, byte counts), the PerFrameData the last
 * vhr_graph_execute ran with -- a restored renderer continues with view_prev / proj_prev = its view / proj and frame_index + 1, which is
 * what Renderer::Render's function-static carries --, then the images in the order integrated[0], integrated[1], previous normals, history,
 * moments history, each as the path's NEXT frame will see it (the moments double buffer's current side; the ping-pong pair in its
 * frame-start order), so a blob loads into any path of the same extent whatever pool indices that path was given.  A context restored
 * from a blob continues bit-identically (tests/test_gpu_svgf.py).  `last_frame` may be NULL.  Options are no part of the blob -- "alpha_test_rays"
 * included: a restored renderer sets it again if it had it on. */
int  vhr_hybrid_state_size(vhr_hybrid_render_path *path, uint64_t *bytes);
int  vhr_hybrid_save_state(vhr_hybrid_render_path *path, void *blob, uint64_t bytes);
int  vhr_hybrid_load_state(vhr_hybrid_render_path *path, const void *blob, uint64_t bytes, vhr_per_frame_data *last_frame);
/* The PerFrameData the last vhr_graph_execute of the context ran with (zeros before the first). */
int  vhr_get_last_per_frame_ubo(vhr_context *ctx, vhr_per_frame_data *out);

/* ---------------------------------------------------------------------------------------------
 * RaytracedRenderPath (src/render_paths/raytraced_render_path.{h,cpp}) re-hosted on
 * the API above (csrc/raytraced_render_path.cpp): "Raytracing Pass" -> "RaytracedOutput" (B8G8R8A8_UNORM) ->
 * external "Composition Pass".  use_anyhit_shader = the "Alpha test for shadows" switch (raytraced_render_path.h:15).
 * ------------------------------------------------------------------------------------------- */
typedef struct vhr_raytraced_render_path vhr_raytraced_render_path;
int  vhr_raytraced_create(vhr_context *ctx, int32_t use_anyhit_shader, vhr_external_pass_callback composition_pass,
                          void *composition_user, vhr_raytraced_render_path **out);
void vhr_raytraced_destroy(vhr_raytraced_render_path *path);
int  vhr_raytraced_build(vhr_raytraced_render_path *path);                              /* RenderPath::Build (render_path.cpp:14-20) */
int  vhr_raytraced_rebuild(vhr_raytraced_render_path *path, int32_t use_anyhit_shader); /* toggle + Rebuild (raytraced_render_path.cpp:90-92) */
const char *vhr_raytraced_last_error(vhr_raytraced_render_path *path);

/* ---------------------------------------------------------------------------------------------
 * RayqueryRenderPath (src/render_paths/rayquery_render_path.{h,cpp}) re-hosted on the API above (csrc/rayquery_render_path.cpp): one
 * external graphics pass, "Forward Pass", with the outputs RENDER_OUTPUT (binding 0) and "Depth" (D32_SFLOAT, binding 1, clear depth 0)
 * (:12-18).  The path owns nothing and has no settings.  Its raster body is the integrator's (forward_pass, may be NULL);
 * vhr_standin_rayquery_forward is the library's stand-in for it.
 * ------------------------------------------------------------------------------------------- */
typedef struct vhr_rayquery_render_path vhr_rayquery_render_path;
int  vhr_rayquery_create(vhr_context *ctx, vhr_external_pass_callback forward_pass, void *forward_user, vhr_rayquery_render_path **out);
void vhr_rayquery_destroy(vhr_rayquery_render_path *path);
int  vhr_rayquery_build(vhr_rayquery_render_path *path);       /* RenderPath::Build (render_path.cpp:14-20), at the context's display extent */
int  vhr_rayquery_rebuild(vhr_rayquery_render_path *path);     /* RenderPath::Rebuild (render_path.cpp:21-27) */
const char *vhr_rayquery_last_error(vhr_rayquery_render_path *path);

/* ---------------------------------------------------------------------------------------------
 * ForwardRasterRenderPath (src/render_paths/forward_raster_render_path.{h,cpp}) re-hosted on the API above
 * (csrc/forward_raster_render_path.cpp): two external graphics passes.  "Depth Prepass" (:12-50) writes "ShadowMap" (4096 x 4096
 * D32_SFLOAT, clear depth 0); "Forward Pass" (:52-96) samples it and writes RENDER_OUTPUT (binding 0) and "Depth" (D32_SFLOAT, binding 1,
 * clear depth 0), both multisampled when enable_msaa (the default, forward_raster_render_path.h:14).  A multisampled RENDER_OUTPUT makes the
 * graph create "Forward Pass_MSAA" (B8G8R8A8_SRGB, 8 samples) to resolve from (render_graph.cpp:929-945).  The bodies are the integrator's
 * (either may be NULL); vhr_standin_shadow_map and vhr_standin_forward_raster are the library's stand-ins for them.
 * ------------------------------------------------------------------------------------------- */
typedef struct vhr_forward_raster_render_path vhr_forward_raster_render_path;
int  vhr_forward_raster_create(vhr_context *ctx, vhr_external_pass_callback depth_prepass, void *depth_user, vhr_external_pass_callback forward_pass,
                               void *forward_user, int32_t enable_msaa, vhr_forward_raster_render_path **out);
void vhr_forward_raster_destroy(vhr_forward_raster_render_path *path);
int  vhr_forward_raster_build(vhr_forward_raster_render_path *path);    /* RenderPath::Build (render_path.cpp:14-20), at the context's display extent */
int  vhr_forward_raster_rebuild(vhr_forward_raster_render_path *path, int32_t enable_msaa);   /* toggle + Rebuild (forward_raster_render_path.cpp:99-111) */
const char *vhr_forward_raster_last_error(vhr_forward_raster_render_path *path);

/* ---------------------------------------------------------------------------------------------
 * Harness / test access (no reference counterpart: the reference inspects images through its ImGui
 * debug-texture viewer, renderer.cpp:215-224)
 * ------------------------------------------------------------------------------------------- */
typedef struct vhr_image_info {
    void    *device_ptr;      /* linear, row-major, tightly packed */
    uint32_t width, height;
    int32_t  format;
    uint32_t bytes_per_pixel;
} vhr_image_info;
int vhr_get_display_size(vhr_context *ctx, uint32_t *width, uint32_t *height);   /* context.swapchain.extent */
int vhr_get_transient_image(vhr_context *ctx, const char *name, vhr_image_info *out);
int vhr_get_storage_image(vhr_context *ctx, int32_t id, vhr_image_info *out);
/* Samples per texel of a transient image: 1, or 8 for one declared multisampled (VK_SAMPLE_COUNT_8_BIT, render_graph.cpp:341).  An 8-sample
 * image is pixel-major with a pixel's 8 samples consecutive in the standard sample order; its bytes_per_pixel (vhr_image_info) covers all
 * 8 samples, so width * height * bytes_per_pixel is still the allocation and the byte count of an upload or download. */
int vhr_get_transient_image_samples(vhr_context *ctx, const char *name, uint32_t *samples);
/* synchronous copies (stream-ordered, then waited) */
int vhr_upload_transient_image(vhr_context *ctx, const char *name, const void *host_data, uint64_t bytes);
int vhr_download_transient_image(vhr_context *ctx, const char *name, void *host_data, uint64_t bytes);
int vhr_upload_storage_image(vhr_context *ctx, int32_t id, const void *host_data, uint64_t bytes);
int vhr_download_storage_image(vhr_context *ctx, int32_t id, void *host_data, uint64_t bytes);

/* Stand-in producer for the untouched G-buffer stage (gbuf.vert:19-28, gbuf.frag:17-59): casts primary
 * rays through the same BVH and writes the three named transient images with gbuf.frag's encodings
 * (normals+object id RGBA16F, motion+metallic/roughness RGBA16F, reverse-Z depth D32F) and the clears of
 * hybrid_render_path.cpp:16-19.  Alpha-masked / fully transparent fragments are discarded like gbuf.frag:27-32 (the
 * primary ray steps past them, up to 32 layers) and normal maps perturb the normal like :35-41 (SURVEY.md section 8 row
 * f2).  Uses the per-frame data of resource_idx. */
int vhr_standin_gbuffer(vhr_context *ctx, uint32_t resource_idx, const char *normals_image,
                        const char *motion_image, const char *depth_image);
/* same, also writing the "Albedo" attachment (B8G8R8A8_UNORM, gbuf.frag:19-33) */
int vhr_standin_gbuffer_with_albedo(vhr_context *ctx, uint32_t resource_idx, const char *albedo_image, const char *normals_image,
                                    const char *motion_image, const char *depth_image);

/* Stand-in for the rasterised "Shadow Map Pass" (hybrid_render_path.cpp:58-99, depth_prepass.vert:16-19; BASELINE configs[0]'s
 * shadow map): fills the named square D32_SFLOAT transient image ("Shadow Map", 4096 x 4096) with the depth of the closest hit of
 * the orthographic ray through every texel centre of PerFrameData.directional_light.projview's frustum (reverse Z: 1 on the near
 * plane, clear value 0 where nothing is hit).  A ray caster on the path's own BVH, not a rasteriser. */
int vhr_standin_shadow_map(vhr_context *ctx, uint32_t resource_idx, const char *shadow_map_image);

/* Next row: stand-in for the untouched composition stage -- composition.vert:5-8 +
 * composition.frag:60-161: shadows ray traced (0), from the shadow map with the shader's 16-tap PCF (1, :81-107) or off (2);
 * ambient occlusion and reflections ray traced (0), screen space (1: ssao.comp + ssao_blur.comp / ssr.comp, row f4) or
 * off (2).  Reads the named transient images, writes swapchain-format texels (B8G8R8A8_SRGB, bytes
 * b g r a, presentation orientation: row 0 = top) into a storage image of 4-byte texels.
 * Refused with VHR_ERROR_INVALID_ARGUMENT, nothing launched: image extents that differ from the depth image's, formats other than
 * 4-byte texels (albedo, output), R16G16B16A16_SFLOAT (normals, motion, ssao), D32_SFLOAT (depth, shadow map) and R16G16_SFLOAT or
 * R16G16B16A16_SFLOAT (shadow_ao), a mode outside 0 .. 2, shadow_mode 1 without a square D32 shadow map, ambient_occlusion_mode 1 without
 * ssao, and reflection_mode 0 or 1 without a reflections image: the blend of composition.frag:139-156 is never skipped silently (the
 * kernel itself would skip it).  These checks follow the host-only refusal (VHR_ERROR_NO_DEVICE) and the image look-up (VHR_ERROR_NOT_FOUND). */
typedef struct vhr_composition_desc {
    int32_t shadow_mode, ambient_occlusion_mode, reflection_mode;      /* the three specialization constants, :6-8 */
    const char *albedo_image, *normals_image, *motion_image, *depth_image;
    const char *shadow_ao_image;      /* "Denoised Raytraced Shadows and Ambient Occlusion" or the raw RG16F image (:353-355) */
    const char *reflections_image;    /* "Raytraced Reflections" (mode 0) / "Screen Space Reflections" (mode 1); may be NULL for mode 2 only */
    int32_t output_storage_image;
    const char *ssao_image;           /* "Screen Space Ambient Occlusion" for ambient_occlusion_mode 1, else may be NULL */
    const char *shadow_map_image;     /* "Shadow Map" (square D32_SFLOAT) for shadow_mode 1, else may be NULL */
} vhr_composition_desc;
int vhr_standin_composition(vhr_context *ctx, uint32_t resource_idx, const vhr_composition_desc *desc);

/* Next row: the raytraced render path (raytraced_render_path.cpp:11-76).  Its "Raytracing Pass"
 * is registered through vhr_graph_add_raytracing_pass with the shader set
 *   raygen "raytraced_render_path/raygen.rgen", miss { ".../miss.rmiss", ".../shadow_miss.rmiss" },
 *   hit group 0 { closest_hit ".../closesthit.rchit" }                                   (:19-34, use_anyhit_shader == 0)
 * or raygen ".../raygen_test_alpha.rgen", the same miss shaders,
 *   hit group 0 { closest_hit ".../closesthit_test_alpha.rchit", any_hit ".../shadow_anyhit.rahit" }   (use_anyhit_shader == 1)
 * and one storage-image output at binding 0 ("RaytracedOutput", B8G8R8A8_UNORM, :15); vhr_trace_rays then launches the
 * primary-ray kernel.  This entry is the stand-in for the path's untouched composition stage
 * (raytraced_render_path/composition.vert:5-8, composition.frag:11-13): the named image sampled at the texel centres and
 * written as swapchain texels (B8G8R8A8_SRGB, presentation orientation) into a storage image of 4-byte texels. */
int vhr_standin_raytraced_composition(vhr_context *ctx, const char *raytraced_output_image, int32_t output_storage_image);

/* Stand-in for the rayquery render path's "Forward Pass" (rayquery_render_path.cpp:11-54, rayquery_render_path/default.vert:19-28,
 * default.frag:16-49), called from that pass's callback.  A ray caster on the path's own BVH, not a rasteriser: per pixel the closest
 * hit of the camera ray through the near-plane point of the pixel centre (the G-buffer stand-in's ray; the raster pass discards nothing,
 * so no alpha test), then default.frag -- one terminate-on-first-hit query from in_pos (tmin 0.1) along -light.direction (tmax 10000),
 * every triangle opaque, and 0.2 * albedo + max(dot(N, L), 0) * albedo * light.color * in_shadow, alpha 1, without light.intensity.
 * Uses the per-frame data of resource_idx and computes the whole display (strips and screen tiles are out of scope).  Writes:
 *   output_storage_image  a pool storage image of 4-byte texels: swapchain texels (B8G8R8A8_SRGB, bytes b g r a), in the presentation
 *                         orientation vhr_standin_composition writes (row 0 = top); a miss is (0, 0, 0, 0)
 *   depth_image           the transient "Depth" (D32_SFLOAT): reverse-Z clip.z / clip.w in the G-buffer stand-in's orientation, 0 for a miss
 *   three optional probes in device memory (NULL = not written), one entry per pixel in Depth's row order:
 *     primary_hits        the committed primary hit (geometry_index 0xFFFFFFFF where nothing is hit; t in the ray's parameterisation,
 *                         1 = the near plane), 4-byte aligned
 *     positions           4 floats: in_pos and w = 1 where covered, (0, 0, 0, 0) where not, 4-byte aligned
 *     shadowed            1 = the inline query found an occluder (0 for a miss)
 * With vhr_set_ray_statistics on, vhr_get_ray_statistics reports one primary ray per pixel + one query per covered pixel, and the
 * stack overflows.  "variant_rayquery" picks the kernel (vhr_set_option); kernel timing kind 10. */
typedef struct vhr_rayquery_forward_desc {
    int32_t output_storage_image;
    const char *depth_image;
    vhr_ray_hit *primary_hits;
    float *positions;
    uint8_t *shadowed;
} vhr_rayquery_forward_desc;
int vhr_standin_rayquery_forward(vhr_context *ctx, uint32_t resource_idx, const vhr_rayquery_forward_desc *desc);

/* Stand-in for the forward raster path's "Forward Pass" (forward_raster_render_path.cpp:52-96, default.vert, forward_raster_render_path/
 * default.frag), called from that pass's callback.  A ray caster on the path's own BVH, not a rasteriser.  S = 8 samples per pixel when
 * "Depth" has 8 (enable_msaa), else 1 at the pixel centre.  The 8 positions are Vulkan's standard locations, in pixel units from the
 * pixel's top-left corner, y down in framebuffer rows: (0.5625,0.3125) (0.4375,0.6875) (0.8125,0.5625) (0.3125,0.1875) (0.1875,0.8125)
 * (0.0625,0.4375) (0.6875,0.9375) (0.9375,0.0625).  A sample's ray is the G-buffer stand-in's camera ray through the sample's point on the
 * near plane (tmin 1).  Its visible triangle: the nearest hit (ties: the smaller flat index) among the triangles whose fragment at this
 * pixel is not discarded; that decision (alpha_mask == 1 && albedo.a < alpha_cutoff, albedo = base_color without a texture) uses the
 * triangle's attributes at the PIXEL CENTRE (the centre ray against the triangle's plane, extrapolated outside it), as the raster pipeline
 * without sample shading does.  Each distinct visible triangle of a pixel is shaded once, at the pixel centre: albedo / pi +
 * max(dot(N, L), 0) * albedo * light.color (shadow forced to 1, alpha 1).  Uses the per-frame data of resource_idx and computes the whole
 * display (strips and screen tiles are out of scope).  Everything is in framebuffer rows (row 0 = the top of the presented image).  Writes:
 *   output_storage_image  a pool storage image of 4-byte texels: the resolved swapchain texels (B8G8R8A8_SRGB, bytes b g r a).  With 8
 *                         samples: per channel the fp32 mean, summed in sample order, of the samples' decoded values (colour from sRGB,
 *                         alpha as UNORM), encoded like every sRGB store here -- Vulkan leaves the arithmetic of an sRGB resolve to the
 *                         implementation, and this is the library's; with 1 sample: the sample itself.  Nothing hit: (0, 0, 0, 0)
 *   depth_image           the transient "Depth" (D32_SFLOAT, 1 or 8 samples): reverse-Z clip.z / clip.w of each sample's own hit, 0 for a miss
 *   msaa_image            the transient "Forward Pass_MSAA" (B8G8R8A8_SRGB, 8 samples): the shaded samples; required when "Depth" has 8
 *                         samples and NULL otherwise (else VHR_ERROR_INVALID_ARGUMENT)
 *   two optional probes in device memory (NULL = not written):
 *     sample_hits         vhr_ray_hit per sample (t in the ray's parameterisation, 1 = the near plane; geometry_index 0xFFFFFFFF for a miss),
 *                         pixel-major with a pixel's samples consecutive, 4-byte aligned
 *     fragments           uint8_t per pixel: the number of fragments shaded (distinct visible triangles)
 * With vhr_set_ray_statistics on, vhr_get_ray_statistics counts W x H x S primary rays.  "variant_standin_forward_raster" picks the kernel
 * (vhr_set_option); kernel timing kind 11. */
typedef struct vhr_forward_raster_desc {
    int32_t output_storage_image;
    const char *depth_image;
    const char *msaa_image;
    vhr_ray_hit *sample_hits;
    uint8_t *fragments;
} vhr_forward_raster_desc;
int vhr_standin_forward_raster(vhr_context *ctx, uint32_t resource_idx, const vhr_forward_raster_desc *desc);

/* Multi-GPU row strips: this context owns rows [row_begin, row_end) of the
 * display.  Ray tracing runs on the owned rows; the SVGF kernels on the owned rows extended by `overlap`
 * rows on each side (recomputed instead of exchanged between a-trous iterations); the blits copy the owned
 * rows extended by `halo` rows (>= overlap: the rows next frame's temporal pass may read) -- a blit fused into
 * the a-trous launch that produced its source ("fuse_blits") stores that launch's rows only, which are the valid
 * ones.  All ranges are clamped to the image.  Default: whole image, overlap 0, halo 0.  The halo rows of the
 * history images are filled by the caller's neighbour exchange (vulkanhybridrenderer_amd/tiling.py over RCCL). */
int vhr_set_strip(vhr_context *ctx, uint32_t row_begin, uint32_t row_end, uint32_t overlap, uint32_t halo);
/* The same for a SCREEN TILE (BASELINE.json north_star: "the framebuffer shards by screen tile"): this context owns the rectangle
 * [col_begin, col_end) x [row_begin, row_end).  The ray queue kernels trace it (plus `overlap` pixels all round with "trace_overlap"),
 * svgf.comp and the a-trous launches compute it extended by `overlap` on both axes, the blits copy it extended by halo_rows /
 * halo_cols (>= overlap: what next frame's svgf.comp may read).  The kernels' A-B variants and the other paths' kernels compute whole
 * rows of the tile's row range instead: a superset, same results inside the rectangle.  vhr_set_strip is the all-columns case. */
int vhr_set_tile(vhr_context *ctx, uint32_t col_begin, uint32_t col_end, uint32_t row_begin, uint32_t row_end, uint32_t overlap,
                 uint32_t halo_rows, uint32_t halo_cols);

/* ---- C1 / C2: the row-strip decomposition's exchanges inside the library (RCCL point-to-point, one process per GPU) ----------
 * The reference is single-GPU (one queue, renderer.cpp:135); these calls exist for an integrator that shards the framebuffer by
 * row strips.  The row arithmetic follows the reference's SVGF schedule (hybrid_render_path.cpp:288-329:
 * the published image is the output of a-trous iteration n-2, iteration i reads +-2*2^i rows) and is the one
 * vulkanhybridrenderer_amd/tiling.py uses (tests/test_comm_plan.py compares the two).  RCCL is loaded on first use: the copy the process
 * already holds (a PyTorch process), else the ROCm installation's; vhr_comm_use_library(path), called before any other vhr_comm_* call,
 * names the library to load instead (a site's own build) -- the library reads no environment variable for this.  vhr_comm_library() says which
 * file the entry points came from.  N > 1 has not run on two DEVICES yet (rounds 1-6 had one GPU per box); world 2, 3 and 4 run on one GPU
 * through tests/rccl_shim (a stand-in for the eight RCCL entry points this file uses, handed over through vhr_comm_use_library), bit-identical to the
 * torch.distributed route and to the single context, with one injected failure per error path (tests/test_comm_shim.py).  The stand-in copies with
 * blocking host calls: the ORDER of this file's stream and event dependencies against real RCCL's asynchronous transport is what stays unverified.
 * Error handling: a failure inside a grouped batch closes the group, marks the communicator unusable and is reported; what was
 * enqueued before it is drained by vhr_comm_finish_frame_exchanges. */
typedef struct vhr_strip_plan {
    uint32_t rank, world, height;
    uint32_t row_begin, row_end;     /* owned rows [g*H/N, (g+1)*H/N) */
    uint32_t overlap;                /* E: rows the SVGF kernels recompute beyond the strip (30 for the reference's 5 iterations) */
    uint32_t halo;                   /* Hh = E + ceil(max |motion.y| * H) + 2: rows of history / moments fetched from each neighbour */
} vhr_strip_plan;
typedef struct vhr_row_exchange { int32_t peer; uint32_t send_begin, send_end, recv_begin, recv_end; } vhr_row_exchange;
/* Screen tiles: a grid of grid_rows x grid_cols rectangles, rank = tile_row * grid_cols + tile_col; tile (r, c) owns columns
 * [c*W/C, (c+1)*W/C) and rows [r*H/R, (r+1)*H/R).  Row strips are the one-column grid. */
#define VHR_TILE_MAX_GRID 16        /* tiles per axis */
typedef struct vhr_tile_plan {
    uint32_t rank, world, width, height;
    uint32_t grid_rows, grid_cols;
    uint32_t col_begin, col_end, row_begin, row_end;     /* the owned rectangle */
    uint32_t overlap;                /* E: pixels the SVGF kernels recompute beyond the rectangle, on every cut side */
    uint32_t halo_rows, halo_cols;   /* E + ceil(max |motion| * extent) + 2 on a cut axis (E on an axis that is not cut): the margin of
                                      * history / moments fetched from the neighbours */
    /* the grid's cut lines: tile (r, c) owns columns [col_cut[c], col_cut[c + 1]) and rows [row_cut[c][r], row_cut[c][r + 1]) -- every COLUMN of tiles has its
     * own row cuts (vhr_tile_plan_make: the same in every column, at equal pixels; vhr_tile_plan_make_weighted: the columns split the cost, then every column
     * splits its own).  col_cut[0] = row_cut[c][0] = 0, col_cut[grid_cols] = width, row_cut[c][grid_rows] = height.  Entries past the grid are 0. */
    uint32_t col_cut[VHR_TILE_MAX_GRID + 1], row_cut[VHR_TILE_MAX_GRID][VHR_TILE_MAX_GRID + 1];
} vhr_tile_plan;
typedef struct vhr_rect { uint32_t x0, x1, y0, y1; } vhr_rect;                 /* [x0, x1) x [y0, y1) */
typedef struct vhr_rect_exchange { int32_t peer; vhr_rect send, recv; } vhr_rect_exchange;     /* an empty rectangle is all zeros */
#define VHR_COMM_UNIQUE_ID_BYTES 128
typedef struct vhr_comm vhr_comm;

uint32_t vhr_atrous_overlap(uint32_t atrous_steps);
uint32_t vhr_atrous_output_extent(uint32_t overlap, uint32_t step);     /* what "strip_shrink_overlap" makes an a-trous launch compute */
/* VHR_ERROR_OUT_OF_SLOTS when the thinnest strip is thinner than the history halo (use fewer GPUs or a taller image) */
int vhr_strip_plan_make(uint32_t height, uint32_t world, uint32_t rank, uint32_t max_motion_rows, uint32_t atrous_steps, vhr_strip_plan *out);
/* the neighbours' row ranges of an n_rows-deep halo; returns their number (0..2) */
int vhr_strip_plan_exchanges(const vhr_strip_plan *plan, uint32_t n_rows, vhr_row_exchange out[2]);

/* (grid_rows, grid_cols) with grid_rows * grid_cols == world that makes a rank compute the fewest pixels, (W / cols + 2E) x (H / rows + 2E) */
int vhr_tile_grid_choose(uint32_t width, uint32_t height, uint32_t world, uint32_t overlap, uint32_t *grid_rows, uint32_t *grid_cols);
/* grid_rows == 0 or grid_cols == 0: vhr_tile_grid_choose picks the grid.  VHR_ERROR_OUT_OF_SLOTS when a tile is thinner than its halo. */
int vhr_tile_plan_make(uint32_t width, uint32_t height, uint32_t world, uint32_t rank, uint32_t grid_rows, uint32_t grid_cols, uint32_t max_motion_rows,
                       uint32_t max_motion_cols, uint32_t atrous_steps, vhr_tile_plan *out);
/* The same grid cut at EQUAL COST instead of equal pixels (round 6).  cost[cy * cost_cols + cx] = what the (cell x cell)-pixel block at
 * (cx * cell, cy * cell) costs to trace -- e.g. the any-hit queue kernel's wave lifetimes of a whole-image frame (vhr_debug_wave_lifetimes: one
 * word per 8 x 8 tile, cell = 8); cost_cols >= ceil(width / cell), cost_rows >= ceil(height / cell).  Column cuts split the column sums, row cuts the
 * cost inside each column of tiles (a column's row cuts are its own: tiles of neighbouring columns meet at different heights, which the exchanges -- rectangle
 * intersections with every peer -- do not mind): cut j is the first cell boundary at which the running sum reaches j / n of the total, moved as far as the
 * halos require (no tile thinner than its halo).  cost == NULL or an all-zero map: equal pixels.  Placement
 * only: the images are those of any other plan, bit for bit.  Every rank must be given the same map. */
int vhr_tile_plan_make_weighted(uint32_t width, uint32_t height, uint32_t world, uint32_t rank, uint32_t grid_rows, uint32_t grid_cols, uint32_t max_motion_rows,
                                uint32_t max_motion_cols, uint32_t atrous_steps, const uint32_t *cost, uint32_t cost_cols, uint32_t cost_rows, uint32_t cell,
                                vhr_tile_plan *out);
/* the rectangles a margin of (halo_rows, halo_cols) pixels takes from / gives to each peer (up to 8); returns their number or < 0 */
int vhr_tile_plan_exchanges(const vhr_tile_plan *plan, uint32_t halo_rows, uint32_t halo_cols, vhr_rect_exchange *out, uint32_t capacity);
/* A re-plan between two frames (the grid cut again, e.g. vhr_tile_plan_make_weighted on a cost map scaled by the ranks' measured frame times): what carries the
 * path's cross-frame state -- the storage images SVGFPushConstants names shadow_and_ao_history, shadow_and_ao_moments_history and
 * prev_frame_normals_and_object_ids (hybrid_render_path.cpp:247-262) -- to the new rectangles.  recv = the pixels of this rank's NEW rectangle grown by the new
 * halo that `peer` OWNED under the old plan (its values are exact there), send = the mirror image; what the rank owned itself stays where it is.  Both plans of
 * the same rank, world and image; up to world - 1 entries; returns their number or < 0.  After the transfers: vhr_set_tile with the new rectangle. */
int vhr_tile_plan_replan(const vhr_tile_plan *old_plan, const vhr_tile_plan *new_plan, vhr_rect_exchange *out, uint32_t capacity);

/* The RCCL library to load, instead of the process's own / the ROCm installation's: before the first other vhr_comm_* call of the process
 * (VHR_ERROR_GRAPH afterwards: the entry points are bound once); NULL or "" = the default resolution.  A path that does not load fails the next call. */
int vhr_comm_use_library(const char *path);
/* The file the RCCL entry points were resolved from (resolves them if nobody has yet), or the reason they could not be. */
const char *vhr_comm_library(void);
int vhr_comm_get_unique_id(uint8_t out[VHR_COMM_UNIQUE_ID_BYTES]);      /* ncclGetUniqueId on one rank; the caller hands it to the others */
/* ncclCommInitRank + vhr_set_strip(plan) / vhr_set_tile(plan): collective over the `world` processes of the plan.  The plan must be one
 * the planner returns (it is recomputed and compared: two ranks that disagree on a rectangle would hang RCCL).  vhr_comm_destroy gives the
 * context the whole image back. */
int vhr_comm_create(vhr_context *ctx, const vhr_strip_plan *plan, const uint8_t unique_id[VHR_COMM_UNIQUE_ID_BYTES], vhr_comm **out);
int vhr_comm_create_tiled(vhr_context *ctx, const vhr_tile_plan *plan, const uint8_t unique_id[VHR_COMM_UNIQUE_ID_BYTES], vhr_comm **out);
void vhr_comm_destroy(vhr_comm *comm);
const char *vhr_comm_last_error(const vhr_comm *comm);
/* Raytrace Pass epilogue, only with "trace_overlap" off: the overlap rows of the raw shadow / AO image from the neighbours, in the
 * context's stream order (exchange #1). */
int vhr_comm_exchange_raytraced(vhr_comm *comm, const char *raytraced_image);
/* SVGF pass epilogue: exchange #2 (halo rows of the history and of the moments history just written, for the NEXT frame's
 * svgf.comp) and, if denoised_image != NULL, the gather of every rank's owned rows into `gathered_frame` on `root` (a device
 * buffer of the whole image there).  Issued on the communicator's own stream behind the context's work so far -- beside the next
 * frame's ray tracing -- and not waited for. */
int vhr_comm_start_frame_exchanges(vhr_comm *comm, int32_t history_storage_image, int32_t moments_storage_image, const char *denoised_image,
                                   int32_t root, void *gathered_frame);
/* Raytrace Pass epilogue of the next frame: the context's stream waits for them (no host synchronisation). */
int vhr_comm_finish_frame_exchanges(vhr_comm *comm);
/* A re-plan between two frames through the library's own RCCL calls: the communicator and the context take `new_plan` (vhr_tile_plan_make_weighted on the map
 * every rank holds; same rank, world and image as the plan the communicator was created with), and the three storage images that carry the path's state from frame
 * to frame travel to the new rectangles (vhr_tile_plan_replan), one grouped batch in the context's stream order.  Collective: every rank, between the same two
 * frames.  The previous frame's exchanges are finished first; a plan of another rank / world / image is refused before anything is enqueued. */
int vhr_comm_replan(vhr_comm *comm, const vhr_tile_plan *new_plan, int32_t history_storage_image, int32_t moments_storage_image, int32_t prev_normals_storage_image);

/* Statistics of the last vhr_trace_rays: out[0] = unique rays traced, out[1] = rays the reference would
 * issue (4x duplicate shadow ray, raygen.rgen:38-40), out[2] = covered (non-sky) pixels, out[3] = traversal
 * stack overflows (must be 0).  Requires vhr_set_ray_statistics(ctx, 1) (costs one counter flush per pass). */
int vhr_set_ray_statistics(vhr_context *ctx, int32_t enable);
int vhr_get_ray_statistics(vhr_context *ctx, uint64_t out[4]);

/* Options.  One table in the library (csrc/vhr_internal.hpp: VHR_OPTION_TABLE) holds every option's name, default, smallest and largest value;
 * vhr_option_count / vhr_option_info enumerate it, vhr_set_option refuses a value outside the range (VHR_ERROR_INVALID_ARGUMENT) and an
 * unknown name (VHR_ERROR_NOT_FOUND).  Every setting publishes identical images (the literal forms of the a-trous filter and of the mirror
 * ray within the float tolerance of tests/); what changes is which kernel runs or what is launched where.
 *  Forms of a shader -- 0 = the literal one-pixel-per-thread form (the in-tree cross-check of the default), 1 = the default:
 *   "raygen_variant"     raygen.rgen's shadow + AO rays: raygen_kernel / raygen_queue_kernel (a ray queue per 8x8-pixel tile and wave)
 *   "reflection_variant" the mirror ray + reflection_hit.rchit: reflection_kernel / reflection_queue_kernel (closest-hit queue per 16x8 tile,
 *                        shading with the whole wave; one or two bounces)
 *   "raytraced_variant"  the raytraced render path's pass: raytraced_kernel / raytraced_queue_kernel
 *   "variant_rayquery"   the rayquery render path's forward pass (vhr_standin_rayquery_forward): rayquery_forward_kernel /
 *                        rayquery_forward_queue_kernel (primary ray + inline query per 16x8 tile and wave)
 *   "variant_standin_forward_raster" the forward raster path's forward pass (vhr_standin_forward_raster): forward_raster_kernel /
 *                        forward_raster_queue_kernel (the tile's S x 128 sample rays per 16x8 tile and wave, fragments shaded by the whole wave)
 *   "atrous_variant"     svgf_atrous_filter.comp: svgf_atrous_kernel (direct cached loads, product-form weights) / svgf_atrous_tile_kernel
 *                        (LDS comb tiles, weights in the exponent)
 *  The queue kernels:
 *   "refill_threshold"   idle lanes per wave that trigger a queue refill (default 16)
 *   "lds_stack_levels"   traversal-stack entries per lane kept in LDS, deeper entries spill to scratch (default 8)
 *   "raygen_early_exit"  n/16: the inner-node loop is left once the walking lanes have dropped to that fraction of those that entered it
 *                        (0 = only when all are done; default 6 -- with "raygen_steal" filling the lanes, leaving a little earlier pays: r4)
 *   "reflection_early_exit" the same fraction for the mirror ray's (closest-hit) walk (default 8)
 *   "raygen_waves_per_block" 1, 2 or 4 tiles (= waves) per workgroup (default 2)
 *   "compact_nodes"      1 (default) = the any-hit queue kernel walks 32-byte nodes: both child boxes as centre and half extent in IEEE halves
 *                        relative to the scene centre, widened until they contain the fp32 boxes in exact arithmetic (vhr_get_bvh_form_checks),
 *                        read straight into v_fma_mix_f32 -- two 16-byte loads per visit instead of three, no unpacking; 0 = the 48-byte
 *                        nodes (fp32 centres, truncated fp32 half extents).  Boxes only cull: bit-identical.  A scene whose extent does not
 *                        fit the half range around its centre has no such nodes and is walked on the 48-byte ones.
 *   "raygen_tile_rows"   rows of the 8-pixel-wide tile a wave owns: 0 (default) = 8, or 6 for a launch whose 8x8 tiles fill less than 70 % of
 *                        the chip's wave slots (a 1080p / 8 screen tile: -8 %); 1..8 = that many (4 and 2 lose on whole frames)
 *   "raygen_cost_order"  1 (default) = the workgroups of a queue kernel's launch start in the order of their lifetimes two launches ago, longest
 *                        first: every wave leaves its lifetime, the launch's first workgroup sorts the previous launch's into 8 classes of cost
 *                        (stable inside a class) before it turns to its own tile, the next launch of the same shape on the same stream reads the
 *                        order.  No kernel, stream or event of its own; launches of >= 2 048 workgroups only.  2 = any launch (tests), 0 = row-major.
 *   "raygen_steal"       n (default 8) = once a wave's ray queue is dry and at least n of its lanes are idle, every idle lane takes the lowest pending
 *                        stack entry of a busy lane and walks that subtree for the same ray: any hit is an OR over the subtrees a ray touches, in
 *                        any order and by any lane, and the pixel keeps one "blocked" bit per ray.  sponza_proc -3 %, bistro_proc -13 % of the
 *                        launch; images identical.  0 = a lane only ever walks the rays it fetched.
 *  The a-trous kernel:
 *   "atrous_small_tiles" -1 (default) = 4-row instead of 8-row tiles when the launch has < 32 8-row tiles per CU (a 1080p frame and every screen
 *                        tile use 4-row tiles, a 4K frame 8-row ones), 0 = never, 1 = always
 *  The frame's schedule:
 *   "reflection_async"   1 (default) = the mirror ray's launch (raygen.rgen:59-65; its image is not denoised, nothing of the SVGF pass reads it) runs
 *                        on a stream of the library's own behind the shadow / AO launch, beside the SVGF pass; the context's stream waits for it
 *                        before the frame's next external pass, at the end of vhr_graph_execute and wherever the library waits or hands an
 *                        image out.  Frame with the mirror ray -2 % (sponza_proc) / -6 % (bistro_proc); "Raytrace Pass" then times the
 *                        shadow / AO launch alone and the SVGF pass's time includes what it shares with the mirror ray.  0 = in the pass, in order;
 *                        2 = as 1, and pass epilogues (vhr_graph_set_pass_epilogue) do not wait for it: for owners whose hooks touch neither the
 *                        Reflections image nor the G-buffer (the multi-GPU harness: its hooks exchange visibility and SVGF history)
 *   "fuse_blits"         1 (default) = a compute pass records its dispatches and blits and issues them when its callback returns; a same-extent
 *                        blit whose source is the output (or the normals input) of a recorded a-trous dispatch becomes a second store of that
 *                        launch instead of a copy kernel (all three blits of hybrid_render_path.cpp:310-325); 0 = every blit is a copy
 *   "svgf_elide_unread"  1 = an a-trous dispatch whose output image nothing later in its pass reads or publishes is not launched -- the
 *                        reference's fifth iteration (hybrid_render_path.cpp:299-328 publishes the fourth).  Everything the pass
 *                        publishes is bit-identical; the skipped dispatch's storage image keeps older contents: opt-in (default 0)
 *   "svgf_async_unread"  1 (default) = that dispatch is issued last, on the side stream (see "Threading and streams" at the top); only with one
 *                        frame in flight, for dispatches of >= 900 000 pixels, and when the pass itself copies what the dispatch reads of the
 *                        G-buffer normals (hybrid_render_path.cpp:319); 2 = whatever the size; 0 = every dispatch in recorded order
 *   "fuse_temporal"      1 = svgf.comp runs in the ray-tracing kernel's tile epilogues when the SVGF pass's first command is that dispatch on the
 *                        launch's own images (whole-image work, one frame in flight, no mirror ray, no epilogue hooked to the ray-tracing pass);
 *                        the pass times shift by that dispatch: default 0
 *   "frames_in_flight"   1 (default), 2 or 3; read by vhr_graph_build.  n > 1: frame f uses resource index f mod n (vulkan_common.h:9,
 *                        renderer.cpp:103-146); the passes up to and including the last ray-tracing pass are issued on a second stream beside the
 *                        previous frame's remaining passes, every graph-owned transient image exists once per index, an external binding belongs
 *                        to the index being executed, the two streams are ordered by events derived from the pass declarations
 *  Screen tiles / row strips (one process per GPU; vhr_set_tile, vhr_set_strip):
 *   "trace_overlap"      1 = the shadow / AO rays of the overlap margin are traced by this context as well, so the raw visibility needs no
 *                        neighbour exchange before svgf.comp (default 0: owned pixels only)
 *   "strip_shrink_overlap" 1 = an a-trous launch with step s computes the owned rectangle extended by overlap - (4s - 2) instead of the full
 *                        overlap -- all that can be valid, and all that is needed, after the reference's doubling schedule 1, 2, 4, ... s
 *                        (hybrid_render_path.cpp:299-319); only for callers that run that schedule (default 0)
 *  Instrumentation:
 *   "pass_timestamps"    1 (default) = begin / end stamps per ray-tracing / compute pass, written by the kernels themselves (see "Threading and
 *                        streams"); 2 = + the one-thread stamp kernel in front of external passes and at the end of vhr_graph_execute; 3 = HIP
 *                        event pairs on the dispatch packets (16 us per frame; the only form with "frames_in_flight" > 1); 0 = off
 *   "kernel_timing_stride" n >= 1: with vhr_set_kernel_timing on, only every n-th launch of a kind carries its event pair (a timed dispatch
 *                        costs ~6 us that the next kernel waits for)
 *  Not in the table (they configure the next vhr_update_geometry): "bvh_leaf_triangles" 1..4 (default 2); "bvh_builder" 1 = binned SAH on the
 *  device (default), where the reference builds its BLAS / TLAS (resource_manager.cpp:650,692,792), 0 = the same algorithm on the host
 *  (csrc/bvh_build.cpp: 8 / 28x slower to build on the two test scenes, the same tree up to the order of leaves in memory; images
 *  bit-identical; also what a host-only context and a device build deeper than the walkers' stacks fall back to -- "bvh_device_max_depth"
 *  1..40 (default 40 = those stacks) lowers the depth at which the device builder gives up, for tests of that hand-over); "bvh_host_checks" 1 =
 *  a device-built tree is fetched and the host's containment checks repeated on it (default 0: they run on the device; vhr_get_bvh_form_checks
 *  reports either); "bvh_build_threads"
 *  (host builder) 0 = up to 16 host threads (default), 1 = serial -- the tree is the same whatever the count; "bvh_presplit" 0 (default) =
 *  one reference per triangle, n = 1..400: triangles whose box wastes more than 1 % of the scene box's half area enter the build once per
 *  grid cell they pass through, with at most about n % more references than triangles (csrc/presplit.hpp, both builders, the same tree;
 *  images bit-identical, vhr_get_bvh_statistics then counts references; on a scene with such triangles the any-hit launch gains and the
 *  mirror ray's closest-hit launch loses, profiles/r5_sponza_hard.txt; vhr_get_bvh_presplit_level tells what the last build did);
 *  "bvh_frame" 1 (default) = the boxes along the frame (a rotation, found by the builder: csrc/bvh_frame.hpp) that minimises the summed area
 *  of the triangles' boxes, if that beats the world axes by 5 % -- a scene whose dominant orientation is not the world's walks up to twice as
 *  fast for it, a scene along the world axes keeps them and its tree, bit for bit (the search costs such a scene ~1.5 ms of K0) --, 0 = the world
 *  axes whatever the scene; a box in a frame is padded by 1e-3 + 1e-5 |frame coordinate| + 2^-18 W, W = the power of two at or above twice the
 *  largest |world coordinate| of the triangles when the tree was built (the rotation's rounding follows the world magnitude; on the world axes
 *  the last term is 0); the walkers rotate a ray once for the box tests and intersect triangles in world space as ever: images
 *  bit-identical, both builders, the same tree (vhr_get_bvh_frame tells which frame the current tree uses; "bvh_presplit" is not combined with a rotated frame).
 *  Not in the table either, because it CHANGES IMAGES (the table's entries are result-neutral), and read at every launch: "alpha_test_rays"
 *  0 (default) = every triangle is opaque to the hybrid path's shadow, AO and mirror rays, as in the reference's hybrid path
 *  (raygen.rgen:32-65); 1 = a candidate hit that gbuf.frag:20-32, evaluated at the hit, would discard does not exist for those rays, both
 *  bounces of the two-bounce extension included -- uv0 interpolated at the hit, albedo = base_color without a base-colour texture, else the
 *  texture through its own sampler at LOD 0; discarded iff (alpha_mask == 1 && albedo.a < alpha_cutoff) || albedo.a == 0 -- so that a ray
 *  sees what the raster pass drew: a fence's shadow, occlusion and mirror image have the fence's holes.  An ignored candidate is skipped
 *  before anything else sees it: it ends no any-hit ray, shrinks no closest t and takes no part in the (t, flat index) tie-break; decision
 *  (vi) comes first, the binary64 re-decision or its deferral included.  This is the G-buffer's rule, not shadow_anyhit.rahit's, which the
 *  raytraced render path keeps.  vhr_update_geometry looks once whether any primitive CAN discard (alpha_mask == 1, a base-colour texture,
 *  or untextured with base_color[3] == 0; a texture's alpha bytes are not scanned): where none can, 1 launches exactly the kernels 0
 *  launches.  Where one can, "fuse_temporal" does not fuse (the epilogue has no alpha form: the SVGF pass runs its own dispatch) and the
 *  launches cost what profiles/alpha_rays_rate.jsonl reports.  vhr_get_option returns this key (not the bvh_* keys); a host-only context
 *  accepts it; it is no part of vhr_hybrid_save_state's blob, of vhr_hybrid_settings or of vhr_trace_params.
 *  "object_motion_vectors" is the third key of that kind (it changes the motion image; not in the table; vhr_get_option returns it; every
 *  context accepts it; refused inside a pass): 0 (default) / 1, described at "Object motion vectors" below the refit calls.
 *  "shadow_ray_mask", "ao_ray_mask", "reflection_ray_mask" (0..255, default 255; they change images, so not in the table; vhr_get_option
 *  returns them; every context accepts them; read at every launch of the hybrid path's rays): the cull mask traceRayEXT is given for that
 *  class of rays (raygen.rgen:39-40,51-52,64 pass 0xFF) -- a candidate hit on primitive p does not exist for the ray iff
 *  (masks[p] & mask) == 0 (vhr_set_primitive_masks, "Ray cull masks" below); the reflection mask holds for both bounces.  A launch none of
 *  whose masks ACTS on the masks the primitives carry is exactly the launch it was without them; where the shadow or AO mask acts,
 *  "fuse_temporal" does not fuse (the epilogue form has no filter, as with alpha).  No part of vhr_trace_params, vhr_hybrid_settings or
 *  vhr_hybrid_save_state's blob.  The rayquery, forward-raster and raytraced render paths ignore these keys and the primitives' masks, as
 *  they ignore "alpha_test_rays". */
int vhr_set_option(vhr_context *ctx, const char *key, int32_t value);
int vhr_get_option(vhr_context *ctx, const char *key, int32_t *value);
int32_t vhr_option_count(void);
int vhr_option_info(int32_t index, const char **name, int32_t *default_value, int32_t *min_value, int32_t *max_value);

/* Per-kernel timing with HIP event pairs attached to every launch of a kernel kind on the context stream (the events ride on
 * the dispatch packet -- hipExtLaunchKernelGGL's start / stop events, the dispatch's own begin / end timestamps -- instead of
 * hipEventRecord, whose barrier packet costs ~4 us of stream time per record)
 * kind: 0 = raygen (K1: shadow + AO rays; with raygen_variant 0 also the mirror ray), 1 = svgf.comp (K3),
 * 2 = svgf_atrous_filter.comp (K4) on the context's stream, 3 = blits (K5), 4 = the mirror-ray kernel (K1's reflection ray + K2),
 * 5 / 6 / 7 = ssao.comp / ssao_blur.comp / ssr.comp, 8 = K4 dispatches issued on the side stream ("svgf_async_unread"),
 * 9 = vhr_ray_query (its two launches, each counted: the walk and decision (vi)'s binary64 redo), 10 = vhr_standin_rayquery_forward,
 * 11 = vhr_standin_forward_raster.
 * kind_mask has bit (1 << kind) set for every kind to time (0 = off).  vhr_get_kernel_time synchronises, folds
 * the recorded pairs into (total milliseconds, launch count) and optionally resets the totals. */
int vhr_set_kernel_timing(vhr_context *ctx, int32_t kind_mask);
int vhr_get_kernel_time(vhr_context *ctx, int32_t kind, double *total_ms, uint64_t *launches, int32_t reset);

/* Traversal work of the last vhr_trace_rays (work-queue raygen, statistics enabled): out[0] = inner-node
 * visits summed over lanes, out[1] = leaf visits, out[2] = ray/triangle tests, out[3] = trips of the two inner
 * loops (node steps + triangle tests) counted once per wave, i.e. by the slowest lane of each round.
 * Active-lane utilisation of the traversal loops = (out[0] + out[2]) / (64 * out[3]). */
/* A hash of the sources this library was built from (16 hex digits).  profiles/pmc_*.json carry the fingerprint of the library their
 * counters were collected on; bench.py quotes them only when it equals the loaded library's. */
const char *vhr_source_fingerprint(void);
/* Diagnostics: the lifetimes (shader clock ticks) of the last ray-tracing launch's waves, as left for "raygen_cost_order"
 * (index = tile pair * waves per workgroup + wave); *count = entries written. */
int vhr_debug_wave_lifetimes(vhr_context *ctx, uint32_t *out, uint32_t capacity, uint32_t *count);
/* Decision (vi) -- the ray / triangle test every walker of the library makes (fp32 Moeller-Trumbore in a fixed order; a candidate whose solution contradicts
 * itself decided again in binary64; the reference leaves this to the driver's traceRayEXT, raygen.rgen:39,51,64) -- on explicit pairs, for parity tests:
 * pairs = count x 17 floats (o[3], d[3], v0[3], e1[3], e2[3], tmin, tmax), HOST memory; hit[count] = 0 / 1, tuv[count x 3] = (t, u, v) of a hit, else 0. */
int vhr_debug_ray_triangle(vhr_context *ctx, const float *pairs, uint32_t count, uint32_t *hit, float *tuv);
/* Diagnostics: the leaf records, nine floats per triangle (v0, e1, e2), to HOST memory in flat triangle order (primitive-major, as the
 * arrays of vhr_update_geometry list them), so the result does not depend on the tree.  previous = 0: the current records; 1: the previous
 * ones (VHR_ERROR_GRAPH with "object_motion_vectors" off).  *count = the scene's triangles, also when capacity_triangles is too small
 * (VHR_ERROR_INVALID_ARGUMENT).  A "bvh_presplit" tree with split references has several records per triangle: VHR_ERROR_UNSUPPORTED.
 * Waits for the context's streams; works on a host-only context. */
int vhr_debug_triangle_records(vhr_context *ctx, int32_t previous, float *out, uint32_t capacity_triangles, uint32_t *count);
/* Diagnostics: the tree's arrays as the walkers read them, byte for byte, to HOST memory -- the bytes in device memory on a device context,
 * the host builder's on a host-only one -- for a judge outside the library (tests/tree_truth.py decodes them from the layouts'
 * description and compares them with exact geometry).  nodes: 64 bytes per node, both child boxes as (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z)
 * floats, then child0, child1, two unused words; nodes_ch: 64 bytes, (c0.x, c1.x, c0.y, c1.y, c0.z, c1.z), h0[3], h1[3], child0, child1,
 * two unused words; nodes48: 48 bytes, the same six centres, three words of two upper-16 half extents each ((h0.x, h0.y), (h0.z, h1.x),
 * (h1.y, h1.z), the first in bits 31..16), child0, child1, one unused word; nodes16: 32 bytes, six IEEE-half centres relative to the
 * scene centre (c0.x, c1.x, c0.y, c1.y, c0.z, c1.z), six half extents in the same order, child0, child1.  A child >= 0 is an inner node's
 * index (nodes, nodes_ch) or its byte offset (nodes48, nodes16); a child < 0 is a leaf, v = ~child, first record v >> 2, (v & 3) + 1 records.
 * records: 48 bytes per record in slot order -- v0[3], e1[3], e2[3] floats, primitive, triangle within it, flat triangle index -- every
 * reference of a "bvh_presplit" tree.  header: [0..2] the scene centre (float bits), [3..11] the frame, row-major, row i = axis i in world
 * coordinates, [12] 1 if the boxes live in that frame, [13] 1 if the 32-byte form is valid for the walkers ("compact_nodes" 1 then walks
 * it), [14] nodes, [15] records, [16] depth, [17] the frame padding's world magnitude (float bits; 0 on the world axes: see "bvh_frame"),
 * [18..23] 0.  counts[0] / counts[1] = nodes / records, also when a capacity is too small or an array is NULL where the count is not 0
 * (VHR_ERROR_INVALID_ARGUMENT).  Checks in this order: NULL header or counts, the capacities, then the state (VHR_ERROR_GRAPH from inside
 * a pass or without geometry).  Waits for the context's streams; launches nothing; works on a host-only context. */
int vhr_debug_bvh_arrays(vhr_context *ctx, uint32_t header[24], void *nodes, void *nodes_ch, void *nodes48, void *nodes16, void *records, uint32_t capacity_nodes,
                         uint32_t capacity_records, uint32_t counts[2]);
/* What the last frame's rays cost, where: those lifetimes -- the any-hit launch's and the mirror ray's -- summed into a map of 8 x 8-pixel cells,
 * out[cy * cols + cx], cols >= ceil(width / 8), rows >= ceil(height / 8).  The cost map vhr_tile_plan_make_weighted cuts a grid by (cell = 8).
 * VHR_ERROR_NOT_FOUND when no queue kernel has left lifetimes ("raygen_cost_order" 0, or 1 on launches below 2 048 workgroups: set it to 2). */
int vhr_get_tile_cost_map(vhr_context *ctx, uint32_t *out, uint32_t cols, uint32_t rows);

int vhr_get_traversal_statistics(vhr_context *ctx, uint64_t out[4]);
/* The same for the mirror-ray launch of the last vhr_trace_rays (raygen.rgen:59-65 + reflection_hit.rchit; the queue kernel, statistics
 * enabled): out[0] = rays walked (first + second bounce), out[1] = second-bounce rays among them, out[2] = inner-node visits summed over
 * lanes, out[3] = leaf visits, out[4] = ray/triangle tests, out[5] = trips of the two inner loops counted once per wave (lane
 * utilisation = (out[2] + out[4]) / (64 * out[5])), out[6] = queue refills, out[7] = waves, out[8] = s_memtime ticks summed over the
 * waves' lifetimes, out[9] = of those, inside the walks (the rest is ray set-up and shading). */
int vhr_get_reflection_statistics(vhr_context *ctx, uint64_t out[10]);
/* Decision (vi)'s binary64 half in the work-queue kernels of the last vhr_trace_rays (statistics enabled).  A candidate whose fp32 solution contradicts
 * itself is decided again in binary64 -- in the per-pixel kernels in place, in the queue kernels outside their loops: the pixel is marked and computed
 * again by the per-pixel code when its tile is done.  out[0] = such pixels of the shadow / AO launch, out[1] = of the mirror ray's launch, out[2] =
 * the launches of the last vhr_trace_rays that ran an "alpha_test_rays" instantiation (0, 1 or 2; counted with or without statistics), out[3] = 0. */
int vhr_get_binary64_statistics(vhr_context *ctx, uint64_t out[4]);

/* Where the waves of the last work-queue raygen launch spent their time (statistics enabled; s_memtime ticks summed
 * over waves): out[0] = whole kernel, out[1] = per-tile pixel setup, out[2] = queue refills (ray generation),
 * out[3] = inner-node loop, out[4] = leaf (triangle) stage, out[5] = refills, out[6] = waves, out[7] = 0. */
int vhr_get_traversal_cycles(vhr_context *ctx, uint64_t out[8]);

/* The drain of the tiles' queues in the last shadow / AO launch (statistics enabled): out[0] = entries of the tiles' tree cuts summed over
 * the launch's waves (vhr_get_traversal_cycles out[6]), out[1..3] = wave-level trips made after the tile's queue had run dry with at most
 * 4 / 8 / 16 of the wave's rays still in flight. */
int vhr_get_drain_statistics(vhr_context *ctx, uint64_t out[4]);

/* Profiling aid: streams a storage image once with 4, 8 or 16 bytes per lane (a read of exactly width * height *
 * bytes-per-pixel bytes), used to calibrate rocprofv3's FETCH_SIZE for the SVGF kernels' access widths. */
int vhr_calibration_stream_read(vhr_context *ctx, int32_t storage_image, uint32_t bytes_per_lane);

/* K0 cost of the last vhr_update_geometry (the reference builds its BLAS / TLAS on the device, resource_manager.cpp:650,692,792; so does
 * "bvh_builder" 1, the default): out[0] = the build, out[1] = the upload of the scene arrays (+ the tree, where the host built it), in
 * milliseconds of host time.  The containment checks of the node forms run where the tree is and are not part of either. */
int vhr_get_build_times(vhr_context *ctx, double out[2]);
/* Which builder made the current tree: 0 = the host's, 1 = the device's ("bvh_builder" 1, the default; it falls back to the host builder
 * for a scene of a single leaf and for a tree deeper than the walkers' stacks) */
int vhr_get_bvh_builder(vhr_context *ctx, int32_t *used);
/* "bvh_presplit": the grid level (cell edge = longest scene edge / 2^level) the current tree's references were split on, -1 = every
 * triangle is one reference (the option is off, no triangle qualified, or the budget allowed no level) */
int vhr_get_bvh_presplit_level(vhr_context *ctx, int32_t *level);
/* "bvh_frame": the frame the current tree's boxes are in, row-major, row i = axis i in world coordinates (the identity: the world axes) */
int vhr_get_bvh_frame(vhr_context *ctx, float out[9]);

/* BVH facts for reporting: out[0] = node count, out[1] = triangle count, out[2] = max depth,
 * out[3] = node bytes, out[4] = triangle bytes */
int vhr_get_bvh_statistics(vhr_context *ctx, uint64_t out[5]);
/* Self-check of the last build (exact arithmetic, on the host): out[0] = child boxes checked, out[1] = centre / half-extent boxes that
 * do not contain their (lo, hi) box, out[2] = 48-byte-node boxes that do not contain the centre / half-extent box (or whose links differ),
 * out[3] = half-precision ("compact_nodes") boxes that do not contain theirs.  All three must be 0: the walkers' bit-identity with the
 * oracle rests on box tests that only cull. */
int vhr_get_bvh_form_checks(vhr_context *ctx, uint64_t out[4]);
/* A 64-bit hash of the last build's nodes and leaf triangles in their final order: two builds of the same input must agree whatever
 * "bvh_build_threads" was. */
int vhr_get_bvh_fingerprint(vhr_context *ctx, uint64_t *out);
/* A 64-bit hash of the TREE rather than of its arrays: per inner node the bits of its two child boxes and its children's hashes, per leaf
 * the flat ids of its triangles in ascending order -- independent of the numbering of the nodes, of the order of the leaves in memory and
 * of the order of the triangles inside a leaf.  The host's and the device's build of a scene agree on it ("bvh_builder" 0 / 1: the same
 * algorithm, the same tree; the reference's BLAS / TLAS are the driver's, resource_manager.cpp:593-801). */
int vhr_get_bvh_tree_fingerprint(vhr_context *ctx, uint64_t *out);
/* The derived node forms -- what the walkers read -- against the one definition of their arithmetic (csrc/bvh_math.hpp).  out[0] = the hash
 * (vhr_get_bvh_fingerprint's mixing) of the scene centre and the centre / half-extent, 48-byte and 32-byte nodes as they stand, fetched
 * from the device if they live there; out[1] = the same hash after the host has derived the forms again from a copy of the (lo, hi) nodes.
 * out[0] == out[1] for every tree, built or refitted by either builder.  The 32-byte nodes are hashed always, in range or not: a scene
 * beyond the half range leaves inf in the same halves on both sides (the host's software float -> half conversions round like the
 * hardware's, overflow included).  VHR_ERROR_GRAPH without a tree. */
int vhr_get_bvh_forms_fingerprint(vhr_context *ctx, uint64_t out[2]);

/* ---- Refit: geometry that moves without a rebuild (an extension; what Vulkan calls VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR) ----
 * The tree of the last vhr_update_geometry keeps its topology; its triangle records and boxes are recomputed from the current vertices and
 * primitive transforms.  Per frame: vhr_update_vertices / vhr_update_primitive_transforms (any number), vhr_refit_geometry,
 * vhr_update_per_frame_ubo, vhr_graph_execute.  Results do not depend on the tree, so a refitted tree publishes exactly the images and ray
 * query answers a rebuild from the same arrays publishes ("alpha_test_rays" and VHR_RAY_QUERY_ALPHA_TEST included: what a ray sees is decided
 * per candidate from the primitive's material and the current vertices' uv0, never from the tree); what degrades is speed (watch vhr_get_bvh_sah_cost and call vhr_rebuild_geometry when it has grown).
 *   - While updates are pending (an update call without a vhr_refit_geometry after it) vhr_graph_execute, vhr_ray_query and the vhr_standin_*
 *     calls fail with VHR_ERROR_GRAPH and a message that names vhr_refit_geometry: a stale tree is never traced silently.
 *   - Refused, with a message in vhr_last_error: no geometry yet (VHR_ERROR_GRAPH); a tree built with "bvh_presplit" whose references were
 *     split (vhr_get_bvh_presplit_level >= 0: VHR_ERROR_UNSUPPORTED; vhr_rebuild_geometry instead, with "bvh_presplit" 0 for a tree that can be refitted); a range outside the buffer, a NULL array with a
 *     non-zero count, an unknown flag, non-finite host data (VHR_ERROR_INVALID_ARGUMENT).  Argument checks come first, on every context.
 *   - Topology changes (triangles or primitives added or removed) need vhr_update_geometry.  Frame state is left alone: the SVGF history,
 *     cost orders, statistics.  By default motion vectors stay what the G-buffer pass makes them (camera motion only), so moving geometry ghosts
 *     in the SVGF history; "object_motion_vectors" 1 (below) makes the stand-in G-buffer follow the geometry the refits moved.
 *   - A host-only context supports all of it on the host (the same arithmetic): it keeps the arrays and the tree of its last build.
 *   - vhr_resize keeps the refitted tree; vhr_update_geometry and vhr_rebuild_geometry (below) replace the tree and everything a refit
 *     prepared; the first discards pending updates, the second builds from them. */
#define VHR_UPDATE_DEVICE_MEMORY 2u   /* vhr_update_vertices: `vertices` is device memory (the counterpart of VHR_RAY_QUERY_HOST_MEMORY's default) */
/* Overwrites vertices [first_vertex, first_vertex + vertex_count) of the last vhr_update_geometry (whole records: the stand-in raster stages
 * read normals, tangents and uvs too).  flags 0: a host array, validated here (finite positions), copied before the call returns.
 * VHR_UPDATE_DEVICE_MEMORY: a device array, copied on the context's stream; the call does not wait for the copy, and finiteness is then
 * checked by the refit.  On either route the FIRST update after a build or a refit waits for every stream of the context before it
 * overwrites anything: frames still in flight read the vertices. */
int vhr_update_vertices(vhr_context *ctx, uint32_t first_vertex, uint32_t vertex_count, const vhr_vertex *vertices, uint32_t flags);
/* Replaces vhr_primitive::transform (16 floats each, host memory, finite) of primitives [first_primitive, first_primitive + count) and their
 * normal matrices: the rigid-motion route (the transform is baked into the world-space triangle records, as at build time). */
int vhr_update_primitive_transforms(vhr_context *ctx, uint32_t first_primitive, uint32_t count, const float *transforms);
/* Brings the acceleration structure up to date: every leaf record re-derived in its slot, the boxes bottom-up in the tree's "bvh_frame" (one
 * launch per level, the top levels in one), padded like a build's, the scene centre and the three derived node forms with their containment
 * check (the half-precision form falls back to the 48-byte nodes exactly as after a build).  With nothing pending: VHR_OK, nothing launched.
 * Synchronises like vhr_update_geometry (it reads its counters back); an asynchronous refit is out of scope.  If it meets non-finite
 * coordinates (device-memory vertices) or, on a tree in a "bvh_frame", record corners beyond the world magnitude the tree's padding was built
 * with (vhr_debug_bvh_arrays header[17]: at least twice the largest |coordinate| at build time -- a refit pads as the build did, so that a
 * partial refit leaves what a whole one leaves), it fails with VHR_ERROR_INVALID_ARGUMENT, the tree's arrays are NOT valid and updates stay
 * pending until a refit succeeds or the geometry is rebuilt (vhr_rebuild_geometry, vhr_update_geometry). */
int vhr_refit_geometry(vhr_context *ctx);
/* out[0] = refits since the last build that succeeded, out[1] = triangle records written by the last refit, out[2] = nodes written, out[3] = records not
 * inside their leaf's box, out[4] = child boxes not inside the slot their parent holds for them (both counted in exact comparisons by a
 * check pass after the refit; must be 0), out[5] = coordinates met that the tree cannot hold: non-finite ones and, on a tree in a "bvh_frame",
 * finite corner coordinates beyond its world magnitude (must be 0), out[6] = 1 if the walkers are on the
 * half-precision nodes after it, out[7] = launches of the upward pass (0 on a host-only context). */
int vhr_get_refit_statistics(vhr_context *ctx, uint64_t out[8]);
/* The last refit, milliseconds: out[0] = host wall time of vhr_refit_geometry; with bit 12 set in vhr_set_kernel_timing's mask also the
 * device time of out[1] = the leaf pass, out[2] = the upward pass, out[3] = the node forms and the two check passes (else 0).  The scene
 * centre's reduction and its 12-word read-back, which lie between out[2] and out[3], are in out[0] only.  (Bit 12 is a mask bit only:
 * vhr_get_kernel_time has no kind 12.)
 * vhr_get_build_times keeps its meaning (the last vhr_update_geometry). */
int vhr_get_refit_times(vhr_context *ctx, double out[4]);
/* ---- Partial refit: only the subtrees that moved geometry touches ----
 * vhr_update_vertices and vhr_update_primitive_transforms also remember the ranges they were given (up to 16 disjoint vertex ranges and 16
 * primitive ranges, merged where they touch; beyond that the two nearest are joined).  vhr_refit_geometry_partial re-derives only the records
 * with a vertex (vertex_offset + index) or a primitive in those ranges, recomputes only the boxes of their leaves' ancestors, level by level,
 * and rewrites the derived forms of those nodes only.  Every array the walkers read is bit for bit what vhr_refit_geometry gives for the same
 * updates, and so are vhr_get_bvh_form_checks and the half-precision fallback.  Preconditions, refusals, error codes and synchronisation are
 * vhr_refit_geometry's; an unknown flag bit is VHR_ERROR_INVALID_ARGUMENT, checked first on every context.
 *   flags 0: the whole-tree refit runs instead where that is cheaper -- the first refit since the build (the per-node boxes a dirty pass
 *     starts from do not exist yet) and a dirty share above the library's threshold.  Where both hold, the first is the reason reported.
 *   VHR_REFIT_FORCE_PARTIAL: the dirty path whatever the share (tests and measurement); the first refit since the build is still whole-tree.
 * If the scene centre's bits change, the half-precision form of every node depends on it: the forms and their checks are redone for all
 * nodes in that call.  The ranges are forgotten by a refit of either kind that succeeds and by vhr_update_geometry.
 * vhr_get_refit_statistics / vhr_get_refit_times describe the last refit of either kind: after a dirty pass out[1] and out[2] are the dirty
 * records and the dirty nodes, out[7] the upward launches made. */
#define VHR_REFIT_FORCE_PARTIAL 1u
int vhr_refit_geometry_partial(vhr_context *ctx, uint32_t flags);
/* out[0] = calls since the last build that took the dirty path and succeeded; of the last call: out[1] = dirty records, out[2] = dirty nodes
 * (ancestors included), out[3] = nodes whose derived forms were rewritten, out[4] = what it ran as (0 = the dirty path, 1 = whole tree: first
 * refit since the build, 2 = whole tree: over the threshold), out[5] = 1 if the scene centre's bits changed and all forms were redone,
 * out[6] = vertex ranges used, out[7] = primitive ranges used. */
int vhr_get_partial_refit_statistics(vhr_context *ctx, uint64_t out[8]);
/* ---- Object motion vectors: the refits keep last frame's triangle records ("object_motion_vectors", vhr_set_option; default 0) ----
 * A leaf record (v0, e1, e2 in world space, the primitive's transform baked in) keeps its slot through a refit, and a visible point is affine
 * in its hit's barycentrics, P = v0 + u e1 + v e2.  With the option on the library keeps, per record, the record the slot held before the
 * last refit; the stand-in G-buffer (vhr_standin_gbuffer) reprojects a hit through P + d, d = (pv0 - v0) + u (pe1 - e1) + v (pe2 - e2), in
 * place of P, so motion.xy follows vertices and transforms alike.  Nothing else of the G-buffer changes, a record that did not move gives d
 * = 0 exactly and its texel's bits stay, and while no record differs from its previous one the plain kernel is launched.
 *   The contract.  Let S0 be the records after the build, or after the option was switched on.  Let Si be the records after the i-th call of
 *   vhr_refit_geometry / vhr_refit_geometry_partial that SUCCEEDS with the option on; a call with nothing pending counts and leaves Si =
 *   Si-1 (it launches one settle pass if the call before it left differing records, else nothing).  After that call the previous record of
 *   every slot k is Si-1(k), bit for bit.  A refit that fails (non-finite coordinates) does not count: once a later one succeeds, previous
 *   is still the state before the failed attempt.  Hence ONE refit call per frame -- also in a frame without updates -- makes previous "last
 *   frame"; two refits between two frames make the motion relative to the state between them.
 * Turning the option on waits for the context's streams, allocates the arrays (52 bytes per record) and sets previous = current; turning it
 * off frees them.  vhr_update_geometry sets previous = current for the new tree; vhr_resize keeps everything.  The arrays take no part in the
 * fingerprints or the form checks, and vhr_hybrid_save_state's blob does not carry them: the first frame after a load has no object motion.
 * The rayquery, forward raster and raytraced paths write no motion image and ignore the option; an integrator whose G-buffer comes from its own
 * raster pass writes object motion itself.  Costs: profiles/object_motion_rate.jsonl (tools/object_motion_rate.py).
 * out[0] = 1 if the option is on and the arrays exist, out[1] = records whose previous differs from current (any of the nine words) after the
 * last successful refit (0 after a build, after switching on and after a settle), out[2] = G-buffer launches since vhr_create that ran the
 * motion instantiation, out[3] = 0. */
int vhr_get_object_motion_statistics(vhr_context *ctx, uint64_t out[4]);
/* ---- Rebuild in place: a new tree from the arrays on the device (refit while the tree is good, rebuild when it is not) ----
 * Builds a new tree over the geometry as it stands -- the arrays of the last vhr_update_geometry with every later vhr_update_vertices and
 * vhr_update_primitive_transforms applied, pending or already refitted -- with the build options as they are set NOW ("bvh_leaf_triangles",
 * "bvh_builder", "bvh_build_threads", "bvh_frame", "bvh_presplit", "bvh_device_max_depth", "bvh_host_checks").  Nothing is handed over again:
 * the device builder reads the scene arrays where the walkers read them.  Every array the walkers read, the fingerprints, the form checks,
 * vhr_get_bvh_statistics / _frame / _presplit_level / _builder and the half-precision fallback are bit for bit those of a fresh context with
 * the same option values after vhr_update_geometry with the current arrays.  vhr_update_geometry's fallbacks apply unchanged (a one-leaf
 * scene, a tree deeper than the walkers' stacks and "bvh_builder" 0 go to the host builder); a device context keeps no host copy of the scene,
 * so the call then fetches vertices, indices and primitives from the device (out[1] below) and uploads the tree as vhr_update_geometry does.
 *   - Pending updates are consumed: nothing is pending afterwards, the dirty ranges are forgotten, vhr_get_refit_statistics and
 *     vhr_get_partial_refit_statistics read as after a build, both words of vhr_get_bvh_sah_cost are the new tree's, and vhr_get_build_times
 *     describes this build (out[0] the build, out[1] the transfers the call had to make: 0 where the device built).
 *   - Kept: the scene arrays and textures on the device, the primitives' ray cull masks (vhr_get_ray_mask_statistics out[0] with them),
 *     whether the scene can discard, every option and the trace parameters, storage images, the render graph and the paths registered on the
 *     context, the SVGF history, cost orders and all frame statistics.  Results never depend on the tree: frames and queries after a rebuild
 *     are bit for bit those after a refit of the same updates.
 *   - A tree built with "bvh_presplit" is NOT refused (updates still cannot be pending on one): the call builds again, and with "bvh_presplit"
 *     set to 0 first it gives a tree that can be refitted, without a re-upload.
 *   - "object_motion_vectors" 1: a successful rebuild counts as one successful refit in the contract above, stated per triangle instead of per
 *     slot: afterwards the previous record of every slot that holds flat triangle f (with "bvh_presplit" there are several) is the current record
 *     f had before the call, bit for bit; a triangle that did not move has previous == current; vhr_get_object_motion_statistics out[1] counts
 *     the records that differ, and the next refit call with nothing pending settles them.
 *   - Waits for every stream of the context before anything is replaced and returns with the tree in place, like vhr_update_geometry.
 *   - Refused, in this order, with a message that names the call: a NULL context; a flag bit (flags must be 0: VHR_ERROR_INVALID_ARGUMENT,
 *     checked first on every context); no geometry yet (VHR_ERROR_GRAPH); called while a graph records or executes or from inside a pass
 *     (VHR_ERROR_GRAPH).  Then every vertex position is checked where it lives, before anything is freed or built: a non-finite coordinate
 *     (vertices written through VHR_UPDATE_DEVICE_MEMORY are unvalidated) gives VHR_ERROR_INVALID_ARGUMENT, the old tree's arrays are
 *     untouched, and updates stay -- or become -- pending, so nothing traces until a later refit or rebuild succeeds.
 *   - A host-only context supports all of it on the host, from the arrays it keeps.
 * Costs (tools/rebuild_rate.py, profiles/rebuild_rate.jsonl; MI355X): about 10 ms on sponza_proc (258 k triangles) and 23 - 24 ms on bistro_proc
 * (2.9 M), about 0.9 and 0.8 of vhr_update_geometry with the same arrays and some 33 and 20 steady-state refits: a call for the frame in which the
 * cost has grown, not for every frame.  The first refit of the new tree makes the refit's plan again (about 1.2 / 13 ms against 0.3 / 1.1 ms). */
int vhr_rebuild_geometry(vhr_context *ctx, uint32_t flags);
/* out[0] = successful rebuilds since the last vhr_update_geometry, out[1] = 1 if the last one fetched the scene arrays from the device for
 * the host builder, out[2] = non-finite coordinates the last call met (0 on success), out[3] = records whose previous differs from current
 * after it (0 with "object_motion_vectors" off), out[4..7] = 0.  All 0 after vhr_create and after vhr_update_geometry. */
int vhr_get_rebuild_statistics(vhr_context *ctx, uint64_t out[8]);
/* The surface-area cost of the tree -- the sum over the inner nodes of child box area x (1 for an inner child, the triangle count for a
 * leaf), over the root's area, on the padded boxes the walkers test: out[0] = as built, out[1] = as it is now.  The number to watch when
 * deciding to call vhr_rebuild_geometry.  One reduction, computed when asked (waits for the context's streams). */
int vhr_get_bvh_sah_cost(vhr_context *ctx, double out[2]);

/* ---- Batched ray queries on the scene's BVH (rayQueryEXT with an opaque TLAS, cull mask 0xFF -- vhr_ray_query_masked below takes the cull mask;
 *      VHR_RAY_QUERY_ALPHA_TEST: a non-opaque one) ----
 * Traces `count` caller-made rays against the geometry of the last vhr_update_geometry.  The flags of rayQueryInitializeEXT this
 * stands for are gl_RayFlagsTerminateOnFirstHitEXT (VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT) or none; the mask is 0xFF (any other: vhr_ray_query_masked).
 *   - All geometry is opaque and two-sided (face culling: vhr_ray_query_faces below); a triangle is hit iff tmin < t < tmax (decision (vi): fp32 Moeller-Trumbore, a candidate whose
 *     solution contradicts itself decided again in binary64 -- the same test, bit for bit, as every walker of the library and the oracle).
 *   - Without the flag: results = vhr_ray_hit[count], the hit of smallest t, ties broken by the smaller flat triangle index (primitive-major
 *     order of vhr_update_geometry); a miss is geometry_index = primitive_index = 0xFFFFFFFF, t = u = v = 0.  With it: results =
 *     uint8_t[count], 1 = some triangle is hit (which one ends the walk depends on the tree; the boolean does not).
 *   - VHR_RAY_QUERY_ALPHA_TEST (16; combines with both other flags; 4 and 8 are no flags): geometry the G-buffer pass cuts holes into is no longer
 *     opaque -- a candidate hit that gbuf.frag:20-32 would discard at the hit (the rule spelled out at "alpha_test_rays" above) does not
 *     exist for the ray, as if a rayQueryEXT loop had not confirmed it: it ends no any-hit ray and is no closest hit.  Otherwise the
 *     contract is unchanged: closest = min t, then the smaller flat index, among the candidates that exist.  Independent of
 *     "alpha_test_rays"; on a scene none of whose primitives can discard the flag launches the plain kernels.
 *   - Degenerate rays are not rejected: a zero or NaN direction or tmin >= tmax misses, an infinite tmax is an unbounded ray.
 *   - Device path (no VHR_RAY_QUERY_HOST_MEMORY): `rays` and `results` are device pointers.  The work is enqueued on the stream
 *     vhr_get_current_stream reports at the time of the call (after a vhr_update_geometry made earlier on it) and the call returns
 *     without synchronising; `results` is complete when that stream is.  It may be called between frames or inside a pass callback.
 *     VHR_RAY_QUERY_HOST_MEMORY: host pointers, staged through device memory of the context's; the call returns with results in place.
 *   - No side effects: no frame state is read or written (statistics, cost-order lifetimes, images), so the frames around a query are
 *     bit-identical to frames without one.  Queries in flight on different streams share nothing (the query's counters and its list of
 *     rays to decide again exist once per stream); a query reads `rays` and writes `results` in its stream's order only.
 *   - VHR_ERROR_INVALID_ARGUMENT (message in vhr_last_error) for a NULL pointer with count > 0, an unknown flag bit, `rays` not 16-byte
 *     aligned or `results` not 4-byte aligned -- checked first, on every context.  Then VHR_ERROR_NO_DEVICE on a host-only context.
 *     count == 0 returns VHR_OK and launches nothing; a context without geometry makes every ray miss. */
int vhr_ray_query(vhr_context *ctx, const vhr_ray *rays, uint32_t count, uint32_t flags, void *results);
/* vhr_ray_query with rayQueryInitializeEXT's cull mask: the same contract, flags, validation order and error codes, and ray i's mask is
 * `cull_mask` if ray_masks == NULL, else ray_masks[i] & cull_mask.  A candidate hit on primitive p does not exist for a ray of mask m iff
 * (masks[p] & m) == 0 (vhr_set_primitive_masks): it ends no any-hit ray, shrinks no closest t and takes no part in the (t, flat index)
 * tie-break; decision (vi) comes first, its binary64 re-decision included, and with VHR_RAY_QUERY_ALPHA_TEST the mask test precedes the
 * alpha rule.  A ray of mask 0 misses everything.  `ray_masks` lives where `rays` live (device memory, or host memory with
 * VHR_RAY_QUERY_HOST_MEMORY: staged) and needs no alignment.  cull_mask > 0xFF: VHR_ERROR_INVALID_ARGUMENT, with the other argument checks.
 * Where the cull mask does not act on the masks the primitives carry and ray_masks is NULL, the launches are vhr_ray_query's own.
 * vhr_ray_query itself is the (0xFF, NULL) case. */
int vhr_ray_query_masked(vhr_context *ctx, const vhr_ray *rays, uint32_t count, uint32_t flags, uint32_t cull_mask, const uint8_t *ray_masks, void *results);
/* The last vhr_ray_query or vhr_ray_query_masked (waits for the device): out[0] = rays, out[1] = rays with a hit, out[2] = rays decided again in binary64 by the
 * second launch, out[3] = waves whose traversal stack overflowed (must be 0).  All 0 before the first query. */
int vhr_get_ray_query_statistics(vhr_context *ctx, uint64_t out[4]);
/* The layouts this library was built with, for bindings: out[0] = sizeof(vhr_ray), out[1] = offsetof(vhr_ray, tmin), out[2] =
 * offsetof(vhr_ray, direction), out[3] = offsetof(vhr_ray, tmax), out[4] = sizeof(vhr_ray_hit), out[5] = offsetof(vhr_ray_hit,
 * geometry_index), out[6] = offsetof(vhr_ray_hit, primitive_index), out[7] = offsetof(vhr_ray_hit, reserved).  Returns 8. */
int vhr_ray_query_struct_layout(uint32_t out[8]);

/* ---- Ray cull masks: per-primitive visibility for rays and ray queries (VkAccelerationStructureInstanceKHR::mask against cullMask) ----
 * Every primitive has an 8-bit mask, 0xFF after vhr_update_geometry (resource_manager.cpp:704-717 builds its instance with one); every ray
 * has one: the hybrid path's by class ("shadow_ray_mask", "ao_ray_mask", "reflection_ray_mask" of vhr_set_option), a query's from
 * vhr_ray_query_masked.  A candidate hit on a triangle of primitive p does not exist for a ray of mask m iff (masks[p] & m) == 0: this object
 * casts no shadow, that proxy is seen by AO rays only, this batch of queries sees colliders only.  Results never depend on the tree: a ray of
 * mask m sees, bit for bit, what the plain ray sees on the scene made of the primitives with masks[p] & m != 0.
 *   - vhr_set_primitive_masks takes host memory.  It is no update in the refit sense: nothing becomes pending, no refit is needed.  It waits
 *     for the context's streams before it overwrites and takes effect at the next launch.  vhr_update_geometry resets every mask to 0xFF;
 *     vhr_resize and both refits keep them.  The masks are no part of vhr_hybrid_save_state's blob or of any fingerprint.  The device array
 *     is made by the first call that stores a value other than 0xFF: a context that never does pays nothing.
 *   - Refused: NULL with count > 0 (VHR_ERROR_INVALID_ARGUMENT, checked first), no geometry yet or called from inside a pass
 *     (VHR_ERROR_GRAPH), a range outside the primitives (VHR_ERROR_INVALID_ARGUMENT).  count == 0 does nothing.  A host-only context keeps
 *     the masks (vhr_get_primitive_masks reads them back).
 *   - The rayquery, forward-raster and raytraced render paths ignore masks. */
int vhr_set_primitive_masks(vhr_context *ctx, uint32_t first_primitive, uint32_t count, const uint8_t *masks);
int vhr_get_primitive_masks(vhr_context *ctx, uint32_t first_primitive, uint32_t count, uint8_t *out);
/* out[0] = primitives whose mask is not 0xFF, out[1] = launches of the last vhr_trace_rays that ran a mask instantiation (0, 1 or 2; 1 at
 * most with "raygen_variant" 0), out[2] = 1 if the last ray query ran one, out[3] = 0. */
int vhr_get_ray_mask_statistics(vhr_context *ctx, uint64_t out[4]);

/* ---- Batched closest-point queries on the scene's BVH: the nearest surface to a point, or whether any lies within a distance ----
 * Triangle i is a CANDIDATE of query q iff d2_i <= fl(max_distance * max_distance) and (masks[primitive of i] & cull_mask) != 0, where d2_i is
 * the squared distance from the point to the closed triangle as the library's one fp32 point / triangle function computes it (every operation
 * rounded once, IEEE division; vhr_debug_point_triangle runs it on explicit pairs).  max_distance = +inf bounds nothing; a negative or NaN
 * max_distance and a non-finite point find nothing.
 *   - Without VHR_POINT_QUERY_ANY_WITHIN: results = vhr_ray_hit[count].  t = the distance, the correctly rounded sqrtf(d2) of the winning
 *     candidate; (u, v) = the barycentrics of its nearest point (v0 + u e1 + v e2, inside the closed unit triangle); geometry_index /
 *     primitive_index as in a ray hit.  The winner has the smallest d2, ties go to the smaller flat triangle index (closest-hit's tie-break).
 *     Nothing found: both indices 0xFFFFFFFF, t = u = v = 0.
 *   - VHR_POINT_QUERY_ANY_WITHIN: results = uint8_t[count], 1 = a candidate exists.
 *   - Results never depend on the tree: a query returns, bit for bit, what a loop of the function over all triangles in flat order returns --
 *     on either builder's tree, with "bvh_frame", "bvh_presplit", any leaf size, after refits.  No alpha rule.  No frame state is read or
 *     written: frames around a query are the frames without it.
 *   - Device pointers by default: enqueued on the stream vhr_get_current_stream reports (between frames or inside a pass callback), the call
 *     returns without synchronising.  VHR_POINT_QUERY_HOST_MEMORY: host pointers, staged; the call returns with results in place.
 *     count == 0 returns VHR_OK and launches nothing; a context without geometry finds nothing.
 *   - VHR_ERROR_INVALID_ARGUMENT (message in vhr_last_error, with the entry point's name) for a NULL pointer with count > 0, an unknown flag
 *     bit, `points` not 16-byte aligned, `results` not 4-byte aligned or cull_mask > 0xFF -- checked first, in that order, on every context.
 *     Then VHR_ERROR_NO_DEVICE on a host-only context, and VHR_ERROR_GRAPH while geometry updates are pending (vhr_refit_geometry first). */
int vhr_closest_point_query(vhr_context *ctx, const vhr_point_query *points, uint32_t count, uint32_t flags, uint32_t cull_mask, void *results);
/* The last vhr_closest_point_query (waits for the device): out[0] = queries, out[1] = queries that found something, out[2] = point / triangle
 * evaluations, out[3] = waves whose traversal stack overflowed (must be 0).  All 0 before the first query. */
int vhr_get_point_query_statistics(vhr_context *ctx, uint64_t out[4]);
/* The query's point / triangle function on explicit pairs (host memory): 12 floats per pair (p, v0, e1, e2) -> 3 floats per pair (d2, u, v).
 * A device context runs the device's copy, one pair per thread; a HOST-ONLY context runs the host's copy of the same source: the arithmetic is
 * testable without a GPU, and the two are comparable, bit for bit, on one. */
int vhr_debug_point_triangle(vhr_context *ctx, const float *pairs, uint32_t count, float *out);

/* ---- Batched k-nearest queries on the scene's BVH: the k nearest triangles to a point, in order ----
 * The CANDIDATES of a query are exactly those of vhr_closest_point_query (above): d2_i <= fl(max_distance * max_distance) by the same fp32
 * point / triangle function, and (masks[primitive of i] & cull_mask) != 0; +inf bounds nothing, a negative or NaN max_distance and a non-finite
 * point find nothing.  They are ORDERED by (d2, flat triangle index) ascending -- a total order, so the answer does not depend on the tree --
 * and every triangle appears at most once, also on a "bvh_presplit" tree that holds several references to it.
 *   - results = vhr_ray_hit[count * k], 1 <= k <= VHR_NEAREST_MAX_K; query q owns entries [q * k, q * k + k).  Entry j is the j-th candidate in
 *     that order: t = the correctly rounded sqrtf(d2), (u, v) = the barycentrics the function settled on, geometry_index / primitive_index as in
 *     a ray hit, reserved = 0.  Once the candidates run out every remaining entry is the miss record: both indices 0xFFFFFFFF, t = u = v = 0.
 *   - k == 1 is vhr_closest_point_query without VHR_POINT_QUERY_ANY_WITHIN, bit for bit.
 *   - Results equal, bit for bit, the brute force over all triangles in flat order: on either builder's tree, with "bvh_frame", "bvh_presplit",
 *     any leaf size, after refits and a rebuild.  No alpha rule.  No frame state is read or written.
 *   - Device pointers, streams and staging as vhr_closest_point_query's.  VHR_POINT_QUERY_HOST_MEMORY is the only flag
 *     (VHR_POINT_QUERY_ANY_WITHIN is an unknown flag here).  count == 0 returns VHR_OK and launches nothing; a context without geometry
 *     returns only miss records.
 *   - VHR_ERROR_INVALID_ARGUMENT (message in vhr_last_error, with the entry point's name) for a NULL pointer with count > 0, an unknown flag
 *     bit, `points` not 16-byte aligned, `results` not 4-byte aligned, cull_mask > 0xFF, k == 0 or k > VHR_NEAREST_MAX_K -- checked first, in that
 *     order, on every context.  Then VHR_ERROR_NO_DEVICE on a host-only context, and VHR_ERROR_GRAPH while geometry updates are pending. */
int vhr_nearest_points_query(vhr_context *ctx, const vhr_point_query *points, uint32_t count, uint32_t k, uint32_t flags, uint32_t cull_mask,
                             vhr_ray_hit *results);
/* The last vhr_nearest_points_query (waits for the device): out[0] = queries, out[1] = entries returned over all queries, out[2] = point /
 * triangle evaluations of the walks (the one more per returned entry that recovers its (u, v) is not counted), out[3] = waves whose traversal
 * stack overflowed (must be 0).  All 0 before the first call. */
int vhr_get_nearest_query_statistics(vhr_context *ctx, uint64_t out[4]);

/* ---- Ray face culling and the hit kind of ray queries (gl_RayFlagsCullBackFacingTrianglesEXT / gl_RayFlagsCullFrontFacingTrianglesEXT of
 *      rayQueryInitializeEXT; rayQueryGetIntersectionFrontFaceEXT, gl_HitKindFrontFacingTriangleEXT) ----
 * A triangle (v0, v1, v2) of primitive p is FRONT-FACING for a ray of direction d iff (det > 0) != flip[p], where det = e1 . (d x e2),
 * e1 = v1 - v0, e2 = v2 - v0 in world space: the vertices appear counter-clockwise from the ray's origin (glTF's winding, the raster pipeline's
 * VK_FRONT_FACE_COUNTER_CLOCKWISE, an instance with VK_GEOMETRY_INSTANCE_TRIANGLE_FRONT_COUNTERCLOCKWISE_BIT_KHR).  det is computed in
 * binary64 from the leaf record's fp32 edges, operation for operation as decision (vi)'s binary64 Moeller-Trumbore computes its determinant
 * (products of two fp32 values exact, every other operation rounded once): at grazing incidence the fp32 determinant's sign is rounding noise.
 * Whatever is not > 0 is back-facing (det == 0, a NaN direction), so the two cull modes partition a ray's candidates.  Facing is decided in
 * OBJECT space, as Vulkan and glTF decide it: flip[p] = 1 iff the determinant of the upper 3 x 3 of vhr_primitive::transform is < 0 (binary64,
 * cofactors along the first row: (m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20)) + m02 (m10 m21 - m11 m20); zero gives 0).
 *   - vhr_ray_query_faces is vhr_ray_query_masked -- contract, flags, validation order, error codes, stream and memory rules, no frame state
 *     read or written, refused while updates are pending -- with one more rule: a candidate on a back-facing triangle does not exist for a ray
 *     with VHR_FACE_CULL_BACK, one on a front-facing triangle does not exist with VHR_FACE_CULL_FRONT.  It ends no any-hit ray, shrinks no
 *     closest t and takes no part in the (t, flat index) tie-break.  Per candidate: decision (vi) with its binary64 re-decision, the mask test,
 *     the face test, the alpha rule.  Results never depend on the tree.  "The closest front-facing hit" is not "the closest hit, dropped if it
 *     faces backwards": the filter sits inside the walk.
 *   - face_cull > 2 (Vulkan forbids both bits together): VHR_ERROR_INVALID_ARGUMENT, checked with the other arguments, behind cull_mask > 0xFF.
 *   - Without VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT, vhr_ray_hit::reserved of a hit is its HIT KIND, VHR_HIT_KIND_FRONT_FACING (0xFE) or
 *     VHR_HIT_KIND_BACK_FACING (0xFF), decided by the same function on the committed triangle; 0 on a miss.  For every face_cull, NONE included.
 *     vhr_ray_query and vhr_ray_query_masked still write 0 there.
 *   - Launches: the face instantiation of the two ray-query kernels where face_cull != 0, and in closest-hit mode whatever face_cull is (the kind
 *     is reported); terminate-on-first-hit with VHR_FACE_CULL_NONE launches exactly what vhr_ray_query_masked launches.
 *   - The flip bytes are computed by vhr_update_geometry and vhr_update_primitive_transforms; both refits, vhr_rebuild_geometry and vhr_resize
 *     keep them.  They are no part of any fingerprint or of vhr_hybrid_save_state's blob.  Their device copy is made by the first query that
 *     needs it: a context that never culls pays nothing.
 *   - Every render path stays two-sided, and closest-point queries have no facing. */
int vhr_ray_query_faces(vhr_context *ctx, const vhr_ray *rays, uint32_t count, uint32_t flags, uint32_t cull_mask,
                        const uint8_t *ray_masks, uint32_t face_cull, void *results);
/* The flip bytes of `count` primitives from first_primitive on (0 or 1 each).  Checks as vhr_get_primitive_masks; works on a host-only context. */
int vhr_get_primitive_facing_flips(vhr_context *ctx, uint32_t first_primitive, uint32_t count, uint8_t *out);
/* out[0] = primitives with flip = 1, out[1] = 1 if the last ray query of any kind launched the face instantiation, else 0, out[2] = out[3] = 0. */
int vhr_get_face_cull_statistics(vhr_context *ctx, uint64_t out[4]);
/* The facing function on explicit pairs (host memory): 9 floats per pair (d, e1, e2), `flips` one byte per pair or NULL for all 0 -> one byte
 * per pair, VHR_HIT_KIND_FRONT_FACING or VHR_HIT_KIND_BACK_FACING.  A device context runs the device's copy, one pair per thread; a HOST-ONLY
 * context runs the host's copy of the same source (as vhr_debug_point_triangle does). */
int vhr_debug_ray_facing(vhr_context *ctx, const float *pairs, const uint8_t *flips, uint32_t count, uint8_t *out);

/* ---- Surface points of hits: where a hit is, which way the surface faces, and what gbuf.frag would have written there ----
 * A vhr_ray_hit says which triangle and where on it (rayQueryGetIntersection*EXT); vhr_resolve_hits turns a batch of them into
 * vhr_surface_point records (include/vhr_types.h) from the scene arrays the context holds -- the current ones, also where the vertices came
 * through VHR_UPDATE_DEVICE_MEMORY -- what reflection_hit.rchit:11-24 and gbuf.frag:19-56 compute from the same indices.
 *   - Only u, v, geometry_index and primitive_index of a hit are read; t and reserved are ignored, so the results of vhr_ray_query* and of
 *     vhr_closest_point_query go in unchanged.
 *   - NOT RESOLVED, the whole record zero (flags == 0): a miss (either index 0xFFFFFFFF), geometry_index not less than the primitive count,
 *     primitive_index not less than that primitive's index_count / 3, u or v not finite.  `hits` is the caller's data: each of these checks
 *     comes before any gather, so no hit array makes the kernel read outside the scene arrays.  A context without geometry resolves nothing.
 *   - The record: (v0, e1, e2) from the primitive's transform and the triangle's three positions by the function the builders and the refits
 *     use (transform * vec4(pos, 1), columns left to right; e1 = w1 - w0, e2 = w2 - w0) -- bit for bit the leaf record the walkers tested.
 *     There is no slot lookup and the tree is never read: results are the same on every tree, with "bvh_presplit", after refits and rebuilds.
 *   - position = (v0 + u e1) + v e2 per component, every operation rounded once: the point the closest-point query measured to, the P of the
 *     object-motion contract.
 *   - geometric_normal = cross(e1, e2), negated where the primitive's flip byte is 1 (vhr_get_primitive_facing_flips), each component divided by
 *     sqrtf(n . n) (IEEE division and square root).  By vhr_ray_query_faces' rule a ray of direction d is front-facing iff
 *     d . geometric_normal < 0; the two can differ in sign only at grazing incidence, where the binary64 determinant and the fp32 cross
 *     product may disagree.  VHR_SURFACE_DEGENERATE and the zero vector where n . n is not a positive finite number: a triangle without area,
 *     and also one whose products underflow to 0 (|e1 x e2| below about 1e-22, e.g. two edges of 1e-11) or overflow.
 *   - uv0, uv1: barycentrics (1 - u - v, u, v), the products summed left to right (as the shaders' interpolation).
 *   - shading_normal: the stand-in G-buffer's gbuf.frag:35-43 operation for operation -- the interpolated object-space normal; with
 *     VHR_SURFACE_MATERIAL and material.normal_map >= 0 its tangent-space perturbation (VHR_SURFACE_NORMAL_MAPPED; the reference's
 *     cross(tangent_space_normal, tangent) included); then the normal matrix and the normalisation.  Where the squared length of what is
 *     normalised is not a positive finite number: 0 and VHR_SURFACE_NO_SHADING_NORMAL, never a NaN.
 *   - VHR_SURFACE_MATERIAL: base_color (gbuf.frag:19-26: the factor, or the base-colour texture's texel), metallic and roughness
 *     (gbuf.frag:50-56), as the stand-in G-buffer evaluates them, before any UNORM or half store; VHR_SURFACE_DISCARDED where gbuf.frag:27-32
 *     would discard the fragment (the rule of VHR_RAY_QUERY_ALPHA_TEST: a hit found with that flag is never DISCARDED).  Without the flag
 *     the three fields are 0, no texture is read and no normal map is applied.
 *   - Memory and streams as for the queries: device pointers by default, enqueued on the stream vhr_get_current_stream reports (between frames
 *     or inside a pass callback), no synchronisation; VHR_SURFACE_HOST_MEMORY: host pointers, staged, the call returns with results in place.
 *     No frame state is read or written.
 *   - VHR_ERROR_INVALID_ARGUMENT (message in vhr_last_error, with the entry point's name) for, in this order: a NULL context; a NULL pointer
 *     with count > 0; an unknown flag bit; `hits` not 4-byte aligned; `out` not 16-byte aligned -- on every context.  count == 0 then returns
 *     VHR_OK.  VHR_ERROR_NO_DEVICE on a host-only context with VHR_SURFACE_MATERIAL or without VHR_SURFACE_HOST_MEMORY.  VHR_ERROR_GRAPH,
 *     naming vhr_refit_geometry, while geometry updates are pending: a hit belongs to the geometry it was found on.
 *   - A HOST-ONLY context answers the geometry part (everything but VHR_SURFACE_MATERIAL) from the arrays it keeps, with the host's copy of the
 *     same source: the arithmetic is testable without a GPU, and the two are comparable, bit for bit, on one. */
int vhr_resolve_hits(vhr_context *ctx, const vhr_ray_hit *hits, uint32_t count, uint32_t flags, vhr_surface_point *out);
/* The last vhr_resolve_hits (waits for the device): out[0] = hits, out[1] = records with VHR_SURFACE_VALID, out[2] = records with
 * VHR_SURFACE_DISCARDED, out[3] = 1 if the material instantiation ran.  All 0 before the first call. */
int vhr_get_surface_statistics(vhr_context *ctx, uint64_t out[4]);
/* The layout this library was built with, for bindings: out[0] = sizeof(vhr_surface_point), then the offsets of flags, geometric_normal,
 * metallic, shading_normal, roughness, base_color and uv0.  Returns 8. */
int vhr_surface_point_layout(uint32_t out[8]);

/* ---- Hemisphere occlusion masks at surface points: raygen.rgen:44-55's AO rays at arbitrary points, `samples` of them, one bit each ----
 * A QUERY POINT is a vhr_ray read differently: `origin` is where the rays start (the caller applies any normal bias), `direction` is the axis N
 * of the hemisphere -- used as given and never normalised, exactly as raygen.rgen uses the rounded G-buffer normal -- and [tmin, tmax] is the
 * interval of every ray of the point.  The array must be 16-byte aligned, as rays are.
 * RAY (i, j) of point i, sample j < samples, 1 <= samples <= VHR_OCCLUSION_MAX_SAMPLES (64):
 *     g     = i * samples + j                      (uint32_t arithmetic)
 *     state = seed_thread(g ^ seed_thread(seed))   (common.glsl:47-55); a state of 0 is replaced by 0x9E3779B9 -- xorshift would stay at 0 for
 *                                                  ever, and seed_thread is a bijection, so exactly one g per seed meets this
 *     rnd1  = random01(state), rnd2 = random01(state)                (common.glsl:57-76)
 *     d     = onb_transform(N, cosine_hemisphere(rnd1, rnd2))        (common.glsl:37-42, 80-93; the library's fixed-polynomial sin / cos)
 *     ray   = { origin, tmin, d, tmax }
 * every operation the render paths' own, individually rounded fp32.  Samples are keyed independently: ray (i, j) depends on (g, seed) only.
 * THE ANSWER: bit j of occluded[i] is 1 iff vhr_ray_query_masked(..., VHR_RAY_QUERY_TERMINATE_ON_FIRST_HIT, cull_mask, NULL, ...) answers 1 for
 * ray (i, j); bits `samples` and above are 0.  That sentence is the whole definition: decision (vi) with its binary64 re-decision, the mask rule
 * and every degenerate case (a zero or NaN axis, tmin >= tmax, an infinite tmax) follow from it.  AO is 1 - popcount / samples; a bent normal is
 * the caller's sum, over the clear bits, of the directions vhr_debug_occlusion_rays reports.  Results never depend on the tree.
 *   - `flags`: VHR_OCCLUSION_HOST_MEMORY (2) is the only one -- host pointers, staged; the call returns with the masks in place.  Without it
 *     `points` and `occluded` are device pointers and the work is enqueued on the stream vhr_get_current_stream reports, with no
 *     synchronisation, between frames or inside a pass callback.  No frame state is read or written; scratch and counters are per stream.
 *   - VHR_ERROR_INVALID_ARGUMENT (message in vhr_last_error, with the entry point's name) for, in this order: a NULL context; a NULL pointer
 *     with count > 0; an unknown flag bit; `points` not 16-byte aligned; `occluded` not 8-byte aligned; cull_mask > 0xFF; samples == 0 or
 *     samples > VHR_OCCLUSION_MAX_SAMPLES -- on every context.  Then VHR_ERROR_NO_DEVICE on a host-only context and VHR_ERROR_GRAPH while
 *     geometry updates are pending.  count == 0 returns VHR_OK and launches nothing; a context without geometry returns all-zero masks.
 *   - OUT OF SCOPE: the alpha rule (VHR_RAY_QUERY_ALPHA_TEST's bit is an unknown flag here); per-point masks and face culling; stratified or
 *     caller-supplied sample sets; floating-point outputs -- a sum over rays that finish in any order is not reproducible, the mask is. */
int vhr_occlusion_query(vhr_context *ctx, const vhr_ray *points, uint32_t count, uint32_t samples, uint32_t seed, uint32_t flags, uint32_t cull_mask,
                        uint64_t *occluded);
/* The last vhr_occlusion_query (waits for the device): out[0] = points, out[1] = occluded rays over all points, out[2] = points computed again
 * in binary64 (decision (vi): all rays of a point with one self-contradicting candidate), out[3] = waves whose traversal stack overflowed (must
 * be 0).  All 0 before the first call. */
int vhr_get_occlusion_statistics(vhr_context *ctx, uint64_t out[4]);
/* The rays themselves (host memory): the count * samples rays of `points`, point-major, ray (i, j) at out[i * samples + j].  A device context
 * runs the device's copy of the generator, one ray per thread; a HOST-ONLY context runs the host's copy of the same source (as
 * vhr_debug_point_triangle does): the generator is testable without a GPU, and the two are comparable, bit for bit, on one.
 * VHR_ERROR_INVALID_ARGUMENT for a NULL pointer with count > 0 and for samples outside 1 .. VHR_OCCLUSION_MAX_SAMPLES. */
int vhr_debug_occlusion_rays(vhr_context *ctx, const vhr_ray *points, uint32_t count, uint32_t samples, uint32_t seed, vhr_ray *out);

#ifdef __cplusplus
}
#endif
#endif /* VHR_AMD_H */
