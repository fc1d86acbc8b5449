// Host side of SURVEY.md section 8 row f4: the passes the raytraced render path registers.
// Reference: src/render_paths/raytraced_render_path.cpp -- "Raytracing Pass" :12-47, "Composition Pass" :49-76,
// DeregisterPath :79 (owns nothing), use_anyhit_shader toggle :81-93.
//
// Written against the vhr:: facade only, like hybrid_render_path.cpp.
#include "path_handle.hpp"

namespace vhr {

namespace {
constexpr const char *kRaytracedOutput = "RaytracedOutput";
}

void RaytracedRenderPath::RegisterPath(DeviceContext &context, RenderGraph &render_graph, ResourceManager &) {
    const uint32_t display_w = context.swapchain.extent.width, display_h = context.swapchain.extent.height;

    RaytracingPipelineDescription pipeline;                                        // :17-35
    pipeline.name = "Raytracing Pipeline";
    pipeline.raygen_shader = use_anyhit_shader ? "raytraced_render_path/raygen_test_alpha.rgen" : "raytraced_render_path/raygen.rgen";
    pipeline.miss_shaders = { "raytraced_render_path/miss.rmiss", "raytraced_render_path/shadow_miss.rmiss" };
    pipeline.hit_shaders = { use_anyhit_shader
                                 ? HitShader{ "raytraced_render_path/closesthit_test_alpha.rchit", "raytraced_render_path/shadow_anyhit.rahit" }
                                 : HitShader{ "raytraced_render_path/closesthit.rchit", nullptr } };
    render_graph.AddRaytracingPass(
        "Raytracing Pass", {},
        { VkUtils::CreateTransientStorageImage(kRaytracedOutput, VHR_FORMAT_B8G8R8A8_UNORM, 0) },      // :13-16
        pipeline,
        [display_w, display_h](ExecuteRaytracingCallback execute_pipeline) {                            // :36-46
            execute_pipeline("Raytracing Pipeline", [display_w, display_h](RaytracingExecutionContext &execution_context) {
                execution_context.TraceRays(display_w, display_h);
            });
        });

    // :49-76 -- fullscreen triangle that samples RaytracedOutput into the swapchain image; raster work, declared so the
    // graph has its single RENDER_OUTPUT writer and the execution order of the reference
    render_graph.AddGraphicsPass("Composition Pass",
                                 { VkUtils::CreateTransientSampledImage(kRaytracedOutput, VHR_FORMAT_B8G8R8A8_UNORM, 0) },
                                 { VkUtils::CreateTransientRenderOutput(0) },
                                 composition_pass);
}

void RaytracedRenderPath::DeregisterPath(DeviceContext &, RenderGraph &, ResourceManager &) {}          // :79

}  // namespace vhr

// ---------------------------------------------------------------------------------------------------------
// C entry points (vhr_amd.h, "RaytracedRenderPath" section) for callers without a C++ toolchain
// ---------------------------------------------------------------------------------------------------------
struct vhr_raytraced_render_path : vhr::PathHandle<vhr::RaytracedRenderPath> { using PathHandle::PathHandle; };

extern "C" {

int vhr_raytraced_create(vhr_context *ctx, int32_t use_anyhit_shader, vhr_external_pass_callback composition_pass, void *composition_user,
                         vhr_raytraced_render_path **out) {
    const int rc = vhr::path_create(ctx, out);
    if (rc < 0) return rc;
    (*out)->path.use_anyhit_shader = use_anyhit_shader != 0;
    (*out)->Bind(0, &vhr::RaytracedRenderPath::composition_pass, composition_pass, composition_user);
    return VHR_OK;
}

void vhr_raytraced_destroy(vhr_raytraced_render_path *p) { vhr::path_destroy(p); }

int vhr_raytraced_build(vhr_raytraced_render_path *p) { return vhr::path_build(p); }

int vhr_raytraced_rebuild(vhr_raytraced_render_path *p, int32_t use_anyhit_shader) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    return vhr::guarded(p, [&] {
        p->path.use_anyhit_shader = use_anyhit_shader != 0;      // the radio button, then Rebuild() (:90-92)
        p->path.Rebuild();
    });
}

const char *vhr_raytraced_last_error(vhr_raytraced_render_path *p) { return vhr::path_last_error(p); }

}  // extern "C"
