// Host side of the forward raster render path: the two passes it registers.
// Reference: src/render_paths/forward_raster_render_path.cpp -- "Depth Prepass" :12-50, "Forward Pass" :52-96, DeregisterPath :98 (owns
// nothing), ImGuiDrawSettings :100-111 (enable_msaa, then Rebuild()).  Both are graphics passes; their bodies (depth_prepass.vert / .frag,
// default.vert / default.frag) stay with the integrator.  vhr_standin_shadow_map and vhr_standin_forward_raster are the library's stand-ins.
//
// Written against the vhr:: facade only, like rayquery_render_path.cpp.
#include "path_handle.hpp"

namespace vhr {

void ForwardRasterRenderPath::RegisterPath(DeviceContext &, RenderGraph &render_graph, ResourceManager &) {
    render_graph.AddGraphicsPass("Depth Prepass", {},
                                 { VkUtils::CreateTransientAttachmentImage("ShadowMap", 4096, 4096, VHR_FORMAT_D32_SFLOAT, 0, VkUtils::ClearDepth(0.0f)) },   // :15
                                 depth_prepass);
    const bool msaa = enable_msaa != 0;
    render_graph.AddGraphicsPass("Forward Pass",
                                 { VkUtils::CreateTransientSampledImage("ShadowMap", 4096, 4096, VHR_FORMAT_D32_SFLOAT, 0) },                           // :54
                                 { VkUtils::CreateTransientRenderOutput(0, msaa),                                                                         // :57
                                   VkUtils::CreateTransientAttachmentImage("Depth", VHR_FORMAT_D32_SFLOAT, 1, VkUtils::ClearDepth(0.0f), msaa) },          // :58
                                 forward_pass);
}

void ForwardRasterRenderPath::DeregisterPath(DeviceContext &, RenderGraph &, ResourceManager &) {}           // :98

}  // namespace vhr

// ---------------------------------------------------------------------------------------------------------
// C entry points (vhr_amd.h, "ForwardRasterRenderPath" section) for callers without a C++ toolchain
// ---------------------------------------------------------------------------------------------------------
struct vhr_forward_raster_render_path : vhr::PathHandle<vhr::ForwardRasterRenderPath> { using PathHandle::PathHandle; };

extern "C" {

int vhr_forward_raster_create(vhr_context *ctx, vhr_external_pass_callback depth_prepass, void *depth_user, vhr_external_pass_callback forward_pass,
                              void *forward_user, int32_t enable_msaa, vhr_forward_raster_render_path **out) {
    const int rc = vhr::path_create(ctx, out);
    if (rc < 0) return rc;
    (*out)->path.enable_msaa = enable_msaa != 0;
    (*out)->Bind(0, &vhr::ForwardRasterRenderPath::depth_prepass, depth_prepass, depth_user);
    (*out)->Bind(1, &vhr::ForwardRasterRenderPath::forward_pass, forward_pass, forward_user);
    return VHR_OK;
}

void vhr_forward_raster_destroy(vhr_forward_raster_render_path *p) { vhr::path_destroy(p); }

int vhr_forward_raster_build(vhr_forward_raster_render_path *p) { return vhr::path_build(p); }

int vhr_forward_raster_rebuild(vhr_forward_raster_render_path *p, int32_t enable_msaa) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    return vhr::guarded(p, [&] {
        p->path.enable_msaa = enable_msaa != 0;          // the radio button, then Rebuild() (:100-111)
        p->path.Rebuild();
    });
}

const char *vhr_forward_raster_last_error(vhr_forward_raster_render_path *p) { return vhr::path_last_error(p); }

}  // extern "C"
