// Host side of the forward raster render path: the two passes it registers.
// Reference: src/render_paths/forward_raster_render_path.cpp -- "Depth Prepass" :12-50, "Forward Pass" :52-96, DeregisterPath :98 (owns
// nothing), ImGuiDrawSettings :100-111 (enable_msaa, then Rebuild()).  Both are graphics passes; their bodies (depth_prepass.vert / .frag,
// default.vert / default.frag) stay with the integrator.  vhr_standin_shadow_map and vhr_standin_forward_raster are the library's stand-ins.
//
// Written against the vhr:: facade only, like rayquery_render_path.cpp.
#include "render_paths.hpp"

#include <string>
#include <utility>

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
struct vhr_forward_raster_render_path {
    vhr::DeviceContext context;
    vhr::ResourceManager resource_manager;
    vhr::RenderGraph render_graph;
    vhr::ForwardRasterRenderPath path;
    vhr_external_pass_callback depth_cb = nullptr, forward_cb = nullptr;
    void *depth_user = nullptr, *forward_user = nullptr;
    std::string error;
    vhr_forward_raster_render_path(vhr_context *ctx, uint32_t w, uint32_t h)
        : context(ctx), resource_manager(context), render_graph(context, resource_manager), path(context, render_graph, resource_manager) {
        context.swapchain.extent = { w, h };
    }
};

template <typename F>
static int guarded(vhr_forward_raster_render_path *p, F &&f) {
    try {
        f();
        return VHR_OK;
    } catch (const std::exception &e) {
        p->error = e.what();
        return VHR_ERROR_GRAPH;
    }
}

extern "C" {

int vhr_forward_raster_create(vhr_context *ctx, vhr_external_pass_callback depth_prepass, void *depth_user, vhr_external_pass_callback forward_pass,
                              void *forward_user, int32_t enable_msaa, vhr_forward_raster_render_path **out) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    uint32_t w = 0, h = 0;
    if (vhr_get_display_size(ctx, &w, &h) < 0) return VHR_ERROR_INVALID_ARGUMENT;
    auto *p = new vhr_forward_raster_render_path(ctx, w, h);
    p->path.enable_msaa = enable_msaa != 0;
    p->depth_cb = depth_prepass;
    p->depth_user = depth_user;
    p->forward_cb = forward_pass;
    p->forward_user = forward_user;
    if (depth_prepass) p->path.depth_prepass = [p](vhr::DeviceContext &c) { p->depth_cb(p->depth_user, c.handle); };
    if (forward_pass) p->path.forward_pass = [p](vhr::DeviceContext &c) { p->forward_cb(p->forward_user, c.handle); };
    *out = p;
    return VHR_OK;
}

void vhr_forward_raster_destroy(vhr_forward_raster_render_path *p) {
    if (!p) return;
    try {
        p->path.DeregisterPath(p->context, p->render_graph, p->resource_manager);
        p->render_graph.DestroyResources();
    } catch (...) {
    }
    delete p;
}

int vhr_forward_raster_build(vhr_forward_raster_render_path *p) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    // (the display extent as the context has it NOW: after vhr_resize this is the second half of the reference's resize route, renderer.cpp:113-118)
    uint32_t w = 0, h = 0;
    if (vhr_get_display_size(p->context.handle, &w, &h) < 0) return VHR_ERROR_INVALID_ARGUMENT;
    p->context.swapchain.extent = { w, h };
    return guarded(p, [&] { p->path.Build(); });
}

int vhr_forward_raster_rebuild(vhr_forward_raster_render_path *p, int32_t enable_msaa) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    return guarded(p, [&] {
        p->path.enable_msaa = enable_msaa != 0;          // the radio button, then Rebuild() (:100-111)
        p->path.Rebuild();
    });
}

const char *vhr_forward_raster_last_error(vhr_forward_raster_render_path *p) { return p ? p->error.c_str() : ""; }

}  // extern "C"
