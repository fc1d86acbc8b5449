// Host side of the rayquery render path: the one pass it registers.
// Reference: src/render_paths/rayquery_render_path.cpp -- "Forward Pass" :12-53, DeregisterPath :56 (owns nothing), ImGuiDrawSettings :58
// (no settings).  The pass is a graphics pass; its body (default.vert / default.frag, whose fragment stage traces one rayQueryEXT shadow
// query) stays with the integrator, and vhr_standin_rayquery_forward is the library's stand-in for it.
//
// Written against the vhr:: facade only, like hybrid_render_path.cpp.
#include "render_paths.hpp"

#include <string>
#include <utility>

namespace vhr {

void RayqueryRenderPath::RegisterPath(DeviceContext &, RenderGraph &render_graph, ResourceManager &) {
    render_graph.AddGraphicsPass("Forward Pass", {},
                                 { VkUtils::CreateTransientRenderOutput(0),                                                      // :16
                                   VkUtils::CreateTransientAttachmentImage("Depth", VHR_FORMAT_D32_SFLOAT, 1, VkUtils::ClearDepth(0.0f)) },   // :17
                                 forward_pass);
}

void RayqueryRenderPath::DeregisterPath(DeviceContext &, RenderGraph &, ResourceManager &) {}           // :56

}  // namespace vhr

// ---------------------------------------------------------------------------------------------------------
// C entry points (vhr_amd.h, "RayqueryRenderPath" section) for callers without a C++ toolchain
// ---------------------------------------------------------------------------------------------------------
struct vhr_rayquery_render_path {
    vhr::DeviceContext context;
    vhr::ResourceManager resource_manager;
    vhr::RenderGraph render_graph;
    vhr::RayqueryRenderPath path;
    vhr_external_pass_callback forward_cb = nullptr;
    void *forward_user = nullptr;
    std::string error;
    vhr_rayquery_render_path(vhr_context *ctx, uint32_t w, uint32_t h)
        : context(ctx), resource_manager(context), render_graph(context, resource_manager), path(context, render_graph, resource_manager) {
        context.swapchain.extent = { w, h };
    }
};

template <typename F>
static int guarded(vhr_rayquery_render_path *p, F &&f) {
    try {
        f();
        return VHR_OK;
    } catch (const std::exception &e) {
        p->error = e.what();
        return VHR_ERROR_GRAPH;
    }
}

extern "C" {

int vhr_rayquery_create(vhr_context *ctx, vhr_external_pass_callback forward_pass, void *forward_user, vhr_rayquery_render_path **out) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    uint32_t w = 0, h = 0;
    if (vhr_get_display_size(ctx, &w, &h) < 0) return VHR_ERROR_INVALID_ARGUMENT;
    auto *p = new vhr_rayquery_render_path(ctx, w, h);
    p->forward_cb = forward_pass;
    p->forward_user = forward_user;
    if (forward_pass) p->path.forward_pass = [p](vhr::DeviceContext &c) { p->forward_cb(p->forward_user, c.handle); };
    *out = p;
    return VHR_OK;
}

void vhr_rayquery_destroy(vhr_rayquery_render_path *p) {
    if (!p) return;
    try {
        p->path.DeregisterPath(p->context, p->render_graph, p->resource_manager);
        p->render_graph.DestroyResources();
    } catch (...) {
    }
    delete p;
}

int vhr_rayquery_build(vhr_rayquery_render_path *p) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    // (the display extent as the context has it NOW: after vhr_resize this is the second half of the reference's resize route, renderer.cpp:113-118)
    uint32_t w = 0, h = 0;
    if (vhr_get_display_size(p->context.handle, &w, &h) < 0) return VHR_ERROR_INVALID_ARGUMENT;
    p->context.swapchain.extent = { w, h };
    return guarded(p, [&] { p->path.Build(); });
}

int vhr_rayquery_rebuild(vhr_rayquery_render_path *p) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    return guarded(p, [&] { p->path.Rebuild(); });
}

const char *vhr_rayquery_last_error(vhr_rayquery_render_path *p) { return p ? p->error.c_str() : ""; }

}  // extern "C"
