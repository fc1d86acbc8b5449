// Host side of the rayquery render path: the one pass it registers.
// Reference: src/render_paths/rayquery_render_path.cpp -- "Forward Pass" :12-53, DeregisterPath :56 (owns nothing), ImGuiDrawSettings :58
// (no settings).  The pass is a graphics pass; its body (default.vert / default.frag, whose fragment stage traces one rayQueryEXT shadow
// query) stays with the integrator, and vhr_standin_rayquery_forward is the library's stand-in for it.
//
// Written against the vhr:: facade only, like hybrid_render_path.cpp.
#include "path_handle.hpp"

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
struct vhr_rayquery_render_path : vhr::PathHandle<vhr::RayqueryRenderPath> { using PathHandle::PathHandle; };

extern "C" {

int vhr_rayquery_create(vhr_context *ctx, vhr_external_pass_callback forward_pass, void *forward_user, vhr_rayquery_render_path **out) {
    const int rc = vhr::path_create(ctx, out);
    if (rc < 0) return rc;
    (*out)->Bind(0, &vhr::RayqueryRenderPath::forward_pass, forward_pass, forward_user);
    return VHR_OK;
}

void vhr_rayquery_destroy(vhr_rayquery_render_path *p) { vhr::path_destroy(p); }

int vhr_rayquery_build(vhr_rayquery_render_path *p) { return vhr::path_build(p); }

int vhr_rayquery_rebuild(vhr_rayquery_render_path *p) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    return vhr::guarded(p, [&] { p->path.Rebuild(); });
}

const char *vhr_rayquery_last_error(vhr_rayquery_render_path *p) { return vhr::path_last_error(p); }

}  // extern "C"
