// What the C entry points of the four render paths (vhr_amd.h: vhr_hybrid_*, vhr_raytraced_*, vhr_rayquery_*, vhr_forward_raster_*) have in
// common: the handle behind the opaque pointer, and create / destroy / build / last_error.  Each *_render_path.cpp derives its opaque struct
// from PathHandle<its path> and says only which settings it applies and which C callback goes in which slot.
#pragma once

#include <cstdint>
#include <exception>
#include <string>

#include "render_paths.hpp"

namespace vhr {

template <typename Path>
struct PathHandle {
    DeviceContext context;
    ResourceManager resource_manager;
    RenderGraph render_graph;
    Path path;
    struct { vhr_external_pass_callback callback = nullptr; void *user = nullptr; } slots[2];     // no path has more than two external passes
    std::string error;

    PathHandle(vhr_context *ctx, uint32_t w, uint32_t h)
        : context(ctx), resource_manager(context), render_graph(context, resource_manager), path(context, render_graph, resource_manager) {
        context.swapchain.extent = { w, h };
    }
    PathHandle(const PathHandle &) = delete;            // the pass bodies below capture `this`

    // A C callback becomes the body of one external pass; without one the member stays an empty std::function.
    void Bind(int slot, ExternalPassCallback Path::*pass, vhr_external_pass_callback callback, void *user) {
        slots[slot].callback = callback;
        slots[slot].user = user;
        if (callback) path.*pass = [this, slot](DeviceContext &c) { slots[slot].callback(slots[slot].user, c.handle); };
    }
};

template <typename Handle, typename F>
int guarded(Handle *p, F &&f) {
    try {
        f();
        return VHR_OK;
    } catch (const std::exception &e) {
        p->error = e.what();
        return VHR_ERROR_GRAPH;
    }
}

// the prologue of every *_create: the handle at the context's display size (settings and callbacks are the caller's to add)
template <typename Handle>
int path_create(vhr_context *ctx, Handle **out) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    uint32_t w = 0, h = 0;
    if (vhr_get_display_size(ctx, &w, &h) < 0) return VHR_ERROR_INVALID_ARGUMENT;
    *out = new Handle(ctx, w, h);
    return VHR_OK;
}

template <typename Handle>
void path_destroy(Handle *p) {
    if (!p) return;
    try {
        p->path.DeregisterPath(p->context, p->render_graph, p->resource_manager);
        p->render_graph.DestroyResources();
    } catch (...) {
    }
    delete p;
}

template <typename Handle>
int path_build(Handle *p) {
    if (!p) return VHR_ERROR_INVALID_ARGUMENT;
    // (the display extent as the context has it NOW: after vhr_resize this is the second half of the reference's resize route, renderer.cpp:113-118)
    uint32_t w = 0, h = 0;
    if (vhr_get_display_size(p->context.handle, &w, &h) < 0) return VHR_ERROR_INVALID_ARGUMENT;
    p->context.swapchain.extent = { w, h };
    return guarded(p, [&] { p->path.Build(); });
}

template <typename Handle>
const char *path_last_error(Handle *p) { return p ? p->error.c_str() : ""; }

}  // namespace vhr
