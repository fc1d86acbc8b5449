// Context + ResourceManager half of the C ABI (include/vhr_amd.h): create and destroy, the context's streams and timers, options, the
// bindless texture table, the storage-image pool, the per-frame uniform data, the ray statistics and the stand-in passes.  The scene arrays
// and the acceleration structure are csrc/geometry.cpp's, the ray and point queries csrc/queries.cpp's.
// Reference: src/rendering_backend/resource_manager.{h,cpp}, vulkan_context.cpp.
#include <cmath>
#include <cstring>
#include <string>

#include "vhr_internal.hpp"
#include "fingerprint.h"      // build/fingerprint.h, written by the Makefile

namespace vhr {
// Every ray-tracing unit's copy of the sRGB decode table (SrgbLutCopy, vhr_internal.hpp).  The head is constant-initialised, so it is there before
// the first unit's constructor runs, in whatever order the units are initialised.
static SrgbLutCopy *g_srgb_lut_copies = nullptr;
SrgbLutCopy::SrgbLutCopy(int (*copy_fn)(const float *)) : copy(copy_fn), next(g_srgb_lut_copies) { g_srgb_lut_copies = this; }
int upload_srgb_lut(const float *lut) {
    if (!g_srgb_lut_copies) return -1;
    for (const SrgbLutCopy *c = g_srgb_lut_copies; c; c = c->next)
        if (c->copy(lut) != 0) return -1;
    return 0;
}

uint32_t format_stride(int32_t format) {      // VkUtils::FormatStride, vulkan_utils.h:128-148
    switch (format) {
        case VHR_FORMAT_R8G8B8A8_UNORM:
        case VHR_FORMAT_R8G8B8A8_SRGB:
        case VHR_FORMAT_B8G8R8A8_UNORM:
        case VHR_FORMAT_B8G8R8A8_SRGB:
        case VHR_FORMAT_R16G16_SFLOAT:
        case VHR_FORMAT_D32_SFLOAT: return 4;
        case VHR_FORMAT_R16G16B16A16_SFLOAT: return 8;
        default: return 0;
    }
}
}  // namespace vhr

using namespace vhr;

static thread_local std::string g_create_error;     // vhr_create has no context to carry its message: per thread

// ---- optional per-kernel event timing -------------------------------------------------------------
static constexpr size_t kTimerCapacity = 16384;     // events per kernel kind (8192 launches between drains)

// Events for the next kernel dispatch.  A kernel kind under vhr_set_kernel_timing gets its own (start, stop) pair; the pass
// whose callback is running gets its begin stamp on its first dispatch and its end stamp on every dispatch (the last one
// stands).  Where both want the same slot the kernel timer wins and the pass falls back to a recorded event.
void vhr_context::dispatch_events(hipEvent_t &start, hipEvent_t &stop) {
    start = stop = nullptr;
    if (timing_kind >= 0 && (kernel_timing_mask & (1u << timing_kind))) {
        KernelTimer &t = kernel_timers[timing_kind];
        // "kernel_timing_stride" n: only every n-th launch of the kind carries an event pair (a profiled dispatch costs ~6 us of
        // completion-signal and release-fence handling that the next kernel waits for; sampling keeps the measured loop honest)
        const uint64_t stride = uint64_t(std::max(1, options[vhr::kOptKernelTimingStride]));
        if ((t.seen++ % stride) == 0 && t.used + 2 <= kTimerCapacity) {
            while (t.events.size() < t.used + 2) {
                hipEvent_t e;
                if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) break;
                t.events.push_back(e);
            }
            if (t.events.size() >= t.used + 2) {
                start = t.events[t.used];
                stop = t.events[t.used + 1];
                t.used += 2;
            }
        }
    }
    if (cur_pass && options[vhr::kOptPassTimestamps] && cur_pass->ev_begin && !(in_kernel_stamps() && cur_pass->stamp_index >= 0)) {
        if (!cur_pass->begin_stamped) {
            if (!start) start = cur_pass->ev_begin;
            else hipEventRecord(cur_pass->ev_begin, stream);
            cur_pass->begin_stamped = true;
        }
        if (!stop) { stop = cur_pass->ev_end; cur_pass->end_on_last_dispatch = true; }
        else cur_pass->end_on_last_dispatch = false;
    }
}

// The stamps of the next kernel launch (vhr::launch): the end of the pass that finished last, the begin of the running pass's first kernel.
vhr::Stamps vhr_context::take_stamps() {
    vhr::Stamps st{ nullptr, nullptr };
    if (!in_kernel_stamps()) pending_end = nullptr;      // (stamps switched to event pairs while an end was pending: nothing will store it)
    if (no_stamps || !in_kernel_stamps()) return st;
    if (pending_end) { st.prev_end = pending_end; pending_end = nullptr; }
    if (cur_pass && options[vhr::kOptPassTimestamps] && cur_pass->stamp_index >= 0 && !cur_pass->begin_stamped) {
        st.begin = &d_stamps[cur_pass->stamp_index].begin;
        cur_pass->begin_stamped = true;
        cur_pass->stamped_in_kernel = true;
    }
    return st;
}

int vhr_context::sync_streams() {
    if (host_only) return VHR_OK;
    if (deferred_raygen) VHR_TRY(vhr::flush_deferred_raygen(this, nullptr));
    if (pending_end) vhr::launch_stamp(this);          // the end of the last pass, before the host waits for it
    if (front_stream && hipStreamSynchronize(front_stream) != hipSuccess) return fail(VHR_ERROR_DEVICE, "hipStreamSynchronize(front stream) failed");
    if (side_stream && hipStreamSynchronize(side_stream) != hipSuccess) return fail(VHR_ERROR_DEVICE, "hipStreamSynchronize(side stream) failed");
    side_pending = false;
    if (refl_stream && hipStreamSynchronize(refl_stream) != hipSuccess) return fail(VHR_ERROR_DEVICE, "hipStreamSynchronize(mirror-ray stream) failed");
    refl_pending = false;
    if (hipStreamSynchronize(stream) != hipSuccess) return fail(VHR_ERROR_DEVICE, "hipStreamSynchronize failed");     // (a null handle is the default stream)
    return VHR_OK;
}

int vhr_context::join_side() {
    if (!side_pending) return VHR_OK;
    side_pending = false;
    if (hipStreamWaitEvent(stream, side_done, 0) != hipSuccess) return fail(VHR_ERROR_DEVICE, "hipStreamWaitEvent(side stream) failed");
    return VHR_OK;
}

int vhr_context::join_refl() {
    if (!refl_pending) return VHR_OK;
    refl_pending = false;
    if (hipStreamWaitEvent(stream, refl_done, 0) != hipSuccess) return fail(VHR_ERROR_DEVICE, "hipStreamWaitEvent(mirror-ray stream) failed");
    return VHR_OK;
}

extern "C" {

int vhr_set_kernel_timing(vhr_context *ctx, int32_t kind_mask) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    ctx->kernel_timing_mask = uint32_t(kind_mask);
    return VHR_OK;
}

int vhr_get_kernel_time(vhr_context *ctx, int32_t kind, double *total_ms, uint64_t *launches, int32_t reset) {
    if (!ctx || kind < 0 || kind >= kKernelKinds) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    KernelTimer &t = ctx->kernel_timers[kind];
    for (size_t i = 0; i + 1 < t.used; i += 2) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, t.events[i], t.events[i + 1]) == hipSuccess) { t.total_ms += ms; ++t.launches; }
    }
    t.used = 0;
    if (total_ms) *total_ms = t.total_ms;
    if (launches) *launches = t.launches;
    if (reset) { t.total_ms = 0.0; t.launches = 0; }
    return VHR_OK;
}

const char *vhr_version(void) { return "vhr_amd 0.1.0 (gfx950)"; }

int vhr_abi_struct_sizes(uint32_t out[8]) {
    out[0] = sizeof(vhr_vertex); out[1] = sizeof(vhr_material); out[2] = sizeof(vhr_primitive);
    out[3] = sizeof(vhr_directional_light); out[4] = sizeof(vhr_per_frame_data); out[5] = sizeof(vhr_svgf_push_constants);
    out[6] = sizeof(vhr_trace_params); out[7] = 0;
    return 7;
}

void vhr_default_trace_params(vhr_trace_params *p) {
    p->shadow_enable = 1;          // raygen.rgen:31-41
    p->ao_spp = 2;                 // raygen.rgen:45
    p->ao_tmax = 5.0f;             // raygen.rgen:52
    p->reflections = 1;            // raygen.rgen:59-65
    p->cone_cos_max = 0.999995f;   // raygen.rgen:34
    p->normal_bias = 0.1f;         // raygen.rgen:29
    p->tmin = 0.01f;               // raygen.rgen:40
    p->tmax = 10000.0f;
}

int vhr_create(const vhr_create_info *info, vhr_context **out) {
    if (!info || !out || info->width == 0 || info->height == 0) { g_create_error = "vhr_create: invalid arguments"; return VHR_ERROR_INVALID_ARGUMENT; }
    if (info->flags & VHR_CREATE_HOST_ONLY) {
        // graph bookkeeping only (pass registry, execution order, SanityCheck): no device is touched and
        // nothing can be executed, uploaded or downloaded
        vhr_context *ctx = new vhr_context();
        ctx->host_only = true;
        ctx->width = info->width;
        ctx->height = info->height;
        ctx->row_end = info->height;
        ctx->col_end = info->width;
        ctx->storage_images.resize(vhr_context::kMaxGlobalResources);
        vhr_default_trace_params(&ctx->trace_params);
        *out = ctx;
        return VHR_OK;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        // the product path never falls back to the CPU
        g_create_error = "vhr_create: no HIP device available (this library has no CPU path)";
        return VHR_ERROR_NO_DEVICE;
    }
    if (info->device < 0 || info->device >= count) { g_create_error = "vhr_create: device ordinal out of range"; return VHR_ERROR_INVALID_ARGUMENT; }
    if (hipSetDevice(info->device) != hipSuccess) { g_create_error = "vhr_create: hipSetDevice failed"; return VHR_ERROR_DEVICE; }
    vhr_context *ctx = new vhr_context();
    ctx->device = info->device;
    ctx->width = info->width;
    ctx->height = info->height;
    ctx->row_begin = 0;
    ctx->row_end = info->height;
    ctx->col_begin = 0;
    ctx->col_end = info->width;
    if (info->flags & VHR_CREATE_INTERNAL_STREAM) {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            g_create_error = "vhr_create: hipStreamCreate failed";
            delete ctx;
            return VHR_ERROR_DEVICE;
        }
        ctx->own_stream = true;
    } else {
        // the caller's stream, used as given; NULL is the device's default stream (which is also what
        // torch.cuda.current_stream().cuda_stream reports for PyTorch's default stream)
        ctx->stream = static_cast<hipStream_t>(info->stream);
    }
    ctx->storage_images.resize(vhr_context::kMaxGlobalResources);
    vhr_default_trace_params(&ctx->trace_params);
    float lut[256];
    for (int i = 0; i < 256; ++i) {
        double c = i / 255.0;
        lut[i] = float(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, info->device) == hipSuccess && prop.multiProcessorCount > 0) ctx->cu_count = prop.multiProcessorCount;
    if (upload_srgb_lut(lut) != 0 || hipMalloc(reinterpret_cast<void **>(&ctx->d_ray_stats), 2 * sizeof(RayStats)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&ctx->d_tile_counter), sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&ctx->d_stamps), sizeof(vhr::PassStampPair) * vhr::kMaxStampedPasses) != hipSuccess ||
        hipMemset(ctx->d_stamps, 0, sizeof(vhr::PassStampPair) * vhr::kMaxStampedPasses) != hipSuccess) {
        g_create_error = "vhr_create: device initialisation failed";
        vhr_destroy(ctx);
        return VHR_ERROR_DEVICE;
    }
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, info->device) == hipSuccess && khz > 0) ctx->wall_clock_khz = double(khz);
    *out = ctx;
    return VHR_OK;
}

void vhr_destroy(vhr_context *ctx) {
    if (!ctx) return;
    if (ctx->host_only) {
        vhr_graph_destroy_resources(ctx);
        delete ctx;
        return;
    }
    hipSetDevice(ctx->device);
    ctx->sync_streams();
    vhr_graph_destroy_resources(ctx);
    if (ctx->front_stream) hipStreamDestroy(ctx->front_stream);
    if (ctx->refl_stream) hipStreamDestroy(ctx->refl_stream);
    if (ctx->refl_ready) hipEventDestroy(ctx->refl_ready);
    if (ctx->refl_done) hipEventDestroy(ctx->refl_done);
    if (ctx->side_stream) hipStreamDestroy(ctx->side_stream);
    if (ctx->side_ready) hipEventDestroy(ctx->side_ready);
    if (ctx->side_done) hipEventDestroy(ctx->side_done);
    hipFree(ctx->d_stamps);
    for (auto &im : ctx->storage_images) {      // {ptr, alt} hold both allocations of a double-buffered image
        if (!im.used) continue;
        hipFree(im.ptr);
        if (im.alt && im.alt != im.ptr) hipFree(im.alt);
    }
    for (auto &t : ctx->textures) hipFree(t.texels);
    hipFree(ctx->d_textures);
    free_scene(ctx);
    hipFree(ctx->d_ray_stats);
    free_query_scratch(ctx);
    hipFree(ctx->d_tile_counter);
    for (vhr_context::CostOrder *co : { &ctx->cost_order_raygen, &ctx->cost_order_reflection, &ctx->cost_order_raytraced })
        for (int i = 0; i < 2; ++i) { hipFree(co->cost[i]); hipFree(co->order[i]); }
    for (auto &t : ctx->kernel_timers)
        for (hipEvent_t e : t.events) hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *vhr_last_error(const vhr_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int vhr_get_current_stream(vhr_context *ctx, void **stream) {
    if (!ctx || !stream) return VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->deferred_raygen) VHR_TRY(vhr::flush_deferred_raygen(ctx, nullptr));      // the caller is about to enqueue behind it
    // ... and its own kernels may read the Reflections image or rewrite the G-buffer the mirror ray's pending launch reads: the stream waits for
    // that launch here ("reflection_async" 2 = the multi-GPU hooks, which only touch SVGF images and join where they must, keep the overlap)
    if (!ctx->host_only && ctx->options[vhr::kOptReflectionAsync] != 2) VHR_TRY(ctx->join_refl());
    *stream = static_cast<void *>(ctx->stream);       // inside a pass callback of vhr_graph_execute: the stream that pass is ordered on
    return VHR_OK;
}

int vhr_synchronize(vhr_context *ctx) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return VHR_OK;
    if (!ctx->recorded.empty()) VHR_TRY(vhr::flush_recorded(ctx));    // called from inside a compute pass
    VHR_TRY(ctx->sync_streams());
    return VHR_OK;
}

int32_t vhr_upload_texture_from_data(vhr_context *ctx, uint32_t width, uint32_t height, const uint8_t *data, int32_t format,
                                     const vhr_sampler_info *sampler_info) {
    // (-1 is the reference's "table exhausted" sentinel, resource_manager.cpp:847-848, and nothing else)
    if (!ctx || !data || !width || !height) return ctx ? ctx->fail(VHR_ERROR_UNSUPPORTED, "UploadTextureFromData: invalid arguments") : VHR_ERROR_UNSUPPORTED;
    if (format != VHR_FORMAT_R8G8B8A8_SRGB && format != VHR_FORMAT_R8G8B8A8_UNORM)
        return ctx->fail(VHR_ERROR_UNSUPPORTED, "UploadTextureFromData: format must be R8G8B8A8_SRGB or R8G8B8A8_UNORM");
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    if (ctx->textures.size() >= vhr_context::kMaxGlobalResources) { ctx->error = "texture table exhausted"; return -1; }   // resource_manager.cpp:847-848
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    vhr_context::Texture t{};
    const size_t bytes = size_t(width) * height * 4;
    HIP_TRY(ctx, hipMalloc(&t.texels, bytes));
    HIP_TRY(ctx, hipMemcpy(t.texels, data, bytes, hipMemcpyHostToDevice));
    t.w = width; t.h = height; t.format = format;
    // default sampler: LINEAR / REPEAT (resource_manager.cpp:58-69)
    t.sampler = sampler_info ? *sampler_info : vhr_sampler_info{ 1, 1, 0, 0 };
    ctx->textures.push_back(t);
    // rebuild the device-side descriptor table (set 0, binding 4: textures[])
    std::vector<DeviceTexture> table(ctx->textures.size());
    for (size_t i = 0; i < table.size(); ++i) {
        const auto &s = ctx->textures[i];
        table[i] = DeviceTexture{ static_cast<const uint8_t *>(s.texels), s.w, s.h, s.format, s.sampler.mag_filter, s.sampler.address_mode_u, s.sampler.address_mode_v, 0 };
    }
    VHR_TRY(ctx->sync_streams());
    hipFree(ctx->d_textures);
    ctx->d_textures = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_textures), sizeof(DeviceTexture) * table.size()));
    HIP_TRY(ctx, hipMemcpy(ctx->d_textures, table.data(), sizeof(DeviceTexture) * table.size(), hipMemcpyHostToDevice));
    return int32_t(ctx->textures.size() - 1);
}

int32_t vhr_upload_new_storage_image(vhr_context *ctx, uint32_t width, uint32_t height, int32_t format) {
    // -1 is the reference's "pool exhausted" sentinel (resource_manager.cpp:876-877) and nothing else: every failure is < -1
    if (!ctx) return VHR_ERROR_UNSUPPORTED;
    const uint32_t bpp = format_stride(format);
    if (!bpp || !width || !height) return ctx->fail(VHR_ERROR_UNSUPPORTED, "UploadNewStorageImage: unsupported format or empty extent");
    if (!ctx->host_only) HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t i = 0; i < vhr_context::kMaxGlobalResources; ++i) {         // first free slot, resource_manager.cpp:866-878
        Image &im = ctx->storage_images[i];
        if (im.used) continue;
        im = Image{};
        im.width = width; im.height = height; im.format = format; im.bpp = bpp;
        if (ctx->host_only) { im.used = true; return int32_t(i); }
        // svgf.comp reads neighbours of, and rewrites, the moments history in one dispatch (svgf.comp:72,140-144): an RG16F image
        // keeps a second buffer so that the dispatch reads a snapshot
        const bool twin = format == VHR_FORMAT_R16G16_SFLOAT;
        hipError_t e = hipMalloc(&im.owned, im.bytes());
        if (e == hipSuccess) e = hipMemsetAsync(im.owned, 0, im.bytes(), ctx->stream);
        if (e == hipSuccess && twin) e = hipMalloc(&im.alt, im.bytes());
        if (e == hipSuccess && twin) e = hipMemsetAsync(im.alt, 0, im.bytes(), ctx->stream);
        if (e != hipSuccess) {                        // nothing half-made stays behind
            hipFree(im.owned);
            hipFree(im.alt);
            im = Image{};
            return ctx->fail(VHR_ERROR_DEVICE, std::string("UploadNewStorageImage: ") + hipGetErrorString(e));
        }
        im.ptr = im.owned;
        im.used = true;
        return int32_t(i);
    }
    ctx->error = "storage image pool exhausted";
    return -1;
}

int vhr_destroy_storage_image(vhr_context *ctx, int32_t id) {
    if (!ctx || id < 0 || uint32_t(id) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[id].used)
        return ctx ? ctx->fail(VHR_ERROR_NOT_FOUND, "DestroyStorageImage: no such image") : VHR_ERROR_INVALID_ARGUMENT;   // assert at resource_manager.cpp:266
    if (ctx->host_only) { ctx->storage_images[id] = Image{}; return VHR_OK; }
    VHR_TRY(ctx->sync_streams());
    Image &im = ctx->storage_images[id];
    // ptr/alt may have been flipped: free both distinct allocations
    void *a = im.ptr, *b = im.alt;
    hipFree(a);
    if (b && b != a) hipFree(b);
    im = Image{};
    return VHR_OK;
}

int vhr_update_per_frame_ubo(vhr_context *ctx, uint32_t resource_idx, const vhr_per_frame_data *pfd) {
    if (!ctx || !pfd || resource_idx >= 3) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdatePerFrameUBO: invalid arguments") : VHR_ERROR_INVALID_ARGUMENT;
    std::memcpy(&ctx->per_frame[resource_idx], pfd, sizeof *pfd);            // resource_manager.cpp:362-364
    return VHR_OK;
}

int vhr_get_last_per_frame_ubo(vhr_context *ctx, vhr_per_frame_data *out) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    std::memcpy(out, &ctx->per_frame[ctx->last_resource_idx], sizeof *out);
    return VHR_OK;
}

int vhr_set_trace_params(vhr_context *ctx, const vhr_trace_params *p) {
    if (!ctx || !p) return VHR_ERROR_INVALID_ARGUMENT;
    if (p->ao_spp > 64) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "trace params: ao_spp > 64");
    ctx->trace_params = *p;
    return VHR_OK;
}

int vhr_set_tile(vhr_context *ctx, uint32_t col_begin, uint32_t col_end, uint32_t row_begin, uint32_t row_end, uint32_t overlap,
                 uint32_t halo_rows, uint32_t halo_cols) {
    if (!ctx || row_begin > row_end || row_end > ctx->height || col_begin > col_end || col_end > ctx->width || halo_rows < overlap || halo_cols < overlap)
        return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "set_tile: need begin <= end <= extent on both axes and halos >= overlap") : VHR_ERROR_INVALID_ARGUMENT;
    ctx->row_begin = row_begin;
    ctx->row_end = row_end;
    ctx->col_begin = col_begin;
    ctx->col_end = col_end;
    ctx->overlap = overlap;
    ctx->halo = halo_rows;
    ctx->halo_cols = halo_cols;
    return VHR_OK;
}

int vhr_set_strip(vhr_context *ctx, uint32_t row_begin, uint32_t row_end, uint32_t overlap, uint32_t halo) {
    if (!ctx || row_begin > row_end || row_end > ctx->height || halo < overlap)
        return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "set_strip: need row_begin <= row_end <= height and halo >= overlap") : VHR_ERROR_INVALID_ARGUMENT;
    return vhr_set_tile(ctx, 0, ctx->width, row_begin, row_end, overlap, halo, std::max(halo, ctx->width));      // every column: a strip
}

int vhr_set_option(vhr_context *ctx, const char *key, int32_t value) {
    if (!ctx || !key) return VHR_ERROR_INVALID_ARGUMENT;
    if (!std::strcmp(key, "bvh_leaf_triangles")) {          // applies to the next vhr_update_geometry
        if (value < 1 || value > kMaxLeafTris) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_leaf_triangles must be 1..4");
        ctx->bvh_leaf_tris = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "bvh_host_checks")) {              // applies to the next vhr_update_geometry
        if (value < 0 || value > 1) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_host_checks must be 0 or 1");
        ctx->bvh_host_checks = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "bvh_device_max_depth")) {         // applies to the next vhr_update_geometry
        if (value < 1 || value > kMaxBvhDepth) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_device_max_depth must be 1..40");
        ctx->bvh_device_max_depth = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "bvh_builder")) {                  // applies to the next vhr_update_geometry
        if (value < 0 || value > 1) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_builder must be 0 (binned SAH on the host) or 1 (binned SAH on the device)");
        ctx->bvh_builder = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "bvh_frame")) {                    // applies to the next vhr_update_geometry
        if (value < 0 || value > 1) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_frame must be 0 (boxes along the world axes) or 1 (along the frame that minimises the triangles' summed box area)");
        ctx->bvh_frame_mode = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "bvh_presplit")) {                 // applies to the next vhr_update_geometry
        if (value < 0 || value > 400) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_presplit must be 0 (off) or the budget of extra triangle references in percent (1..400)");
        ctx->bvh_presplit = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "bvh_build_threads")) {            // applies to the next vhr_update_geometry; the tree does not depend on it
        if (value < 0 || value > 64) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "bvh_build_threads must be 0..64");
        ctx->bvh_build_threads = value;
        return VHR_OK;
    }
    if (!std::strcmp(key, "alpha_test_rays")) {              // read at every launch of the hybrid path's rays
        if (value < 0 || value > 1) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "alpha_test_rays must be 0 (every triangle is opaque to the hybrid path's rays) or 1 (they skip what the G-buffer pass discards)");
        ctx->alpha_test_rays = value;
        return VHR_OK;
    }
    {   // the hybrid path's ray-class cull masks: read at every launch of its rays, like "alpha_test_rays"
        int *const slot = !std::strcmp(key, "shadow_ray_mask") ? &ctx->shadow_ray_mask : !std::strcmp(key, "ao_ray_mask") ? &ctx->ao_ray_mask :
                          !std::strcmp(key, "reflection_ray_mask") ? &ctx->reflection_ray_mask : nullptr;
        if (slot) {
            if (value < 0 || value > 255) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(key) + " must be 0..255 (a primitive whose mask shares no bit with it does not exist for that class of rays)");
            *slot = value;
            return VHR_OK;
        }
    }
    if (!std::strcmp(key, "object_motion_vectors")) {        // the refits keep last frame's triangle records; the stand-in G-buffer reprojects through them
        if (value < 0 || value > 1)
            return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "object_motion_vectors must be 0 (motion vectors follow the camera only) or 1 (and the geometry the refits moved)");
        if (ctx->recording || ctx->cur_pass) return ctx->fail(VHR_ERROR_GRAPH, "object_motion_vectors: set from inside a pass");
        if (value == ctx->object_motion_vectors) return VHR_OK;
        if (!ctx->host_only) {                               // frames in flight read the arrays that are about to be made or freed
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            VHR_TRY(ctx->sync_streams());
        }
        ctx->object_motion_vectors = value;
        const int rc = reset_motion(ctx);
        if (rc != VHR_OK) ctx->object_motion_vectors = 0;
        return rc;
    }
    for (int i = 0; i < vhr::kOptCount; ++i) {
        const vhr::OptionInfo &o = vhr::kOptionInfo[i];
        if (std::strcmp(key, o.name)) continue;
        if (value < o.lo || value > o.hi)
            return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(o.name) + " must be " + std::to_string(o.lo) + ".." + std::to_string(o.hi));
        ctx->options[i] = value;
        return VHR_OK;
    }
    return ctx->fail(VHR_ERROR_NOT_FOUND, std::string("unknown option '") + key + "'");
}

int32_t vhr_option_count(void) { return vhr::kOptCount; }

int vhr_option_info(int32_t index, const char **name, int32_t *default_value, int32_t *min_value, int32_t *max_value) {
    if (index < 0 || index >= vhr::kOptCount) return VHR_ERROR_INVALID_ARGUMENT;
    const vhr::OptionInfo &o = vhr::kOptionInfo[index];
    if (name) *name = o.name;
    if (default_value) *default_value = o.def;
    if (min_value) *min_value = o.lo;
    if (max_value) *max_value = o.hi;
    return VHR_OK;
}

int vhr_get_option(vhr_context *ctx, const char *key, int32_t *value) {
    if (!ctx || !key || !value) return VHR_ERROR_INVALID_ARGUMENT;
    if (!std::strcmp(key, "alpha_test_rays")) { *value = ctx->alpha_test_rays; return VHR_OK; }
    if (!std::strcmp(key, "object_motion_vectors")) { *value = ctx->object_motion_vectors; return VHR_OK; }
    if (!std::strcmp(key, "shadow_ray_mask")) { *value = ctx->shadow_ray_mask; return VHR_OK; }
    if (!std::strcmp(key, "ao_ray_mask")) { *value = ctx->ao_ray_mask; return VHR_OK; }
    if (!std::strcmp(key, "reflection_ray_mask")) { *value = ctx->reflection_ray_mask; return VHR_OK; }
    for (int i = 0; i < vhr::kOptCount; ++i)
        if (!std::strcmp(key, vhr::kOptionInfo[i].name)) { *value = ctx->options[i]; return VHR_OK; }
    return ctx->fail(VHR_ERROR_NOT_FOUND, std::string("unknown option '") + key + "'");
}

int vhr_set_ray_statistics(vhr_context *ctx, int32_t enable) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    ctx->ray_stats_enabled = enable != 0;
    return VHR_OK;
}

int vhr_get_ray_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    const vhr_trace_params &tp = ctx->trace_params;
    const uint64_t covered = ctx->h_ray_stats.covered_pixels;
    if (ctx->raytraced_pixels) {          // raytraced render path: one primary ray per pixel + one shadow ray per primary hit
        out[0] = out[1] = ctx->raytraced_pixels + covered;
        out[2] = covered;
        out[3] = ctx->h_ray_stats.stack_overflows;
        return VHR_OK;
    }
    const uint64_t second = ctx->h_ray_stats.second_bounce_rays;       // two-bounce extension: one more ray per first-bounce hit
    out[0] = covered * (uint64_t(tp.shadow_enable ? 1 : 0) + tp.ao_spp + (tp.reflections ? 1 : 0)) + second;
    out[1] = covered * (uint64_t(tp.shadow_enable ? 4 : 0) + tp.ao_spp + (tp.reflections ? 1 : 0)) + second;   // raygen.rgen:38-40 duplicates
    out[2] = covered;
    out[3] = ctx->h_ray_stats.stack_overflows;
    return VHR_OK;
}

int vhr_get_traversal_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    out[0] = ctx->h_ray_stats.node_visits; out[1] = ctx->h_ray_stats.leaf_visits;
    out[2] = ctx->h_ray_stats.triangle_tests; out[3] = ctx->h_ray_stats.wave_iterations;
    return VHR_OK;
}

int vhr_get_reflection_statistics(vhr_context *ctx, uint64_t out[10]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    const RayStats &r = ctx->h_refl_stats;
    out[0] = r.unique_rays; out[1] = r.second_bounce_rays; out[2] = r.node_visits; out[3] = r.leaf_visits; out[4] = r.triangle_tests;
    out[5] = r.wave_iterations; out[6] = r.refills; out[7] = r.waves; out[8] = r.cycles_total; out[9] = r.cycles_nodes;
    return VHR_OK;
}

int vhr_get_binary64_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    out[0] = ctx->h_ray_stats.pending_rays; out[1] = ctx->h_refl_stats.pending_rays; out[2] = ctx->alpha_launches; out[3] = 0;
    return VHR_OK;
}

int vhr_get_traversal_cycles(vhr_context *ctx, uint64_t out[8]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    const RayStats &r = ctx->h_ray_stats;
    out[0] = r.cycles_total; out[1] = r.cycles_setup; out[2] = r.cycles_refill; out[3] = r.cycles_nodes;
    out[4] = r.cycles_leaves; out[5] = r.refills; out[6] = r.waves; out[7] = r.drain_iterations;
    return VHR_OK;
}

int vhr_get_drain_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->sync_streams());
    const RayStats &r = ctx->h_ray_stats;
    out[0] = r.cut_entries; out[1] = r.drain_le4; out[2] = r.drain_le8; out[3] = r.drain_le16;
    return VHR_OK;
}

int vhr_calibration_stream_read(vhr_context *ctx, int32_t storage_image, uint32_t bytes_per_lane) {
    if (!ctx || ctx->host_only || storage_image < 0 || uint32_t(storage_image) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[storage_image].used)
        return ctx ? ctx->fail(VHR_ERROR_NOT_FOUND, "calibration: no such storage image") : VHR_ERROR_INVALID_ARGUMENT;
    return launch_calibration_read(ctx, ctx->storage_images[storage_image], bytes_per_lane, ctx->d_tile_counter);
}

const char *vhr_source_fingerprint(void) { return VHR_SOURCE_FINGERPRINT; }

/* Diagnostics: the waves' lifetimes (s_memtime ticks) the last ray-tracing launch left for "raygen_cost_order" (index = tile pair * waves + wave). */
int vhr_debug_wave_lifetimes(vhr_context *ctx, uint32_t *out, uint32_t capacity, uint32_t *count) {
    if (!ctx || !out || !count) return VHR_ERROR_INVALID_ARGUMENT;
    VHR_TRY(ctx->sync_streams());
    const vhr_context::CostOrder &co = ctx->cost_order_raygen;
    // (the words the launch wrote: its blocks x the waves per block it ran with -- "raygen_waves_per_block" 3 runs as 2 -- and never more than the buffer holds)
    const uint32_t n = std::min<uint32_t>(capacity, co.cost_blocks[co.slot] ? std::min(co.cost_waves[co.slot], co.capacity) : 0u);
    *count = n;
    if (n && hipMemcpy(out, co.cost[co.slot], size_t(n) * 4, hipMemcpyDeviceToHost) != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "wave lifetimes: copy failed");
    return VHR_OK;
}

// What the last frame's rays cost, where: the wave lifetimes the queue kernels leave for "raygen_cost_order" -- the any-hit launch's and the mirror ray's --
// summed into a map of 8 x 8-pixel cells (a tile of fewer rows is charged to the cell of its first row).  The input of vhr_tile_plan_make_weighted.
int vhr_get_tile_cost_map(vhr_context *ctx, uint32_t *out, uint32_t cols, uint32_t rows) {
    if (!ctx || !out || cols == 0 || rows == 0) return VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    if (uint64_t(cols) * 8 < ctx->width || uint64_t(rows) * 8 < ctx->height) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "tile cost map: the map does not cover the image");
    VHR_TRY(ctx->sync_streams());
    std::fill(out, out + size_t(cols) * rows, 0u);
    std::vector<uint32_t> host;
    int found = 0;
    for (const vhr_context::CostOrder *co : { &ctx->cost_order_raygen, &ctx->cost_order_reflection }) {
        const uint32_t slot = co->slot;
        const vhr_context::CostOrder::Shape &sh = co->shape[slot];
        const uint32_t n = co->cost_blocks[slot] ? std::min(co->cost_waves[slot], co->capacity) : 0u;
        if (!n || !sh.tiles_x) continue;
        host.resize(n);
        if (hipMemcpy(host.data(), co->cost[slot], size_t(n) * 4, hipMemcpyDeviceToHost) != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, "tile cost map: copy failed");
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t block = i / sh.wv, wave = i % sh.wv;
            const uint32_t by = block / sh.blocks_x, bx = block % sh.blocks_x;
            const uint32_t x = sh.col_begin + (bx * sh.wv + wave) * sh.tile_w, y = sh.row_begin + by * sh.tile_h;
            if (x >= ctx->width || y >= ctx->height) continue;
            uint32_t &cell = out[size_t(y / 8) * cols + x / 8];
            cell = uint32_t(std::min<uint64_t>(0xffffffffull, uint64_t(cell) + host[i]));
        }
        ++found;
    }
    if (!found) return ctx->fail(VHR_ERROR_NOT_FOUND, "tile cost map: no queue-kernel launch has left its wave lifetimes (\"raygen_cost_order\" 0, or a launch below 2 048 workgroups with the option at 1)");
    return VHR_OK;
}

// VulkanContext::Resize (vulkan_context.cpp:118-120 -> InitSwapchain) as far as it concerns this library: a new display extent.  What depends on
// the extent goes -- the graph with its transient images and pass registry (RenderPath::Build destroys it first anyway, render_path.cpp:14-20), every image
// of the storage pool (the path's SVGF history: the reference's RegisterPath allocates its five again on Build) -- and what does not stays:
// geometry, acceleration structure, textures, options, trace parameters, timers.  The screen tile is the whole image again.
int vhr_resize(vhr_context *ctx, uint32_t width, uint32_t height) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (width == 0 || height == 0) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_resize: zero extent");
    if (ctx->recording || ctx->cur_pass) return ctx->fail(VHR_ERROR_GRAPH, "vhr_resize: called from inside a pass");
    if (!ctx->host_only) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (ctx->deferred_raygen) VHR_TRY(vhr::flush_deferred_raygen(ctx, nullptr));
        VHR_TRY(ctx->sync_streams());
    }
    VHR_TRY(vhr_graph_destroy_resources(ctx));
    for (Image &im : ctx->storage_images) {
        if (!im.used) continue;
        if (!ctx->host_only) {
            void *a = im.ptr, *b = im.alt;
            hipFree(a);
            if (b && b != a) hipFree(b);
        }
        im = Image{};
    }
    ctx->width = width;
    ctx->height = height;
    ctx->row_begin = 0; ctx->row_end = height;
    ctx->col_begin = 0; ctx->col_end = width;
    ctx->overlap = 0; ctx->halo = 0; ctx->halo_cols = 0;
    ctx->last_resource_idx = 0;
    ctx->error.clear();
    return VHR_OK;
}

int vhr_get_display_size(vhr_context *ctx, uint32_t *width, uint32_t *height) {
    if (!ctx || !width || !height) return VHR_ERROR_INVALID_ARGUMENT;
    *width = ctx->width;
    *height = ctx->height;
    return VHR_OK;
}

static int image_info(vhr_context *ctx, const Image &im, vhr_image_info *out) {
    out->device_ptr = im.ptr; out->width = im.width; out->height = im.height; out->format = im.format; out->bytes_per_pixel = im.bpp * im.samples;
    (void)ctx;
    return VHR_OK;
}

int vhr_get_transient_image(vhr_context *ctx, const char *name, vhr_image_info *out) {
    if (!ctx || !name || !out) return VHR_ERROR_INVALID_ARGUMENT;
    auto it = ctx->images.find(name);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, std::string("no transient image named '") + name + "'");
    // (the caller is about to use the pointer on the context's stream: the mirror ray's pending launch writes this image)
    if (!ctx->host_only && it->second.ptr == ctx->refl_writes) VHR_TRY(ctx->join_refl());
    return image_info(ctx, it->second, out);
}

int vhr_get_transient_image_samples(vhr_context *ctx, const char *name, uint32_t *samples) {
    if (!ctx || !name || !samples) return VHR_ERROR_INVALID_ARGUMENT;
    auto it = ctx->images.find(name);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, std::string("no transient image named '") + name + "'");
    *samples = it->second.samples;
    return VHR_OK;
}

int vhr_get_storage_image(vhr_context *ctx, int32_t id, vhr_image_info *out) {
    if (!ctx || !out || id < 0 || uint32_t(id) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[id].used)
        return ctx ? ctx->fail(VHR_ERROR_NOT_FOUND, "no such storage image") : VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->host_only) VHR_TRY(ctx->join_side());      // the caller is about to use the pointer on the context's stream
    return image_info(ctx, ctx->storage_images[id], out);
}

static int copy_image(vhr_context *ctx, const Image &im, void *host, uint64_t bytes, bool to_device, bool storage = false) {
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    if (!host || bytes != im.bytes()) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "image copy: byte count does not match the image (" + std::to_string(im.bytes()) + ")");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->recorded.empty()) VHR_TRY(vhr::flush_recorded(ctx));    // called from inside a compute pass
    if (ctx->deferred_raygen) VHR_TRY(vhr::flush_deferred_raygen(ctx, nullptr));
    if (to_device || im.ptr == ctx->refl_writes) VHR_TRY(ctx->join_refl());      // (an upload may rewrite what the mirror ray reads)
    if (storage || to_device) VHR_TRY(ctx->join_side());      // (a side-stream dispatch reads storage images and the pass's published copies)
    if (to_device) HIP_TRY(ctx, hipMemcpyAsync(im.ptr, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(ctx, hipMemcpyAsync(host, im.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VHR_TRY(ctx->sync_streams());
    return VHR_OK;
}

int vhr_upload_transient_image(vhr_context *ctx, const char *name, const void *host_data, uint64_t bytes) {
    if (!ctx || !name) return VHR_ERROR_INVALID_ARGUMENT;
    auto it = ctx->images.find(name);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, std::string("no transient image named '") + name + "'");
    return copy_image(ctx, it->second, const_cast<void *>(host_data), bytes, true);
}
int vhr_download_transient_image(vhr_context *ctx, const char *name, void *host_data, uint64_t bytes) {
    if (!ctx || !name) return VHR_ERROR_INVALID_ARGUMENT;
    auto it = ctx->images.find(name);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, std::string("no transient image named '") + name + "'");
    return copy_image(ctx, it->second, host_data, bytes, false);
}
int vhr_upload_storage_image(vhr_context *ctx, int32_t id, const void *host_data, uint64_t bytes) {
    if (!ctx || id < 0 || uint32_t(id) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[id].used)
        return ctx ? ctx->fail(VHR_ERROR_NOT_FOUND, "no such storage image") : VHR_ERROR_INVALID_ARGUMENT;
    return copy_image(ctx, ctx->storage_images[id], const_cast<void *>(host_data), bytes, true, true);
}
int vhr_download_storage_image(vhr_context *ctx, int32_t id, void *host_data, uint64_t bytes) {
    if (!ctx || id < 0 || uint32_t(id) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[id].used)
        return ctx ? ctx->fail(VHR_ERROR_NOT_FOUND, "no such storage image") : VHR_ERROR_INVALID_ARGUMENT;
    return copy_image(ctx, ctx->storage_images[id], host_data, bytes, false, true);
}

int vhr_standin_gbuffer(vhr_context *ctx, uint32_t resource_idx, const char *normals_image, const char *motion_image, const char *depth_image) {
    return vhr_standin_gbuffer_with_albedo(ctx, resource_idx, nullptr, normals_image, motion_image, depth_image);
}

int vhr_standin_composition(vhr_context *ctx, uint32_t resource_idx, const vhr_composition_desc *d) {
    if (!ctx || !d || resource_idx >= 3 || !d->albedo_image || !d->normals_image || !d->motion_image || !d->depth_image || !d->shadow_ao_image)
        return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: missing image name") : VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    auto find = [&](const char *n) -> Image * { auto it = ctx->images.find(n); return it == ctx->images.end() ? nullptr : &it->second; };
    Image *al = find(d->albedo_image), *no = find(d->normals_image), *mo = find(d->motion_image), *de = find(d->depth_image), *sa = find(d->shadow_ao_image);
    Image *re = d->reflections_image ? find(d->reflections_image) : nullptr;
    Image *ss = d->ssao_image ? find(d->ssao_image) : nullptr;
    Image *sm = d->shadow_map_image ? find(d->shadow_map_image) : nullptr;
    if (!al || !no || !mo || !de || !sa || (d->reflections_image && !re) || (d->ssao_image && !ss) || (d->shadow_map_image && !sm))
        return ctx->fail(VHR_ERROR_NOT_FOUND, "composition: unknown transient image");
    if ((d->reflection_mode == 0 || d->reflection_mode == 1) && !re) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "composition: reflection_mode 0 / 1 needs a reflections image");
    if (d->output_storage_image < 0 || uint32_t(d->output_storage_image) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[d->output_storage_image].used)
        return ctx->fail(VHR_ERROR_NOT_FOUND, "composition: output storage image is not allocated");
    VHR_TRY(ctx->refuse_if_stale("vhr_standin_composition"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_composition(ctx, ctx->per_frame[resource_idx], *d, *al, *no, *mo, *de, *sa, re, ss, sm, ctx->storage_images[d->output_storage_image]);
}

int vhr_standin_shadow_map(vhr_context *ctx, uint32_t resource_idx, const char *shadow_map_image) {
    if (!ctx || !shadow_map_image || resource_idx >= 3) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_shadow_map: bad argument") : VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    auto it = ctx->images.find(shadow_map_image);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_shadow_map: unknown transient image");
    VHR_TRY(ctx->refuse_if_stale("vhr_standin_shadow_map"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_standin_shadow_map(ctx, ctx->per_frame[resource_idx], it->second);
}

int vhr_standin_raytraced_composition(vhr_context *ctx, const char *raytraced_output_image, int32_t output_storage_image) {
    if (!ctx || !raytraced_output_image) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "raytraced composition: missing image name") : VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    auto it = ctx->images.find(raytraced_output_image);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, "raytraced composition: unknown transient image");
    if (it->second.format != VHR_FORMAT_B8G8R8A8_UNORM) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "raytraced composition: RaytracedOutput must be B8G8R8A8_UNORM (raytraced_render_path.cpp:15)");
    if (output_storage_image < 0 || uint32_t(output_storage_image) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[output_storage_image].used)
        return ctx->fail(VHR_ERROR_NOT_FOUND, "raytraced composition: output storage image is not allocated");
    VHR_TRY(ctx->refuse_if_stale("vhr_standin_raytraced_composition"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_raytraced_composition(ctx, it->second, ctx->storage_images[output_storage_image]);
}

int vhr_standin_gbuffer_with_albedo(vhr_context *ctx, uint32_t resource_idx, const char *albedo_image, const char *normals_image,
                                    const char *motion_image, const char *depth_image) {
    if (!ctx || !normals_image || !motion_image || !depth_image || resource_idx >= 3) return VHR_ERROR_INVALID_ARGUMENT;
    auto n = ctx->images.find(normals_image), m = ctx->images.find(motion_image), d = ctx->images.find(depth_image);
    if (n == ctx->images.end() || m == ctx->images.end() || d == ctx->images.end())
        return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_gbuffer: unknown transient image");
    if (n->second.format != VHR_FORMAT_R16G16B16A16_SFLOAT || m->second.format != VHR_FORMAT_R16G16B16A16_SFLOAT || d->second.format != VHR_FORMAT_D32_SFLOAT)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_gbuffer: formats must be RGBA16F, RGBA16F, D32F (hybrid_render_path.cpp:16-19)");
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    Image *albedo = nullptr;
    if (albedo_image) {
        auto al = ctx->images.find(albedo_image);
        if (al == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_gbuffer: unknown albedo image");
        albedo = &al->second;
    }
    VHR_TRY(ctx->refuse_if_stale("vhr_standin_gbuffer"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_standin_gbuffer(ctx, ctx->per_frame[resource_idx], n->second, m->second, d->second, albedo);
}

int vhr_standin_rayquery_forward(vhr_context *ctx, uint32_t resource_idx, const vhr_rayquery_forward_desc *d) {
    if (!ctx || !d || !d->depth_image || resource_idx >= 3)
        return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_rayquery_forward: bad argument") : VHR_ERROR_INVALID_ARGUMENT;
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    auto it = ctx->images.find(d->depth_image);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_rayquery_forward: unknown transient image");
    if (d->output_storage_image < 0 || uint32_t(d->output_storage_image) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[d->output_storage_image].used)
        return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_rayquery_forward: output storage image is not allocated");
    VHR_TRY(ctx->refuse_if_stale("vhr_standin_rayquery_forward"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_rayquery_forward(ctx, ctx->per_frame[resource_idx], ctx->storage_images[d->output_storage_image], it->second, d->primary_hits,
                                   d->positions, d->shadowed);
}

int vhr_standin_forward_raster(vhr_context *ctx, uint32_t resource_idx, const vhr_forward_raster_desc *d) {
    if (!ctx || !d || !d->depth_image || resource_idx >= 3)
        return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: bad argument") : VHR_ERROR_INVALID_ARGUMENT;
    auto it = ctx->images.find(d->depth_image);
    if (it == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_forward_raster: unknown transient image");
    Image *msaa = nullptr;
    if (it->second.samples == kMsaaSamples) {
        if (!d->msaa_image) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: \"Depth\" has 8 samples, so msaa_image is required");
        auto m = ctx->images.find(d->msaa_image);
        if (m == ctx->images.end()) return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_forward_raster: unknown msaa image");
        msaa = &m->second;
    } else if (d->msaa_image) {
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "standin_forward_raster: \"Depth\" has 1 sample, so msaa_image must be NULL");
    }
    if (ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "host-only context: no device work");
    if (d->output_storage_image < 0 || uint32_t(d->output_storage_image) >= vhr_context::kMaxGlobalResources || !ctx->storage_images[d->output_storage_image].used)
        return ctx->fail(VHR_ERROR_NOT_FOUND, "standin_forward_raster: output storage image is not allocated");
    VHR_TRY(ctx->refuse_if_stale("vhr_standin_forward_raster"));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_forward_raster(ctx, ctx->per_frame[resource_idx], ctx->storage_images[d->output_storage_image], it->second, msaa, d->sample_hits,
                                 d->fragments);
}

}  // extern "C"
