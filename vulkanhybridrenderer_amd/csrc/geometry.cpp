// Geometry half of the C ABI (include/vhr_amd.h): the scene arrays and the acceleration structure's lifecycle -- build (vhr_update_geometry),
// refit and partial refit, rebuild in place -- with what hangs on the tree: primitive masks, facing flips, the previous records of
// "object_motion_vectors", the tree's statistics, SAH cost and fingerprints.
// Reference: src/rendering_backend/resource_manager.{h,cpp} (UpdateGeometry, UpdateBLAS / UpdateTLAS).
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "vhr_internal.hpp"
#include "ray_facing.hpp"     // facing_flip

using namespace vhr;

// the primitives' ray cull masks on the device, for a launch that filters (vhr_set_primitive_masks below)
int vhr::ensure_device_prim_masks(vhr_context *ctx) {
    if (ctx->d_prim_masks || ctx->primitive_count == 0) return VHR_OK;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_prim_masks), ctx->primitive_count));
    if (ctx->h_prim_masks.empty()) HIP_TRY(ctx, hipMemsetAsync(ctx->d_prim_masks, 0xFF, ctx->primitive_count, ctx->stream));
    else HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prim_masks, ctx->h_prim_masks.data(), ctx->primitive_count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (once per scene; launches on the context's other streams may read it next)
    return VHR_OK;
}

// the primitives' facing-flip bytes on the device, for a launch of the ray query's face instantiation (h_prim_flips: one byte per primitive, kept
// by vhr_update_geometry and vhr_update_primitive_transforms)
int vhr::ensure_device_prim_flips(vhr_context *ctx) {
    if (ctx->d_prim_flips || ctx->primitive_count == 0) return VHR_OK;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_prim_flips), ctx->primitive_count));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prim_flips, ctx->h_prim_flips.data(), ctx->primitive_count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (once per scene; launches on the context's other streams may read it next)
    return VHR_OK;
}

vhr::DeviceScene vhr_context::device_scene() const {
    DeviceScene s;
    s.nodes = d_nodes;
    s.nodes16 = d_nodes16;
    s.nodes_ch = d_nodes_ch;
    s.nodes48 = d_nodes48;
    s.centre[0] = bvh_centre[0]; s.centre[1] = bvh_centre[1]; s.centre[2] = bvh_centre[2];
    s.pad0 = 0.0f;
    s.tris = d_tris;
    s.vertices = d_vertices;
    s.indices = d_indices;
    s.primitives = d_primitives;
    s.normal_matrices = d_normal_matrices;
    s.textures = d_textures;
    s.node_count = node_count;
    s.tri_count = tri_count;
    s.primitive_count = primitive_count;
    s.texture_count = uint32_t(textures.size());
    for (int i = 0; i < 9; ++i) s.frame[i] = bvh_frame[i];
    s.frame_on = bvh_frame_on ? 1u : 0u;
    return s;
}

// "object_motion_vectors": the previous records and their bookkeeping
static void free_motion(vhr_context *ctx) {
    if (!ctx->host_only) { hipFree(ctx->d_prev_tris); hipFree(ctx->d_prev_saved); }
    ctx->d_prev_tris = nullptr; ctx->d_prev_saved = nullptr;
    ctx->h_bvh.prev_tris.clear(); ctx->h_bvh.prev_saved.clear();
    ctx->h_bvh.prev_differing = 0;
    ctx->motion_epoch = 1;
    ctx->motion_differing = ctx->motion_refit_differing = 0;
}
// previous = current for the tree the context holds (none yet: nothing to keep); the caller has waited for the context's streams
int vhr::reset_motion(vhr_context *ctx) {
    free_motion(ctx);
    if (!ctx->object_motion_vectors || !ctx->tri_count) return VHR_OK;
    if (ctx->host_only) {
        ctx->h_bvh.prev_tris = ctx->h_bvh.tris;
        ctx->h_bvh.prev_saved.assign(ctx->h_bvh.tris.size(), 0u);
        return VHR_OK;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&ctx->d_prev_tris), sizeof(BvhTri) * ctx->tri_count);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&ctx->d_prev_saved), sizeof(uint32_t) * ctx->tri_count);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_prev_tris, ctx->d_tris, sizeof(BvhTri) * ctx->tri_count, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemset(ctx->d_prev_saved, 0, sizeof(uint32_t) * ctx->tri_count);
    if (e != hipSuccess) {
        free_motion(ctx);
        return ctx->fail(VHR_ERROR_DEVICE, std::string("object_motion_vectors: allocating the previous records: ") + hipGetErrorString(e));
    }
    return VHR_OK;
}

void vhr::free_tree(vhr_context *ctx) {
    hipFree(ctx->d_nodes); hipFree(ctx->d_nodes16); hipFree(ctx->d_nodes_ch); hipFree(ctx->d_nodes48); hipFree(ctx->d_tris);
    ctx->d_nodes = nullptr; ctx->d_nodes16 = nullptr; ctx->d_nodes_ch = nullptr; ctx->d_nodes48 = nullptr; ctx->d_tris = nullptr;
    ctx->node_count = ctx->tri_count = 0;
}

void vhr::free_scene(vhr_context *ctx) {
    vhr::free_refit_plan(ctx);
    free_motion(ctx);
    hipFree(ctx->d_vertices); hipFree(ctx->d_indices); hipFree(ctx->d_primitives); hipFree(ctx->d_normal_matrices);
    free_tree(ctx);
    hipFree(ctx->d_prim_masks); ctx->d_prim_masks = nullptr;
    hipFree(ctx->d_prim_flips); ctx->d_prim_flips = nullptr;
    ctx->d_vertices = nullptr; ctx->d_indices = nullptr; ctx->d_primitives = nullptr; ctx->d_normal_matrices = nullptr;
    ctx->vertex_count = ctx->index_count = ctx->primitive_count = 0;
}

// a build replaces whatever updates were pending and everything a refit had prepared for the old tree
static void discard_refit_state(vhr_context *ctx) {
    ctx->refit_pending = ctx->sah_cost_built_valid = false;
    for (uint64_t &w : ctx->refit_stats) w = 0;
    for (uint64_t &w : ctx->partial_stats) w = 0;
    ctx->refit_dirty = RefitDirty{};
}

// the first vertex of `vertices` with a non-finite position, or `count` if every position is finite (a NaN / Inf coordinate would reach the
// builder's bin index -- float -> int of a NaN is undefined -- and its comparators)
static uint32_t first_non_finite_position(const vhr_vertex *vertices, uint32_t count) {
    for (uint32_t v = 0; v < count; ++v)
        if (!std::isfinite(vertices[v].pos[0]) || !std::isfinite(vertices[v].pos[1]) || !std::isfinite(vertices[v].pos[2])) return v;
    return count;
}

// what the entry points that need a tree, or take a range of its primitives, say when there is none, or when the range leaves them
static int no_geometry(vhr_context *ctx, const std::string &who) { return ctx->fail(VHR_ERROR_GRAPH, who + ": no geometry yet (vhr_update_geometry first)"); }
static std::string range_exceeds(const std::string &who, uint32_t first, uint32_t count, const char *what, uint32_t size) {
    return who + ": range [" + std::to_string(first) + ", +" + std::to_string(count) + ") exceeds " + what + " (" + std::to_string(size) + ")";
}

// inverseTranspose(mat3(transform)) -- hybrid_render_path.cpp:44 (the stand-in G-buffer and vhr_resolve_hits)
void vhr::normal_matrix3(const float *m, float out[9]) {
    double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
    double c00 = e * i - f * h, c01 = -(d * i - f * g), c02 = d * h - e * g;
    double c10 = -(b * i - c * h), c11 = a * i - c * g, c12 = -(a * h - b * g);
    double c20 = b * f - c * e, c21 = -(a * f - c * d), c22 = a * e - b * d;
    double det = a * c00 + b * c01 + c * c02;
    double id = det != 0.0 ? 1.0 / det : 0.0;
    out[0] = float(c00 * id); out[3] = float(c01 * id); out[6] = float(c02 * id);
    out[1] = float(c10 * id); out[4] = float(c11 * id); out[7] = float(c12 * id);
    out[2] = float(c20 * id); out[5] = float(c21 * id); out[8] = float(c22 * id);
}

extern "C" {

// the device-built tree on the host (for "bvh_host_checks" and the fingerprint)
static int fetch_device_tree(vhr_context *ctx, HostBvh &bvh) {
    bvh.nodes.resize(ctx->node_count); bvh.nodes_ch.resize(ctx->node_count); bvh.nodes48.resize(ctx->node_count); bvh.nodes16.resize(ctx->node_count);
    bvh.tris.resize(ctx->tri_count);
    HIP_TRY(ctx, hipMemcpy(bvh.nodes.data(), ctx->d_nodes, sizeof(BvhNode) * ctx->node_count, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(bvh.nodes_ch.data(), ctx->d_nodes_ch, sizeof(BvhNodeCH) * ctx->node_count, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(bvh.nodes48.data(), ctx->d_nodes48, sizeof(BvhNode48) * ctx->node_count, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(bvh.nodes16.data(), ctx->d_nodes16, sizeof(BvhNode16) * ctx->node_count, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(bvh.tris.data(), ctx->d_tris, sizeof(BvhTri) * ctx->tri_count, hipMemcpyDeviceToHost));
    for (int a = 0; a < 3; ++a) bvh.centre[a] = ctx->bvh_centre[a];
    bvh.nodes16_valid = nodes16_in_range(bvh);
    bvh.max_depth = ctx->bvh_depth;
    return VHR_OK;
}

static hipError_t upload_array(void **dst, const void *src, size_t bytes) {
    *dst = nullptr;
    if (bytes == 0) return hipSuccess;
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
}

// The part of a build vhr_update_geometry and vhr_rebuild_geometry share: which builder, the device builder's fallbacks, the self-checks and
// fingerprints, and the tree where the context keeps it (uploaded on a device context, in h_bvh on a host-only one).  The caller has put the
// scene arrays where the builders read them (a device context: d_vertices / d_indices / d_primitives), set ctx->prim_tri_prefix, waited for the
// context's streams and freed the old tree.  `scene`: the arrays in host memory for the host builder; all NULL on a device context that keeps no
// host copy (vhr_rebuild_geometry): they are then fetched from the device if, and only if, the host builder runs (*fetched = true).
// `who` names the entry point in messages; upload_ms grows by the transfers made here.
struct HostSceneArrays { const vhr_vertex *vertices; const uint32_t *indices; const vhr_primitive *primitives; };
static int build_and_install_tree(vhr_context *ctx, const char *who, HostSceneArrays scene, uint32_t primitive_count, uint64_t total_triangles, double &upload_ms, bool *fetched) {
    HostBvh bvh;
    bool device_built = false;
    ctx->bvh_builder_used = 0;
    // ---- "bvh_builder" 1: the tree built on the device (csrc/kernels_bvh.hip), where the reference builds its BLAS / TLAS ----
    if (ctx->bvh_builder >= 1 && !ctx->host_only && total_triangles >= 2ull * uint64_t(ctx->bvh_leaf_tris)) {
        // first flat triangle of every primitive
        // (a primitive without triangles shares its prefix with the next one: the search below picks the LAST primitive whose prefix is
        // <= t, which is the one that owns triangle t, because an empty primitive's successor starts at the same value)
        const std::vector<uint32_t> prefix(ctx->prim_tri_prefix.begin(), ctx->prim_tri_prefix.begin() + primitive_count);
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = device_build_bvh(ctx, prefix, uint32_t(total_triangles), ctx->bvh_leaf_tris, ctx->bvh_presplit, ctx->bvh_frame_mode);
        const auto t1 = std::chrono::steady_clock::now();
        if (rc == VHR_OK) {
            device_built = true;
            ctx->bvh_builder_used = 1;
            ctx->bvh_build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
            // its self-checks ran on the device (k0_check_forms_kernel); "bvh_host_checks" 1 fetches the tree and repeats them with the host's
            // code (tests hold the two equal).  The fingerprint is computed when somebody asks for it (vhr_get_bvh_fingerprint).
            ctx->bvh_fingerprint_valid = false;
            if (ctx->bvh_host_checks) VHR_TRY(fetch_device_tree(ctx, bvh));
        } else {
            free_tree(ctx);
            if (rc != VHR_ERROR_OUT_OF_SLOTS) return rc;          // (out of slots: deeper than the walkers' stacks, or a one-leaf scene -> the host builder)
        }
    }
    std::vector<vhr_vertex> fetched_vertices;
    std::vector<uint32_t> fetched_indices;
    std::vector<vhr_primitive> fetched_primitives;
    if (!device_built && !ctx->host_only && !scene.vertices && !scene.indices && !scene.primitives) {      // no host copy: the host builder's input comes back from the device
        const auto t0 = std::chrono::steady_clock::now();
        fetched_vertices.resize(ctx->vertex_count); fetched_indices.resize(ctx->index_count); fetched_primitives.resize(ctx->primitive_count);
        if (ctx->vertex_count) HIP_TRY(ctx, hipMemcpy(fetched_vertices.data(), ctx->d_vertices, sizeof(vhr_vertex) * ctx->vertex_count, hipMemcpyDeviceToHost));
        if (ctx->index_count) HIP_TRY(ctx, hipMemcpy(fetched_indices.data(), ctx->d_indices, sizeof(uint32_t) * ctx->index_count, hipMemcpyDeviceToHost));
        if (ctx->primitive_count) HIP_TRY(ctx, hipMemcpy(fetched_primitives.data(), ctx->d_primitives, sizeof(vhr_primitive) * ctx->primitive_count, hipMemcpyDeviceToHost));
        scene = HostSceneArrays{ fetched_vertices.data(), fetched_indices.data(), fetched_primitives.data() };
        upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (fetched) *fetched = true;
    }
    const auto t_build0 = std::chrono::steady_clock::now();
    if (!device_built) {
        build_bvh(scene.vertices, scene.indices, scene.primitives, primitive_count, bvh, ctx->bvh_leaf_tris, ctx->bvh_build_threads, ctx->bvh_presplit, ctx->bvh_frame_mode);          // UpdateBLAS + UpdateTLAS
        ctx->bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build0).count();
        ctx->bvh_presplit_level = bvh.presplit_level;
        for (int i = 0; i < 9; ++i) ctx->bvh_frame[i] = bvh.frame[i];
        ctx->bvh_frame_on = bvh.frame_on;
        ctx->bvh_frame_magnitude = bvh.frame_magnitude;
    }
    if (uint64_t(device_built ? ctx->node_count : bvh.nodes48.size()) * sizeof(BvhNode48) >= (1ull << 31))     // an inner link of the 48-byte nodes is a non-negative 32-bit byte offset
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(who) + ": more than 44 million BVH nodes");
    const auto t_build1 = std::chrono::steady_clock::now();       // K0 proper ends here; the self-checks below are timed apart
    if (!device_built || ctx->bvh_host_checks) {
        check_node_forms(bvh, ctx->bvh_form_checks, ctx->bvh_build_threads);
        ctx->nodes16_valid = bvh.nodes16_valid && ctx->bvh_form_checks[3] == 0;      // else the walkers stay on the 48-byte nodes
        ctx->bvh_fingerprint = bvh_fingerprint(bvh);
        ctx->bvh_tree_fingerprint = bvh_tree_fingerprint(bvh);
        ctx->bvh_fingerprint_valid = true;
    }
    ctx->bvh_check_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build1).count();
    if (ctx->host_only) {
        ctx->node_count = uint32_t(bvh.nodes.size());
        ctx->tri_count = uint32_t(bvh.tris.size());
        ctx->bvh_depth = bvh.max_depth;
        ctx->geometry_upload_ms = 0.0;
        ctx->h_bvh = std::move(bvh);
        return VHR_OK;
    }
    if (!device_built) {
        const auto t_upload0 = std::chrono::steady_clock::now();
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_nodes), bvh.nodes.data(), sizeof(BvhNode) * bvh.nodes.size()));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_nodes16), bvh.nodes16.data(), sizeof(BvhNode16) * bvh.nodes16.size()));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_nodes_ch), bvh.nodes_ch.data(), sizeof(BvhNodeCH) * bvh.nodes_ch.size()));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_nodes48), bvh.nodes48.data(), sizeof(BvhNode48) * bvh.nodes48.size()));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_tris), bvh.tris.data(), sizeof(BvhTri) * bvh.tris.size()));
        for (int a = 0; a < 3; ++a) ctx->bvh_centre[a] = bvh.centre[a];
        ctx->node_count = uint32_t(bvh.nodes.size());
        ctx->tri_count = uint32_t(bvh.tris.size());
        ctx->bvh_depth = bvh.max_depth;
        upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_upload0).count();
    }
    return VHR_OK;
}

int vhr_update_geometry(vhr_context *ctx, const vhr_vertex *vertices, uint32_t vertex_count, const uint32_t *indices,
                        uint32_t index_count, const vhr_primitive *primitives, uint32_t primitive_count) {
    if (!ctx || (!vertices && vertex_count) || (!indices && index_count) || (!primitives && primitive_count))
        return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: null array") : VHR_ERROR_INVALID_ARGUMENT;
    // (a host-only context validates, builds the tree and checks its node forms, and stops before the upload: the builder is host code,
    // and the CPU tests exercise it this way)
    // Validate every offset the kernels will dereference (an out-of-range index would fault the GPU).
    uint64_t total_triangles = 0;
    for (uint32_t p = 0; p < primitive_count; ++p) {
        const vhr_primitive &pr = primitives[p];
        if (uint64_t(pr.index_offset) + pr.index_count > index_count)
            return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: primitive " + std::to_string(p) + " index range exceeds the index buffer");
        for (uint32_t k = 0; k < pr.index_count; ++k)
            if (uint64_t(pr.vertex_offset) + indices[pr.index_offset + k] >= vertex_count)
                return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: primitive " + std::to_string(p) + " references a vertex beyond the vertex buffer");
        const int32_t tex[2] = { pr.material.base_color_texture, pr.material.metallic_roughness_texture };
        for (int32_t t : tex)
            if (t < -1) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: negative texture index other than -1");
        for (int k = 0; k < 16; ++k)            // (like a non-finite position, below)
            if (!std::isfinite(pr.transform[k])) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: primitive " + std::to_string(p) + " has a non-finite transform");
        total_triangles += pr.index_count / 3;
    }
    if (const uint32_t v = first_non_finite_position(vertices, vertex_count); v < vertex_count)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: vertex " + std::to_string(v) + " has a non-finite position");
    if (total_triangles >= (1ull << 29))            // a leaf link packs (first triangle << 2 | count - 1) into 31 bits
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "UpdateGeometry: 2^29 triangles or more");
    // "alpha_test_rays" / VHR_RAY_QUERY_ALPHA_TEST: can gbuf.frag:20-32 discard a fragment of any primitive?  (A texture's alpha bytes are not
    // scanned: a base-colour texture counts as able to.)
    ctx->scene_can_discard = false;
    for (uint32_t p = 0; p < primitive_count; ++p) {
        const vhr_material &m = primitives[p].material;
        if (m.alpha_mask == 1 || m.base_color_texture != -1 || m.base_color[3] == 0.0f) ctx->scene_can_discard = true;
    }
    // ... and every primitive's ray cull mask is 0xFF again (the device array goes with the scene's, below)
    ctx->h_prim_masks.clear();
    ctx->mask_present[0] = ctx->mask_present[1] = ctx->mask_present[2] = 0; ctx->mask_present[3] = 1ull << 63;
    ctx->masks_not_ff = 0;
    discard_refit_state(ctx);
    for (uint64_t &w : ctx->rebuild_stats) w = 0;
    ctx->prim_tri_prefix.assign(size_t(primitive_count) + 1u, 0u);
    for (uint32_t p = 0; p < primitive_count; ++p) ctx->prim_tri_prefix[p + 1u] = ctx->prim_tri_prefix[p] + primitives[p].index_count / 3;
    if (!ctx->host_only) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
        free_scene(ctx);
    }

    double upload_ms = 0.0;
    if (!ctx->host_only) {                 // the scene arrays first: the device builder reads them where the walkers will
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<float> nm(size_t(primitive_count) * 9);
        for (uint32_t p = 0; p < primitive_count; ++p) normal_matrix3(primitives[p].transform, &nm[size_t(p) * 9]);
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_vertices), vertices, sizeof(vhr_vertex) * vertex_count));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_indices), indices, sizeof(uint32_t) * index_count));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_primitives), primitives, sizeof(vhr_primitive) * primitive_count));
        HIP_TRY(ctx, upload_array(reinterpret_cast<void **>(&ctx->d_normal_matrices), nm.data(), sizeof(float) * nm.size()));
        upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    {   // builder choice, fallback, self-checks and the tree's upload: shared with vhr_rebuild_geometry
        const HostSceneArrays scene{ vertices, indices, primitives };
        VHR_TRY(build_and_install_tree(ctx, "UpdateGeometry", scene, primitive_count, total_triangles, upload_ms, nullptr));
    }
    // every primitive's facing flip by its transform (vhr_ray_query_faces; the device copy went with the scene's arrays and is made again on demand)
    ctx->h_prim_flips.resize(primitive_count);
    for (uint32_t p = 0; p < primitive_count; ++p) ctx->h_prim_flips[p] = facing_flip(primitives[p].transform);
    if (ctx->host_only) {
        // ... and keeps the arrays and the tree: the refit's host twin works on them (vhr_update_vertices, vhr_refit_geometry)
        ctx->h_vertices.assign(vertices, vertices + vertex_count);
        ctx->h_indices.assign(indices, indices + index_count);
        ctx->h_primitives.assign(primitives, primitives + primitive_count);
    } else {
        ctx->geometry_upload_ms = upload_ms;
    }
    ctx->vertex_count = vertex_count;
    ctx->index_count = index_count;
    ctx->primitive_count = primitive_count;
    return reset_motion(ctx);               // "object_motion_vectors": previous = current for the new tree
}

int vhr_get_bvh_builder(vhr_context *ctx, int32_t *used) {
    if (!ctx || !used) return VHR_ERROR_INVALID_ARGUMENT;
    *used = ctx->bvh_builder_used;
    return VHR_OK;
}

int vhr_get_bvh_frame(vhr_context *ctx, float out[9]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < 9; ++i) out[i] = ctx->bvh_frame[i];
    return VHR_OK;
}

int vhr_get_bvh_presplit_level(vhr_context *ctx, int32_t *level) {
    if (!ctx || !level) return VHR_ERROR_INVALID_ARGUMENT;
    *level = ctx->bvh_presplit_level;
    return VHR_OK;
}

int vhr_get_build_times(vhr_context *ctx, double out[2]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = ctx->bvh_build_ms;
    out[1] = ctx->geometry_upload_ms;
    return VHR_OK;
}

// ---- refit: vertices or primitive transforms change, the tree keeps its topology (VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR) ----
static int refit_state_checks(vhr_context *ctx, const char *who) {
    if (!ctx->has_geometry()) return no_geometry(ctx, who);
    if (ctx->bvh_presplit_level >= 0)
        return ctx->fail(VHR_ERROR_UNSUPPORTED, std::string(who) + ": the tree was built with \"bvh_presplit\" (its references are clipped boxes, which a refit cannot keep): rebuild with vhr_update_geometry");
    return VHR_OK;
}
// what is about to be overwritten may still be read by frames in flight: the first update after a build or refit waits for them
static int begin_update(vhr_context *ctx) {
    if (ctx->host_only) return VHR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->refit_pending) VHR_TRY(ctx->sync_streams());
    return VHR_OK;
}

int vhr_update_vertices(vhr_context *ctx, uint32_t first_vertex, uint32_t vertex_count, const vhr_vertex *vertices, uint32_t flags) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (flags & ~uint32_t(VHR_UPDATE_DEVICE_MEMORY)) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_update_vertices: unknown flag bits " + std::to_string(flags));
    if (vertex_count > 0 && !vertices) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_update_vertices: vertices must not be NULL when vertex_count > 0");
    if ((flags & VHR_UPDATE_DEVICE_MEMORY) && ctx->host_only) return ctx->fail(VHR_ERROR_NO_DEVICE, "vhr_update_vertices: host-only context: no device memory");
    VHR_TRY(refit_state_checks(ctx, "vhr_update_vertices"));
    if (uint64_t(first_vertex) + vertex_count > ctx->vertex_count)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, range_exceeds("vhr_update_vertices", first_vertex, vertex_count, "the vertex buffer", ctx->vertex_count));
    if (vertex_count == 0) return VHR_OK;
    if (!(flags & VHR_UPDATE_DEVICE_MEMORY))
        if (const uint32_t v = first_non_finite_position(vertices, vertex_count); v < vertex_count)
            return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_update_vertices: vertex " + std::to_string(first_vertex + v) + " has a non-finite position");
    VHR_TRY(begin_update(ctx));
    if (ctx->host_only) {
        std::memcpy(ctx->h_vertices.data() + first_vertex, vertices, sizeof(vhr_vertex) * vertex_count);
    } else if (flags & VHR_UPDATE_DEVICE_MEMORY) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vertices + first_vertex, vertices, sizeof(vhr_vertex) * vertex_count, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vertices + first_vertex, vertices, sizeof(vhr_vertex) * vertex_count, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the caller's array is free when the call returns
    }
    ctx->refit_pending = true;
    ctx->refit_dirty.vertices.add(first_vertex, vertex_count);
    return VHR_OK;
}

int vhr_update_primitive_transforms(vhr_context *ctx, uint32_t first_primitive, uint32_t count, const float *transforms) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (count > 0 && !transforms) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_update_primitive_transforms: transforms must not be NULL when count > 0");
    VHR_TRY(refit_state_checks(ctx, "vhr_update_primitive_transforms"));
    if (uint64_t(first_primitive) + count > ctx->primitive_count)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, range_exceeds("vhr_update_primitive_transforms", first_primitive, count, "the primitives", ctx->primitive_count));
    if (count == 0) return VHR_OK;
    for (uint64_t k = 0; k < uint64_t(count) * 16u; ++k)
        if (!std::isfinite(transforms[k])) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_update_primitive_transforms: primitive " + std::to_string(first_primitive + k / 16u) + " has a non-finite transform");
    VHR_TRY(begin_update(ctx));
    if (ctx->host_only) {
        for (uint32_t p = 0; p < count; ++p) std::memcpy(ctx->h_primitives[first_primitive + p].transform, transforms + size_t(p) * 16, sizeof(float) * 16);
    } else {
        // the primitives' other fields stay what the device holds: the range is fetched, patched and written back, with its normal matrices
        std::vector<vhr_primitive> prims(count);
        std::vector<float> nm(size_t(count) * 9);
        HIP_TRY(ctx, hipMemcpyAsync(prims.data(), ctx->d_primitives + first_primitive, sizeof(vhr_primitive) * count, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t p = 0; p < count; ++p) {
            std::memcpy(prims[p].transform, transforms + size_t(p) * 16, sizeof(float) * 16);
            normal_matrix3(prims[p].transform, &nm[size_t(p) * 9]);
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_primitives + first_primitive, prims.data(), sizeof(vhr_primitive) * count, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_normal_matrices + size_t(first_primitive) * 9, nm.data(), sizeof(float) * nm.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the facing flips follow the new transforms (no query runs while the update is pending; the refit brings the records the bytes belong to)
    for (uint32_t p = 0; p < count; ++p) ctx->h_prim_flips[first_primitive + p] = facing_flip(transforms + size_t(p) * 16);
    if (ctx->d_prim_flips) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prim_flips + first_primitive, ctx->h_prim_flips.data() + first_primitive, count, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->refit_pending = true;
    ctx->refit_dirty.primitives.add(first_primitive, count);
    return VHR_OK;
}

// ---- ray cull masks: one byte per primitive, tested against the ray's mask at every candidate (the tree does not depend on them) ----
static int mask_state_checks(vhr_context *ctx, const char *who, uint32_t first_primitive, uint32_t count, bool writes) {
    if (!ctx->has_geometry()) return no_geometry(ctx, who);
    if (writes && (ctx->recording || ctx->cur_pass || ctx->in_execute)) return ctx->fail(VHR_ERROR_GRAPH, std::string(who) + ": called from inside a pass");
    if (uint64_t(first_primitive) + count > ctx->primitive_count)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, range_exceeds(who, first_primitive, count, "the primitives", ctx->primitive_count));
    return VHR_OK;
}

int vhr_set_primitive_masks(vhr_context *ctx, uint32_t first_primitive, uint32_t count, const uint8_t *masks) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (count > 0 && !masks) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_set_primitive_masks: masks must not be NULL when count > 0");
    VHR_TRY(mask_state_checks(ctx, "vhr_set_primitive_masks", first_primitive, count, true));
    if (count == 0) return VHR_OK;
    if (ctx->h_prim_masks.empty()) {
        bool all_ff = true;
        for (uint32_t p = 0; p < count; ++p) all_ff = all_ff && masks[p] == 0xFFu;
        if (all_ff) return VHR_OK;                             // nothing to store: every mask is 0xFF already
        ctx->h_prim_masks.assign(ctx->primitive_count, uint8_t(0xFF));
    }
    std::memcpy(ctx->h_prim_masks.data() + first_primitive, masks, count);
    for (uint64_t &w : ctx->mask_present) w = 0;
    ctx->masks_not_ff = 0;
    for (const uint8_t v : ctx->h_prim_masks) {
        ctx->mask_present[v >> 6] |= 1ull << (v & 63u);
        if (v != 0xFFu) ++ctx->masks_not_ff;
    }
    if (ctx->host_only) return VHR_OK;
    // frames and queries in flight read the array that is about to be overwritten: wait for them (not an update in the refit sense: nothing is pending)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    VHR_TRY(ctx->sync_streams());
    if (!ctx->d_prim_masks) return vhr::ensure_device_prim_masks(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prim_masks + first_primitive, masks, count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the caller's array is free when the call returns
    return VHR_OK;
}

int vhr_get_primitive_masks(vhr_context *ctx, uint32_t first_primitive, uint32_t count, uint8_t *out) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (count > 0 && !out) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_get_primitive_masks: out must not be NULL when count > 0");
    VHR_TRY(mask_state_checks(ctx, "vhr_get_primitive_masks", first_primitive, count, false));
    if (count == 0) return VHR_OK;
    if (ctx->h_prim_masks.empty()) std::memset(out, 0xFF, count);
    else std::memcpy(out, ctx->h_prim_masks.data() + first_primitive, count);
    return VHR_OK;
}

int vhr_get_ray_mask_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = ctx->masks_not_ff; out[1] = ctx->mask_launches; out[2] = ctx->rq_mask_ran; out[3] = 0;
    return VHR_OK;
}

// the share of the scene the pending ranges touch, from what the host knows: the triangles of the primitive ranges, and the vertex ranges' share of
// the vertices taken as their share of the triangles (an estimate; it only chooses between two routes to the same arrays).  The two shares
// are added, so a range reported both ways counts twice; clamped to 1
static double dirty_share(const vhr_context *ctx) {
    uint64_t tris = 0;
    const DirtyRanges &pr = ctx->refit_dirty.primitives;
    for (uint32_t i = 0; i < pr.count; ++i) tris += ctx->prim_tri_prefix[pr.hi[i]] - ctx->prim_tri_prefix[pr.lo[i]];
    const double total = double(ctx->prim_tri_prefix.empty() ? 0u : ctx->prim_tri_prefix.back());
    return std::min(1.0, (total > 0.0 ? double(tris) / total : 1.0) + (ctx->vertex_count ? double(ctx->refit_dirty.vertices.covered()) / double(ctx->vertex_count) : 1.0));
}

// vhr_refit_geometry (partial == false) and vhr_refit_geometry_partial: the same preconditions, refusals and synchronisation
static int refit_geometry(vhr_context *ctx, const char *who, bool partial, bool force) {
    VHR_TRY(refit_state_checks(ctx, who));
    if (ctx->recording || ctx->cur_pass) return ctx->fail(VHR_ERROR_GRAPH, std::string(who) + ": called from inside a pass");
    if (!ctx->refit_pending) {                           // nothing changed: nothing is launched ...
        if (!ctx->motion_valid() || ctx->motion_differing == 0) return VHR_OK;
        // ... but "object_motion_vectors" counts the call as a refit: what the last one moved has stopped (one settle pass)
        if (ctx->host_only) {
            HostBvh &b = ctx->h_bvh;
            for (size_t i = 0; i < b.tris.size(); ++i) if (b.prev_saved[i] == ctx->motion_epoch) b.prev_tris[i] = b.tris[i];
        } else {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            VHR_TRY(ctx->sync_streams());
            VHR_TRY(device_motion_settle(ctx));
        }
        ++ctx->motion_epoch;
        ctx->motion_differing = 0;
        return VHR_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t ran_as = kRanDirty;
    const bool asked_partial = partial;
    // the first refit since the build has no per-node boxes to start from: whole tree, whatever the flags and the share (this reason is the one reported)
    if (partial && !(ctx->host_only ? !ctx->h_bvh.self_box.empty() : device_refit_boxes_valid(ctx))) { partial = false; ran_as = kRanWholeFirst; }
    if (partial && !force && dirty_share(ctx) > kPartialRefitMaxShare) { partial = false; ran_as = kRanWholeThreshold; }
    if (ctx->host_only) {
        if (!ctx->sah_cost_built_valid) { ctx->sah_cost_built = bvh_sah_cost(ctx->h_bvh); ctx->sah_cost_built_valid = true; }
        uint64_t counts[3], dirty_counts[4] = { ctx->h_bvh.tris.size(), ctx->h_bvh.nodes.size(), ctx->h_bvh.nodes.size(), 0 };
        const uint32_t motion_epoch = ctx->motion_valid() ? ctx->motion_epoch + 1u : 0u;
        const bool walked = partial ? refit_bvh_partial(ctx->h_vertices.data(), ctx->h_indices.data(), ctx->h_primitives.data(), ctx->primitive_count, ctx->h_bvh,
                                                        ctx->refit_dirty, counts, dirty_counts, ctx->bvh_build_threads, motion_epoch)
                                    : refit_bvh(ctx->h_vertices.data(), ctx->h_indices.data(), ctx->h_primitives.data(), ctx->primitive_count, ctx->h_bvh, counts, ctx->bvh_build_threads,
                                                motion_epoch);
        if (!walked)
            return ctx->fail(VHR_ERROR_GRAPH, std::string(who) + (partial ? ": the tree or its per-node boxes are not what a dirty pass can walk (a record outside its primitive's triangles)"
                                                                          : ": the tree's nodes are not numbered parents before children"));
        check_node_forms(ctx->h_bvh, ctx->bvh_form_checks, ctx->bvh_build_threads);
        ctx->nodes16_valid = ctx->h_bvh.nodes16_valid && ctx->bvh_form_checks[3] == 0;
        ctx->bvh_fingerprint = bvh_fingerprint(ctx->h_bvh);
        ctx->bvh_tree_fingerprint = bvh_tree_fingerprint(ctx->h_bvh);
        ctx->bvh_fingerprint_valid = true;
        ctx->refit_stats[kRefitRecords] = dirty_counts[0];
        ctx->refit_stats[kRefitNodes] = dirty_counts[1];
        if (asked_partial) { ctx->partial_stats[kPartialForms] = dirty_counts[2]; ctx->partial_stats[kPartialCentreMoved] = dirty_counts[3]; }
        ctx->refit_stats[kRefitRecordsOutside] = counts[0];
        ctx->refit_stats[kRefitChildrenOutside] = counts[1];
        ctx->refit_stats[kRefitNonFinite] = counts[2];
        ctx->refit_beyond = ctx->h_bvh.refit_beyond;
        ctx->refit_stats[kRefitHalfNodes] = ctx->nodes16_valid ? 1u : 0u;
        ctx->motion_refit_differing = ctx->h_bvh.prev_differing;
        for (int i = 1; i < 4; ++i) ctx->refit_times_ms[i] = 0.0;
    } else {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
        bool ran_whole = false;
        VHR_TRY(partial ? device_refit_bvh_partial(ctx, &ran_whole) : device_refit_bvh(ctx));
        if (ran_whole) ran_as = kRanWholeFirst;
        ctx->bvh_fingerprint_valid = false;              // the hashes describe the refitted arrays: taken again when somebody asks
    }
    ctx->refit_times_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (asked_partial) {                                 // what the last partial call did, whether it succeeds or not
        ctx->partial_stats[kPartialRecords] = ctx->refit_stats[kRefitRecords];
        ctx->partial_stats[kPartialNodes] = ctx->refit_stats[kRefitNodes];
        if (ran_as != kRanDirty) { ctx->partial_stats[kPartialForms] = ctx->refit_stats[kRefitNodes]; ctx->partial_stats[kPartialCentreMoved] = 0; }
        ctx->partial_stats[kPartialRanAs] = ran_as;
        ctx->partial_stats[kPartialVertexRanges] = ctx->refit_dirty.vertices.count;
        ctx->partial_stats[kPartialPrimitiveRanges] = ctx->refit_dirty.primitives.count;
    }
    if (ctx->refit_stats[kRefitNonFinite]) {             // (updates stay pending: nothing may trace these arrays; not counted as a refit)
        const uint64_t beyond = ctx->refit_beyond, non_finite = ctx->refit_stats[kRefitNonFinite] - beyond;
        std::string met;
        if (non_finite) met = std::to_string(non_finite) + " non-finite coordinates in the triangle records (update the vertices / transforms and refit again, or rebuild)";
        if (beyond) met += std::string(non_finite ? " and " : "") + std::to_string(beyond) + " coordinates beyond the world magnitude " + std::to_string(ctx->bvh_frame_magnitude) +
                           " the padding of this \"bvh_frame\" tree was built with (the scene has moved too far for a refit: vhr_rebuild_geometry)";
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(who) + ": " + met + ": the tree's arrays are not valid");
    }
    ++ctx->refit_stats[kRefitCount];
    if (asked_partial && ran_as == kRanDirty) ++ctx->partial_stats[kPartialCount];
    if (ctx->motion_valid()) { ++ctx->motion_epoch; ctx->motion_differing = ctx->motion_refit_differing; }      // (a failed attempt leaves both: its retry has the same number)
    ctx->refit_pending = false;
    ctx->refit_dirty = RefitDirty{};
    return VHR_OK;
}

int vhr_refit_geometry(vhr_context *ctx) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    return refit_geometry(ctx, "vhr_refit_geometry", false, false);
}

int vhr_refit_geometry_partial(vhr_context *ctx, uint32_t flags) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (flags & ~uint32_t(VHR_REFIT_FORCE_PARTIAL)) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_refit_geometry_partial: unknown flag bits " + std::to_string(flags));
    return refit_geometry(ctx, "vhr_refit_geometry_partial", true, (flags & VHR_REFIT_FORCE_PARTIAL) != 0);
}

int vhr_get_partial_refit_statistics(vhr_context *ctx, uint64_t out[8]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < kPartialStatWords; ++i) out[i] = ctx->partial_stats[i];
    return VHR_OK;
}

int vhr_get_refit_statistics(vhr_context *ctx, uint64_t out[8]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < kRefitStatWords; ++i) out[i] = ctx->refit_stats[i];
    return VHR_OK;
}

int vhr_get_refit_times(vhr_context *ctx, double out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = ctx->refit_times_ms[i];
    return VHR_OK;
}

// ---- rebuild in place: a new tree over the scene arrays the context holds (refit while the tree is good, rebuild when it is not) ----
int vhr_rebuild_geometry(vhr_context *ctx, uint32_t flags) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    static const char *who = "vhr_rebuild_geometry";
    if (flags) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(who) + ": unknown flag bits " + std::to_string(flags));
    if (!ctx->has_geometry()) return no_geometry(ctx, who);
    if (ctx->recording || ctx->cur_pass || ctx->in_execute) return ctx->fail(VHR_ERROR_GRAPH, std::string(who) + ": called from inside a pass");
    const uint32_t primitive_count = ctx->primitive_count;
    const uint64_t total_triangles = ctx->prim_tri_prefix.empty() ? 0u : ctx->prim_tri_prefix.back();
    if (!ctx->host_only) {                   // frames in flight read the tree; a pending device-memory update is a copy on the context's stream
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
    }
    // every position, before anything is freed or built: device-memory vertices are unvalidated, and the builder's bin index must not see a NaN
    uint64_t non_finite = 0;
    if (ctx->host_only) non_finite = count_non_finite_positions(ctx->h_vertices.data(), ctx->vertex_count);
    else VHR_TRY(device_count_non_finite_positions(ctx, &non_finite));
    ctx->rebuild_stats[kRebuildNonFinite] = non_finite;
    if (non_finite) {                        // (the old tree's arrays are untouched, but they are not these vertices' tree: nothing traces until a refit or a rebuild succeeds)
        ctx->refit_pending = true;
        ctx->refit_dirty.vertices.add(0u, ctx->vertex_count);
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(non_finite) +
                         " non-finite coordinates in the vertex positions: nothing was rebuilt; update the vertices and rebuild or refit again");
    }
    // "object_motion_vectors": the old tree's current records in flat triangle order, for the new tree's slots (vhr_internal.hpp has the rules)
    const bool carry = ctx->motion_valid();
    const uint32_t epoch = ctx->motion_epoch + 1u;
    std::vector<BvhTri> h_flat;
    BvhTri *d_flat = nullptr;
    if (carry) {
        if (ctx->host_only) rebuild_gather_records(ctx->h_bvh.tris, ctx->h_bvh.prev_tris, ctx->h_bvh.prev_saved, epoch, uint32_t(total_triangles), h_flat);
        else VHR_TRY(device_rebuild_gather(ctx, uint32_t(total_triangles), &d_flat));
    }
    // the old tree and everything a refit had prepared for it; the scene arrays, the textures and the primitives' masks stay where they are
    discard_refit_state(ctx);
    ctx->rebuild_stats[kRebuildFetched] = ctx->rebuild_stats[kRebuildDiffering] = 0;
    if (!ctx->host_only) {
        vhr::free_refit_plan(ctx);
        free_tree(ctx);
    }
    double transfer_ms = 0.0;
    bool fetched = false;
    const HostSceneArrays scene = ctx->host_only ? HostSceneArrays{ ctx->h_vertices.data(), ctx->h_indices.data(), ctx->h_primitives.data() } : HostSceneArrays{ nullptr, nullptr, nullptr };
    int rc = build_and_install_tree(ctx, who, scene, primitive_count, total_triangles, transfer_ms, &fetched);
    uint64_t differing = 0;
    if (rc == VHR_OK && carry) {
        if (ctx->host_only) differing = rebuild_scatter_records(ctx->h_bvh, h_flat, epoch);
        else rc = device_rebuild_scatter(ctx, d_flat, uint32_t(total_triangles), &differing);
    }
    if (d_flat) hipFree(d_flat);
    if (rc != VHR_OK) {                      // no tree, as after a vhr_update_geometry that failed: the previous records go with it
        free_motion(ctx);
        return rc;
    }
    // the facing flips stay: they follow the transforms, which a rebuild does not change (a host-only context holds them and computes the bytes again)
    if (ctx->host_only) for (uint32_t p = 0; p < primitive_count; ++p) ctx->h_prim_flips[p] = facing_flip(ctx->h_primitives[p].transform);
    if (!ctx->host_only) ctx->geometry_upload_ms = transfer_ms;
    if (carry) {                            // the rebuild is refit number `epoch` of the contract at vhr_get_object_motion_statistics
        ctx->motion_epoch = epoch;
        ctx->motion_differing = ctx->motion_refit_differing = differing;
    } else {
        VHR_TRY(reset_motion(ctx));          // (option off: frees nothing; on without arrays: previous = current)
    }
    ctx->rebuild_stats[kRebuildFetched] = fetched ? 1u : 0u;
    ctx->rebuild_stats[kRebuildDiffering] = differing;
    ++ctx->rebuild_stats[kRebuildCount];
    return VHR_OK;
}

int vhr_get_rebuild_statistics(vhr_context *ctx, uint64_t out[8]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < kRebuildStatWords; ++i) out[i] = ctx->rebuild_stats[i];
    return VHR_OK;
}

int vhr_get_bvh_sah_cost(vhr_context *ctx, double out[2]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->has_geometry()) return no_geometry(ctx, "vhr_get_bvh_sah_cost");
    double now = 0.0;
    if (ctx->host_only) {
        now = bvh_sah_cost(ctx->h_bvh);
    } else {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
        VHR_TRY(device_bvh_sah_cost(ctx, &now));
    }
    if (!ctx->sah_cost_built_valid) { ctx->sah_cost_built = now; ctx->sah_cost_built_valid = true; }      // no refit has touched the tree yet
    out[0] = ctx->sah_cost_built;
    out[1] = now;
    return VHR_OK;
}

int vhr_get_primitive_facing_flips(vhr_context *ctx, uint32_t first_primitive, uint32_t count, uint8_t *out) {
    if (!ctx) return VHR_ERROR_INVALID_ARGUMENT;
    if (count > 0 && !out) return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_get_primitive_facing_flips: out must not be NULL when count > 0");
    VHR_TRY(mask_state_checks(ctx, "vhr_get_primitive_facing_flips", first_primitive, count, false));
    if (count == 0) return VHR_OK;
    std::memcpy(out, ctx->h_prim_flips.data() + first_primitive, count);
    return VHR_OK;
}

int vhr_get_face_cull_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    uint64_t flipped = 0;
    if (ctx->has_geometry()) for (uint32_t p = 0; p < ctx->primitive_count; ++p) flipped += ctx->h_prim_flips[p];
    out[0] = flipped; out[1] = ctx->rq_face_ran; out[2] = 0; out[3] = 0;
    return VHR_OK;
}

int vhr_debug_triangle_records(vhr_context *ctx, int32_t previous, float *out, uint32_t capacity_triangles, uint32_t *count) {
    if (!ctx || !count || (previous != 0 && previous != 1)) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_debug_triangle_records: null count, or previous is neither 0 nor 1") : VHR_ERROR_INVALID_ARGUMENT;
    *count = 0;
    if (!ctx->has_geometry()) return no_geometry(ctx, "vhr_debug_triangle_records");
    if (ctx->bvh_presplit_level >= 0)
        return ctx->fail(VHR_ERROR_UNSUPPORTED, "vhr_debug_triangle_records: the tree was built with \"bvh_presplit\" and has several records per triangle: there is no record per flat triangle to report");
    if (previous && !ctx->motion_valid())
        return ctx->fail(VHR_ERROR_GRAPH, "vhr_debug_triangle_records: no previous records (vhr_set_option \"object_motion_vectors\" 1 first)");
    *count = ctx->tri_count;
    if (capacity_triangles < ctx->tri_count || !out)
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, "vhr_debug_triangle_records: room for " + std::to_string(capacity_triangles) + " triangles, the scene has " + std::to_string(ctx->tri_count));
    std::vector<BvhTri> fetched;
    const BvhTri *records = previous ? ctx->h_bvh.prev_tris.data() : ctx->h_bvh.tris.data();
    if (!ctx->host_only) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
        fetched.resize(ctx->tri_count);
        HIP_TRY(ctx, hipMemcpy(fetched.data(), previous ? ctx->d_prev_tris : ctx->d_tris, sizeof(BvhTri) * ctx->tri_count, hipMemcpyDeviceToHost));
        records = fetched.data();
    }
    for (uint32_t k = 0; k < ctx->tri_count; ++k) {          // flat triangle order: independent of the tree
        const BvhTri &t = records[k];
        if (t.flat >= ctx->tri_count) return ctx->fail(VHR_ERROR_GRAPH, "vhr_debug_triangle_records: a record's flat index lies outside the scene's triangles");
        float *o = out + size_t(t.flat) * 9;
        for (int c = 0; c < 3; ++c) { o[c] = t.v0[c]; o[3 + c] = t.e1[c]; o[6 + c] = t.e2[c]; }
    }
    return VHR_OK;
}

// The tree as the walkers read it, for a judge outside the library (tests/tree_truth.py): bytes only, nothing derived or checked here.
int vhr_debug_bvh_arrays(vhr_context *ctx, uint32_t header[24], void *nodes, void *nodes_ch, void *nodes48, void *nodes16, void *records, uint32_t capacity_nodes,
                         uint32_t capacity_records, uint32_t counts[2]) {
    static const char *who = "vhr_debug_bvh_arrays";
    if (!ctx || !header || !counts) return ctx ? ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(who) + ": header and counts must not be NULL") : VHR_ERROR_INVALID_ARGUMENT;
    const bool tree = ctx->has_geometry();
    counts[0] = tree ? ctx->node_count : 0u;
    counts[1] = tree ? ctx->tri_count : 0u;
    if (capacity_nodes < counts[0] || capacity_records < counts[1] || (counts[0] && (!nodes || !nodes_ch || !nodes48 || !nodes16)) || (counts[1] && !records))
        return ctx->fail(VHR_ERROR_INVALID_ARGUMENT, std::string(who) + ": room for " + std::to_string(capacity_nodes) + " nodes and " + std::to_string(capacity_records) +
                         " records (or a NULL array), the tree has " + std::to_string(counts[0]) + " and " + std::to_string(counts[1]));
    if (ctx->recording || ctx->cur_pass || ctx->in_execute) return ctx->fail(VHR_ERROR_GRAPH, std::string(who) + ": called from inside a pass");
    if (!tree) return no_geometry(ctx, who);
    HostBvh fetched;
    if (!ctx->host_only) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
        VHR_TRY(fetch_device_tree(ctx, fetched));
    }
    const HostBvh &bvh = ctx->host_only ? ctx->h_bvh : fetched;
    std::memcpy(nodes, bvh.nodes.data(), sizeof(BvhNode) * counts[0]);
    std::memcpy(nodes_ch, bvh.nodes_ch.data(), sizeof(BvhNodeCH) * counts[0]);
    std::memcpy(nodes48, bvh.nodes48.data(), sizeof(BvhNode48) * counts[0]);
    std::memcpy(nodes16, bvh.nodes16.data(), sizeof(BvhNode16) * counts[0]);
    std::memcpy(records, bvh.tris.data(), sizeof(BvhTri) * counts[1]);
    for (int i = 0; i < 24; ++i) header[i] = 0u;
    std::memcpy(header, ctx->host_only ? ctx->h_bvh.centre : ctx->bvh_centre, 3 * sizeof(float));
    std::memcpy(header + 3, ctx->bvh_frame, 9 * sizeof(float));
    header[12] = ctx->bvh_frame_on ? 1u : 0u;
    header[13] = ctx->nodes16_valid ? 1u : 0u;
    header[14] = ctx->node_count;
    header[15] = ctx->tri_count;
    header[16] = ctx->bvh_depth;
    std::memcpy(header + 17, &ctx->bvh_frame_magnitude, sizeof(float));
    return VHR_OK;
}

int vhr_get_object_motion_statistics(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = ctx->motion_valid() ? 1u : 0u;
    out[1] = ctx->motion_valid() ? ctx->motion_differing : 0u;
    out[2] = ctx->motion_launches;
    out[3] = 0;
    return VHR_OK;
}

int vhr_get_bvh_statistics(vhr_context *ctx, uint64_t out[5]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    out[0] = ctx->node_count; out[1] = ctx->tri_count; out[2] = ctx->bvh_depth;
    out[3] = uint64_t(ctx->node_count) * sizeof(BvhNode); out[4] = uint64_t(ctx->tri_count) * sizeof(BvhTri);
    return VHR_OK;
}

static int fingerprints_of_device_tree(vhr_context *ctx) {      // a device-built tree: fetched when somebody asks, hashed like the host's
    if (ctx->bvh_fingerprint_valid || ctx->host_only || !ctx->has_geometry()) return VHR_OK;
    HostBvh bvh;
    VHR_TRY(fetch_device_tree(ctx, bvh));
    ctx->bvh_fingerprint = bvh_fingerprint(bvh);
    ctx->bvh_tree_fingerprint = bvh_tree_fingerprint(bvh);
    ctx->bvh_fingerprint_valid = true;
    return VHR_OK;
}

int vhr_get_bvh_fingerprint(vhr_context *ctx, uint64_t *out) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    VHR_TRY(fingerprints_of_device_tree(ctx));
    *out = ctx->bvh_fingerprint;
    return VHR_OK;
}

int vhr_get_bvh_tree_fingerprint(vhr_context *ctx, uint64_t *out) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    VHR_TRY(fingerprints_of_device_tree(ctx));
    *out = ctx->bvh_tree_fingerprint;
    return VHR_OK;
}
// The forms as they stand against the forms the host derives from the same (lo, hi) nodes: equal hashes say that the builder that made the
// tree (or refitted it) and the host run the same bvh_math.hpp, conversions included.
int vhr_get_bvh_forms_fingerprint(vhr_context *ctx, uint64_t out[2]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    if (!ctx->has_geometry()) return no_geometry(ctx, "vhr_get_bvh_forms_fingerprint");
    HostBvh fetched, again;
    if (!ctx->host_only) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        VHR_TRY(ctx->sync_streams());
        VHR_TRY(fetch_device_tree(ctx, fetched));
    }
    const HostBvh &tree = ctx->host_only ? ctx->h_bvh : fetched;
    out[0] = bvh_forms_fingerprint(tree);
    again.nodes = tree.nodes;
    derive_node_forms(again, ctx->bvh_build_threads);
    out[1] = bvh_forms_fingerprint(again);
    return VHR_OK;
}

int vhr_get_bvh_form_checks(vhr_context *ctx, uint64_t out[4]) {
    if (!ctx || !out) return VHR_ERROR_INVALID_ARGUMENT;
    for (int i = 0; i < 4; ++i) out[i] = ctx->bvh_form_checks[i];
    return VHR_OK;
}

}  // extern "C"
