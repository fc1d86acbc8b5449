// What the two device BVH units share: kernels_bvh.hip (the build) and kernels_bvh_refit.hip (refit, partial refit, motion settle, the
// rebuild's passes, SAH cost).  Types and inline functions live here, in an unnamed namespace like the kernels that take them; the kernels both
// units need (node bounds, derived forms, form checks) are compiled in kernels_bvh.hip alone and reached through the launchers at the end.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "vhr_internal.hpp"
#include "bvh_math.hpp"

namespace vhr {
namespace {

struct Box6 { float lo[3], hi[3]; };

__device__ __forceinline__ uint32_t ordered(float f) {          // monotone float -> uint32 (for atomicMin / atomicMax)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float unordered(uint32_t u) {
    const uint32_t v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// min / max into a word many waves aim at: look first (most values no longer move it), then the atomic
__device__ __forceinline__ void atomic_min_checked(uint32_t *p, uint32_t v) {
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}
__device__ __forceinline__ void atomic_max_checked(uint32_t *p, uint32_t v) {
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

// A partial refit runs the per-node kernels on the nodes whose bit is set in `dirty` (one word per 32 nodes); nullptr = every node.
__device__ __forceinline__ bool node_selected(const uint32_t *dirty, uint32_t k) { return !dirty || ((dirty[k >> 5] >> (k & 31u)) & 1u) != 0u; }

// the scene centre from what the node-bounds kernel left (lo[3], hi[3] as ordered uints)
inline void centre_from_bounds(const uint32_t bounds[6], float centre[3]) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = unordered(bounds[a]); hi[a] = unordered(bounds[3 + a]); }
    bvh_math::centre_of(lo, hi, centre);
}

struct Scratch {            // device allocations of one build, freed together
    std::vector<void *> ptrs;
    template <typename T>
    hipError_t alloc(T **p, size_t count) {
        *p = nullptr;
        if (!count) return hipSuccess;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    ~Scratch() { for (void *p : ptrs) hipFree(p); }
};

}  // namespace

// a failed HIP call ends the function with the context's error set: "<what>: <the call>: <HIP's text>" (what: "device K0", "refit", "rebuild")
#define BVH_TRY(what, expr)                                                                                 \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return ctx->fail(VHR_ERROR_DEVICE, std::string(what ": ") + #expr + ": " + hipGetErrorString(e_)); \
    } while (0)

// The kernels both units launch (compiled in kernels_bvh.hip), on ctx->stream over the first `count` nodes of ctx->d_nodes, with ctx->bvh_centre:
// the bounds of all child boxes into bounds[0..5] (ordered uints); the derived forms into ctx->d_nodes_ch / d_nodes48 / d_nodes16; check_forms'
// five counters summed into out[0..4].  `dirty` (nullptr = every node) and `status`: see k0_check_forms_kernel.
void launch_node_bounds(vhr_context *ctx, uint32_t count, uint32_t *bounds);
void launch_forms(vhr_context *ctx, uint32_t count, const uint32_t *dirty);
void launch_check_forms(vhr_context *ctx, uint32_t count, unsigned long long *out, const uint32_t *dirty, uint16_t *status);
// The rule for the 32-byte half-precision nodes after a build or a refit: the walkers use them if no box left the half range (`out_of_range`,
// check_forms' out[4]), no link's byte offset needs more than 31 bits, and none failed its containment check (`not_contained`, out[3], which
// means something only where the form is in range).  Sets ctx->bvh_form_checks[3] and ctx->nodes16_valid.
void publish_half_nodes(vhr_context *ctx, uint32_t n_nodes, uint64_t not_contained, uint64_t out_of_range);

}  // namespace vhr
