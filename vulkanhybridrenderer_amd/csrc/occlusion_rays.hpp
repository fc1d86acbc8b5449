// The rays of vhr_occlusion_query (include/vhr_amd.h): ONE definition for the device (kernels_occlusion.hip: the fetch of the query kernel's
// walk, the binary64 launch and the kernel of vhr_debug_occlusion_rays) and for the host (queries.cpp: vhr_debug_occlusion_rays on a host-only
// context).  The counterpart of closest_point.hpp and ray_facing.hpp; every unit that includes it is built with -ffp-contract=off: the two
// copies owe each other bits.
//
// raygen.rgen:44-55 draws a pixel's AO rays by stepping one generator; here every (point, sample) is keyed on its own, so that no lane has to
// step a generator j times and a ray does not depend on the `samples` it was asked with beyond its index g.  The generator, the sample and the
// basis are device_math.hpp's, each operation rounded once.
#pragma once

#include "device_math.hpp"

namespace vhr {

constexpr uint32_t kOcclusionZeroState = 0x9E3779B9u;      // xorshift stays at 0 for ever: the one g per seed that hashes to 0 starts here instead

// A query point and a ray share a layout (vhr_ray): the point's `d` is the hemisphere's axis, used as given, never normalised.
struct OcclusionRay { f3 o; float tmin; f3 d; float tmax; };

// ray (i, j) of `point`, j < samples
__host__ __device__ __forceinline__ OcclusionRay occlusion_ray(const OcclusionRay &point, uint32_t i, uint32_t j, uint32_t samples, uint32_t seed) {
    const uint32_t g = i * samples + j;
    uint32_t state = seed_thread(g ^ seed_thread(seed));
    if (state == 0u) state = kOcclusionZeroState;
    const float rnd1 = random01(state);
    const float rnd2 = random01(state);
    return OcclusionRay{ point.o, point.tmin, onb_transform(point.d, cosine_hemisphere(rnd1, rnd2)), point.tmax };
}

}  // namespace vhr
