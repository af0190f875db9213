// rays_model.hpp -- TEST INFRASTRUCTURE: what rays_stub.cpp writes for a ray and rays_driver.cpp expects, and the record
// of a launch the two share.  A pattern of the ray's six components and its index, not a march: the driver checks the host
// side's bookkeeping (which ray went where, how many, through which pointers), the GPU tests check the kernel.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../kifs_raymarching_amd/csrc/kifs_params.hpp"

// What the latest launch that was not made to fail carried.
struct RaysStubLaunch {
    kifs::rays::Params params;
    uint32_t group, primitive;
    hipStream_t stream;
    uint32_t workgroups;
};

namespace rays_model {

constexpr int MODEL_RAYS = 1 << 16;  // the stand-in models launches up to this many rays and only records larger ones

inline uint32_t word(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
// ray: eight floats (origin.xyz, -, direction.xyz, -); the reserved words are not read.
inline uint32_t mix(const float* ray, size_t k) {
    uint32_t h = 0x9e3779b9u * uint32_t(k + 1);
    for (int i : {0, 1, 2, 4, 5, 6}) h = (h ^ word(ray[i])) * 2654435761u;
    return h;
}
inline void texel(const float* ray, size_t k, uint32_t out[4]) {
    const uint32_t h = mix(ray, k);
    out[0] = h;
    out[1] = ~h;
    out[2] = h * 3u;
    out[3] = uint32_t(k);
}
inline uint32_t pixel(const float* ray, size_t k, int encode) { return (mix(ray, k) >> (encode ? 8 : 4)) | 0xff000000u; }

}  // namespace rays_model
