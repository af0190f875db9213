// occlusion_model.hpp -- TEST INFRASTRUCTURE: what occlusion_stub.cpp records of a launch and the word patterns its
// model of the launch stores, shared with occlusion_driver.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../kifs_raymarching_amd/csrc/kifs_params.hpp"

struct OcclusionStubLaunch {
    kifs::occl::Params params;
    uint32_t group, primitive;
    hipStream_t stream;
};

namespace occlusion_model {

// The pixel of view v at frame row y, column x: never the drivers' sentinel 0xA5A5A5A5 (alpha 255).
inline uint32_t pixel(int v, int y, int x, int encode, int k) {
    return 0xff000000u | (uint32_t(v & 0x3f) << 18) | (uint32_t(encode & 1) << 17) | (uint32_t(k & 7) << 14) |
           (uint32_t(y & 0x7f) << 7) | uint32_t(x & 0x7f);
}
// The plane's value there: a number in [0, 1) that tells the three apart, and the probe count.
inline float factor(int v, int y, int x, int samples) {
    return float((v * 131 + y * 17 + x * 3 + samples) & 1023) / 1024.0f;
}

}  // namespace occlusion_model
