// fold_model.hpp -- TEST INFRASTRUCTURE: what fold_stub.cpp records of a launch and the word pattern its model
// of the launch stores, shared with fold_driver.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../kifs_raymarching_amd/csrc/kifs_params.hpp"

// (what the stand-in for launch_eval_fold records, and the values it stores for position i)
struct FoldStubEval {
    kifs::fold::EvalParams params;
    uint32_t group, primitive;
    hipStream_t stream;
};

struct FoldStubLaunch {
    kifs::fold::Params params;
    uint32_t group, primitive;
    hipStream_t stream;
};

namespace fold_model {

// The pixel of view v at frame row y, column x: never the drivers' sentinel 0xA5A5A5A5 (alpha 255).  `term`: whether the
// launch carried one; e: the light's shininess_log2; N: the system's iterations.
inline uint32_t pixel(int v, int y, int x, int encode, int k, bool term, int e, int N) {
    return 0xff000000u | (uint32_t((v + e + N) & 0x1f) << 19) | (uint32_t(term) << 18) | (uint32_t(encode & 1) << 17) |
           (uint32_t(k & 7) << 14) | (uint32_t(y & 0x7f) << 7) | uint32_t(x & 0x7f);
}

inline float sdf_of(int i, int N) { return float(i) * 0.5f + float(N); }
inline float normal_of(int i, int axis) { return float(3 * i + axis) * 0.25f; }

}  // namespace fold_model
