// fold_trap_model.hpp -- TEST INFRASTRUCTURE: what fold_trap_stub.cpp records of a launch and the word patterns its model
// of the launch stores, shared with fold_trap_driver.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../kifs_raymarching_amd/csrc/kifs_params.hpp"

// (what the stand-in for launch_eval_fold_trap records)
struct FoldTrapStubEval {
    kifs::foldorbit::EvalParams params;
    uint32_t group, primitive;
    hipStream_t stream;
};

// The launch's Params and THE RECORD'S CONTENTS AS THE COPY LEFT THEM AT LAUNCH TIME (read through Params::record).
struct FoldTrapStubLaunch {
    kifs::foldorbit::Params params;
    kifs::foldorbit::Record record;
    uint32_t group, primitive;
    hipStream_t stream;
};

namespace fold_trap_model {

// The pixel of view v at frame row y, column x: never the drivers' sentinel 0xA5A5A5A5 (alpha 255).  `term`: whether the
// launch carried one; e: the light's shininess_log2; N, K: the record's iterations.
inline uint32_t pixel(int v, int y, int x, int encode, int k, bool term, int e, int N, int K) {
    return 0xff000000u | (uint32_t((v + e + N + 3 * K) & 0x1f) << 19) | (uint32_t(term) << 18) | (uint32_t(encode & 1) << 17) |
           (uint32_t(k & 7) << 14) | (uint32_t(y & 0x7f) << 7) | uint32_t(x & 0x7f);
}

// The plane's value there: never the sentinel's bit pattern.
inline float u_of(int v, int y, int x, int N, int K) { return float(v) * 1024.0f + float(y) * 8.0f + float(x) * 0.03125f + float(N) * 0.25f + float(K) * 65536.0f; }

inline float eval_of(int i, int N, int K) { return float(i) * 0.5f + float(N) + 100.0f * float(K); }

}  // namespace fold_trap_model
