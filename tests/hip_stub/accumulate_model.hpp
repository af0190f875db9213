// accumulate_model.hpp -- TEST INFRASTRUCTURE, shared by accumulate_family_stub.cpp (the stand-in for the accumulate launchers)
// and the four drivers of the accumulated calls (which restate what the stand-in must have written): the stand-in "colour" of a sub-frame's
// pixel and the order-dependent fold of a frame's sub-frames into one output pixel.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../kifs_raymarching_amd/csrc/kifs_params.hpp"

namespace accumulate_model {

inline uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// A sub-frame's pixel: a function of the view's camera, of all of its scene record but the padding, and of the pixel's
// FRAME coordinates.
inline uint32_t sample(const kifs::BatchView& v, const kifs::anim::SceneView& s, int x, int y) {
    const float f[23] = {v.origin.x, v.origin.y, v.origin.z, v.m0.x, v.m0.y, v.m0.z, v.m1.x, v.m1.y, v.m1.z, v.m2.x, v.m2.y, v.m2.z,
                         s.c.x, s.c.y, s.c.z, s.c.w, s.power, s.fractal_color.x, s.fractal_color.y, s.fractal_color.z,
                         s.background_color.x, s.background_color.y, s.background_color.z};
    uint32_t k = 2166136261u;
    for (float value : f) k = (k ^ bits(value)) * 16777619u;
    return k ^ (uint32_t(x) * 73856093u) ^ (uint32_t(y) * 19349663u);
}
// The fold of the sub-frames, in order (not commutative: a stand-in that took them in another order shows).
inline uint32_t fold(uint32_t acc, uint32_t next) { return acc * 31u + next; }
inline uint32_t pixel(uint32_t acc, int samples) { return (acc ^ uint32_t(samples)) | 0xff000000u; }

}  // namespace accumulate_model
