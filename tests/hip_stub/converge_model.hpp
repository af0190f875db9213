// converge_model.hpp -- TEST INFRASTRUCTURE, shared by accumulate_family_stub.cpp (the stand-in for the accumulate launchers) and
// converge_driver.cpp (which restates what the stand-in must have written): the stand-in state of a pixel of a
// converging pass and a stand-in stopping rule.  Nothing here is the kernel's arithmetic: it only has to depend on
// everything the host side hands over -- both planes as read, min_samples, tol2, the pass's sub-frames -- so that a
// wrong pointer, pitch, flag or rule shows as a wrong texel, pixel or count.
#pragma once

#include "accumulate_model.hpp"

namespace converge_model {

struct Pixel {
    uint32_t acc = 0u;  // word 0 of the texel: accumulate_model's fold
    float n = 0.0f;     // word 3: the pixel's own count
    uint32_t q = 0u;    // the moment's word
};

// One sub-frame into the state; `first`: the pass starts from nothing (a restart, or a carried pass with prior == 0).
inline void add(Pixel& p, uint32_t one, bool first) {
    p.acc = first ? one : accumulate_model::fold(p.acc, one);
    p.q = first ? one * 7u : p.q * 5u + one;
}

// The stand-in rule: a pixel with min_samples sub-frames stops when a hash of its state falls under a threshold that grows
// with tol2 (+inf: always; 0: never), and any pixel freezes when its count could leave 2^24.
inline bool active(const Pixel& p, uint32_t min_samples, float tol2, int samples) {
    const uint32_t hash = ((p.acc ^ p.q) * 2654435761u) >> 24;  // 0..255
    const float bound = tol2 * 256.0f;
    const bool settled = p.n >= float(min_samples) && float(hash) < bound;
    return !settled && p.n + float(samples) <= 16777216.0f;
}

}  // namespace converge_model
