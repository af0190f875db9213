// occlusion_stub.cpp -- TEST INFRASTRUCTURE, never shipped: a stand-in for launch_occlusion (kifs_occlusion_kernels.hip)
// for occlusion_driver.cpp (`make asan-occlusion`).  It RECORDS what a launch carries -- the occl::Params, the pipeline
// and the stream -- refuses what the API must have refused before it got here, and models the launch's stores: every row
// of every view's band receives a word pattern of (view, row, column) in the colour destination and, when a plane is
// given, in the plane, through need_device, so that a byte outside the caller's arrays aborts.
// occlusion_stub_fail_next(): the next launch fails once.
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "occlusion_model.hpp"

namespace {

bool g_fail_next = false;
long g_launches = 0;
OcclusionStubLaunch g_last{};

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "occlusion_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "occlusion_stub: %s\n", what);
    std::abort();
}

}  // namespace

extern "C" {
void occlusion_stub_fail_next() { g_fail_next = true; }
long occlusion_stub_launches() { return g_launches; }
}
const OcclusionStubLaunch& occlusion_stub_last() { return g_last; }

namespace kifs {

hipError_t launch_occlusion(const occl::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream) {
    ++g_launches;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    const FrameParams& P = O.B.frame;
    // what the API must have refused before it got here
    if (O.B.count < 1 || O.B.count > MAX_BATCH_INLINE || O.B.table) refuse("a count the kernel argument cannot hold");
    if (P.ssaa < 1 || P.ssaa > 4 || (O.plane && P.ssaa > 1)) refuse("a bad supersampling factor, or a plane beside one");
    if (O.ao.samples < 1 || O.ao.samples > 16 || !(O.ao.step > 0.0f) || !(O.ao.decay > 0.0f) || !(O.ao.decay <= 1.0f) ||
        !(O.ao.strength >= 0.0f) || !(O.ao.step <= FLT_MAX) || !(O.ao.strength <= FLT_MAX))
        refuse("a term outside its ranges");
    if (group > 2u) refuse("no pipeline");
    if (P.encode != 0 && P.encode != 1) refuse("a bad encode");
    if (P.y0 < 0 || P.y1 <= P.y0 || P.width < 1) refuse("an empty or inverted band");
    if (P.stripe_rows || P.geom || P.tile_cost || P.counters || P.round_steps || P.workgroups_per_cu) refuse("not the fixed launch shape");
    if (!P.tile_order || P.tile_count != uint32_t((P.width + 31) / 32) * uint32_t((P.y1 - P.y0 + 7) / 8)) refuse("not the band's tile table");
    if (P.pitch_words < uint32_t(P.width)) refuse("a colour pitch below the width");
    if (O.plane && ((reinterpret_cast<uintptr_t>(O.plane) & 3u) || O.pitch_words < uint32_t(P.width) ||
                    (O.B.count > 1 && size_t(O.stride_words) < size_t(P.y1 - P.y0) * O.pitch_words)))
        refuse("a bad plane layout");
    need_device(P.srgb_table, 256 * sizeof(float), "the sRGB table");
    need_device(P.tile_order, size_t(P.tile_count) * 4, "the tile order");
    g_last = OcclusionStubLaunch{O, group, primitive, stream};
    const int rows = P.y1 - P.y0;
    for (int v = 0; v < O.B.count; ++v) {
        uint32_t* out = O.B.count > 1 ? O.B.view[v].out : P.out;
        if (!out || (reinterpret_cast<uintptr_t>(out) & 3u)) refuse("a null or misaligned destination");
        for (int r = 0; r < rows; ++r) {
            uint32_t* row = out + size_t(r) * P.pitch_words;
            need_device(row, size_t(P.width) * 4, "a colour row");
            for (int x = 0; x < P.width; ++x) row[x] = occlusion_model::pixel(v, P.y0 + r, x, P.encode, P.ssaa);
            if (!O.plane) continue;
            float* prow = O.plane + size_t(v) * O.stride_words + size_t(r) * O.pitch_words;
            need_device(prow, size_t(P.width) * 4, "a plane row");
            for (int x = 0; x < P.width; ++x) prow[x] = occlusion_model::factor(v, P.y0 + r, x, O.ao.samples);
        }
    }
    return hipSuccess;
}

}  // namespace kifs
