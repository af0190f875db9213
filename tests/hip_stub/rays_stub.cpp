// rays_stub.cpp -- TEST INFRASTRUCTURE, never shipped: a stand-in for launch_trace_rays (kifs_rays_kernels.hip) for
// rays_driver.cpp (`make asan-rays`).  It RECORDS what a launch carries -- the rays::Params, the pipeline, the stream and
// the grid rays::workgroups() gives the count -- and, for a count it can afford (up to MODEL_RAYS), models the launch:
// every ray's two 16-byte rows are read and each given output receives a word pattern of the ray and its index, through
// need_device, so that a byte outside the caller's arrays aborts.  A larger count is recorded only: KIFS_MAX_RAYS rays
// are 8 GB.  rays_stub_fail_next(): the next launch fails once.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "rays_model.hpp"

namespace {

bool g_fail_next = false;
long g_launches = 0;
RaysStubLaunch g_last{};

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "rays_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "rays_stub: %s\n", what);
    std::abort();
}

}  // namespace

extern "C" {
void rays_stub_fail_next() { g_fail_next = true; }
long rays_stub_launches() { return g_launches; }
}
const RaysStubLaunch& rays_stub_last() { return g_last; }

namespace kifs {

hipError_t launch_trace_rays(const rays::Params& R, uint32_t group, uint32_t primitive, hipStream_t stream) {
    ++g_launches;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    // what the API must have refused before it got here
    if (R.n < 1 || !R.rays || (!R.geom && !R.rgba)) refuse("an empty launch, no rays or no output");
    if ((reinterpret_cast<uintptr_t>(R.rays) & 15u) || (reinterpret_cast<uintptr_t>(R.geom) & 15u) || (reinterpret_cast<uintptr_t>(R.rgba) & 3u))
        refuse("a misaligned array");
    if (group > 2u) refuse("no pipeline");
    if (R.frame.encode != 0 && R.frame.encode != 1) refuse("a bad encode");
    need_device(R.frame.srgb_table, 256 * sizeof(float), "the sRGB table");
    g_last = RaysStubLaunch{R, group, primitive, stream, rays::workgroups(R.n)};
    if (R.n > rays_model::MODEL_RAYS) return hipSuccess;
    const size_t n = size_t(R.n);
    need_device(R.rays, n * 32, "the rays");
    if (R.geom) need_device(R.geom, n * 16, "the texels");
    if (R.rgba) need_device(R.rgba, n * 4, "the pixels");
    for (size_t k = 0; k < n; ++k) {
        uint32_t words[4];
        rays_model::texel(R.rays + 8 * k, k, words);
        if (R.geom) std::memcpy(R.geom + 4 * k, words, 16);
        if (R.rgba) R.rgba[k] = rays_model::pixel(R.rays + 8 * k, k, R.frame.encode);
    }
    return hipSuccess;
}

}  // namespace kifs
