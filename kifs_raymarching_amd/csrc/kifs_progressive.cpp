// kifs_progressive.cpp -- the host side of progressive accumulation (kifs_render_accumulate_resume_async,
// include/kifs_hip.h): one PASS of a frame whose linear sums are carried across launches in a plane of the caller's.  A
// pass is the jittered accumulated call (accum::check and check_jitter of kifs_accumulate.cpp, then the SceneLaunch of
// kifs_animation.cpp: the same views, scene table, rings and debug hooks) with another kernel behind it: the launch step wraps the filled Params into
// a CarryParams -- the plane, the sub-frames it already holds, whether the pass has destinations -- for
// launch_accumulate_carry (kifs_accumulate_kernels.hip).  The library keeps nothing between passes.
#include "kifs_context.hpp"

namespace kifs {
namespace accum {

// The plane of a pass, as the caller gave it.
struct Plane {
    float* sums;
    size_t pitch, stride;  // bytes
    uint32_t prior;
    bool picture;
};

static hipError_t launch_carry(const Params& A, uint32_t group, uint32_t primitive, hipStream_t stream, void* user) {
    const Plane& p = *static_cast<const Plane*>(user);
    CarryParams K;
    K.A = A;
    K.sums = p.sums;
    K.sums_pitch_texels = uint32_t(p.pitch >> 4);
    K.sums_stride_texels = uint32_t(p.stride >> 4);
    K.prior = p.prior;
    K.picture = p.picture ? 1u : 0u;
    return launch_accumulate_carry(K, group, primitive, stream);
}

}  // namespace accum
}  // namespace kifs

extern "C" int kifs_render_accumulate_resume_async(kifs_ctx* c, void* hip_stream, int count, int samples,
                                                   const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid,
                                                   const KifsSubpixel* cells, float* dev_sums, size_t sums_pitch, size_t sums_stride,
                                                   uint32_t prior_samples, uint8_t* const* dev_outs, size_t pitch, int y0, int y1,
                                                   int encode) {
    using namespace kifs;
    if (const int st = accum::check(c, count, samples, cameras, options, dev_outs, pitch, y0, y1, encode, true); st != KIFS_OK) return st;
    const accum::Jitter jitter{grid, cells};
    if (const int st = accum::check_jitter(c, count, samples, jitter); st != KIFS_OK) return st;
    // What the pass refuses beyond check() and check_jitter(): after them, so that every refusal of the jittered call
    // keeps its status.
    int w = 0, h = 0;
    if (const int st = host::frame_dims(c, &w, &h); st != KIFS_OK) return st;
    if (const int st = accum::check_plane(dev_sums, sums_pitch, sums_stride, 16, w, size_t(y1 - y0), count); st != KIFS_OK) return st;
    if (uint64_t(prior_samples) + uint64_t(samples) > uint64_t(KIFS_MAX_PROGRESSIVE_SAMPLES)) return KIFS_ERR_BAD_ARG;
    accum::Plane plane{dev_sums, sums_pitch, sums_stride, prior_samples, dev_outs != nullptr};
    return anim::launch_scenes(c, hip_stream, anim::SceneLaunch{count, samples, cameras, options, &jitter, dev_outs, pitch, y0, y1, encode,
                                                                KIFS_KERNEL_ACCUMULATE, accum::launch_carry, &plane,
                                                                accum::WORKGROUPS_PER_ENTRY});
}
