// kifs_converge.cpp -- the host side of converging accumulation (kifs_render_accumulate_converge_async,
// include/kifs_hip.h): one pass of a progressive frame that marches only the pixels whose mean has not settled.  A pass
// is the jittered accumulated call (accum::check and check_jitter of kifs_accumulate.cpp, then the SceneLaunch of
// kifs_animation.cpp) with a launch step of its own, as kifs_progressive.cpp has: it zeroes the caller's counts on the stream and wraps the filled Params
// into a ConvergeParams -- the two planes, the rule, whether the pass restarts and whether it has destinations -- for
// launch_accumulate_converge (kifs_accumulate_kernels.hip).  The library keeps nothing between passes.
#include <cmath>

#include "kifs_context.hpp"

namespace kifs {
namespace accum {

// The state and the rule of a pass, as the caller gave them.
struct Converging {
    float* sums;
    size_t sums_pitch, sums_stride;  // bytes
    float* moments;
    size_t moments_pitch, moments_stride;  // bytes
    bool restart, picture;
    KifsConvergence rule;
    uint32_t* counts;  // may be null
};

static hipError_t launch_converge(const Params& A, uint32_t group, uint32_t primitive, hipStream_t stream, void* user) {
    const Converging& p = *static_cast<const Converging*>(user);
    ConvergeParams K;
    K.A = A;
    K.sums = p.sums;
    K.sums_pitch_texels = uint32_t(p.sums_pitch >> 4);
    K.sums_stride_texels = uint32_t(p.sums_stride >> 4);
    K.moments = p.moments;
    K.moments_pitch_words = uint32_t(p.moments_pitch >> 2);
    K.moments_stride_words = uint32_t(p.moments_stride >> 2);
    K.restart = p.restart ? 1u : 0u;
    K.picture = p.picture ? 1u : 0u;
    K.min_samples = p.rule.min_samples;
    K.tol2 = p.rule.tolerance * p.rule.tolerance;  // the rule's one f32 multiply (+inf stays +inf)
    K.counts = p.counts;
    // the blocks add to the frames' words: zero them first, on the stream (as the adaptive call's edge counts)
    if (p.counts)
        if (hipError_t e = hipMemsetAsync(p.counts, 0, size_t(A.frames) * sizeof(uint32_t), stream); e != hipSuccess) return e;
    return launch_accumulate_converge(K, group, primitive, stream);
}

}  // namespace accum
}  // namespace kifs

extern "C" int kifs_render_accumulate_converge_async(kifs_ctx* c, void* hip_stream, int count, int samples,
                                                     const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid,
                                                     const KifsSubpixel* cells, float* dev_sums, size_t sums_pitch, size_t sums_stride,
                                                     float* dev_moments, size_t moments_pitch, size_t moments_stride, int restart,
                                                     const KifsConvergence* rule, uint32_t* dev_active_counts,
                                                     uint8_t* const* dev_outs, size_t pitch, int y0, int y1, int encode) {
    using namespace kifs;
    if (const int st = accum::check(c, count, samples, cameras, options, dev_outs, pitch, y0, y1, encode, true); st != KIFS_OK) return st;
    const accum::Jitter jitter{grid, cells};
    if (const int st = accum::check_jitter(c, count, samples, jitter); st != KIFS_OK) return st;
    // What the pass refuses beyond check() and check_jitter(): after them, so that every refusal of the resume call
    // keeps its status.  The sums plane's rules are that call's; the moments plane's are the same with 4 bytes per pixel.
    int w = 0, h = 0;
    if (const int st = host::frame_dims(c, &w, &h); st != KIFS_OK) return st;
    const size_t rows = size_t(y1 - y0);
    if (const int st = accum::check_plane(dev_sums, sums_pitch, sums_stride, 16, w, rows, count); st != KIFS_OK) return st;
    if (const int st = accum::check_plane(dev_moments, moments_pitch, moments_stride, 4, w, rows, count); st != KIFS_OK) return st;
    if (!rule) return KIFS_ERR_BAD_ARG;
    if (std::isnan(rule->tolerance) || rule->tolerance < 0.0f) return KIFS_ERR_BAD_ARG;
    if (rule->min_samples < 2u || rule->min_samples > KIFS_MAX_PROGRESSIVE_SAMPLES) return KIFS_ERR_BAD_ARG;
    accum::Converging state{dev_sums, sums_pitch, sums_stride, dev_moments, moments_pitch, moments_stride, restart != 0,
                            dev_outs != nullptr, *rule, dev_active_counts};
    // (an empty band returns before the launch step: nothing enqueued, the counts untouched)
    return anim::launch_scenes(c, hip_stream, anim::SceneLaunch{count, samples, cameras, options, &jitter, dev_outs, pitch, y0, y1, encode,
                                                                KIFS_KERNEL_ACCUMULATE, accum::launch_converge, &state,
                                                                accum::WORKGROUPS_PER_ENTRY});
}
