// kifs_accumulate.cpp -- the host side of accumulated frames (kifs_render_accumulate_async, include/kifs_hip.h): the
// argument checks of the family, and the call itself as a SceneLaunch (kifs_animation.cpp: the sub-frames laid out as the
// views of one launch, a scene record per view, filled with the context's scene when the caller gives no options) whose
// last step is launch_accumulate_render (kifs_accumulate_kernels.hip).
// kifs_render_accumulate_jittered_async is the same call with a cell of a g x g grid inside the pixel per sub-frame (a
// Jitter: null for the unjittered call): the cell travels in pad[0] of the view's scene record, the grid as the launch's
// FrameParams::ssaa, and the launcher takes the jitter kernel from g = 2.
#include "kifs_context.hpp"

namespace kifs {
namespace accum {

// (Jitter, check, check_jitter and check_plane are declared in kifs_context.hpp: the two kinds of pass share them.)
int check_jitter(const kifs_ctx* c, int count, int samples, const Jitter& j) {
    if (j.grid < 1 || j.grid > KIFS_MAX_JITTER_GRID) return KIFS_ERR_BAD_ARG;
    if (!j.cells && samples != j.grid * j.grid) return KIFS_ERR_BAD_ARG;
    if (j.cells)
        for (int v = 0; v < count * samples; ++v)
            if (j.cells[v].i >= j.grid || j.cells[v].j >= j.grid) return KIFS_ERR_BAD_ARG;
    int w = 0, h = 0;
    if (const int st = host::frame_dims(c, &w, &h); st != KIFS_OK) return st;
    // the virtual g W x g H screen stays within frame_dims' limit, as a supersampled launch's (render_dims)
    return (int64_t(w) * j.grid > 65536 || int64_t(h) * j.grid > 65536) ? KIFS_ERR_BAD_SIZE : KIFS_OK;
}

int check(const kifs_ctx* c, int count, int samples, const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
          uint8_t* const* outs, size_t pitch, int y0, int y1, int encode, bool outs_optional) {
    if (!c || !cameras || (!outs && !outs_optional)) return KIFS_ERR_BAD_ARG;
    if (samples < 1 || samples > KIFS_MAX_ACCUMULATE || count < 1 || count > MAX_BATCH / samples) return KIFS_ERR_BAD_ARG;
    for (int i = 0; outs && i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    if (c->supersampling > 1) return KIFS_ERR_BAD_ARG;  // out of scope, as for the geometry output
    if (!c->have_screen || (!options && !c->have_options)) return KIFS_ERR_UNCONFIGURED;
    const KifsOptionsUniform& first = options ? options[0] : c->options;
    if (first.fractal_group_id > 2u) return KIFS_ERR_BAD_ARG;
    if (options)
        for (int v = 1; v < count * samples; ++v)
            if (!anim::same_pipeline(first, options[v])) return KIFS_ERR_BAD_ARG;
    int w = 0, h = 0;
    if (const int st = host::frame_dims(c, &w, &h); st != KIFS_OK) return st;
    if (y0 < 0 || y1 > h || y0 > y1) return KIFS_ERR_BAD_ARG;
    if (outs && (pitch < size_t(w) * 4 || (pitch & 3u) != 0 || (pitch >> 2) > 0xffffffffull)) return KIFS_ERR_BAD_SIZE;
    return KIFS_OK;
}

int check_plane(const void* plane, size_t pitch, size_t stride, size_t texel_bytes, int width, size_t rows, int count) {
    const size_t low = texel_bytes - 1;  // (16 or 4: a power of two)
    if (!plane || (reinterpret_cast<uintptr_t>(plane) & low) != 0) return KIFS_ERR_BAD_ARG;
    if (pitch < size_t(width) * texel_bytes || (pitch & low) != 0 || pitch / texel_bytes > 0xffffffffull) return KIFS_ERR_BAD_ARG;
    if ((stride & low) != 0 || stride / texel_bytes > 0xffffffffull) return KIFS_ERR_BAD_ARG;
    if (count > 1 && stride < rows * pitch) return KIFS_ERR_BAD_ARG;
    return KIFS_OK;
}

// The launch step of the two calls below.
static hipError_t launch_render(const Params& A, uint32_t group, uint32_t primitive, hipStream_t stream, void*) {
    return launch_accumulate_render(A, group, primitive, stream);
}

}  // namespace accum
}  // namespace kifs

extern "C" int kifs_render_accumulate_async(kifs_ctx* c, void* hip_stream, int count, int samples, const KifsCameraUniform* cameras,
                                            const KifsOptionsUniform* options, uint8_t* const* dev_outs, size_t pitch, int y0,
                                            int y1, int encode) {
    using namespace kifs;
    if (const int st = accum::check(c, count, samples, cameras, options, dev_outs, pitch, y0, y1, encode); st != KIFS_OK) return st;
    return anim::launch_scenes(c, hip_stream, anim::SceneLaunch{count, samples, cameras, options, nullptr, dev_outs, pitch, y0, y1, encode,
                                                                KIFS_KERNEL_ACCUMULATE, accum::launch_render, nullptr,
                                                                accum::WORKGROUPS_PER_ENTRY});
}

extern "C" int kifs_render_accumulate_jittered_async(kifs_ctx* c, void* hip_stream, int count, int samples,
                                                     const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid,
                                                     const KifsSubpixel* cells, uint8_t* const* dev_outs, size_t pitch, int y0,
                                                     int y1, int encode) {
    using namespace kifs;
    if (const int st = accum::check(c, count, samples, cameras, options, dev_outs, pitch, y0, y1, encode); st != KIFS_OK) return st;
    const accum::Jitter jitter{grid, cells};
    if (const int st = accum::check_jitter(c, count, samples, jitter); st != KIFS_OK) return st;
    return anim::launch_scenes(c, hip_stream, anim::SceneLaunch{count, samples, cameras, options, &jitter, dev_outs, pitch, y0, y1, encode,
                                                                KIFS_KERNEL_ACCUMULATE, accum::launch_render, nullptr,
                                                                accum::WORKGROUPS_PER_ENTRY});
}
