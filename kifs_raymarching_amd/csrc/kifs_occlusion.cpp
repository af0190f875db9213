// kifs_occlusion.cpp -- the host side of ambient occlusion (kifs_render_occlusion_async, include/kifs_hip.h): the
// argument checks, a BatchParams filled the way enqueue_batch fills a supersampled launch's -- frame constants, views,
// destination, the band's tile table, the fixed launch shape -- the term and the plane beside it, and one launch of
// occl::render_kernel (kifs_occlusion_kernels.hip).  It is not a feedback launch: it reads the band's tile order where the
// plain launches left it, records no costs, moves no sort, touches no profiling record and leaves the kifs_debug_last_*
// values as they were.
#include <cmath>

#include "kifs_context.hpp"

namespace kifs {
namespace occl {

static_assert(KIFS_MAX_OCCLUSION_BATCH == MAX_BATCH_INLINE, "the views of a call travel in the kernel argument");

// What a caller can get wrong that needs no look at the frame.
static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, const KifsAmbientOcclusion* ao,
                 const float* plane, int encode) {
    if (!c || !outs || !ao) return KIFS_ERR_BAD_ARG;
    if (!term_ok(*ao)) return KIFS_ERR_BAD_ARG;
    if (count < 1 || count > KIFS_MAX_OCCLUSION_BATCH) return KIFS_ERR_BAD_ARG;
    if (!cameras && count != 1) return KIFS_ERR_BAD_ARG;  // NULL: the context's camera, one frame
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (plane && c->supersampling > 1) return KIFS_ERR_BAD_ARG;  // a resolved pixel has no single factor
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    return KIFS_OK;
}

// The plane's layout: 4-byte texels, rows of a band packed, one plane per view `stride` bytes apart.
static int check_plane(const float* plane, size_t pitch, size_t stride, int width, size_t rows, int count) {
    if (!plane) return KIFS_OK;
    if ((reinterpret_cast<uintptr_t>(plane) & 3u) != 0 || pitch < size_t(width) * 4 || (pitch & 3u) != 0 || (stride & 3u) != 0 ||
        (count > 1 && stride < rows * pitch) || (pitch >> 2) > 0xffffffffull || (stride >> 2) > 0xffffffffull)
        return KIFS_ERR_BAD_ARG;
    return KIFS_OK;
}

static int enqueue(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, size_t pitch,
                   const KifsAmbientOcclusion& ao, float* plane, size_t plane_pitch, size_t plane_stride, int y0, int y1, int encode) {
    host::hip_ok(hipGetLastError(), "stale error before enqueue");
    Params O;
    FrameParams& P = O.B.frame;
    int st, rw, rh;
    if ((st = host::fill_params(c, &P)) != KIFS_OK) return st;      // (ssaa and ssaa_inv_height: the context's factor)
    if ((st = host::render_dims(c, &rw, &rh)) != KIFS_OK) return st;  // (the virtual screen of a supersampled launch)
    O.B.count = count;
    O.B.table = nullptr;
    const int h = P.y1;  // the frame's height
    if ((st = host::set_destination(c, P, count, outs[0], pitch, y0, y1, encode, false, nullptr, 0, 0)) != KIFS_OK) return st;
    if ((st = check_plane(plane, plane_pitch, plane_stride, P.width, size_t(y1 - y0), count)) != KIFS_OK) return st;
    host::fill_views(c, P, O.B.view, count, cameras, outs);
    if (y1 == y0) return KIFS_OK;
    TileTable* tt = host::tile_table(c, P.width, h, y0, y1);
    if (!tt) return KIFS_ERR_RUNTIME;
    P.tile_order = tt->d_order;
    P.tile_count = tt->count;
    // the fixed shape of a geometry or supersampled launch: whole rays, no costs, no diagnostics, no residency cap
    P.tile_cost = nullptr;
    P.counters = nullptr;
    P.round_steps = 0;
    P.workgroups_per_cu = 0;
    O.ao = AO{ao.samples, ao.step, ao.decay, ao.strength};
    O.plane = plane;
    O.pitch_words = uint32_t(plane_pitch >> 2);
    O.stride_words = uint32_t(plane_stride >> 2);
    if (!host::order_around(tt, stream, true)) return KIFS_ERR_RUNTIME;
    if (!host::hip_ok(launch_occlusion(O, c->options.fractal_group_id, c->options.primitive_id, stream), "occlusion render_kernel launch"))
        return KIFS_ERR_RUNTIME;
    return host::order_around(tt, stream, false) ? KIFS_OK : KIFS_ERR_RUNTIME;
}

}  // namespace occl
}  // namespace kifs

extern "C" int kifs_render_occlusion_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                           uint8_t* const* dev_outs, size_t pitch, const KifsAmbientOcclusion* ao,
                                           float* dev_occlusion, size_t occlusion_pitch, size_t occlusion_stride, int y0, int y1,
                                           int encode) {
    using namespace kifs;
    if (const int st = occl::check(c, count, cameras, dev_outs, ao, dev_occlusion, encode); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return occl::enqueue(c, s, count, cameras, dev_outs, pitch, *ao, dev_occlusion, occlusion_pitch, occlusion_stride, y0, y1, encode);
}
