// kifs_lighting.cpp -- the host side of the configurable light (kifs_render_lit_async, include/kifs_hip.h): the argument
// checks, a BatchParams filled the way kifs_occlusion.cpp fills its launch's -- frame constants, views, destination, the
// band's tile table, the fixed launch shape -- the light and the optional term beside it, and one launch of
// light::render_kernel (kifs_lighting_kernels.hip).  Like the occlusion call it is not a feedback launch: it reads the
// band's tile order where the plain launches left it, records no costs, moves no sort, touches no profiling record and
// leaves the kifs_debug_last_* values as they were.
#include <cmath>

#include "kifs_context.hpp"

namespace kifs {
namespace light {

static_assert(KIFS_MAX_LIGHT_BATCH == MAX_BATCH_INLINE, "the views of a call travel in the kernel argument");

// (light_ok and device_light -- the ranges of KifsLight, the light as the kernel reads it -- are kifs_context.hpp's, shared
// with kifs_trap.cpp.)

// What a caller can get wrong that needs no look at the frame.
static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, const KifsLight* light,
                 const KifsAmbientOcclusion* ao, int encode) {
    if (!c || !outs || !light) return KIFS_ERR_BAD_ARG;
    if (!light_ok(*light)) return KIFS_ERR_BAD_ARG;
    if (ao && !occl::term_ok(*ao)) return KIFS_ERR_BAD_ARG;
    if (count < 1 || count > KIFS_MAX_LIGHT_BATCH) return KIFS_ERR_BAD_ARG;
    if (!cameras && count != 1) return KIFS_ERR_BAD_ARG;  // NULL: the context's camera, one frame
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    return KIFS_OK;
}

static int enqueue(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, size_t pitch,
                   const KifsLight& light, const KifsAmbientOcclusion* ao, int y0, int y1, int encode) {
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
    O.light = device_light(light);
    O.ao = ao ? occl::AO{ao->samples, ao->step, ao->decay, ao->strength} : occl::AO{0, 0.0f, 0.0f, 0.0f};
    O.has_ao = ao ? 1u : 0u;
    if (!host::order_around(tt, stream, true)) return KIFS_ERR_RUNTIME;
    if (!host::hip_ok(launch_lit(O, c->options.fractal_group_id, c->options.primitive_id, stream), "lit render_kernel launch"))
        return KIFS_ERR_RUNTIME;
    return host::order_around(tt, stream, false) ? KIFS_OK : KIFS_ERR_RUNTIME;
}

}  // namespace light
}  // namespace kifs

extern "C" int kifs_render_lit_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                     uint8_t* const* dev_outs, size_t pitch, const KifsLight* light, const KifsAmbientOcclusion* ao,
                                     int y0, int y1, int encode) {
    using namespace kifs;
    if (const int st = light::check(c, count, cameras, dev_outs, light, ao, encode); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return light::enqueue(c, s, count, cameras, dev_outs, pitch, *light, ao, y0, y1, encode);
}
