// kifs_trap.cpp -- the host side of orbit-trap surface colouring (kifs_render_trapped_async and kifs_eval_trap,
// include/kifs_hip.h): the argument checks, a BatchParams filled the way kifs_lighting.cpp fills its launch's -- frame
// constants, views, destination, the band's tile table, the fixed launch shape -- the light, the optional term and the
// trap beside it, and one launch of trap::render_kernel (kifs_trap_kernels.hip).  Like the lit call it is not a feedback
// launch: it reads the band's tile order where the plain launches left it, records no costs, moves no sort, touches no
// profiling record and leaves the kifs_debug_last_* values as they were.
#include <cmath>

#include "kifs_context.hpp"

namespace kifs {
namespace trap {

static_assert(KIFS_MAX_TRAP_BATCH == MAX_BATCH_INLINE, "the views of a call travel in the kernel argument");
static_assert(sizeof(KifsOrbitTrap) == sizeof(Trap), "the record travels as it is given");

static const KifsLight REFERENCE_LIGHT = {{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 0};

// What a caller can get wrong that needs no look at the frame.
static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, const KifsOrbitTrap* trap,
                 const KifsLight* light, const KifsAmbientOcclusion* ao, int encode) {
    if (!c || !outs || !trap) return KIFS_ERR_BAD_ARG;
    if (!trap_ok(*trap)) return KIFS_ERR_BAD_ARG;
    if (light && !light::light_ok(*light)) return KIFS_ERR_BAD_ARG;  // NULL: the reference's light
    if (ao && !occl::term_ok(*ao)) return KIFS_ERR_BAD_ARG;
    if (count < 1 || count > KIFS_MAX_TRAP_BATCH) return KIFS_ERR_BAD_ARG;
    if (!cameras && count != 1) return KIFS_ERR_BAD_ARG;  // NULL: the context's camera, one frame
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    return KIFS_OK;
}

static int enqueue(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, size_t pitch,
                   const KifsOrbitTrap& trap, const KifsLight& light, const KifsAmbientOcclusion* ao, int y0, int y1, int encode) {
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
    O.light = light::device_light(light);
    O.ao = ao ? occl::AO{ao->samples, ao->step, ao->decay, ao->strength} : occl::AO{0, 0.0f, 0.0f, 0.0f};
    O.has_ao = ao ? 1u : 0u;
    O.trap = device_trap(trap);
    if (!host::order_around(tt, stream, true)) return KIFS_ERR_RUNTIME;
    if (!host::hip_ok(launch_trapped(O, c->options.fractal_group_id, c->options.primitive_id, stream), "trapped render_kernel launch"))
        return KIFS_ERR_RUNTIME;
    return host::order_around(tt, stream, false) ? KIFS_OK : KIFS_ERR_RUNTIME;
}

}  // namespace trap
}  // namespace kifs

extern "C" int kifs_render_trapped_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                         uint8_t* const* dev_outs, size_t pitch, const KifsOrbitTrap* trap, const KifsLight* light,
                                         const KifsAmbientOcclusion* ao, int y0, int y1, int encode) {
    using namespace kifs;
    if (const int st = trap::check(c, count, cameras, dev_outs, trap, light, ao, encode); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return trap::enqueue(c, s, count, cameras, dev_outs, pitch, *trap, light ? *light : trap::REFERENCE_LIGHT, ao, y0, y1, encode);
}

// Host pointers, like kifs_eval_points: the positions go up, one launch of trap::eval_kernel, the u come back.
extern "C" int kifs_eval_trap(kifs_ctx* c, const KifsOrbitTrap* trap, const float* pts, int n, float* u_out) {
    using namespace kifs;
    if (!c || !trap || !pts || !u_out || n < 0) return KIFS_ERR_BAD_ARG;
    if (!trap::orbit_ok(*trap)) return KIFS_ERR_BAD_ARG;
    if (!c->have_options) return KIFS_ERR_UNCONFIGURED;
    if (n == 0) return KIFS_OK;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    trap::EvalParams E;
    const KifsScreenUniform saved_screen = c->screen;  // options-only evaluation: any valid screen does
    c->screen = {1.0f, 1.0f, 1.0f};
    const int st = host::fill_params(c, &E.frame);
    c->screen = saved_screen;
    if (st != KIFS_OK) return st;
    E.trap = trap::device_trap(*trap);
    E.n = n;
    float *d_pts = nullptr, *d_u = nullptr;
    int rc = KIFS_ERR_RUNTIME;
    const size_t nb = size_t(n) * sizeof(float);
    do {
        if (hipMalloc(reinterpret_cast<void**>(&d_pts), 3 * nb) != hipSuccess) break;
        if (hipMalloc(reinterpret_cast<void**>(&d_u), nb) != hipSuccess) break;
        if (hipMemcpyAsync(d_pts, pts, 3 * nb, hipMemcpyHostToDevice, c->stream) != hipSuccess) break;
        E.points = d_pts;
        E.u = d_u;
        if (launch_eval_trap(E, c->options.fractal_group_id, c->options.primitive_id, c->stream) != hipSuccess) break;
        if (hipMemcpyAsync(u_out, d_u, nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) break;
        rc = KIFS_OK;
    } while (0);
    if (d_pts) (void)hipFree(d_pts);
    if (d_u) (void)hipFree(d_u);
    return rc;
}
