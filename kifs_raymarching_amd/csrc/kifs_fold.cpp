// kifs_fold.cpp -- the host side of kaleidoscopic IFS scenes (kifs_render_folded_async and kifs_eval_fold,
// include/kifs_hip.h): the argument checks, a BatchParams filled the way kifs_trap.cpp fills its launch's -- frame
// constants, views, destination, the band's tile table, the fixed launch shape -- WITH EVERY CULL OFF, the light, the
// optional term and the fold system beside it, and one launch of fold::render_kernel (kifs_fold_kernels.hip).  Like the
// lit call it is not a feedback launch: it reads the band's tile order where the plain launches left it, records no
// costs, moves no sort, touches no profiling record and leaves the kifs_debug_last_* values as they were.
#include <cmath>

#include "kifs_context.hpp"

namespace kifs {
namespace fold {

static_assert(KIFS_MAX_FOLD_BATCH == MAX_BATCH_INLINE, "the views of a call travel in the kernel argument");
static_assert(sizeof(KifsFoldSystem) == 60, "the record is 60 bytes");
static_assert(KIFS_FOLD_ABS == ABS && KIFS_FOLD_SORT == SORT && KIFS_FOLD_TETRA == TETRA && KIFS_FOLD_ROTATE == ROTATE &&
                  KIFS_FOLD_MIRROR_Z == MIRROR_Z,
              "the stage bits travel as they are given");

static const KifsLight REFERENCE_LIGHT = {{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 0};

// What a caller can get wrong that needs no look at the frame.
static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, const KifsFoldSystem* fold,
                 const KifsLight* light, const KifsAmbientOcclusion* ao, int encode) {
    if (!c || !outs || !fold) return KIFS_ERR_BAD_ARG;
    if (!fold_ok(*fold)) return KIFS_ERR_BAD_ARG;
    if (light && !light::light_ok(*light)) return KIFS_ERR_BAD_ARG;  // NULL: the reference's light
    if (ao && !occl::term_ok(*ao)) return KIFS_ERR_BAD_ARG;
    if (count < 1 || count > KIFS_MAX_FOLD_BATCH) return KIFS_ERR_BAD_ARG;
    if (!cameras && count != 1) return KIFS_ERR_BAD_ARG;  // NULL: the context's camera, one frame
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    if (c->options.fractal_group_id != uint32_t(KIFS_GROUP_KIFS)) return KIFS_ERR_BAD_ARG;  // no folded Julia pipelines
    return KIFS_OK;
}

static int enqueue(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, size_t pitch,
                   const KifsFoldSystem& fold, const KifsLight& light, const KifsAmbientOcclusion* ao, int y0, int y1, int encode) {
    host::hip_ok(hipGetLastError(), "stale error before enqueue");
    Params O;
    FrameParams& P = O.B.frame;
    int st, rw, rh;
    if ((st = host::fill_params(c, &P)) != KIFS_OK) return st;      // (ssaa and ssaa_inv_height: the context's factor)
    if ((st = host::render_dims(c, &rw, &rh)) != KIFS_OK) return st;  // (the virtual screen of a supersampled launch)
    culls_off(P);
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
    O.fold = device_fold(fold);
    if (!host::order_around(tt, stream, true)) return KIFS_ERR_RUNTIME;
    if (!host::hip_ok(launch_folded(O, c->options.fractal_group_id, c->options.primitive_id, stream), "folded render_kernel launch"))
        return KIFS_ERR_RUNTIME;
    return host::order_around(tt, stream, false) ? KIFS_OK : KIFS_ERR_RUNTIME;
}

}  // namespace fold
}  // namespace kifs

extern "C" int kifs_render_folded_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                        uint8_t* const* dev_outs, size_t pitch, const KifsFoldSystem* fold, const KifsLight* light,
                                        const KifsAmbientOcclusion* ao, int y0, int y1, int encode) {
    using namespace kifs;
    if (const int st = fold::check(c, count, cameras, dev_outs, fold, light, ao, encode); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return fold::enqueue(c, s, count, cameras, dev_outs, pitch, *fold, light ? *light : fold::REFERENCE_LIGHT, ao, y0, y1, encode);
}

// Host pointers, like kifs_eval_points: the positions go up, one launch of fold::eval_kernel, the values come back.
extern "C" int kifs_eval_fold(kifs_ctx* c, const KifsFoldSystem* fold, const float* pts, int n, float* sdf_out, float* nrm_out) {
    using namespace kifs;
    if (!c || !fold || !pts || n < 0) return KIFS_ERR_BAD_ARG;
    if (!fold::fold_ok(*fold)) return KIFS_ERR_BAD_ARG;
    if (!c->have_options) return KIFS_ERR_UNCONFIGURED;
    if (c->options.fractal_group_id != uint32_t(KIFS_GROUP_KIFS)) return KIFS_ERR_BAD_ARG;
    if (n == 0 || (!sdf_out && !nrm_out)) return KIFS_OK;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    fold::EvalParams E;
    const KifsScreenUniform saved_screen = c->screen;  // options-only evaluation: any valid screen does
    c->screen = {1.0f, 1.0f, 1.0f};
    const int st = host::fill_params(c, &E.frame);
    c->screen = saved_screen;
    if (st != KIFS_OK) return st;
    E.fold = fold::device_fold(*fold);
    E.n = n;
    float *d_pts = nullptr, *d_sdf = nullptr, *d_nrm = nullptr;
    int rc = KIFS_ERR_RUNTIME;
    const size_t nb = size_t(n) * sizeof(float);
    do {
        if (hipMalloc(reinterpret_cast<void**>(&d_pts), 3 * nb) != hipSuccess) break;
        if (sdf_out && hipMalloc(reinterpret_cast<void**>(&d_sdf), nb) != hipSuccess) break;
        if (nrm_out && hipMalloc(reinterpret_cast<void**>(&d_nrm), 3 * nb) != hipSuccess) break;
        if (hipMemcpyAsync(d_pts, pts, 3 * nb, hipMemcpyHostToDevice, c->stream) != hipSuccess) break;
        E.points = d_pts;
        E.sdf = d_sdf;
        E.normal = d_nrm;
        if (launch_eval_fold(E, c->options.fractal_group_id, c->options.primitive_id, c->stream) != hipSuccess) break;
        if (sdf_out && hipMemcpyAsync(sdf_out, d_sdf, nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) break;
        if (nrm_out && hipMemcpyAsync(nrm_out, d_nrm, 3 * nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) break;
        rc = KIFS_OK;
    } while (0);
    if (d_pts) (void)hipFree(d_pts);
    if (d_sdf) (void)hipFree(d_sdf);
    if (d_nrm) (void)hipFree(d_nrm);
    return rc;
}
