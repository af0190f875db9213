// kifs_fold_trap.cpp -- the host side of orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async and
// kifs_eval_fold_trap, include/kifs_hip.h): the argument checks of the folded and the trapped call and the occlusion
// call's of a plane, a BatchParams filled the way kifs_fold.cpp fills its launch's -- frame constants, views, destination,
// the band's tile table, the fixed launch shape, EVERY CULL OFF -- the light and the optional term beside it, and one
// launch of foldorbit::render_kernel (kifs_fold_trap_kernels.hip).  The fold system and the trap do not fit into the kernel
// argument beside them: they go through a slot of the context's scene-table ring (kifs_animation.cpp) -- written into the
// slot's pinned image, copied to its device record on the launch's stream before the launch, the slot's event recorded
// behind the launch.  Like the folded call it is not a feedback launch: it reads the band's tile order where the plain
// launches left it, records no costs, moves no sort, touches no profiling record and leaves the kifs_debug_last_* values
// as they were.
#include <cmath>
#include <cstring>

#include "kifs_context.hpp"

namespace kifs {
namespace foldorbit {

static_assert(KIFS_MAX_FOLD_TRAP_BATCH == MAX_BATCH_INLINE, "the views of a call travel in the kernel argument");
static_assert(sizeof(Record) <= kifs_ctx::SCENE_SLOT_BYTES, "a ring slot holds the record");

static const KifsLight REFERENCE_LIGHT = {{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 0};

// What a caller can get wrong that needs no look at the frame.
static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, const KifsFoldSystem* fold,
                 const KifsOrbitTrap* trap, const KifsLight* light, const KifsAmbientOcclusion* ao, const float* plane, int encode) {
    if (!c || !outs || !fold || !trap) return KIFS_ERR_BAD_ARG;
    if (!fold::fold_ok(*fold) || !trap::trap_ok(*trap)) return KIFS_ERR_BAD_ARG;
    if (light && !light::light_ok(*light)) return KIFS_ERR_BAD_ARG;  // NULL: the reference's light
    if (ao && !occl::term_ok(*ao)) return KIFS_ERR_BAD_ARG;
    if (count < 1 || count > KIFS_MAX_FOLD_TRAP_BATCH) return KIFS_ERR_BAD_ARG;
    if (!cameras && count != 1) return KIFS_ERR_BAD_ARG;  // NULL: the context's camera, one frame
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (plane && c->supersampling > 1) return KIFS_ERR_BAD_ARG;  // a resolved pixel has no single u
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    if (c->options.fractal_group_id != uint32_t(KIFS_GROUP_KIFS)) return KIFS_ERR_BAD_ARG;  // no folded Julia pipelines
    return KIFS_OK;
}

// The plane's layout, as the occlusion call's: 4-byte texels, rows of a band packed, one plane per view `stride` bytes apart.
static int check_plane(const float* plane, size_t pitch, size_t stride, int width, size_t rows, int count) {
    if (!plane) return KIFS_OK;
    if ((reinterpret_cast<uintptr_t>(plane) & 3u) != 0 || pitch < size_t(width) * 4 || (pitch & 3u) != 0 || (stride & 3u) != 0 ||
        (count > 1 && stride < rows * pitch) || (pitch >> 2) > 0xffffffffull || (stride >> 2) > 0xffffffffull)
        return KIFS_ERR_BAD_ARG;
    return KIFS_OK;
}

static int enqueue(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, size_t pitch,
                   const KifsFoldSystem& fold, const KifsOrbitTrap& trap, const KifsLight& light, const KifsAmbientOcclusion* ao,
                   float* plane, size_t plane_pitch, size_t plane_stride, int y0, int y1, int encode) {
    host::hip_ok(hipGetLastError(), "stale error before enqueue");
    Params O;
    FrameParams& P = O.B.frame;
    int st, rw, rh;
    if ((st = host::fill_params(c, &P)) != KIFS_OK) return st;      // (ssaa and ssaa_inv_height: the context's factor)
    if ((st = host::render_dims(c, &rw, &rh)) != KIFS_OK) return st;  // (the virtual screen of a supersampled launch)
    fold::culls_off(P);
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
    O.light = light::device_light(light);
    O.ao = ao ? occl::AO{ao->samples, ao->step, ao->decay, ao->strength} : occl::AO{0, 0.0f, 0.0f, 0.0f};
    O.has_ao = ao ? 1u : 0u;
    O.plane = plane;
    O.pitch_words = uint32_t(plane_pitch >> 2);
    O.stride_words = uint32_t(plane_stride >> 2);
    // the record: the slot's pinned image, then its device record on the launch's stream, before the launch
    int ss = -1;
    if ((st = anim::take_scene_slot(c, &ss)) != KIFS_OK) return st;
    Record* const image = static_cast<Record*>(c->h_scenes[ss]);
    std::memset(image, 0, sizeof(Record));
    image->fold = fold::device_fold(fold);
    image->trap = trap::device_trap(trap);
    if (!host::order_around(tt, stream, true)) return KIFS_ERR_RUNTIME;
    if (!host::hip_ok(hipMemcpyAsync(c->d_scenes[ss], image, sizeof(Record), hipMemcpyHostToDevice, stream), "copy(fold and trap record)"))
        return KIFS_ERR_RUNTIME;  // (nothing enqueued reads the image)
    O.record = static_cast<const Record*>(c->d_scenes[ss]);
    const bool launched =
        host::hip_ok(launch_folded_trapped(O, c->options.fractal_group_id, c->options.primitive_id, stream), "folded trapped render_kernel launch");
    // (also after a failed launch: the copy above is enqueued and reads the pinned image)
    const bool marked = anim::mark_scene_slot(c, ss, stream);
    if (!launched || !marked) return KIFS_ERR_RUNTIME;
    return host::order_around(tt, stream, false) ? KIFS_OK : KIFS_ERR_RUNTIME;
}

}  // namespace foldorbit
}  // namespace kifs

extern "C" int kifs_render_folded_trapped_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                                uint8_t* const* dev_outs, size_t pitch, const KifsFoldSystem* fold,
                                                const KifsOrbitTrap* trap, const KifsLight* light, const KifsAmbientOcclusion* ao,
                                                float* dev_trap_u, size_t u_pitch, size_t u_stride, int y0, int y1, int encode) {
    using namespace kifs;
    if (const int st = foldorbit::check(c, count, cameras, dev_outs, fold, trap, light, ao, dev_trap_u, encode); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    return foldorbit::enqueue(c, s, count, cameras, dev_outs, pitch, *fold, *trap, light ? *light : foldorbit::REFERENCE_LIGHT, ao,
                             dev_trap_u, u_pitch, u_stride, y0, y1, encode);
}

// Host pointers, like kifs_eval_trap: the positions go up, one launch of foldorbit::eval_kernel, the u come back.  The two
// records fit into this kernel's argument.
extern "C" int kifs_eval_fold_trap(kifs_ctx* c, const KifsFoldSystem* fold, const KifsOrbitTrap* trap, const float* pts, int n,
                                   float* u_out) {
    using namespace kifs;
    if (!c || !fold || !trap || !pts || !u_out || n < 0) return KIFS_ERR_BAD_ARG;
    if (!fold::fold_ok(*fold) || !trap::orbit_ok(*trap)) return KIFS_ERR_BAD_ARG;
    if (!c->have_options) return KIFS_ERR_UNCONFIGURED;
    if (c->options.fractal_group_id != uint32_t(KIFS_GROUP_KIFS)) return KIFS_ERR_BAD_ARG;
    if (n == 0) return KIFS_OK;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    foldorbit::EvalParams E;
    const KifsScreenUniform saved_screen = c->screen;  // options-only evaluation: any valid screen does
    c->screen = {1.0f, 1.0f, 1.0f};
    const int st = host::fill_params(c, &E.frame);
    c->screen = saved_screen;
    if (st != KIFS_OK) return st;
    E.fold = fold::device_fold(*fold);
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
        if (launch_eval_fold_trap(E, c->options.fractal_group_id, c->options.primitive_id, c->stream) != hipSuccess) break;
        if (hipMemcpyAsync(u_out, d_u, nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) break;
        rc = KIFS_OK;
    } while (0);
    if (d_pts) (void)hipFree(d_pts);
    if (d_u) (void)hipFree(d_u);
    return rc;
}
