// kifs_accumulate.cpp -- the host side of accumulated frames (kifs_render_accumulate_async, include/kifs_hip.h): the
// argument checks, the sub-frames laid out as the views of one launch (view f * samples + s is sub-frame s of output
// frame f and carries that frame's destination), a scene record per view in a slot of the scene-table ring that
// kifs_render_animation_async uses (filled with the context's scene when the caller gives no options: the kernel has one
// path), the view-table ring beyond MAX_BATCH_INLINE views, view 0's options standing in for the context's for the
// length of a call, and the one launch (launch_accumulate_render, kifs_accumulate_kernels.hip).
// kifs_render_accumulate_jittered_async is the same call with a cell of a g x g grid inside the pixel per sub-frame (a
// Jitter: null for the unjittered call): the cell travels in pad[0] of the view's scene record, the grid as the launch's
// FrameParams::ssaa, and the launcher takes the jitter kernel from g = 2.
#include <cstring>
#include <vector>

#include "kifs_context.hpp"

namespace kifs {
namespace accum {

// (Jitter, check, check_jitter and enqueue are declared in kifs_context.hpp: kifs_progressive.cpp shares them.)
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

int enqueue(kifs_ctx* c, hipStream_t stream, int count, int samples, const KifsCameraUniform* cameras,
            const KifsOptionsUniform* options, const Jitter* jitter, uint8_t* const* outs, size_t pitch, int y0, int y1, int encode,
            LaunchFn launch, void* user) {
    host::hip_ok(hipGetLastError(), "stale error before enqueue");
    const int views = count * samples;
    Params A;
    FrameParams& P = A.B.frame;
    if (const int st = host::fill_params(c, &P); st != KIFS_OK) return st;  // (view 0's options: OptionsOfFrame0)
    const int h = P.y1;  // the frame's height
    A.B.count = views;
    A.B.table = nullptr;
    A.frames = count;
    A.samples = samples;
    P.y0 = y0;
    P.y1 = y1;
    P.encode = encode;
    P.pitch_words = outs ? uint32_t(pitch >> 2) : 0u;
    P.out = outs ? reinterpret_cast<uint32_t*>(outs[0]) : nullptr;
    // whole rays, one kernel form for every scene: no costs, no diagnostics, no rounds, the plain orbit trip
    P.tile_cost = nullptr;
    P.counters = nullptr;
    P.round_steps = 0;
    P.workgroups_per_cu = 0;
    P.orbit_x2 = 0;
    // (the context's own factor is 1: check)  A grid of 1 is the unjittered call: its kernel, zero pad words.
    const int grid = jitter ? jitter->grid : 1;
    P.ssaa = grid;
    P.ssaa_inv_height = 1.0f / (float(grid) * c->screen.height);  // as fill_params computes a supersampled launch's
    if (options) host::julia_culls_of_frames(c, P, options, views);  // (fill_params certified view 0's constant alone)
    if (y1 == y0) return KIFS_OK;

    const bool big = views > MAX_BATCH_INLINE;
    int vs = -1, ss = -1;
    if (big)
        if (const int st = host::take_view_slot(c, &vs); st != KIFS_OK) return st;
    std::vector<uint8_t*> view_outs(size_t(views), nullptr);  // every sub-frame of a frame carries the frame's destination
    for (int v = 0; outs && v < views; ++v) view_outs[size_t(v)] = outs[v / samples];
    host::fill_views(c, P, big ? c->h_views[vs] : A.B.view, views, cameras, view_outs.data());
    if (const int st = anim::take_scene_slot(c, &ss); st != KIFS_OK) return st;
    anim::SceneView* const scenes = static_cast<anim::SceneView*>(c->h_scenes[ss]);
    for (int v = 0; v < views; ++v) {
        const KifsOptionsUniform& o = options ? options[v] : c->options;
        anim::SceneView& s = scenes[v];
        s.c = {o.constant[0], o.constant[1], o.constant[2], o.constant[3]};
        s.power = o.power;
        s.fractal_color = {o.fractal_color[0], o.fractal_color[1], o.fractal_color[2]};
        s.background_color = {o.background_color[0], o.background_color[1], o.background_color[2]};
        s.background_rgba = host::background_pixel(c, s.background_color, encode);  // (not read: a miss is averaged too)
        std::memset(s.pad, 0, sizeof s.pad);
        if (grid > 1) {  // the view's cell: pad[0] = i | j << 8
            const int n = v % samples;
            const KifsSubpixel cell = jitter->cells ? jitter->cells[v] : KifsSubpixel{uint8_t(n % grid), uint8_t(n / grid)};
            s.pad[0] = uint32_t(cell.i) | uint32_t(cell.j) << 8;
        }
    }
    P.background_rgba = scenes[0].background_rgba;

    TileTable* const tt = host::tile_table(c, P.width, h, y0, y1);
    if (!tt) return KIFS_ERR_RUNTIME;
    // four workgroups per entry of the order and output frame: the grid's one dimension must hold them
    if (uint64_t(tt->count) * 4u * uint64_t(count) > 0x7fffffffull) return KIFS_ERR_BAD_SIZE;
    if (const int st = anim::follow_stream_change(tt, stream); st != KIFS_OK) return st;
    P.tile_order = tt->d_order;
    P.tile_count = tt->count;

    if (big) {
        if (!host::hip_ok(hipMemcpyAsync(c->d_views[vs], c->h_views[vs], sizeof(BatchView) * size_t(views), hipMemcpyHostToDevice, stream),
                          "copy(view table)"))
            return KIFS_ERR_RUNTIME;
        A.B.table = c->d_views[vs];
    }
    if (!host::hip_ok(hipMemcpyAsync(c->d_scenes[ss], scenes, sizeof(anim::SceneView) * size_t(views), hipMemcpyHostToDevice, stream),
                      "copy(scene table)"))
        return KIFS_ERR_RUNTIME;
    A.scenes = static_cast<const anim::SceneView*>(c->d_scenes[ss]);
    c->last_round_steps = 0;
    c->last_group_tiles = -1;
    c->last_bunny_form = -1;
    c->last_kernel = KIFS_KERNEL_ACCUMULATE;
    const KifsOptionsUniform& first = options ? options[0] : c->options;
    const bool launched = host::hip_ok(launch(A, first.fractal_group_id, first.primitive_id, stream, user),
                                       "accumulate render_kernel launch");
    // (also after a failed launch: the copies above are enqueued and read the pinned images)
    bool marked = host::hip_ok(hipEventRecord(c->scenes_used[ss], stream), "record(scene table)");
    c->scenes_busy[ss] = true;
    if (big) {
        marked = host::hip_ok(hipEventRecord(c->views_used[vs], stream), "record(view table)") && marked;
        c->views_busy[vs] = true;
    }
    return launched && marked ? KIFS_OK : KIFS_ERR_RUNTIME;
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
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    anim::OptionsOfFrame0 scope(c, options ? options[0] : c->options);
    return accum::enqueue(c, s, count, samples, cameras, options, nullptr, dev_outs, pitch, y0, y1, encode, accum::launch_render,
                          nullptr);
}

extern "C" int kifs_render_accumulate_jittered_async(kifs_ctx* c, void* hip_stream, int count, int samples,
                                                     const KifsCameraUniform* cameras, const KifsOptionsUniform* options, int grid,
                                                     const KifsSubpixel* cells, uint8_t* const* dev_outs, size_t pitch, int y0,
                                                     int y1, int encode) {
    using namespace kifs;
    if (const int st = accum::check(c, count, samples, cameras, options, dev_outs, pitch, y0, y1, encode); st != KIFS_OK) return st;
    const accum::Jitter jitter{grid, cells};
    if (const int st = accum::check_jitter(c, count, samples, jitter); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    anim::OptionsOfFrame0 scope(c, options ? options[0] : c->options);
    return accum::enqueue(c, s, count, samples, cameras, options, &jitter, dev_outs, pitch, y0, y1, encode, accum::launch_render,
                          nullptr);
}
