// kifs_animation.cpp -- the host side of animated batches (kifs_render_animation_async, include/kifs_hip.h) and the launch
// path of every call that carries a scene table (launch_scenes: the animated call and the accumulated ones of
// kifs_accumulate.cpp, kifs_progressive.cpp and kifs_converge.cpp): the ring of scene tables (device table, pinned image,
// event per slot), the view-table ring it shares with kifs_render_batch_async beyond MAX_BATCH_INLINE views, view 0's
// options standing in for the context's for the length of a call, and the one launch, whose last step the caller
// brings (the animated call's: launch_animation_render, kifs_animation_kernels.hip).  No launcher is named by the path.
#include <cstring>

#include "kifs_context.hpp"

namespace kifs {
namespace anim {

// The fields every frame of a launch shares: one pipeline, one march budget.  Bit patterns, not values: -0.0f is not 0.0f
// and a NaN equals itself here.  Padding words are not looked at.
bool same_pipeline(const KifsOptionsUniform& a, const KifsOptionsUniform& b) {
    return a.max_iterations == b.max_iterations && std::memcmp(&a.max_distance, &b.max_distance, sizeof(float)) == 0 &&
           std::memcmp(&a.epsilon, &b.epsilon, sizeof(float)) == 0 && a.is_heatmap == b.is_heatmap &&
           a.fractal_group_id == b.fractal_group_id && a.primitive_id == b.primitive_id;
}

static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
                 uint8_t* const* outs, size_t pitch, int y0, int y1, int encode) {
    if (!c || !options || !outs) return KIFS_ERR_BAD_ARG;
    if (count < 1 || count > MAX_BATCH) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    if (c->supersampling > 1) return KIFS_ERR_BAD_ARG;  // out of scope, as for the geometry output
    if (options[0].fractal_group_id > 2u) return KIFS_ERR_BAD_ARG;
    for (int i = 1; i < count; ++i)
        if (!same_pipeline(options[0], options[i])) return KIFS_ERR_BAD_ARG;
    if (!c->have_screen || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    int w = 0, h = 0;
    if (const int st = host::frame_dims(c, &w, &h); st != KIFS_OK) return st;
    if (y0 < 0 || y1 > h || y0 > y1) return KIFS_ERR_BAD_ARG;
    if (pitch < size_t(w) * 4 || (pitch & 3u) != 0 || (pitch >> 2) > 0xffffffffull) return KIFS_ERR_BAD_SIZE;
    return KIFS_OK;
}

// The next slot of the scene-table ring, as take_view_slot takes one of the view tables: allocated on first use, and
// rewritten only after the launch that last read it is over.
int take_scene_slot(kifs_ctx* c, int* slot) {
    const int ss = *slot = c->scene_slot;
    c->scene_slot = (ss + 1) % kifs_ctx::SCENE_RING;
    // (each part on its own: a slot that a failed allocation left half made is completed when the ring comes round to it)
    if ((!c->d_scenes[ss] && !host::hip_ok(hipMalloc(&c->d_scenes[ss], kifs_ctx::SCENE_SLOT_BYTES), "hipMalloc(scene table)")) ||
        (!c->h_scenes[ss] &&
         !host::hip_ok(hipHostMalloc(&c->h_scenes[ss], kifs_ctx::SCENE_SLOT_BYTES, hipHostMallocDefault), "hipHostMalloc(scene table)")) ||
        (!c->scenes_used[ss] && !host::hip_ok(hipEventCreateWithFlags(&c->scenes_used[ss], hipEventDisableTiming), "hipEventCreate(scene table)")))
        return KIFS_ERR_RUNTIME;
    if (c->scenes_busy[ss] && !host::hip_ok(hipEventSynchronize(c->scenes_used[ss]), "wait(scene table)")) return KIFS_ERR_RUNTIME;
    c->scenes_busy[ss] = false;
    return KIFS_OK;
}

// The event behind the launch that reads the slot (kifs_context.hpp).
bool mark_scene_slot(kifs_ctx* c, int slot, hipStream_t stream) {
    const bool marked = host::hip_ok(hipEventRecord(c->scenes_used[slot], stream), "record(scene table)");
    c->scenes_busy[slot] = true;
    return marked;
}

// A launch on another stream than the tile table's feedback launches follows them, as a geometry launch does
// (feedback_before in kifs_schedule.cpp): the sort rotates the order's two buffers on the understanding that nobody still
// reads the one it writes.  Nothing else of the feedback is touched: no costs, no step of the sort.
static int follow_stream_change(TileTable* tt, hipStream_t stream) {
    if (tt->last_stream && tt->last_stream != stream &&
        (!host::hip_ok(hipEventRecord(tt->stream_left, tt->last_stream), "record(stream change)") ||
         !host::hip_ok(hipStreamWaitEvent(stream, tt->stream_left, 0), "wait(stream change)")))
        return KIFS_ERR_RUNTIME;
    tt->last_stream = stream;
    return KIFS_OK;
}

// The one launch of a SceneLaunch.  The Params are the accumulated calls': a grid of 1 and one sub-frame per frame are
// the animated call's, whose ssaa fields fill_params wrote with the same bits (the context's own factor is 1: check).
static int enqueue(kifs_ctx* c, hipStream_t stream, const SceneLaunch& L) {
    host::hip_ok(hipGetLastError(), "stale error before enqueue");
    const int views = L.frames * L.samples;
    accum::Params A;
    FrameParams& P = A.B.frame;
    if (const int st = host::fill_params(c, &P); st != KIFS_OK) return st;  // (view 0's options: OptionsOfFrame0)
    const int h = P.y1;  // the frame's height
    A.B.count = views;
    A.B.table = nullptr;
    A.frames = L.frames;
    A.samples = L.samples;
    P.y0 = L.y0;
    P.y1 = L.y1;
    P.encode = L.encode;
    P.pitch_words = L.outs ? uint32_t(L.pitch >> 2) : 0u;
    P.out = L.outs ? reinterpret_cast<uint32_t*>(L.outs[0]) : nullptr;
    // whole rays, one kernel form for every scene: no costs, no diagnostics, no rounds, the plain orbit trip
    P.tile_cost = nullptr;
    P.counters = nullptr;
    P.round_steps = 0;
    P.workgroups_per_cu = 0;
    P.orbit_x2 = 0;
    // A grid of 1 is the unjittered call: its kernel, zero pad words.
    const int grid = L.jitter ? L.jitter->grid : 1;
    P.ssaa = grid;
    P.ssaa_inv_height = 1.0f / (float(grid) * c->screen.height);  // as fill_params computes a supersampled launch's
    if (L.options) host::julia_culls_of_frames(c, P, L.options, views);  // (fill_params certified view 0's constant alone)
    if (L.y1 == L.y0) return KIFS_OK;

    const bool big = views > MAX_BATCH_INLINE;
    int vs = -1, ss = -1;
    if (big)
        if (const int st = host::take_view_slot(c, &vs); st != KIFS_OK) return st;
    std::vector<uint8_t*> view_outs(size_t(views), nullptr);  // every sub-frame of a frame carries the frame's destination
    for (int v = 0; L.outs && v < views; ++v) view_outs[size_t(v)] = L.outs[v / L.samples];
    host::fill_views(c, P, big ? c->h_views[vs] : A.B.view, views, L.cameras, view_outs.data());
    if (const int st = take_scene_slot(c, &ss); st != KIFS_OK) return st;
    SceneView* const scenes = static_cast<SceneView*>(c->h_scenes[ss]);
    for (int v = 0; v < views; ++v) {
        const KifsOptionsUniform& o = L.options ? L.options[v] : c->options;
        SceneView& s = scenes[v];
        s.c = {o.constant[0], o.constant[1], o.constant[2], o.constant[3]};
        s.power = o.power;
        s.fractal_color = {o.fractal_color[0], o.fractal_color[1], o.fractal_color[2]};
        s.background_color = {o.background_color[0], o.background_color[1], o.background_color[2]};
        // (the animation kernel takes every view's from the table; an accumulated launch reads none: a miss is averaged too)
        s.background_rgba = host::background_pixel(c, s.background_color, L.encode);
        std::memset(s.pad, 0, sizeof s.pad);
        if (grid > 1) {  // the view's cell: pad[0] = i | j << 8
            const int n = v % L.samples;
            const KifsSubpixel cell = L.jitter->cells ? L.jitter->cells[v] : KifsSubpixel{uint8_t(n % grid), uint8_t(n / grid)};
            s.pad[0] = uint32_t(cell.i) | uint32_t(cell.j) << 8;
        }
    }
    P.background_rgba = scenes[0].background_rgba;

    TileTable* const tt = host::tile_table(c, P.width, h, L.y0, L.y1);
    if (!tt) return KIFS_ERR_RUNTIME;
    // the grid's one dimension must hold the launcher's workgroups
    if (L.workgroups_per_entry && uint64_t(tt->count) * L.workgroups_per_entry * uint64_t(L.frames) > 0x7fffffffull) return KIFS_ERR_BAD_SIZE;
    if (const int st = follow_stream_change(tt, stream); st != KIFS_OK) return st;
    P.tile_order = tt->d_order;
    P.tile_count = tt->count;

    if (big) {
        if (!host::hip_ok(hipMemcpyAsync(c->d_views[vs], c->h_views[vs], sizeof(BatchView) * size_t(views), hipMemcpyHostToDevice, stream),
                          "copy(view table)"))
            return KIFS_ERR_RUNTIME;
        A.B.table = c->d_views[vs];
    }
    if (!host::hip_ok(hipMemcpyAsync(c->d_scenes[ss], scenes, sizeof(SceneView) * size_t(views), hipMemcpyHostToDevice, stream),
                      "copy(scene table)"))
        return KIFS_ERR_RUNTIME;
    A.scenes = static_cast<const SceneView*>(c->d_scenes[ss]);
    c->last_round_steps = 0;
    c->last_group_tiles = -1;
    c->last_bunny_form = -1;
    c->last_kernel = L.last_kernel;
    const KifsOptionsUniform& first = L.options ? L.options[0] : c->options;
    const bool launched = host::hip_ok(L.launch(A, first.fractal_group_id, first.primitive_id, stream, L.user),
                                       L.last_kernel == KIFS_KERNEL_ANIMATION ? "animation render_kernel launch" : "accumulate render_kernel launch");
    // (also after a failed launch: the copies above are enqueued and read the pinned images)
    bool marked = mark_scene_slot(c, ss, stream);
    if (big) {
        marked = host::hip_ok(hipEventRecord(c->views_used[vs], stream), "record(view table)") && marked;
        c->views_busy[vs] = true;
    }
    return launched && marked ? KIFS_OK : KIFS_ERR_RUNTIME;
}

int launch_scenes(kifs_ctx* c, void* hip_stream, const SceneLaunch& L) {
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    OptionsOfFrame0 scope(c, L.options ? L.options[0] : c->options);
    return enqueue(c, s, L);
}

// The launch step of the animated call: the kernel's argument is the batch and the scene table.
static hipError_t launch_render(const accum::Params& A, uint32_t group, uint32_t primitive, hipStream_t stream, void*) {
    return launch_animation_render(Params{A.B, A.scenes}, group, primitive, stream);
}

}  // namespace anim
}  // namespace kifs

extern "C" int kifs_render_animation_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                           const KifsOptionsUniform* options, uint8_t* const* dev_outs, size_t pitch, int y0,
                                           int y1, int encode) {
    using namespace kifs;
    if (const int st = anim::check(c, count, cameras, options, dev_outs, pitch, y0, y1, encode); st != KIFS_OK) return st;
    // (0: the animated launch's grid, one workgroup per entry and frame, has no bound -- a known gap)
    return anim::launch_scenes(c, hip_stream, anim::SceneLaunch{count, 1, cameras, options, nullptr, dev_outs, pitch, y0, y1, encode,
                                                                KIFS_KERNEL_ANIMATION, anim::launch_render, nullptr, 0u});
}
