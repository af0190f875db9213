// kifs_animation_kernels.hip -- animated batches (kifs_render_animation_async, include/kifs_hip.h): the frames of one
// launch differ not only in camera but in the Julia constant, the power and the two colours -- a morph, rendered with the
// long rays of all its frames side by side as kifs_render_batch_async renders an orbit.
//
//   anim::render_kernel<GROUP, PRIM>  256 threads per 32 x 8 tile of the launch's tile order, exactly as
//                                     kifs::render_kernel takes them: wave w owns 8 x 8 block w and marches its 64 rays
//                                     from start to finish.  What is new is the view's SCENE: a 64-byte record per view in
//                                     a device table (c, power, the colours, the encoded background), read with scalar
//                                     loads -- the view index is workgroup-uniform -- and laid over the launch's frame
//                                     constants before anything uses them.
// Cameras and destinations travel as in every batch: inline in the kernel argument up to MAX_BATCH_INLINE views, through
// the context's view-table ring beyond.  Tile table, bands and order are the plain launch's.
// This file also holds the entry point's host side: the sanitizer build of the host units (make asan) links against a
// stand-in that knows no launcher of this file, so none of those units refers to one.
#include <cstring>

#include "kifs_context.hpp"
#include "kifs_render_common.hpp"

namespace kifs {
namespace anim {

// What may differ between the frames of a launch besides the camera: frame i's values of the FrameParams fields of the
// same names, background_rgba encoded on the host as set_destination encodes the plain launch's.  One record is four
// 16-byte rows; the table is indexed by view.
struct alignas(16) SceneView {
    V4 c;
    float power;
    V3 fractal_color;
    V3 background_color;
    uint32_t background_rgba;
    uint32_t pad[4];
};
static_assert(sizeof(SceneView) == 64, "a scene record is 64 bytes");
static_assert(sizeof(SceneView) * size_t(MAX_BATCH) == kifs_ctx::SCENE_SLOT_BYTES, "a ring slot holds MAX_BATCH records");
static_assert(kifs_ctx::SCENE_RING == KIFS_ANIMATION_RING, "header and context agree on the ring's depth");

// The kernel argument: the launch's frame constants and views as every render kernel takes them, and the scene table.
struct Params {
    BatchParams B;
    const SceneView* scenes;  // view i's record at scenes + i (device memory)
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

// View `view`'s scene over its frame constants.  The table is read through the constant address space, as batch_frame
// reads a view table: the index is uniform, so these are scalar loads like the kernel argument's own.
__device__ __forceinline__ void overlay_scene(FrameParams& P, const SceneView* scenes, uint32_t view) {
    typedef const SceneView __attribute__((address_space(4))) * ConstScene;
    const ConstScene s = (ConstScene)(scenes + view);
    P.c = V4{s->c.x, s->c.y, s->c.z, s->c.w};
    P.power = s->power;
    P.fractal_color = V3{s->fractal_color.x, s->fractal_color.y, s->fractal_color.z};
    P.background_color = V3{s->background_color.x, s->background_color.y, s->background_color.z};
    P.background_rgba = s->background_rgba;
}

// (amdgpu_waves_per_eu: as geom::render_kernel)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const Params A) {
    __shared__ float s_srgb[256];
    __shared__ uint32_t s_tile[TILE_H][TILE_W];

    TileFrame F = tile_frame(A.B, s_srgb);  // (the prologue reads no field of the scene)
    overlay_scene(F.P, A.scenes, F.view);
    const FrameParams& P = F.P;

    const bool culled = wave_is_culled(P, F.x, F.y, F.valid);  // wave-uniform

    V3 colour{0.0f, 0.0f, 0.0f};
    if (!culled && __ballot(F.valid) != 0ull) {
        int steps = 0;
        const V3 dir = ray_direction(P, F.x, F.y);
        colour = raymarch<GROUP, PRIM>(P, dir, F.valid, steps);
    }
    __syncthreads();  // s_srgb visible
    uint32_t rgba = P.background_rgba;  // the view's own
    if (!culled) rgba = encode_rgba(colour, F.srgb, s_srgb);
    s_tile[F.ly][F.lx] = rgba;
    __syncthreads();
    store_tile(P, F.tile_x, F.tile_y, F.frame_y, s_tile, int(threadIdx.x));
}

template <int GROUP, int PRIM>
static hipError_t launch(const Params& A, hipStream_t stream) {
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(A.B.frame.tile_count * uint32_t(A.B.count)), dim3(BLOCK), 0, stream, A);
    return hipGetLastError();
}

static hipError_t launch_render(const Params& A, uint32_t group, uint32_t primitive, hipStream_t stream) {
    // Julia: the short divide / square root by sdf_iters; the doubled orbit trip is the throughput kernels' only.
    // The bunny: per-lane bunny_sdf -- slow, correct.
    return dispatch_pipeline<2>(group, primitive, uint32_t(A.B.frame.sdf_iters <= 24), [&](auto g, auto prim) {
        return launch<decltype(g)::value, decltype(prim)::value>(A, stream);
    });
}

// ---- host side --------------------------------------------------------------------------------------------------
// The fields every frame of a launch shares: one pipeline, one march budget.  Bit patterns, not values: -0.0f is not 0.0f
// and a NaN equals itself here.  Padding words are not looked at.
static bool same_pipeline(const KifsOptionsUniform& a, const KifsOptionsUniform& b) {
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

// The launch's frame constants come from fill_params, which reads the context's options: for the length of a call the
// context holds frame 0's image in their place and gets its own back at the end, set or not.
struct OptionsOfFrame0 {
    kifs_ctx* c;
    KifsOptionsUniform saved;
    bool had;
    OptionsOfFrame0(kifs_ctx* ctx, const KifsOptionsUniform& first) : c(ctx), saved(ctx->options), had(ctx->have_options) {
        c->options = first;
        c->have_options = true;
    }
    ~OptionsOfFrame0() {
        c->options = saved;
        c->have_options = had;
    }
    OptionsOfFrame0(const OptionsOfFrame0&) = delete;
    OptionsOfFrame0& operator=(const OptionsOfFrame0&) = delete;
};

// The next slot of the scene-table ring, as take_view_slot takes one of the view tables: allocated on first use, and
// rewritten only after the launch that last read it is over.
static int take_scene_slot(kifs_ctx* c, int* slot) {
    const int ss = *slot = c->scene_slot;
    c->scene_slot = (ss + 1) % kifs_ctx::SCENE_RING;
    if (!c->d_scenes[ss]) {
        if (!host::hip_ok(hipMalloc(&c->d_scenes[ss], kifs_ctx::SCENE_SLOT_BYTES), "hipMalloc(scene table)") ||
            !host::hip_ok(hipHostMalloc(&c->h_scenes[ss], kifs_ctx::SCENE_SLOT_BYTES, hipHostMallocDefault), "hipHostMalloc(scene table)") ||
            !host::hip_ok(hipEventCreateWithFlags(&c->scenes_used[ss], hipEventDisableTiming), "hipEventCreate(scene table)"))
            return KIFS_ERR_RUNTIME;
    }
    if (c->scenes_busy[ss] && !host::hip_ok(hipEventSynchronize(c->scenes_used[ss]), "wait(scene table)")) return KIFS_ERR_RUNTIME;
    c->scenes_busy[ss] = false;
    return KIFS_OK;
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

static int enqueue(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
                   uint8_t* const* outs, size_t pitch, int y0, int y1, int encode) {
    host::hip_ok(hipGetLastError(), "stale error before enqueue");
    Params A;
    FrameParams& P = A.B.frame;
    if (const int st = host::fill_params(c, &P); st != KIFS_OK) return st;  // (frame 0's options: OptionsOfFrame0)
    const int h = P.y1;  // the frame's height
    A.B.count = count;
    A.B.table = nullptr;
    P.y0 = y0;
    P.y1 = y1;
    P.encode = encode;
    P.pitch_words = uint32_t(pitch >> 2);
    P.out = reinterpret_cast<uint32_t*>(outs[0]);
    // whole rays, one kernel form for every scene: no costs, no diagnostics, no rounds, the plain orbit trip
    P.tile_cost = nullptr;
    P.counters = nullptr;
    P.round_steps = 0;
    P.workgroups_per_cu = 0;
    P.orbit_x2 = 0;
    if (y1 == y0) return KIFS_OK;

    const bool big = count > MAX_BATCH_INLINE;
    int vs = -1, ss = -1;
    if (big)
        if (const int st = host::take_view_slot(c, &vs); st != KIFS_OK) return st;
    host::fill_views(c, P, big ? c->h_views[vs] : A.B.view, count, cameras, outs);
    if (const int st = take_scene_slot(c, &ss); st != KIFS_OK) return st;
    SceneView* const scenes = static_cast<SceneView*>(c->h_scenes[ss]);
    for (int i = 0; i < count; ++i) {
        const KifsOptionsUniform& o = options[i];
        SceneView& s = scenes[i];
        s.c = {o.constant[0], o.constant[1], o.constant[2], o.constant[3]};
        s.power = o.power;
        s.fractal_color = {o.fractal_color[0], o.fractal_color[1], o.fractal_color[2]};
        s.background_color = {o.background_color[0], o.background_color[1], o.background_color[2]};
        s.background_rgba = host::background_pixel(c, s.background_color, encode);
        std::memset(s.pad, 0, sizeof s.pad);
    }
    P.background_rgba = scenes[0].background_rgba;  // (the kernel takes every view's from the table)

    TileTable* const tt = host::tile_table(c, P.width, h, y0, y1);
    if (!tt) return KIFS_ERR_RUNTIME;
    if (const int st = follow_stream_change(tt, stream); st != KIFS_OK) return st;
    P.tile_order = tt->d_order;
    P.tile_count = tt->count;

    if (big) {
        if (!host::hip_ok(hipMemcpyAsync(c->d_views[vs], c->h_views[vs], sizeof(BatchView) * size_t(count), hipMemcpyHostToDevice, stream),
                          "copy(view table)"))
            return KIFS_ERR_RUNTIME;
        A.B.table = c->d_views[vs];
    }
    if (!host::hip_ok(hipMemcpyAsync(c->d_scenes[ss], scenes, sizeof(SceneView) * size_t(count), hipMemcpyHostToDevice, stream),
                      "copy(scene table)"))
        return KIFS_ERR_RUNTIME;
    A.scenes = static_cast<const SceneView*>(c->d_scenes[ss]);
    c->last_round_steps = 0;
    c->last_group_tiles = -1;
    c->last_bunny_form = -1;
    c->last_kernel = KIFS_KERNEL_ANIMATION;
    const bool launched = host::hip_ok(launch_render(A, options[0].fractal_group_id, options[0].primitive_id, stream),
                                       "animation render_kernel launch");
    // (also after a failed launch: the copies above are enqueued and read the pinned images)
    bool marked = host::hip_ok(hipEventRecord(c->scenes_used[ss], stream), "record(scene table)");
    c->scenes_busy[ss] = true;
    if (big) {
        marked = host::hip_ok(hipEventRecord(c->views_used[vs], stream), "record(view table)") && marked;
        c->views_busy[vs] = true;
    }
    return launched && marked ? KIFS_OK : KIFS_ERR_RUNTIME;
}

}  // namespace anim
}  // namespace kifs

extern "C" int kifs_render_animation_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                           const KifsOptionsUniform* options, uint8_t* const* dev_outs, size_t pitch, int y0,
                                           int y1, int encode) {
    using namespace kifs;
    if (const int st = anim::check(c, count, cameras, options, dev_outs, pitch, y0, y1, encode); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    anim::OptionsOfFrame0 scope(c, options[0]);
    return anim::enqueue(c, s, count, cameras, options, dev_outs, pitch, y0, y1, encode);
}
