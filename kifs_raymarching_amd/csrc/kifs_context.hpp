// kifs_context.hpp -- the host side's private types and helpers, shared by the translation units behind
// include/kifs_hip.h:
//   kifs_api.cpp       context lifetime, uniforms, the render entry points, profiling, diagnostics
//   kifs_schedule.cpp  one launch: parameters, tile tables, tile-order feedback, launch shape (enqueue_batch)
//   kifs_shards.cpp    row shards and sparse shards (the multi-GPU partition's per-device entry points)
//   kifs_multi.cpp     one process driving several devices (kifs_multi_*)
//   kifs_adaptive.cpp  adaptive anti-aliasing (kifs_render_adaptive_async): scratch block, rounds, the three passes
//   kifs_animation.cpp animated batches (kifs_render_animation_async), and the launch path of every call that carries
//                      a scene table (launch_scenes): the scene-table ring, one launch
//   kifs_accumulate.cpp accumulated frames (kifs_render_accumulate_async, _jittered_async): sub-frames as views
//   kifs_progressive.cpp progressive accumulation (kifs_render_accumulate_resume_async): a plane of sums across launches
//   kifs_converge.cpp  converging accumulation (kifs_render_accumulate_converge_async): sums, moments and a rule
//   kifs_rays.cpp      ray queries (kifs_trace_rays_async): caller-supplied rays, one launch
//   kifs_occlusion.cpp ambient occlusion (kifs_render_occlusion_async): the batch call's frames, hits attenuated, one launch
//   kifs_lighting.cpp  a configurable light (kifs_render_lit_async): the batch call's frames under the caller's light, one launch
//   kifs_trap.cpp      orbit-trap colouring (kifs_render_trapped_async, kifs_eval_trap): the lit call's frames, hits coloured by a trap
//   kifs_fold.cpp      kaleidoscopic IFS scenes (kifs_render_folded_async, kifs_eval_fold): the lit call's frames through a fold system
//   kifs_fold_trap.cpp orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async, kifs_eval_fold_trap): the
//                      two above composed, their records in a slot of the scene-table ring
// A kifs_ctx plays the part of the reference's GraphicState (render/graphics.rs:25-37): it owns the
// "device objects" (stream, events, the sRGB table in HBM, a scratch frame for host-destination renders)
// and a copy of the three uniform images.  There is no CPU path: every entry point that produces pixels
// launches the HIP kernels or fails.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/kifs_hip.h"
#include "kifs_internal.hpp"

// A row shard is a list of 8-row stripes of the frame (kifs_shard_stripes); its device image --
// first frame row of every stripe -- is cached per context (a root unpacks the shards of every peer).
struct RowTable {
    std::vector<int> stripes;  // stripe indices, ascending
    uint32_t* d_rows = nullptr;
};

// Tile order tables are keyed by the geometry they were built for and kept on the
// device; a context alternates between very few geometries (full frame, its band or shard).
struct TileTable {
    int width = 0, height = 0, y0 = 0, y1 = 0;
    const RowTable* rows = nullptr;   // non-null: the table of a row shard (then y0 = 0, y1 = height)
    uint32_t* d_order = nullptr;      // order used by the next launch
    uint32_t* d_order_alt = nullptr;  // the other half of the double buffer (the sort's target)
    uint32_t* d_cost = nullptr;       // per-tile cost, written by the first launch of a feedback period, read by the sort
    uint32_t* d_seen = nullptr;       // a batch's sorts: every tile's largest cost of the last few of them (tile_order_kernel)
    uint32_t cost_shift = 0;          // the sort's shift for what d_cost holds: set by the launch that records (work_cost_shift)
    uint64_t seen_scene = 0;          // what d_seen's costs were recorded with: options, iteration counts and shift (scene_key)
    bool seen_stale = false;          // d_cost comes from another scene or scale than d_seen: the next sort starts the memory afresh
    hipEvent_t costs_written = nullptr;  // recorded after the launch that wrote d_cost
    hipEvent_t stream_left = nullptr;    // recorded on the stream the caller moved away from
    hipEvent_t sorted = nullptr;      // recorded after the sort that fills d_order_alt
    uint64_t launches = 0;            // consecutive feedback launches made with this table
    hipStream_t last_stream = nullptr;  // stream of the latest of them
    bool sort_pending = false;        // d_order_alt holds (or will hold) a fresh order
    bool costs_marked = false;        // costs_written was recorded after the launch that last wrote d_cost
    bool feedback = true;             // reorder from costs (off once the caller pins an order)
    uint32_t count = 0;
    uint64_t last_use = 0;
};
constexpr int MAX_TILE_TABLES = 8;

struct kifs_ctx {
    int device = 0;
    TileTable tables[MAX_TILE_TABLES];
    std::vector<RowTable*> row_tables;  // never evicted while the context lives (a few hundred bytes each)
    uint64_t use_clock = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;  // tile-order sorts run here, beside the renders
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    hipEvent_t ev_order = nullptr;  // kifs_order_after: recorded on the producer's stream, waited for on the launch stream
    float* d_srgb = nullptr;       // 256 thresholds
    uint8_t* d_scratch = nullptr;  // frame staging for host destinations
    size_t scratch_bytes = 0;
    uint8_t* d_adaptive = nullptr;  // kifs_render_adaptive_async: geometry planes, edge queues and edge counters
    size_t adaptive_bytes = 0;
    hipEvent_t adaptive_done = nullptr;     // recorded behind the latest adaptive call's last pass
    hipStream_t adaptive_stream = nullptr;  // and the stream it ran on: a call on another stream waits for the event
    KifsScreenUniform screen{};
    KifsCameraUniform camera{};
    KifsOptionsUniform options{};
    bool have_screen = false, have_camera = false, have_options = false;
    int sdf_iters = 100, normal_iters = 10, fold_iters = 10;  // julia.wgsl:2-3, kifs.wgsl:72
    KifsExtensions ext{};  // all zero: the reference's behaviour
    int supersampling = 1;  // kifs_set_supersampling: k x k samples per pixel (1: the reference's one)
    int frames_in_flight = 1;  // kifs_set_frames_in_flight
    int last_round_steps = 0;  // kifs_debug_last_round_steps
    int last_group_tiles = -1; // kifs_debug_last_group_tiles
    int last_kernel = -1;      // kifs_debug_last_kernel
    int last_bunny_form = -1;  // kifs_debug_last_bunny_form
    float h_srgb[256] = {};    // host copy of the sRGB threshold table (d_srgb)
    // per-launch profiling ring (kifs_set_profiling)
    bool profiling = false;
    int prof_every = 1;      // time every n-th launch
    uint64_t prof_seen = 0;  // launches seen while profiling
    std::vector<hipEvent_t> prof_a, prof_b;
    size_t prof_count = 0;
    double last_ms = -1.0;
    bool timing_pending = false;
    unsigned long long* d_counters = nullptr;  // diagnostics buffer, see FrameParams
    size_t counter_words = 0;
    // View tables of batches beyond MAX_BATCH_INLINE: a ring of device tables, each with its pinned host
    // image and an event recorded after the launch that read it (allocated on first use).
    static constexpr int VIEW_RING = 4;
    kifs::BatchView* d_views[VIEW_RING] = {};
    kifs::BatchView* h_views[VIEW_RING] = {};
    hipEvent_t views_used[VIEW_RING] = {};
    bool views_busy[VIEW_RING] = {};
    int view_slot = 0;
    // Scene tables of kifs_render_animation_async (anim::SceneView records, kifs_params.hpp): the same kind of
    // ring -- device table, pinned host image, event behind the launch that read it -- one slot per call.
    static constexpr int SCENE_RING = 4;
    static constexpr size_t SCENE_SLOT_BYTES = size_t(64) * size_t(kifs::MAX_BATCH);
    void* d_scenes[SCENE_RING] = {};
    void* h_scenes[SCENE_RING] = {};
    hipEvent_t scenes_used[SCENE_RING] = {};
    bool scenes_busy[SCENE_RING] = {};
    int scene_slot = 0;
};
static_assert(sizeof(kifs::anim::SceneView) * size_t(kifs::MAX_BATCH) == kifs_ctx::SCENE_SLOT_BYTES, "a ring slot holds MAX_BATCH records");
static_assert(kifs_ctx::SCENE_RING == KIFS_ANIMATION_RING, "header and context agree on the ring's depth");

namespace kifs {
namespace host {

// KIFS_DEBUG=1 prints the failing HIP call to stderr (status codes stay the contract).
bool hip_ok(hipError_t e, const char* what);

struct DeviceGuard {  // make ctx's device current for the duration of a call
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int frame_dims(const kifs_ctx* c, int* w, int* h);
// frame_dims for a render: with k x k supersampling the virtual k W x k H screen must meet the same limit (BAD_SIZE)
int render_dims(const kifs_ctx* c, int* w, int* h);
int fill_params(const kifs_ctx* c, kifs::FrameParams* P);
// The certified radius of the power-2 Julia set for these options, 0: none; `bound` (may be null) receives the lower bound
// of the estimate beyond it.  julia_culls(): the cull thresholds of a Julia launch from the radius its frames share
// (fill_params does it for the context's options; a launch with options per frame calls julia_culls_of_frames after it).
double julia_cull_radius(const float c[4], float epsilon, float max_distance, int sdf_iters, double* bound);
bool takes_julia_culls(const kifs::FrameParams& P, uint32_t group);
void julia_culls(kifs::FrameParams& P, double rho, bool tile);
void julia_culls_of_frames(const kifs_ctx* c, kifs::FrameParams& P, const KifsOptionsUniform* options, int count);
// The views of a launch (cameras NULL: the context's camera) into `views`, and what they decide for all of it: P's
// camera is view 0's, and the culls go when a view does not meet what they assume.
void fill_views(const kifs_ctx* c, kifs::FrameParams& P, kifs::BatchView* views, int count, const KifsCameraUniform* cameras,
                uint8_t* const* outs);
// The next slot of the view-table ring (batches beyond MAX_BATCH_INLINE), free to be rewritten when the call returns.
int take_view_slot(kifs_ctx* c, int* slot);
bool is_device_pointer(const void* p);
void free_table(TileTable& t);
// Device image of a stripe list, cached by content.  Stripes must be ascending and inside the frame.
const RowTable* row_table(kifs_ctx* c, const int* stripes, int n, int height);
// `rows` non-null: the table of a row shard (tile row j = stripe rows->stripes[j]; y0 = 0, y1 = height).
TileTable* tile_table(kifs_ctx* c, int width, int height, int y0, int y1, const RowTable* rows = nullptr);
// The background pixel, encoded exactly as the kernels would (unorm8 / srgb8 of kifs_device_math.hpp).
uint32_t background_pixel(const kifs_ctx* c, kifs::V3 colour, int encode);
// Band, pitch and geometry plane of a launch: checked against the frame (P.y1 still its height), then written into P
// (kifs_schedule.cpp; kifs_occlusion.cpp and kifs_lighting.cpp fill their launches with it as enqueue_batch does).
int set_destination(const kifs_ctx* c, kifs::FrameParams& P, int count, uint8_t* out, size_t pitch, int y0, int y1, int encode,
                    bool striped, float* geom, size_t geom_pitch, size_t geom_stride);
// One launch: `count` frames (count == 1 and cameras NULL: the context's camera; else cameras[i] -> outs[i])
// sharing everything else.  `stripes` non-null: the launch renders that row shard (y0 = 0, y1 = height)
// instead of a band, into packed rows (in_place == 0) or at the rows' frame positions (in_place != 0).
// `geom` non-null: the launch also writes the geometry plane (kifs_render_geometry_async: 16-byte texels, rows
// `geom_pitch` bytes apart, view i's plane at geom + i * geom_stride bytes); bands only, no supersampling.
int enqueue_batch(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras,
                  uint8_t* const* outs, size_t pitch, int y0, int y1, int encode,
                  const int* stripes = nullptr, int n_stripes = 0, int in_place = 0,
                  float* geom = nullptr, size_t geom_pitch = 0, size_t geom_stride = 0);
int enqueue(kifs_ctx* c, hipStream_t stream, uint8_t* dev_out, size_t pitch, int y0, int y1, int encode);
// A launch that reads the table's current order without becoming one of its feedback launches (kifs_occlusion.cpp,
// kifs_lighting.cpp).  When the table's feedback launches run on another stream, the buffer rotation's "nobody still
// reads it" guarantee (feedback_before, kifs_schedule.cpp) needs this launch ordered after theirs (`before`), and theirs
// to come after it (!before).
bool order_around(TileTable* tt, hipStream_t stream, bool before);
// hipMalloc-backed buffer that only ever grows
bool grow(uint8_t*& buf, size_t& have, size_t need, const char* what);

}  // namespace host

// The ranges of KifsAmbientOcclusion (include/kifs_hip.h): kifs_occlusion.cpp's term, which kifs_lighting.cpp takes too.
namespace occl {
inline bool term_ok(const KifsAmbientOcclusion& ao) {
    return ao.samples >= 1 && ao.samples <= KIFS_MAX_AO_SAMPLES && std::isfinite(ao.step) && ao.step > 0.0f &&
           std::isfinite(ao.decay) && ao.decay > 0.0f && ao.decay <= 1.0f && std::isfinite(ao.strength) && ao.strength >= 0.0f;
}
}  // namespace occl

// The ranges of KifsLight and the light as the kernels read it: kifs_lighting.cpp's, which kifs_trap.cpp takes too.
namespace light {
// The contract's dot3 and normalize3 in f32 (the units are built with -ffp-contract=off; fmaf is the one fused operation).
inline float dot3(const float a[3], const float b[3]) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }

inline bool weight_ok(float w) { return std::isfinite(w) && w >= 0.0f; }

inline bool light_ok(const KifsLight& l) {
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(l.direction[i]) || !weight_ok(l.specular[i])) return false;
    const float d2 = dot3(l.direction, l.direction);
    if (!std::isnormal(d2)) return false;  // zero, subnormal, infinite: no unit vector to march towards
    return weight_ok(l.ambient) && weight_ok(l.diffuse) && l.shininess_log2 >= 0 && l.shininess_log2 <= KIFS_MAX_SHININESS_LOG2;
}

// The light as the kernel reads it: the direction as given, Lh = normalize3(direction) with IEEE divide and square root.
inline Light device_light(const KifsLight& l) {
    const float len = std::sqrt(dot3(l.direction, l.direction));
    Light d;
    d.direction = V3{l.direction[0], l.direction[1], l.direction[2]};
    d.unit = V3{l.direction[0] / len, l.direction[1] / len, l.direction[2] / len};
    d.ambient = l.ambient;
    d.diffuse = l.diffuse;
    d.specular = V3{l.specular[0], l.specular[1], l.specular[2]};
    d.shininess_log2 = l.shininess_log2;
    d.highlight = (l.specular[0] != 0.0f || l.specular[1] != 0.0f || l.specular[2] != 0.0f) ? 1u : 0u;
    return d;
}
}  // namespace light

// The ranges of KifsOrbitTrap and the trap as the kernels read it: kifs_trap.cpp's, which kifs_fold_trap.cpp takes too.
namespace trap {
// What kifs_eval_trap reads of a trap: where it is and how far the orbit runs.
inline bool orbit_ok(const KifsOrbitTrap& t) {
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(t.centre[i])) return false;
    return t.axes >= 1u && t.axes <= 15u && t.iterations >= 0 && t.iterations <= KIFS_MAX_TRAP_ITERATIONS;
}

inline bool trap_ok(const KifsOrbitTrap& t) {
    if (!orbit_ok(t) || !std::isfinite(t.scale) || !std::isfinite(t.bias)) return false;
    for (int i = 0; i < 3; ++i)
        if (!light::weight_ok(t.mid[i]) || !light::weight_ok(t.far[i])) return false;
    return true;
}

inline Trap device_trap(const KifsOrbitTrap& t) {
    return Trap{V4{t.centre[0], t.centre[1], t.centre[2], t.centre[3]}, t.axes, t.iterations, t.scale, t.bias,
                V3{t.mid[0], t.mid[1], t.mid[2]}, V3{t.far[0], t.far[1], t.far[2]}};
}
}  // namespace trap

// The ranges of KifsFoldSystem, the system as the kernels read it and the launch without a cull: kifs_fold.cpp's, which
// kifs_fold_trap.cpp takes too.
namespace fold {
inline bool fold_ok(const KifsFoldSystem& f) {
    if (f.stages > 31u || f.iterations < 0 || f.iterations > KIFS_MAX_FOLD_ITERATIONS) return false;
    if (!std::isfinite(f.scale) || !(f.scale >= 1.0f && f.scale <= 16.0f)) return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(f.offset[i])) return false;
    if (f.stages & KIFS_FOLD_ROTATE)  // without the bit the matrix is not looked at
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(f.rotation[i])) return false;
    return true;
}

// The record as the kernels read it: the constants of the scaling step in f32, t_i = -((s - 1) c_i) and h = t_z / 2.  A
// matrix that the stages do not name is not carried (it may hold anything): the kernel argument gets zeros.
inline Fold device_fold(const KifsFoldSystem& f) {
    Fold F{};
    F.stages = f.stages;
    F.iterations = f.iterations;
    F.scale = f.scale;
    const float k = f.scale - 1.0f;
    for (int i = 0; i < 3; ++i) F.t[i] = -(k * f.offset[i]);
    F.h = 0.5f * F.t[2];
    if (f.stages & KIFS_FOLD_ROTATE)
        for (int i = 0; i < 9; ++i) F.R[i] = f.rotation[i];
    return F;
}

// A folded scene reaches beyond the bounding sphere of its base primitive, on whose radius fill_params stands the per-ray
// cull, the wave-level quick exit and the tile-level one; the contract has no cull.  0 is each test's "disabled".
inline void culls_off(FrameParams& P) {
    P.cull_n2 = 0.0f;
    P.quick_cull_n2 = 0.0f;
    P.tile_cull_beta = 0.0f;
    P.tile_cull_sqrtk = 0.0f;
}
}  // namespace fold

// What every launch that carries a scene table shares (kifs_animation.cpp): the animated call and the four accumulated
// ones differ in their checks and in the last step, the launch itself.
namespace accum {

// The sub-pixel cells of a jittered call: sub-frame v goes through cell cells[v] of the grid x grid cells of its pixel;
// cells == nullptr (samples == grid * grid): sub-frame s of every frame through cell (s % grid, s / grid).
struct Jitter {
    int grid;
    const KifsSubpixel* cells;
};
// The launch step of a SceneLaunch: receives the filled Params, the pipeline and the stream.
typedef hipError_t (*LaunchFn)(const Params& A, uint32_t group, uint32_t primitive, hipStream_t stream, void* user);

}  // namespace accum

namespace anim {

// The fields every view of a launch shares (one pipeline, one march budget), compared as bit patterns.
bool same_pipeline(const KifsOptionsUniform& a, const KifsOptionsUniform& b);

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

// One call that its entry point has checked: `frames` output frames of `samples` sub-frames each, the views of one launch
// (view f * samples + s is sub-frame s of frame f and carries that frame's destination; an animated batch has samples 1).
struct SceneLaunch {
    int frames, samples;
    const KifsCameraUniform* cameras;   // a camera per view; null: the context's
    const KifsOptionsUniform* options;  // a scene per view; null: the context's for every view
    const accum::Jitter* jitter;        // null: no cell, a grid of 1
    uint8_t* const* outs;               // null: a pass without a picture (every view a null destination, no pitch)
    size_t pitch;
    int y0, y1, encode;
    int last_kernel;                    // what kifs_debug_last_kernel reports afterwards
    // The last step: `launch` receives the filled accum::Params (an animated batch's step makes its anim::Params of
    // them) and `user`.  `workgroups_per_entry` != 0: the launcher's grid is that many workgroups per entry of the
    // tile order and frame, and a call whose grid would pass 2^31 - 1 is refused (KIFS_ERR_BAD_SIZE).
    accum::LaunchFn launch;
    void* user;
    uint32_t workgroups_per_entry;
};
// The call itself: the context's device and stream (`hip_stream` null), view 0's options for the context's, and the one
// launch -- views, scene table, rings, tile table, copies, launch step, events.
int launch_scenes(kifs_ctx* c, void* hip_stream, const SceneLaunch& L);

// The scene-table ring's two steps, for a call that brings a record of its own through a slot (kifs_fold_trap.cpp).
// take_scene_slot: the next slot -- allocated on first use, and free to be rewritten when the call returns: it has waited
// for the launch that last read the slot.  mark_scene_slot: the event behind the launch that reads the slot, recorded on
// that launch's stream (also after a failed launch, once the copy is enqueued: it reads the pinned image); false when
// the record failed.
int take_scene_slot(kifs_ctx* c, int* slot);
bool mark_scene_slot(kifs_ctx* c, int slot, hipStream_t stream);

}  // namespace anim

// What kifs_accumulate.cpp shares with kifs_progressive.cpp and kifs_converge.cpp: a pass of a progressive frame is the
// jittered call with more to refuse and another launch step.
namespace accum {

// What every accumulated call refuses.  `outs_optional`: a null `outs` array is accepted (a pass without a picture); a
// null or misaligned entry of a given array is refused either way.
int check(const kifs_ctx* c, int count, int samples, const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
          uint8_t* const* outs, size_t pitch, int y0, int y1, int encode, bool outs_optional = false);
// What the jittered call refuses beyond check(): after it, so that every refusal of the unjittered call keeps its status.
int check_jitter(const kifs_ctx* c, int count, int samples, const Jitter& j);
// What a pass refuses of a plane it carries across launches -- the sums (16-byte texels) or the moments (4-byte ones):
// `count` bands of `rows` rows of `width` texels, `pitch` and `stride` in bytes.  The layout rules are the geometry
// output's (set_destination, kifs_schedule.cpp).
int check_plane(const void* plane, size_t pitch, size_t stride, size_t texel_bytes, int width, size_t rows, int count);
// The three accumulate launchers' grid: four workgroups per entry of the order and output frame (SceneLaunch).
constexpr uint32_t WORKGROUPS_PER_ENTRY = 4;

}  // namespace accum
}  // namespace kifs
