// kifs_params.hpp -- plain data shared by the host side of the library and the kernels.
#pragma once

#include <stdint.h>

namespace kifs {

struct V2 { float x, y; };
struct V3 { float x, y, z; };
struct V4 { float x, y, z, w; };  // quaternion (real, i, j, k) -- quaternions.wgsl:2-3

enum : int { GROUP_KIFS = 0, GROUP_JULIA = 1, GROUP_GENJULIA = 2 };  // data/scene.rs:4-11
enum : int {                                                           // data/scene.rs:35-45
    PRIM_SPHERE = 0, PRIM_CYLINDER, PRIM_BOX, PRIM_TORUS, PRIM_SIERPINSKI, PRIM_BUNNY, PRIM_OTHER
};

// Everything a frame needs, passed by value as the kernel argument (scalar loads ->
// SGPRs).  Unpacked from the three uniform images of bindings.wgsl:1-35.
struct FrameParams {
    float height, aspect;               // ScreenUniform; the width is `width` below
    V3 origin, m0, m1, m2;              // CameraUniform: origin + matrix columns
    int max_iterations;                 // OptionsUniform
    float max_distance, epsilon;
    V3 fractal_color, background_color;
    uint32_t is_heatmap;
    float power;
    V4 c;
    int sdf_iters, normal_iters, fold_iters;  // julia.wgsl:2-3, kifs.wgsl:72 made parameters
    // Largest f32 v with sqrt(v) <= 2 + epsilon: `length(p) > 2 + epsilon` (julia.wgsl:8) is
    // exactly `dot(p,p) > bound_n2` because correctly rounded sqrt is monotone.
    float bound_n2;
    int orbit_blocks, orbit_rem;        // sdf_iters = 6 * orbit_blocks + orbit_rem
    // (2 + epsilon)^2 * 1.1 for the bounding-sphere culls (0 disables them: NaN/odd epsilon); the power-2 Julia set
    // with a certified radius rho: (1 + 2^-6) rho^2 (fill_params)
    float cull_n2;
    // Smallest f32 v with sqrt(v) >= max_distance: `length(pos) < max_distance` (kifs.wgsl:72)
    // is exactly `dot(pos,pos) < fold_n2_stop`.
    float fold_n2_stop;
    // extension (include/kifs_hip.h KifsExtensions); soft_shadow == 0: the reference's shading
    uint32_t soft_shadow;
    int shadow_steps;
    float shadow_k, shadow_t0, shadow_max_t;
    int width, y0, y1;                  // frame width, row band [y0, y1)
    // Row shards (multi-GPU): when non-null, local tile row j of the launch is the 8-row stripe that
    // starts at frame row stripe_rows[j] (device table; y0 = 0, y1 = frame height); when null, tile
    // row j starts at frame row y0 + 8 j (a contiguous band).
    const uint32_t* stripe_rows;
    // 0: row k of the launch's rows goes to out + k * pitch (a packed band or shard);
    // 1: every row goes to its FRAME position, out + y * pitch (a shard rendered in place).
    int out_frame_rows;
    int encode;                         // KifsEncode
    uint32_t pitch_words;               // output row pitch in 32-bit words
    uint32_t* out;                      // first row of the band
    const float* srgb_table;            // 256 thresholds, device memory
    const uint32_t* tile_order;         // workgroup b renders tile (order[b] & 0xffff, order[b] >> 16)
    uint32_t tile_count;
    uint32_t* tile_cost;                // per tile (row-major tile index): its cost for the next order (kifs_render_common.hpp)
    // Optional device counters (nullptr in normal operation): [0] wave-steps taken in the
    // hand-written long-ray loop, [1] wave-steps taken on the general path, [2] entries into
    // the long-ray loop, [3] waves.  Enabled by kifs_debug_counters().
    unsigned long long* counters;
    // Wave-level early exit (see wave_is_culled in kifs_render_common.hpp): a cheaper, more conservative
    // form of the bounding-sphere cull, evaluated before any ray is set up.  0 disables it.
    float quick_cull_n2;                // 1.2 (B + epsilon)^2: well outside cull_n2
    float inv_height;                   // ~1 / height (the quick test needs no exact uv)
    // Tile-level form of the same exit (tile_is_culled in kifs_render_common.hpp): the quick test at the tile's
    // centre against a sphere grown by what the tile subtends.  tile_cull_beta bounds the angle (radians)
    // between the centre's ray and any ray of a 32 x 8 tile; 0 disables the test (camera matrix not
    // orthonormal, frame under 64 rows, quick cull off).  tile_cull_sqrtk = sqrt(quick_cull_n2).
    float tile_cull_beta, tile_cull_sqrtk;
    uint32_t background_rgba;           // the encoded background pixel (same encoder, run on the host)
    // Ray re-queuing (render_kernel): march steps per round between two re-packings of the
    // workgroup's surviving rays into full waves; 0 = every wave marches its own 64 pixels to the end.
    int round_steps;
    // tiles (consecutive entries of the order) per 256-thread workgroup of that path: 1 or 2;
    // 0: one single-wave workgroup per tile (render_wave_kernel)
    int group_tiles;
    // the bunny's throughput path, decided on the host from the launch's load (rules::BUNNY_* in kifs_schedule.cpp):
    // 0 = four lanes per ray, weights in VGPRs (render_group_kernel<KIFS, BUNNY, T>); 1 = four waves per 64 rays
    // (render_bunny_coop_kernel); 2 = four lanes per ray with layer 2 in LDS (render_group_kernel<KIFS, BUNNY, 2, true>)
    int bunny_coop;
    // Host-side launch hint, not read by the kernels: how many workgroups may share a CU
    // (0 = no cap).  See residency_for() in kifs_api.cpp.
    int workgroups_per_cu;
    // (at the end: the fields above keep their offsets in the kernel argument)
    // The throughput kernels' orbit trip in doubled coordinates (KIFS_FAST_TRIP_X2_ in kifs_scene.hpp): its constants
    // 2c and 4 max_distance (exact), and whether the scene meets the conditions under which it equals the contract's
    // trip bit for bit (orbit_x2_eligible() in kifs_schedule.cpp).  0: the plain trip.
    V4 c2;
    float max_distance4;
    int orbit_x2;
    // k x k supersampling (kifs_set_supersampling; kifs_ssaa_kernels.hip): 1 = one ray per pixel, the plain kernels;
    // k > 1 = the samples are the pixels of a virtual k W x k H screen, whose 1 / height the quick cull takes from here
    int ssaa;
    float ssaa_inv_height;
    // Geometry output (kifs_render_geometry_async; kifs_geometry_kernels.hip): the first row of view 0's plane of 16-byte
    // texels (n.x, n.y, n.z, t); null = a plain launch.  Row pitch and per-view stride in texels: view i's plane starts at
    // geom + 4 * i * geom_stride_texels floats, for the inline views and the device table alike (a pointer per BatchView
    // would not fit the kernel argument and would move every kernel's view loads).
    float* geom;
    uint32_t geom_pitch_texels, geom_stride_texels;
    // Host-side, not read by the kernels: 1.1 (B + epsilon)^2 of the scene's bounding radius B (0: culls off) -- what
    // cull_n2 holds unless a certified radius of the Julia set replaced it (julia_cull_radius() in kifs_schedule.cpp).
    // The launch-shape rules (disc_tiles, residency_for) were swept in this sphere's units and keep reading it.
    float shape_n2;
};

// A launch renders a batch of up to MAX_BATCH frames that share screen, options and tile
// order and differ in camera and destination (the frames of an orbit).  One frame's run time
// is the critical path of a few long rays with most SIMDs idle; a batch fills them.  Up to
// MAX_BATCH_INLINE views travel in the kernel argument (56 B each: 3.9 KB with the frame constants,
// limit 4 KB); a bigger batch -- the row shards of a multi-GPU step: a rank's eighth of 384 frames is
// the work of 48 whole ones -- reads them from a device table the host uploads before the launch.
constexpr int MAX_BATCH = 512;
constexpr int MAX_BATCH_INLINE = 64;
struct BatchView {
    V3 origin, m0, m1, m2;  // CameraUniform of this frame
    uint32_t* out;          // first row of its band
};
struct BatchParams {
    FrameParams frame;      // everything common; its camera fields and `out` are those of view 0
    int count;              // 1..MAX_BATCH
    const BatchView* table; // non-null: the views live there (count > MAX_BATCH_INLINE)
    BatchView view[MAX_BATCH_INLINE];
};
static_assert(sizeof(BatchParams) <= 4096, "the kernel argument is limited to 4 KB");

namespace adaptive {

// The argument of adaptive::render_kernel (pass C of kifs_render_adaptive_async, kifs_adaptive_kernels.hip): the launch's
// frame constants and views as every render kernel takes them (frame.ssaa = k, frame.out / view[i].out = the
// destinations pass A wrote), and the queues pass B filled.
struct Params {
    BatchParams B;
    const uint32_t* queues;  // view i's entries at queues + i * capacity
    const uint32_t* counts;  // view i's number of entries
    uint32_t capacity;
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace adaptive

namespace anim {

// What may differ between the frames of an animated launch (kifs_render_animation_async, kifs_animation_kernels.hip)
// besides the camera: frame i's values of the FrameParams fields of the same names, background_rgba encoded on the host
// as set_destination encodes the plain launch's.  One record is four 16-byte rows; the table is indexed by view.
struct alignas(16) SceneView {
    V4 c;
    float power;
    V3 fractal_color;
    V3 background_color;
    uint32_t background_rgba;
    uint32_t pad[4];
};
static_assert(sizeof(SceneView) == 64, "a scene record is 64 bytes");
// (that a ring slot of the context holds MAX_BATCH of them is asserted beside kifs_ctx, kifs_context.hpp)

// The kernel argument: the launch's frame constants and views as every render kernel takes them, and the scene table.
struct Params {
    BatchParams B;
    const SceneView* scenes;  // view i's record at scenes + i (device memory)
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace anim

namespace accum {

// The argument of accum::render_kernel (kifs_render_accumulate_async, kifs_accumulate_kernels.hip): the launch's frame
// constants as every render kernel takes them; its VIEWS are the sub-frames -- B.count = frames * samples, view
// f * samples + s is sub-frame s of output frame f and carries that frame's destination -- and a scene record per view.
struct Params {
    BatchParams B;
    const anim::SceneView* scenes;  // view v's record at scenes + v (device memory)
    int frames, samples;            // output frames; sub-frames per output frame, 1..KIFS_MAX_ACCUMULATE
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

// The argument of accum::carry_render_kernel (kifs_render_accumulate_resume_async): one PASS of a progressive frame.  A is
// the pass's own launch, exactly as the jittered call fills it (A first: the kernel argument's address is A's); the plane
// of 16-byte texels (sum.r, sum.g, sum.b, float(total)) is laid out as the geometry output's -- row r of the band of
// output frame f at sums + 4 * (f * sums_stride_texels + r * sums_pitch_texels) floats.
struct CarryParams {
    Params A;
    float* sums;                                     // first row of frame 0's plane (device memory, 16-byte aligned)
    uint32_t sums_pitch_texels, sums_stride_texels;  // row pitch and per-frame stride in texels
    uint32_t prior;                                  // sub-frames already in the plane; 0: the plane is not read
    uint32_t picture;                                // 0: no destinations, the pass only advances the plane
};
static_assert(sizeof(CarryParams) <= 4096, "the kernel argument is limited to 4 KB");

// The argument of accum::converge_render_kernel (kifs_render_accumulate_converge_async): one pass that marches only the
// pixels whose mean has not settled.  A first, as in CarryParams; the sums plane is the resume call's, with the texel's w
// word the PIXEL'S OWN count, read here; the moments plane holds one f32 per pixel, the sum of the squared luminances of
// the pixel's sub-frames -- row r of the band of output frame f at moments + f * moments_stride_words +
// r * moments_pitch_words floats.
struct ConvergeParams {
    Params A;
    float* sums;                                       // as CarryParams::sums
    uint32_t sums_pitch_texels, sums_stride_texels;
    float* moments;                                    // first row of frame 0's plane (device memory, 4-byte aligned)
    uint32_t moments_pitch_words, moments_stride_words;
    uint32_t restart;                                  // != 0: neither plane is read, every pixel is active with n = 0
    uint32_t picture;                                  // 0: no destinations, the pass only advances the planes
    uint32_t min_samples;                              // KifsConvergence::min_samples, 2..2^24
    float tol2;                                        // tolerance * tolerance, one f32 multiply on the host
    uint32_t* counts;                                  // null, or per output frame the pixels still active after the pass
};
static_assert(sizeof(ConvergeParams) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace accum

namespace rays {

// The argument of rays::trace_render_kernel (kifs_trace_rays_async, kifs_rays_kernels.hip): the scene's frame constants
// -- nothing of a screen or a camera is read: the origin is the lane's -- and the caller's arrays.  Ray k is the two
// 16-byte rows (origin, -), (direction, -) at rays + 8 k floats.
struct Params {
    FrameParams frame;
    const float* rays;   // n records of 32 bytes (device memory, 16-byte aligned)
    int n;               // 1..KIFS_MAX_RAYS
    float* geom;         // null, or n texels of 16 bytes (16-byte aligned)
    uint32_t* rgba;      // null, or n pixels
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");
// The launch's grid: one ray per lane, 256 lanes per workgroup (n up to KIFS_MAX_RAYS = 2^28: 2^20 workgroups).
constexpr uint32_t RAYS_PER_WORKGROUP = 256;
constexpr uint32_t workgroups(int n) { return n > 0 ? (uint32_t(n) + RAYS_PER_WORKGROUP - 1u) / RAYS_PER_WORKGROUP : 0u; }

}  // namespace rays

namespace occl {

// The ambient-occlusion term of kifs_render_occlusion_async (KifsAmbientOcclusion, include/kifs_hip.h), as the kernels
// read it.
struct AO {
    int samples;                  // 1..KIFS_MAX_AO_SAMPLES
    float step, decay, strength;
};

// The argument of occl::render_kernel (kifs_occlusion_kernels.hip): the launch's frame constants and views as every render
// kernel takes them (frame.ssaa = k, 1 included), the term, and the optional plane of one f32 per pixel -- row r of the
// band of view i at plane + i * stride_words + r * pitch_words floats.
struct Params {
    BatchParams B;
    AO ao;
    float* plane;                 // null: no plane (always with k > 1)
    uint32_t pitch_words, stride_words;
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace occl

namespace light {

// The light of kifs_render_lit_async (KifsLight, include/kifs_hip.h), as the kernels read it: the caller's direction as
// given (the direct term's) and normalised on the host (`unit`: the shadow ray's and the highlight's), the weights, the
// highlight's squarings.
struct Light {
    V3 direction;
    V3 unit;             // normalize(direction), f32 with IEEE divide and square root (kifs_lighting.cpp)
    float ambient, diffuse;
    V3 specular;
    int shininess_log2;  // 0..KIFS_MAX_SHININESS_LOG2
    uint32_t highlight;  // != 0: some weight of `specular` is not zero (decided on the host: a scalar branch here)
};

// The argument of light::render_kernel (kifs_lighting_kernels.hip): the launch's frame constants and views as every
// render kernel takes them (frame.ssaa = k, 1 included), the light, and the occlusion term with the flag that says
// whether there is one.
struct Params {
    BatchParams B;
    Light light;
    occl::AO ao;         // read only when has_ao != 0
    uint32_t has_ao;
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace light

namespace trap {

// The orbit trap of kifs_render_trapped_async (KifsOrbitTrap, include/kifs_hip.h), as the kernels read it: the record as
// the caller gave it, field for field.
struct Trap {
    V4 centre;
    uint32_t axes;       // 1..15: bit i set, component i takes part in the distance
    int iterations;      // 0..KIFS_MAX_TRAP_ITERATIONS
    float scale, bias;
    V3 mid, far;
};
static_assert(sizeof(Trap) == 56, "the record is KifsOrbitTrap's 56 bytes");

// The argument of trap::render_kernel (kifs_trap_kernels.hip): light::Params -- the same fields at the same offsets --
// and the trap behind them.
struct Params {
    BatchParams B;
    light::Light light;
    occl::AO ao;         // read only when has_ao != 0
    uint32_t has_ao;
    Trap trap;
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

// The argument of trap::eval_kernel (kifs_eval_trap): the scene's frame constants -- nothing of a screen or a camera is
// read -- the trap, of which only centre, axes and iterations are, and the arrays.
struct EvalParams {
    FrameParams frame;
    Trap trap;
    const float* points;  // n positions of three floats (device memory)
    int n;
    float* u;             // n floats
};
static_assert(sizeof(EvalParams) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace trap

namespace fold {

// The fold system of kifs_render_folded_async (KifsFoldSystem, include/kifs_hip.h), as the kernels read it: the stage
// mask, the trip count and the scale as given, the constants of the scaling step computed on the host in f32 --
// t_i = -((scale - 1) * offset[i]), h = 0.5 * t_z -- and the matrix as given, row-major.
enum : uint32_t { ABS = 1u, SORT = 2u, TETRA = 4u, ROTATE = 8u, MIRROR_Z = 16u };
struct Fold {
    uint32_t stages;     // 0..31
    int iterations;      // 0..KIFS_MAX_FOLD_ITERATIONS
    float scale;         // 1..16
    float t[3];
    float h;
    float R[9];          // read only with ROTATE
};
static_assert(sizeof(Fold) == 64, "the record is 64 bytes");

// The argument of fold::render_kernel (kifs_fold_kernels.hip): light::Params -- the same fields at the same offsets --
// and the fold system behind them.
struct Params {
    BatchParams B;
    light::Light light;
    occl::AO ao;         // read only when has_ao != 0
    uint32_t has_ao;
    Fold fold;
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

// The argument of fold::eval_kernel (kifs_eval_fold): the scene's frame constants -- nothing of a screen or a camera is
// read -- the fold system and the arrays.
struct EvalParams {
    FrameParams frame;
    Fold fold;
    const float* points;  // n positions of three floats (device memory)
    int n;
    float* sdf;           // null, or n floats
    float* normal;        // null, or n normals of three floats
};
static_assert(sizeof(EvalParams) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace fold

namespace foldorbit {

// What kifs_render_folded_trapped_async carries beside light::Params' fields: the fold system and the trap as the two
// calls' kernels read them.  light::Params is 4024 of the kernel argument's 4096 bytes and the two records are 120, so
// they travel in device memory -- one record per launch, in a slot of the context's scene-table ring -- and the argument
// holds a pointer.  Nothing writes the record while a launch that reads it runs.
struct Record {
    fold::Fold fold;
    trap::Trap trap;
    uint32_t pad[2];
};
static_assert(sizeof(Record) == 128, "the record is 128 bytes: the fold system, the trap, padding");

// The argument of foldorbit::render_kernel (kifs_fold_trap_kernels.hip): light::Params -- the same fields at the same
// offsets -- and behind them the record, and the optional plane of one f32 per pixel, laid out as occl::Params' -- row r
// of the band of view i at plane + i * stride_words + r * pitch_words floats.
struct Params {
    BatchParams B;
    light::Light light;
    occl::AO ao;         // read only when has_ao != 0
    uint32_t has_ao;
    const Record* record;  // device memory
    float* plane;          // null: no plane (always with k > 1)
    uint32_t pitch_words, stride_words;
};
static_assert(sizeof(Params) == 4048, "the kernel argument is limited to 4 KB");

// The argument of foldorbit::eval_kernel (kifs_eval_fold_trap): the scene's frame constants -- nothing of a screen or a
// camera is read -- the two records, which fit here, and the arrays.  Of the trap only centre, axes and iterations are read.
struct EvalParams {
    FrameParams frame;
    fold::Fold fold;
    trap::Trap trap;
    const float* points;  // n positions of three floats (device memory)
    int n;
    float* u;             // n floats
};
static_assert(sizeof(EvalParams) <= 4096, "the kernel argument is limited to 4 KB");

}  // namespace foldorbit

}  // namespace kifs
