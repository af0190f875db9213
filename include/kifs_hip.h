/*
 * kifs_hip.h -- C ABI of the MI355X-native raymarching library (libkifs_hip.so).
 *
 * Drop-in boundary for the one hot path of LesbianLemon/kifs-raymarching: the
 * per-pixel sphere-tracing fragment shader.  The reference has no FFI today;
 * the seam this ABI replaces is `GraphicState` (src/render/graphics.rs:25-37):
 *
 *   reference call (file:line)                         this ABI
 *   -------------------------------------------------  ---------------------------
 *   GraphicState::new            graphics.rs:183-232   kifs_create
 *   update_screen_data           graphics.rs:262-266   kifs_set_screen   (12 B image)
 *   zoom_camera / rotate_camera  graphics.rs:268-302   kifs_set_camera   (64 B image)
 *   update_options               graphics.rs:304-308   kifs_set_options  (80 B image)
 *   render (set_pipeline by fractal_group, bind group,
 *           draw(0..3, 0..2))    graphics.rs:310-325   kifs_render / kifs_render_async
 *   drop(RenderState)            application.rs:86-91  kifs_destroy
 *
 * The three uniform structs are byte-identical to the reference's Pod structs
 * (src/data.rs:17-49) and to the WGSL declarations
 * (src/shaders/dependencies/bindings.wgsl:1-35), so a Rust host passes
 * `bytemuck::bytes_of(&data.into_buffer_data())` unchanged.
 *
 * Plain pointers and sizes only; no exceptions cross the boundary; every entry
 * point returns a KifsStatus.  A context is not thread-safe: one caller thread
 * per context, mirroring the reference's single winit thread
 * (src/application.rs:37-48).
 */
#ifndef KIFS_HIP_H
#define KIFS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KIFS_ABI_VERSION 4

/* ---- uniform images (data.rs:17-49) --------------------------------------- */

typedef struct KifsScreenUniform { /* ScreenUniformData, data.rs:17-23 */
    float width;
    float height;
    float aspect_ratio;
} KifsScreenUniform; /* 12 bytes */

typedef struct KifsCameraUniform { /* CameraUniformData, data.rs:25-31 */
    float origin[3];
    uint32_t _padding;
    float matrix[3][4]; /* mat3x3 as 3 columns with 16-byte stride (packed.rs:78-92) */
} KifsCameraUniform; /* 64 bytes */

typedef struct KifsOptionsUniform { /* OptionsUniformData, data.rs:33-49 */
    int32_t max_iterations;
    float max_distance;
    float epsilon;
    uint32_t _padding1;
    float fractal_color[3]; /* linear RGB */
    uint32_t _padding2;
    float background_color[3];
    uint32_t is_heatmap;
    uint32_t fractal_group_id; /* KifsFractalGroup, scene.rs:4-11 */
    uint32_t primitive_id;     /* KifsPrimitiveShape, scene.rs:35-45 */
    float power;
    uint32_t _padding3;
    float constant[4]; /* quaternion (real, i, j, k) */
} KifsOptionsUniform; /* 80 bytes */

typedef enum KifsFractalGroup { /* data/scene.rs:4-11 */
    KIFS_GROUP_KIFS = 0,
    KIFS_GROUP_JULIA = 1,
    KIFS_GROUP_GEN_JULIA = 2
} KifsFractalGroup;

typedef enum KifsPrimitiveShape { /* data/scene.rs:35-45 */
    KIFS_PRIM_SPHERE = 0,
    KIFS_PRIM_CYLINDER = 1,
    KIFS_PRIM_BOX = 2,
    KIFS_PRIM_TORUS = 3,
    KIFS_PRIM_SIERPINSKI = 4,
    KIFS_PRIM_BUNNY = 5
} KifsPrimitiveShape;

/* Colour-target encoding: the reference picks the first sRGB surface format if
 * any, else formats[0] (render.rs:72-80); blend REPLACE (graphics.rs:87-91). */
typedef enum KifsEncode {
    KIFS_ENCODE_UNORM = 0, /* linear -> UNORM8 */
    KIFS_ENCODE_SRGB = 1   /* linear -> sRGB OETF -> UNORM8 (alpha stays linear) */
} KifsEncode;

/* Status codes; taxonomy follows src/error.rs:66-92. */
typedef enum KifsStatus {
    KIFS_OK = 0,
    KIFS_ERR_NO_DEVICE = 1,    /* ~ RenderStateError::RequestAdapter */
    KIFS_ERR_DEVICE_INIT = 2,  /* ~ RenderStateError::RequestDevice */
    KIFS_ERR_BAD_SIZE = 3,     /* ~ RenderError::SurfaceMissized; zero size (render.rs:211) */
    KIFS_ERR_UNCONFIGURED = 4, /* render before all three uniforms were set */
    KIFS_ERR_RUNTIME = 5,      /* HIP error: fatal for the context */
    KIFS_ERR_COMM = 6,         /* an inter-GPU transfer failed: RCCL (init, group, send/recv) or a peer copy */
    KIFS_ERR_BAD_ARG = 7       /* null pointer, unknown enum value, bad range */
} KifsStatus;

typedef struct kifs_ctx kifs_ctx;

/* ---- lifetime --------------------------------------------------------------
 * Replaces GraphicState::new (graphics.rs:183-232) + adapter/device request
 * (render.rs:42-69).  Binds the context to HIP device `device_ordinal`, creates
 * its stream and events and uploads the sRGB threshold table.  Returns NULL
 * and sets *status on failure. */
kifs_ctx* kifs_create(int device_ordinal, int* status);

/* Replaces the explicit drop (application.rs:86-91).  NULL is a no-op. */
void kifs_destroy(kifs_ctx* ctx);

/* ---- uniforms (each call COPIES its argument, like queue.write_buffer) ------ */
int kifs_set_screen(kifs_ctx* ctx, const KifsScreenUniform* screen);    /* graphics.rs:262 */
int kifs_set_camera(kifs_ctx* ctx, const KifsCameraUniform* camera);    /* graphics.rs:268,280 */
int kifs_set_options(kifs_ctx* ctx, const KifsOptionsUniform* options); /* graphics.rs:304 */

/* The reference hard-codes JULIA_ITERATIONS = 100, JULIA_NORMAL_ITERATIONS = 10
 * (julia.wgsl:2-3, gen_julia.wgsl:2-3) and 10 Sierpinski folds (kifs.wgsl:72).
 * Those are the defaults; BASELINE configs override them.  All must be >= 0. */
int kifs_set_iters(kifs_ctx* ctx, int sdf_iters, int normal_iters, int fold_iters);

/* ---- extension: soft shadows ---------------------------------------------------------
 * NOT part of the reference (its whole shading model is entry.wgsl:6-29); BASELINE config 5
 * names "soft-shadow secondary rays", so it exists as an explicit opt-in whose semantics this
 * library defines.  With soft_shadow != 0, every hit pixel marches a secondary ray from
 * p + 2*epsilon*n towards L = normalize((1,1,1)) (the direction of the reference's light
 * vector, entry.wgsl:17):
 *     res = 1; t = shadow_t0
 *     up to shadow_steps times: h = scene_SDF(start + t*L); if h < epsilon -> res = 0, stop;
 *                               res = min(res, shadow_k*h/t); t += h; stop if t > shadow_max_t
 * and the direct term is attenuated: diffuse = 0.1 + 0.9 * clamp(n.(1,1,1), 0, 1) * res.  A hit whose direct term
 * is not positive (it faces away from the light) marches no secondary ray (res = 1: there is nothing to attenuate).
 * All zero (the default) is the reference's behaviour exactly. */
typedef struct KifsExtensions {
    uint32_t soft_shadow;
    int32_t shadow_steps;
    float shadow_k;
    float shadow_t0;
    float shadow_max_t;
} KifsExtensions;
int kifs_set_extensions(kifs_ctx* ctx, const KifsExtensions* ext);

/* ---- extension: k x k supersampled anti-aliasing ------------------------------------------
 * NOT part of the reference (one sample per pixel at its centre: MultisampleState { count: 1 },
 * graphics.rs:107-108).  A per-context factor k, 1 <= k <= KIFS_MAX_SUPERSAMPLING (default 1);
 * another value gives KIFS_ERR_BAD_ARG.  With k > 1 output pixel (x, y) of the W x H frame takes k^2 samples:
 *   sample (i, j), 0 <= i, j < k, is fs_main at fragment centre (k x + i + 0.5, k y + j + 0.5) of a VIRTUAL screen
 *   of width k W, height k H and the same aspect_ratio float (camera, options, iteration counts and extensions the
 *   context's own; soft shadows apply per sample) -- i.e. pixel (k x + i, k y + j) of that screen;
 *   resolve, per channel in f32: acc = c(0,0); acc = acc + c(i,j) for the others, j outer, i inner, no fma;
 *   mean = acc / float(k*k), correctly rounded; then the frame's encoder (sRGB or UNORM; alpha 255).  Heatmap
 *   frames resolve their heatmap colours the same way.
 * k W and k H must be at most 65536: otherwise a render returns KIFS_ERR_BAD_SIZE and writes nothing.  The factor
 * applies to kifs_render, kifs_render_async, kifs_render_batch_async and kifs_render_shard_async; pixel coordinates
 * stay global, so bands, shards and batch frames are bit-identical to the same rows of the lone frame, and
 * kifs_multi_set_supersampling gives the kifs_multi_* renders the same frames.  k = 1 is the plain path exactly. */
#define KIFS_MAX_SUPERSAMPLING 4
int kifs_set_supersampling(kifs_ctx* ctx, int factor);

/* ---- render ---------------------------------------------------------------
 * Replaces GraphicState::render (graphics.rs:310-325): pipeline chosen by
 * options.fractal_group_id, one kernel launch instead of draw(0..3, 0..2).
 *
 * Renders rows [y0, y1) of the W x H frame (W, H from the screen uniform; pixel
 * coordinates stay global, so a band is bit-identical to the same rows of the
 * full frame).  Row y goes to out + (y - y0) * pitch_bytes, 4 bytes per pixel,
 * R G B A.  pitch_bytes >= 4*W and a multiple of 4.
 *
 * The library launches on non-blocking streams (its own, or the caller's `hip_stream`): work the caller has
 * pending on OTHER streams for the destination (a fill, a previous consumer) is not ordered before the render
 * unless the caller orders it, as with any asynchronous HIP work.  kifs_order_after does that in one call: the
 * context's NEXT work on `hip_stream` (NULL = the context's own stream, the one kifs_render uses) runs after
 * everything `producer_stream` (a hipStream_t of the context's device; NULL = the legacy default stream) holds
 * when the call is made -- an event recorded there and waited for on the launch stream; nothing blocks the host;
 * the same stream twice is a no-op.  (The reference has one queue and copies on every update,
 * util/uniform.rs:23-35, so the question does not arise there.)
 *
 * kifs_render: `out` may be a device pointer of the context's device or a host
 * pointer; returns once `out` holds the pixels.
 * kifs_render_async: `out` must be device memory; the launch is enqueued on
 * `hip_stream` (a hipStream_t; NULL = the context's own stream) and the call
 * returns without synchronising. */
int kifs_render(kifs_ctx* ctx, uint8_t* out_rgba8, size_t pitch_bytes, int y0, int y1,
                int encode);
int kifs_render_async(kifs_ctx* ctx, void* hip_stream, uint8_t* dev_out_rgba8,
                      size_t pitch_bytes, int y0, int y1, int encode);
int kifs_order_after(kifs_ctx* ctx, void* hip_stream, void* producer_stream);

/* A batch of frames in one launch: frame i is rendered with cameras[i] (the context's screen,
 * options, iteration counts and extensions; the context's own camera is neither used nor
 * changed) into dev_outs[i], same pitch / band / encoding for all.  1 <= count <= KIFS_MAX_BATCH.
 * This is the throughput path for sequences of independent frames (the frames of an orbit,
 * cf. rotate_camera graphics.rs:280-302): one frame of these scenes keeps most of the device
 * idle -- its run time is the critical path of a few long rays -- and the workgroups of a batch
 * are interleaved frame by frame, so the long rays of all its frames march side by side.
 * Every frame is bit-identical to the same frame rendered alone. */
#define KIFS_MAX_BATCH 512
int kifs_render_batch_async(kifs_ctx* ctx, void* hip_stream, int count,
                            const KifsCameraUniform* cameras, uint8_t* const* dev_outs_rgba8,
                            size_t pitch_bytes, int y0, int y1, int encode);

/* ---- extension: geometry output -- per-pixel hit distance and surface normal ----------------
 * NOT part of the reference (its fragment shader returns a colour and nothing else, entry.wgsl:49-59).
 * kifs_render_batch_async that ALSO writes, for every pixel of the band, what the march and the shading held:
 * whether the primary ray hit, its parameter t at the hit and the normal the shading used.
 *   colour    frame i goes to dev_outs_rgba8[i] exactly as kifs_render_batch_async writes it: the same bytes,
 *             heatmap and soft shadows included.  cameras == NULL with count == 1: the context's camera.
 *   layout    one 16-byte texel per pixel, four f32 (n.x, n.y, n.z, t).  Row y of frame i sits at
 *             dev_geometry + i * geometry_stride_bytes + (y - y0) * geometry_pitch_bytes (byte offsets).  The base is
 *             16-byte aligned; the pitch is at least 16 W and a multiple of 16; the stride is a multiple of 16 and, when
 *             count > 1, at least (y1 - y0) * pitch.  Otherwise the call returns KIFS_ERR_BAD_ARG and launches nothing.
 *             (One base plus a stride, not a pointer per frame: the views of a batch travel in the 4 KB kernel
 *             argument, where a second pointer per view does not fit.)
 *   hit       the march of entry.wgsl:11-25 broke at d < epsilon.  t is the ray parameter at the break: the position
 *             that was tested is fma(t, dir, origin), or the origin itself with t = 0 for a hit on the first step.
 *             n is the vector get_normal returned there -- the same vector the shading dots with (1,1,1), not a
 *             second evaluation.
 *   miss      the loop ended any other way (every ray the bounding-sphere, wave and tile culls drop included):
 *             the texel is (0, 0, 0, +inf), bit pattern 0, 0, 0, 0x7f800000.
 *   coverage  every pixel of the band gets a texel; bytes of a row beyond 16 W are not touched.
 *   options   heatmap frames and soft shadows change the colour only: the hit test is the same and the geometry is
 *             the primary ray's.  No per-pixel step count is given out: the culls make the loop counter
 *             unobservable outside heatmap mode, and heatmap frames already show it.
 *   refusals  with the context's supersampling factor above 1 the call returns KIFS_ERR_BAD_ARG and writes nothing
 *             (a resolved pixel has no single hit).  Row shards and kifs_multi_* have no geometry form.
 *   bands     rows [y0, y1) are bit-identical to the same rows of the full frame; every frame of a batch is
 *             bit-identical to the lone call's.
 *   ordering  as the other async renders: kifs_order_after applies.
 *   launch    a geometry launch neither records tile costs nor advances the tile-order sort (as a supersampled launch
 *             does not); kifs_debug_last_kernel reports KIFS_KERNEL_GEOMETRY.
 * Every value equals the CPU restatement of the contract bit for bit (tests/geometry_reference.c). */
int kifs_render_geometry_async(kifs_ctx* ctx, void* hip_stream, int count,
                               const KifsCameraUniform* cameras,
                               uint8_t* const* dev_outs_rgba8, size_t pitch_bytes,
                               float* dev_geometry, size_t geometry_pitch_bytes, size_t geometry_stride_bytes,
                               int y0, int y1, int encode);

/* ---- extension: adaptive anti-aliasing -- supersample only the pixels on an edge -----------------
 * NOT part of the reference.  kifs_set_supersampling pays k^2 rays for every pixel; nine tenths of a frame of these
 * scenes are flat background or smooth surface, where a second sample changes nothing.  This call renders the frame
 * once with its geometry (kifs_render_geometry_async's texels, kept in memory the context owns), marks the pixels whose
 * geometry differs from a neighbour's and gives only those the k x k resolve.  Whole frames only.
 *   frames    frame i is rendered with cameras[i] into dev_outs_rgba8[i] (rows pitch_bytes apart, pitch_bytes >= 4 W and
 *             a multiple of 4); cameras == NULL with count == 1: the context's camera.  1 <= count <= KIFS_MAX_BATCH; a
 *             large batch may run as several launches over the same scratch memory.  Stream, ordering and
 *             kifs_order_after as the other async renders.
 *   texel     g(p) = (n, t): the texel kifs_render_geometry_async defines for pixel p.  hit(p): t's bit pattern is not
 *             0x7f800000.
 *   pair      for p and a 4-neighbour q INSIDE the frame, (x +- 1, y) or (x, y +- 1) -- neighbours outside it do not
 *             exist -- in f32 without fma: d = (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z;
 *             pair(p, q) = hit(p) != hit(q), or both hit and ( !(d >= normal_cos) or
 *             fabsf(t_p - t_q) > depth_rel * fminf(t_p, t_q) ).  E(p) = the OR of pair(p, q) over p's neighbours.  The
 *             rule is symmetric: a background pixel beside a hit is an edge pixel too.
 *   output    where E(p) is false the pixel holds exactly the bytes kifs_render_batch_async writes; where it is true,
 *             exactly the bytes a render with kifs_set_supersampling(ctx, factor) writes for it: the same virtual
 *             k W x k H screen, sample order, division by k^2 and encode; heatmap frames resolve heatmap colours, soft
 *             shadows apply per sample.  The mask always comes from the primary ray's geometry.  Bytes of a row beyond
 *             4 W are not touched.
 *   counts    dev_edge_counts, when not NULL, points to `count` words of device memory: word i receives the number of
 *             edge pixels of frame i, valid once the stream has reached that point.
 *   refusals  a refused call launches and writes nothing.  KIFS_ERR_BAD_ARG: a null ctx, dev_outs_rgba8 or aa; a factor
 *             outside 2 .. KIFS_MAX_SUPERSAMPLING; a NaN normal_cos; a NaN or negative depth_rel; the context's own
 *             supersampling factor above 1; a bad pitch.  KIFS_ERR_BAD_SIZE: k W or k H above 65536.
 *             KIFS_ERR_RUNTIME is no refusal: a HIP call failed after work was enqueued, and the destinations and the
 *             counts are undefined.
 *   streams   the scratch memory belongs to the context: a call on another stream than the context's previous adaptive
 *             call is ordered after that call by the library (an event behind its last pass), so calls of one context
 *             may alternate between streams without caller-side ordering; they then run one after the other.
 *   no bands  bands, row shards and kifs_multi_* have no adaptive form: the mask of a band's first and last row needs
 *             rows outside the band.
 *   launch    like a geometry launch the call neither records tile costs nor advances the tile-order sort;
 *             kifs_debug_last_kernel reports KIFS_KERNEL_ADAPTIVE. */
typedef struct KifsAdaptiveAA {
    int32_t factor;    /* k: 2 .. KIFS_MAX_SUPERSAMPLING */
    float normal_cos;  /* two hits whose normals' dot product is not >= this are an edge */
    float depth_rel;   /* two hits with |t_p - t_q| > depth_rel * min(t_p, t_q) are an edge; >= 0, +inf allowed */
} KifsAdaptiveAA;
int kifs_render_adaptive_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras,
                               uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsAdaptiveAA* aa,
                               uint32_t* dev_edge_counts /* may be NULL */, int encode);

/* ---- extension: animated batches -- per-frame Julia constant, power and colours in one launch -----
 * NOT part of the reference (it renders the GUI's current options, one frame per draw: graphics.rs:304-325).
 * kifs_render_batch_async varies the camera only; the sequence made most often with these scenes is a MORPH -- the
 * constant, the power or the colours change from frame to frame (the sliders of GuiData.constant, .power,
 * .fractal_color, .background_color).  This call renders such a sequence as one launch, the long rays of all its frames
 * side by side.
 *   frames    frame i is rendered into dev_outs_rgba8[i] with cameras[i] (cameras == NULL: the context's camera for every
 *             frame) and options[i]: `count` option images, one per frame, never NULL.  Screen, iteration counts and
 *             extensions are the context's.  Rows [y0, y1), pitch_bytes, encode, stream and kifs_order_after as
 *             kifs_render_batch_async.  1 <= count <= KIFS_MAX_BATCH.
 *   context   the context's own options are neither read nor changed and need not have been set.  The screen must be
 *             set; the camera only when cameras == NULL.
 *   varying   constant, power, fractal_color and background_color may differ from frame to frame.  max_iterations,
 *             max_distance, epsilon, is_heatmap, fractal_group_id and primitive_id must be bit-identical to options[0]'s
 *             in every frame (a sequence shares one pipeline and one march budget): otherwise KIFS_ERR_BAD_ARG.  Padding
 *             words are ignored.
 *   output    frame i holds exactly the bytes kifs_render_async writes for those rows after kifs_set_camera(cameras[i])
 *             and kifs_set_options(options[i]), for every pipeline, heatmap frames and soft shadows included.  Bytes of a
 *             row beyond 4 W are not touched.
 *   refusals  a refused call launches and writes nothing.  KIFS_ERR_BAD_ARG: a null ctx, options or dev_outs_rgba8; a
 *             null or misaligned destination; count out of range; a bad encode or band; a fractal_group_id above 2; frames
 *             that differ where they may not; the context's supersampling factor above 1 (an anti-aliased morph is
 *             kifs_render_accumulate_jittered_async's whole-grid form).  KIFS_ERR_BAD_SIZE: a bad pitch.
 *             KIFS_ERR_UNCONFIGURED: no screen, or no camera with
 *             cameras == NULL.
 *   tables    the frames' scenes reach the kernel through a device table: a ring of KIFS_ANIMATION_RING tables per
 *             context, each rewritten only once the launch that read it is over -- a call that finds its table busy
 *             (more than KIFS_ANIMATION_RING calls ahead of the device) waits for that launch on the host.
 *   launch    like a geometry launch the call neither records tile costs nor advances the tile-order sort;
 *             kifs_debug_last_kernel reports KIFS_KERNEL_ANIMATION, kifs_debug_last_round_steps 0,
 *             kifs_debug_last_group_tiles and kifs_debug_last_bunny_form -1.
 *   no shards row shards and kifs_multi_* have no animated form. */
#define KIFS_ANIMATION_RING 4
int kifs_render_animation_async(kifs_ctx* ctx, void* hip_stream, int count,
                                const KifsCameraUniform* cameras,   /* NULL: the context's camera for every frame */
                                const KifsOptionsUniform* options,  /* count images, one per frame; not NULL */
                                uint8_t* const* dev_outs_rgba8, size_t pitch_bytes,
                                int y0, int y1, int encode);

/* ---- extension: accumulated frames -- motion blur, depth of field and temporal anti-aliasing in one launch -----
 * NOT part of the reference (every frame it draws is an instantaneous pinhole exposure: entry.wgsl:49-59).  A film made
 * of these sequences wants motion blur over the shutter interval, depth of field from a finite lens, a morph without
 * temporal aliasing.  All three are one operation: the average of several SUB-FRAMES that differ in camera, scene or
 * both, taken in linear colour before the encode -- which no caller can do from encoded RGBA8 bytes.
 *   sub-frames  output frame i, 0 <= i < count, has sub-frames s = 0 .. samples-1; sub-frame s is view v = i * samples + s.
 *             Its colour c_s(p) is the linear colour fs_main returns for pixel p with cameras[v] and options[v]
 *             (options == NULL: the context's options for every view).  Screen, iteration counts and extensions are the
 *             context's; heatmap colours and soft shadows apply per sub-frame.  These are exactly the values a plain
 *             render encodes.  The context's own camera is neither used nor changed.
 *   resolve   per channel in f32, without fma: acc = c_0(p); acc = acc + c_s(p) for s = 1 .. samples-1, in that order;
 *             mean = acc / float(samples), correctly rounded; then the frame's encoder (sRGB or UNORM; alpha 255), into
 *             dev_outs_rgba8[i].
 *   single    samples = 1 gives the bytes of kifs_render_batch_async exactly.
 *   misses    a sub-frame whose ray misses contributes its own background_color; rays dropped by any cull are misses.  A
 *             pixel that every sub-frame misses is the same formula applied to the backgrounds -- not the encoded
 *             background pixel: three equal f32 values summed and divided by 3 need not give the value back, and the
 *             sub-frames' backgrounds may differ.
 *   limits    1 <= samples <= KIFS_MAX_ACCUMULATE, 1 <= count, count * samples <= KIFS_MAX_BATCH.
 *   varying   as kifs_render_animation_async, over all count * samples images: constant, power, fractal_color and
 *             background_color may differ; max_iterations, max_distance, epsilon, is_heatmap, fractal_group_id and
 *             primitive_id must be bit-identical to options[0]'s in every image.  Padding words are ignored.
 *   bands     rows [y0, y1), pitch_bytes, encode, stream and kifs_order_after as kifs_render_batch_async: a band is
 *             bit-identical to the same rows of the whole frame; bytes of a row beyond 4 W are not touched.
 *   refusals  a refused call launches and writes nothing.  KIFS_ERR_BAD_ARG: a null ctx, cameras or dev_outs_rgba8; a
 *             null or misaligned destination; samples outside 1 .. KIFS_MAX_ACCUMULATE; count below 1 or count * samples
 *             above KIFS_MAX_BATCH; a bad encode or band; a fractal_group_id above 2; images that differ where they may
 *             not; the context's supersampling factor above 1 (sub-frames that also anti-alias are
 *             kifs_render_accumulate_jittered_async's, below).  KIFS_ERR_BAD_SIZE: a bad pitch.  KIFS_ERR_UNCONFIGURED: no screen, or no options with options == NULL.
 *   tables    the views' scenes travel through the ring of kifs_render_animation_async's tables (KIFS_ANIMATION_RING
 *             per context, shared by both calls), with the context's scene in every record when options == NULL.
 *   launch    like an animated launch the call neither records tile costs nor advances the tile-order sort and is not
 *             timed by kifs_set_profiling; kifs_debug_last_kernel reports KIFS_KERNEL_ACCUMULATE,
 *             kifs_debug_last_round_steps 0, kifs_debug_last_group_tiles and kifs_debug_last_bunny_form -1.
 *   no shards row shards, the geometry output, adaptive anti-aliasing and kifs_multi_* have no accumulated form. */
#define KIFS_MAX_ACCUMULATE 64
int kifs_render_accumulate_async(kifs_ctx* ctx, void* hip_stream, int count, int samples,
                                 const KifsCameraUniform* cameras,   /* count * samples images; not NULL */
                                 const KifsOptionsUniform* options,  /* count * samples images, or NULL: the context's options */
                                 uint8_t* const* dev_outs_rgba8,     /* count destinations */
                                 size_t pitch_bytes, int y0, int y1, int encode);

/* ---- extension: jittered accumulated frames -- a sub-pixel cell per sub-frame, so that blur also anti-aliases -----
 * NOT part of the reference.  kifs_render_accumulate_async sends every sub-frame's ray through the pixel centre: its
 * frames are blurred where something moves and stair-stepped where nothing does.  Distributed ray tracing gives each
 * sub-frame another point of the pixel instead, and the S rays of the blur anti-alias as well -- not S k^2 rays.
 *   base      everything kifs_render_accumulate_async says holds: sub-frames and views, the resolve and its order, misses,
 *             limits, what may vary between option images, bands, tables and the launch's debug hooks
 *             (KIFS_KERNEL_ACCUMULATE; not timed by kifs_set_profiling).
 *   cells     the one difference.  With g = grid, sub-frame v = i_frame * samples + s shades pixel
 *             (g x + cells[v].i, g y + cells[v].j) of the VIRTUAL screen kifs_set_supersampling defines for k = g: width
 *             g W, height g H, the same aspect_ratio float, the same fs_main at the same kind of fragment centre.  (x, y)
 *             is the output pixel, global in a band.  Heatmap colours and soft shadows apply per sub-frame at the
 *             sub-frame's own point.
 *   NULL      cells == NULL is allowed only with samples == grid * grid: sub-frame s of every frame then takes cell
 *             (s % grid, s / grid) -- the supersampling order.  With one camera and one scene for all of a frame's
 *             sub-frames and grid <= KIFS_MAX_SUPERSAMPLING the frame holds exactly the bytes
 *             kifs_set_supersampling(ctx, grid) + kifs_render_batch_async write.
 *   grid 1    cells must be (0, 0) or NULL, and the call is kifs_render_accumulate_async exactly (the same kernel).
 *   refusals  a refused call launches and writes nothing.  KIFS_ERR_BAD_ARG: everything kifs_render_accumulate_async
 *             refuses with that status, the context's own supersampling factor above 1 included; grid outside
 *             1 .. KIFS_MAX_JITTER_GRID; a cell with i >= grid or j >= grid; cells == NULL with samples != grid * grid.
 *             KIFS_ERR_BAD_SIZE: a bad pitch; g W or g H above 65536, as for supersampling.  KIFS_ERR_UNCONFIGURED as the
 *             unjittered call. */
#define KIFS_MAX_JITTER_GRID 8
typedef struct KifsSubpixel { uint8_t i, j; } KifsSubpixel;   /* cell of the g x g grid inside a pixel: column i, row j */
int kifs_render_accumulate_jittered_async(kifs_ctx* ctx, void* hip_stream, int count, int samples,
                                          const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
                                          int grid, const KifsSubpixel* cells /* count * samples, or NULL */,
                                          uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, int y0, int y1, int encode);

/* ---- extension: progressive accumulation -- a frame's linear sums carried across launches ----
 * NOT part of the reference.  The two calls above average at most KIFS_MAX_ACCUMULATE sub-frames and start from nothing
 * every time: the running f32 sum lives inside the launch, and no caller can continue it from encoded RGBA8 bytes.  This
 * call makes the resolve's accumulator resumable: a PASS starts from a plane of f32 sums left by earlier passes, adds its
 * own sub-frames in the contract's order, writes the sums back and, when asked, encodes sum / float(total).  A lens at
 * hundreds of samples per pixel is a sequence of passes; so is a viewer that refines its picture while nothing moves.
 *   base      everything kifs_render_accumulate_jittered_async says holds for the pass's own count * samples views: views
 *             and cells (grid = 1: cells (0, 0) or NULL, the pixel centre), what may vary between option images, misses,
 *             limits (samples <= KIFS_MAX_ACCUMULATE PER PASS), bands, the tables and the debug hooks
 *             (KIFS_KERNEL_ACCUMULATE; not timed by kifs_set_profiling).
 *   plane     one 16-byte texel per pixel, four f32: (sum.r, sum.g, sum.b, float(total)).  The layout is the geometry
 *             output's: row y of frame i at (char*)dev_sums + i * sums_stride_bytes + (y - y0) * sums_pitch_bytes.  The base
 *             is 16-byte aligned; the pitch is >= 16 W and a multiple of 16; the stride is a multiple of 16 and, with
 *             count > 1, >= (y1 - y0) * sums_pitch_bytes.  Bytes of a row beyond 16 W are not touched.
 *   fold      per channel in f32, without fma.  prior_samples == 0: the plane is NOT READ, whatever it holds (NaNs
 *             included): acc = c_0(p); acc = acc + c_s(p) for s = 1 .. samples-1.  prior_samples > 0: acc = the texel's
 *             sum; acc = acc + c_s(p) for s = 0 .. samples-1.  Either way total = prior_samples + samples and the texel
 *             becomes (acc, float(total)).  The w word is written and never read: it makes the plane self-describing for
 *             a caller that wants the linear HDR mean, sum / w.
 *   picture   with dev_outs_rgba8 != NULL frame i receives encode(acc / float(total)): the divide correctly rounded, the
 *             encoder the frame's, exactly as the resolve of the calls above.  With NULL the pass only advances the
 *             plane, and pitch_bytes is ignored.
 *   identities (a) prior_samples == 0 with a picture gives the bytes of kifs_render_accumulate_jittered_async for the
 *             same arguments (at grid 1: of kifs_render_accumulate_async).  (b) Passes whose views concatenate to one
 *             call's views give that call's bytes after the last pass, for any split: the fold is a left fold.  Beyond
 *             KIFS_MAX_ACCUMULATE sub-frames the same formula defines the result.  (c) The library keeps NO STATE between
 *             passes: the plane and prior_samples are the whole state.  Passes may come from different streams or from
 *             different contexts of the device; passes on different streams must be ordered by the caller, e.g. with
 *             kifs_order_after.
 *   refusals  a refused call launches and writes nothing.  Everything kifs_render_accumulate_jittered_async refuses, with
 *             its status, except that dev_outs_rgba8 itself may be NULL (a null or misaligned ENTRY of a non-NULL array
 *             is still KIFS_ERR_BAD_ARG).  Then KIFS_ERR_BAD_ARG: a null or misaligned dev_sums; a bad plane pitch or
 *             stride; prior_samples + samples > KIFS_MAX_PROGRESSIVE_SAMPLES.
 *   no shards row shards, the geometry output, adaptive anti-aliasing and kifs_multi_* have no progressive form. */
#define KIFS_MAX_PROGRESSIVE_SAMPLES 16777216u   /* 2^24: float(total) stays exact */
int kifs_render_accumulate_resume_async(kifs_ctx* ctx, void* hip_stream, int count, int samples,
                                        const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
                                        int grid, const KifsSubpixel* cells,
                                        float* dev_sums, size_t sums_pitch_bytes, size_t sums_stride_bytes, uint32_t prior_samples,
                                        uint8_t* const* dev_outs_rgba8 /* NULL: no picture from this pass */,
                                        size_t pitch_bytes, int y0, int y1, int encode);

/* ---- extension: converging accumulation -- stop sampling the pixels whose mean has settled ----
 * NOT part of the reference.  A progressive frame of the call above marches every pixel in every pass.  This pass carries
 * a per-pixel count and a per-pixel second moment beside the sums, marches only the pixels whose mean has not settled,
 * skips the 8 x 8 blocks in which none is left, and tells the caller how many pixels remain.
 *   base      everything kifs_render_accumulate_resume_async says holds for the pass's own count * samples views: views,
 *             cells and grid 1, what may vary between option images, misses, bands, samples <= KIFS_MAX_ACCUMULATE per
 *             pass, the debug hooks (KIFS_KERNEL_ACCUMULATE; not timed by kifs_set_profiling); no shard, geometry,
 *             adaptive or kifs_multi_* form.
 *   state     two planes of the caller's and nothing in the library.  dev_sums is the resume call's plane, same layout and
 *             rules: (sum.r, sum.g, sum.b, n) -- here n is THE PIXEL'S OWN count of sub-frames, and it is read.
 *             dev_moments holds one f32 per pixel, q = the sum of the squared luminances of the pixel's sub-frames: row y
 *             of frame i at (char*)dev_moments + i * moments_stride_bytes + (y - y0) * moments_pitch_bytes.  Its base is
 *             4-byte aligned; the pitch is >= 4 W and a multiple of 4; the stride is a multiple of 4 and, with count > 1,
 *             >= (y1 - y0) * moments_pitch_bytes.  Bytes of a row beyond 4 W are not touched.
 *   rule      all in f32, without fma; tolerance * tolerance is one f32 multiply done on the host.
 *                 Y(c)       = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b
 *                 L = Y(sum);  d = n*q - L*L;  b = (tolerance*tolerance) * ((n*n) * (n - 1.0f))
 *                 settled(p) = n >= float(min_samples)  &&  d <= b        (a NaN compares false: not settled)
 *                 active(p)  = !settled(p)  &&  n + float(samples) <= 16777216.0f
 *             i.e. "variance of the mean <= tolerance^2", multiplied out so that there is no divide.  With restart != 0
 *             NEITHER PLANE IS READ, whatever they hold (NaNs included): every pixel is active with n = 0.  With
 *             restart == 0 `active` is evaluated on the state the planes hold when the pass starts, with THIS call's rule:
 *             a caller may tighten the tolerance between passes.  At tolerance 0 even identical samples need not settle:
 *             n*q - L*L rounds.
 *   pass      an active pixel folds all `samples` sub-frames in the contract's order, exactly as the resume call does: on
 *             restart acc = c_0, then + c_s; otherwise acc = sum, then + c_0 ...; q folds the same way over Y(c_s)*Y(c_s);
 *             its texel becomes (acc, n + float(samples)) and its moment the new q.  An inactive pixel's texel and moment
 *             are NOT WRITTEN and none of its rays is marched.
 *   picture   with dev_outs_rgba8 != NULL every pixel of the band receives encode(sum / n) of its state after the pass, an
 *             inactive pixel from the texel as it stands.  NULL: the pass only advances the planes.
 *   counts    dev_active_counts[i], when given, receives the number of pixels of rows [y0, y1) of frame i for which
 *             `active` holds on the state AFTER the pass, with this call's rule and samples; the words are zeroed on the
 *             stream first.  Zero: the frame is done.
 *   identities (a) a restart pass with a picture writes the bytes of kifs_render_accumulate_jittered_async, and its sums
 *             plane has the resume call's bits.  (b) With min_samples above every count reached, any sequence of passes
 *             leaves the sums plane and the pictures of the same sequence of resume passes.  (c) With tolerance +inf every
 *             pixel stops at the end of the first pass after which n >= min_samples.  (d) No state between passes: they
 *             may come from other streams or contexts, ordered by the caller.
 *   refusals  a refused call launches and writes nothing.  Everything kifs_render_accumulate_resume_async refuses, with
 *             its status.  Then KIFS_ERR_BAD_ARG: a null or misaligned dev_moments, a bad moments pitch or stride; a null
 *             rule; a NaN or negative tolerance (+inf is allowed); min_samples < 2 or > 2^24.  y1 == y0 returns KIFS_OK,
 *             enqueues nothing and leaves the counts untouched. */
typedef struct KifsConvergence {
    float    tolerance;    /* standard error of the mean linear luminance at which a pixel stops; >= 0, not NaN, +inf allowed */
    uint32_t min_samples;  /* a pixel holding fewer sub-frames than this never stops; >= 2 */
} KifsConvergence;
int kifs_render_accumulate_converge_async(kifs_ctx* ctx, void* hip_stream, int count, int samples,
                                          const KifsCameraUniform* cameras, const KifsOptionsUniform* options,
                                          int grid, const KifsSubpixel* cells,
                                          float* dev_sums, size_t sums_pitch_bytes, size_t sums_stride_bytes,
                                          float* dev_moments, size_t moments_pitch_bytes, size_t moments_stride_bytes,
                                          int restart, const KifsConvergence* rule,
                                          uint32_t* dev_active_counts /* may be NULL */,
                                          uint8_t* const* dev_outs_rgba8 /* may be NULL */,
                                          size_t pitch_bytes, int y0, int y1, int encode);

/* ---- extension: ray queries -- trace caller-supplied rays to hit, normal and colour ---------------
 * NOT part of the reference, whose every ray is a pixel of its pinhole camera (entry.wgsl:49-59).  Every other entry
 * point shades the rays of that camera model; this one takes the RAYS: picking and autofocus (what does this pixel hit,
 * and how far away), collision probes along a path, secondary rays from a hit point, and cameras the library does not
 * model (an equirectangular panorama, a fisheye, an orthographic view) are each just another set of rays.
 *   rays      n records of 32 bytes in device memory, 16-byte aligned; the two reserved words are not read.
 *   march     ray k is marched exactly as entry.wgsl:11-25 marches a pixel's ray, in the contract's arithmetic, with the
 *             record's origin and direction in the camera's place: t = 0, p = origin; while i < max_iterations and
 *             t < max_distance: d = scene_SDF(p); d < epsilon: the ray hits and the loop breaks with i un-incremented;
 *             otherwise t = t + d and p = fma(t, direction, origin) per component.
 *   direction used as given, NOT normalised: t is in units of its length.  A zero direction is a ray that stands still.
 *   state     the scene is the context's options, iteration counts and extensions at the call.  The screen, the camera
 *             and the supersampling factor are not read: the call works on a context that never had kifs_set_screen or
 *             kifs_set_camera called, and at any supersampling factor.
 *   texel     dev_geometry[4 k ..]: (n.x, n.y, n.z, t) on a hit -- n the vector get_normal returned at the tested
 *             position, t the parameter at the break -- and (0, 0, 0, +inf), bit pattern 0, 0, 0, 0x7f800000, on a miss:
 *             the words of kifs_render_geometry_async's texel.
 *   colour    dev_rgba8[4 k ..]: the pixel the same ray would have produced in a frame -- the shading of
 *             entry.wgsl:16-19 encoded with `encode`, alpha 255; the heatmap colour from i; the soft-shadow secondary
 *             march from the hit when the extension is on; the background on a miss.
 *   outputs   either may be NULL, not both.  The bytes of the one that is given do not depend on whether the other is.
 *             Exactly 16 n and 4 n bytes are written.  dev_geometry is 16-byte aligned, dev_rgba8 4-byte aligned.
 *   non-finite  a ray with a NaN or an infinity among its six components gets unspecified words in its own two slots; it
 *             cannot affect another ray and cannot run longer than max_iterations steps.
 *   refusals  a refused call launches nothing and writes nothing.  KIFS_ERR_BAD_ARG: n < 0 or n > KIFS_MAX_RAYS; a NULL or
 *             misaligned dev_rays; a misaligned output; both outputs NULL; a bad encode.  KIFS_ERR_UNCONFIGURED: options
 *             never set.  n == 0 (with otherwise good arguments) returns KIFS_OK and enqueues nothing.
 *   ordering  enqueued on hip_stream (NULL: the context's own) as the other async calls: kifs_order_after applies.
 *   launch    not a render launch: it neither records tile costs nor advances the tile order, leaves
 *             kifs_debug_last_kernel and kifs_debug_last_round_steps as they were and touches no profiling record.
 * Every word equals the CPU restatement of the contract bit for bit (tests/ray_reference.c). */
typedef struct KifsRay {          /* 32 bytes, 16-byte aligned */
    float origin[3];    float reserved0;   /* reserved words are not read */
    float direction[3]; float reserved1;
} KifsRay;
#define KIFS_MAX_RAYS (1 << 28)
int kifs_trace_rays_async(kifs_ctx* ctx, void* hip_stream, const KifsRay* dev_rays, int n,
                          float* dev_geometry /* n texels of 16 B, or NULL */,
                          uint8_t* dev_rgba8  /* n pixels of 4 B, or NULL */, int encode);

/* ---- extension: ambient occlusion (not in the reference) ------------------------------------------------------------
 * kifs_render_batch_async whose hits are additionally attenuated by how closed the surface is around them: a few
 * estimates taken along the normal, each compared with how far it stands off the hit.  The call is a render of its own
 * (kifs_occlusion_kernels.hip); no other entry point computes the term.
 *   factor    a primary ray that hit at the tested position p with the normal n the shading used (the vector get_normal
 *             returned, kifs_render_geometry_async's texel), S = samples; all f32, no fused operation but the one written:
 *                 occ = 0; w = 1
 *                 for i = 1..S:  h = step * float(i);  q = fma(h, n, p) per component;  d = scene_SDF(q)
 *                                occ = occ + w * (h - d);  w = w * decay
 *                 a = min(max(1 - strength * occ, 0), 1)      (as C ternaries: a NaN stays a NaN)
 *   colour    (a r, a g, a b) of the hit's colour (r, g, b) exactly as every other entry point computes it, the
 *             soft-shadow factor included when that extension is on; a miss -- every ray the culls drop -- is the
 *             background; a heatmap frame's colour is the counter's, unattenuated.  A NaN factor makes a NaN colour, which
 *             the encoders map to 0 (the generalised Julia set's NaN normals).
 *   samples   the context's supersampling factor k is honoured: each of the k^2 samples of a pixel is attenuated by its
 *             own factor and the samples are resolved exactly as kifs_set_supersampling specifies.
 *   plane     dev_occlusion NULL, or one f32 per pixel: row y of frame i at dev_occlusion + i * occlusion_stride_bytes +
 *             (y - y0) * occlusion_pitch_bytes.  A hit stores a (in heatmap mode too), a miss 1.0f; bytes beyond 4 W of a
 *             row are not touched.  The base is 4-byte aligned, the pitch at least 4 W and a multiple of 4, the stride a
 *             multiple of 4 and, for count > 1, at least (y1 - y0) * pitch.  With k > 1 a resolved pixel has no single
 *             factor: a plane is refused.
 *   frames    1 <= count <= KIFS_MAX_OCCLUSION_BATCH; cameras NULL with count 1: the context's camera.  Rows [y0, y1) are
 *             bit-identical to the same rows of the full frame, every frame of a batch to the lone call.
 *   refusals  a refused call launches nothing and writes nothing.  KIFS_ERR_BAD_ARG: a NULL ctx, dev_outs_rgba8 or ao; a
 *             field of ao outside its range or not finite; count outside 1..KIFS_MAX_OCCLUSION_BATCH; NULL cameras with
 *             count != 1; a bad band, plane layout or encode; a plane with k > 1.  KIFS_ERR_BAD_SIZE (pitch, frame size)
 *             and KIFS_ERR_UNCONFIGURED as kifs_render_batch_async.
 *   ordering  enqueued on hip_stream (NULL: the context's own) as the other async calls: kifs_order_after applies.
 *   launch    not a feedback launch: it neither records tile costs nor advances the tile order, leaves
 *             kifs_debug_last_kernel and kifs_debug_last_round_steps as they were and touches no profiling record.
 * Every byte and every factor equals the CPU restatement of the contract bit for bit (tests/occlusion_reference.c). */
#define KIFS_MAX_AO_SAMPLES 16
#define KIFS_MAX_OCCLUSION_BATCH 64
typedef struct KifsAmbientOcclusion {
    int32_t samples;   /* S: 1..KIFS_MAX_AO_SAMPLES */
    float   step;      /* probe spacing along the normal, scene units: finite, > 0 */
    float   decay;     /* weight of probe i+1 over probe i: finite, 0 < decay <= 1 */
    float   strength;  /* finite, >= 0 */
} KifsAmbientOcclusion;
int kifs_render_occlusion_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsAmbientOcclusion* ao,
                                float* dev_occlusion, size_t occlusion_pitch_bytes, size_t occlusion_stride_bytes,
                                int y0, int y1, int encode);

/* ---- extension: a configurable light (not in the reference) --------------------------------------------------------
 * kifs_render_batch_async with a different shading of the hits: the light's direction, its ambient and diffuse weights
 * and a Blinn-Phong highlight are the caller's, and the occlusion term of kifs_render_occlusion_async may be applied on
 * top.  The call is a render of its own (kifs_lighting_kernels.hip); one light per call.
 *   hit       p is the tested position, n the normal the shading uses, dir the ray direction of the sample, fc the
 *             fractal colour.  All f32 with dot3(a,b) = fma(a.z,b.z, fma(a.y,b.y, a.x*b.x)), normalize3(v) =
 *             v / sqrt(dot3(v,v)) with IEEE divide and square root, clamp_ as C ternaries (a NaN stays a NaN); no fused
 *             operation but those written:
 *                 l = light.direction;  Lh = normalize3(l);  lit0 = clamp_(dot3(n, l), 0, 1)
 *                 sh = 1;  if the soft-shadow extension is on and lit0 > 0: sh = the secondary march of
 *                          KifsExtensions, unchanged, with Lh in the place of normalize((1,1,1))
 *                 lit = lit0 * sh  (only when the extension is on; otherwise lit = lit0)
 *                 k = fma(light.diffuse, lit, light.ambient);  c = (k fc.r, k fc.g, k fc.b)
 *                 if any of light.specular[] is not zero:
 *                     h = normalize3(Lh - dir);  s = clamp_(dot3(n, h), 0, 1);  e times: s = s * s
 *                     spec = (lit0 > 0) ? s * sh : 0      (a select: a NaN in the unselected arm is not used)
 *                     c.x = fma(light.specular[x], spec, c.x)  per channel
 *                 if ao != NULL: a = the factor of kifs_render_occlusion_async at (p, n), unchanged;  c = (a c.r, a c.g, a c.b)
 *   other     a miss -- every ray the culls drop -- is the background; a heatmap frame's colour is the counter's, unlit
 *             and unattenuated.
 *   samples   the context's supersampling factor k is honoured sample by sample, as kifs_render_occlusion_async does.
 *   frames    1 <= count <= KIFS_MAX_LIGHT_BATCH; cameras NULL with count 1: the context's camera.  Rows [y0, y1) are
 *             bit-identical to the same rows of the full frame, every frame of a batch to the lone call.
 *   identity  the light {(1,1,1), 0.1, 0.9, (0,0,0), any e} with ao NULL writes the bytes of kifs_render_batch_async, and
 *             with a term those of kifs_render_occlusion_async -- for every pipeline, with soft shadows, heatmap and
 *             k > 1: with l = (1,1,1) the fma chain of dot3 is (n.x + n.y) + n.z bit for bit.
 *   refusals  a refused call launches nothing and writes nothing.  KIFS_ERR_BAD_ARG: a NULL ctx, dev_outs_rgba8 or
 *             light; a direction component that is not finite, or a direction whose dot3(l,l) in f32 is zero, subnormal
 *             or infinite; a negative or non-finite ambient, diffuse or specular weight; shininess_log2 outside
 *             0..KIFS_MAX_SHININESS_LOG2; a non-NULL ao that kifs_render_occlusion_async would refuse; count outside
 *             1..KIFS_MAX_LIGHT_BATCH; NULL cameras with count != 1; a bad band or encode; a NULL or misaligned
 *             destination entry.  KIFS_ERR_BAD_SIZE and KIFS_ERR_UNCONFIGURED as kifs_render_occlusion_async.  y1 == y0
 *             returns KIFS_OK and enqueues nothing.
 *   launch    exactly the occlusion call's: not a feedback launch, no tile costs, no sort, no profiling record, the
 *             kifs_debug_last_* values left alone; ordered around the table's feedback launches on other streams.
 *   scope     deliberately absent: a plane of factors (the occlusion call has one); per-frame lights; a form in the
 *             accumulate, animation, adaptive, geometry and ray-query calls, in kifs_multi_* or in the viewer; a light
 *             colour; a second light.
 * Every byte equals the CPU restatement of the contract (tests/lighting_reference.c), which is normative where this text
 * and it could be read differently. */
#define KIFS_MAX_SHININESS_LOG2 10
#define KIFS_MAX_LIGHT_BATCH 64
typedef struct KifsLight {
    float   direction[3];    /* towards the light; used AS GIVEN in the direct term, normalised for shadow and highlight */
    float   ambient;         /* finite, >= 0   (reference: 0.1) */
    float   diffuse;         /* finite, >= 0   (reference: 0.9) */
    float   specular[3];     /* linear RGB weight of the highlight; finite, >= 0; all three zero: no highlight is computed */
    int32_t shininess_log2;  /* e: the Blinn-Phong exponent is 2^e, by e squarings; 0..KIFS_MAX_SHININESS_LOG2 */
} KifsLight;
int kifs_render_lit_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras,
                          uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsLight* light,
                          const KifsAmbientOcclusion* ao /* may be NULL */, int y0, int y1, int encode);

/* ---- extension: orbit-trap surface colouring (not in the reference) ------------------------------------------------
 * kifs_render_lit_async with a colour per hit in the place of the one fractal colour: a gradient over how close the
 * orbit that the pipeline iterates from the hit point comes to a trap -- a point, a line or a plane of orbit space.  The
 * call is a render of its own (kifs_trap_kernels.hip); one trap per call.  All f32 in the order written, fma only where
 * written, square root correctly rounded, comparisons as C ternaries.
 *   orbit     of a hit at the tested position p (the geometry texel's, the occlusion probes'): z_0 = (p.x, p.y, p.z, w0),
 *             w0 = 0.1 for the two Julia groups and 0 for KIFS_GROUP_KIFS.
 *               Julia (power 2)      z_{k+1} = quat_sq_add(z_k, c): real = fma(x,x,-d) + c.x with d = fma(w,w, y*y + z*z),
 *                                    ijk = fma(2x, ijk, c.ijk).  Point k+1 takes part in the minimum; after that the orbit
 *                                    stops if fma(x,x,d) of z_{k+1} > max_distance.
 *               generalised Julia    z_{k+1} = quat_pow(z_k, power) + c per component, quat_pow as the normal's
 *                                    estimate takes it; the stop rule is the Julia one.
 *               Sierpinski           z_{k+1}.xyz = fma(2, tetrahedral_fold(z_k.xyz), -1) per component, w stays 0; no stop
 *                                    rule.
 *               every other primitive, the bunny and unknown primitive ids: z_0 only -- the trap is a function of position.
 *   distance  e = z - centre per component; d(z) = 0, then d = fma(e_i, e_i, d) for the components i of `axes` in the
 *             order x, y, z, w (all four bits: a point trap; one bit: a plane; two or three: a line or an axis).
 *             m = d(z_0), then m = (d(z_k) < m) ? d(z_k) : m for k = 1..K as far as the orbit ran (a NaN distance is
 *             never taken);  u = sqrt(m).
 *   gradient  v = fma(scale, u, bias);  t = (v > 0) ? v : 0, then t = (t < 1) ? t : 1 (a NaN gives 0);  x = t * 2;
 *             j = (x >= 1) ? 1 : 0;  f = x - float(j);  the stops are s_0 = the options' fractal_color, s_1 = mid,
 *             s_2 = far;  per channel col = fma(f, s_{j+1} - s_j, s_j).
 *   shading   exactly kifs_render_lit_async's with col in the place of fc -- the direct term, the soft-shadow march
 *             towards the light, the weights, the highlight and the optional occlusion factor, in that call's order.
 *             light NULL: the light {(1,1,1), 0.1, 0.9, no highlight}.  A miss -- every ray the culls drop -- is the
 *             background; a heatmap frame's colour is the counter's and no trap is evaluated.
 *   samples, frames, ordering, launch: kifs_render_lit_async's -- supersampling honoured sample by sample; 1..
 *             KIFS_MAX_TRAP_BATCH frames, cameras NULL with count 1; bands bit-identical to the frame's rows and every
 *             frame of a batch to the lone call; not a feedback launch, the kifs_debug_last_* values left alone.
 *   identity  (a) scale = bias = 0 writes the bytes of kifs_render_lit_async for the same light and term -- with light
 *             NULL those of kifs_render_batch_async, and with a term those of kifs_render_occlusion_async: t = 0, f = 0 and
 *             fma(0, ., s_0) = s_0; a NaN or infinite u cannot leak through the ternaries.  (b) mid = far = fractal_color
 *             with any scale and bias writes the same bytes as (a).  Both hold for every pipeline, with soft shadows,
 *             heatmap and k > 1.
 *   refusals  a refused call launches nothing and writes nothing.  Everything kifs_render_lit_async refuses is refused
 *             with its status (a NULL light is not refused here).  KIFS_ERR_BAD_ARG also: a NULL trap; a centre
 *             component, scale or bias that is not finite; axes 0 or above 15; iterations outside
 *             0..KIFS_MAX_TRAP_ITERATIONS; a negative or non-finite colour.  y1 == y0 returns KIFS_OK and enqueues nothing.
 *   scope     deliberately absent: a plane of u; more than three stops; per-frame traps; a form in the accumulate,
 *             animation, adaptive, geometry, ray-query and multi-GPU calls or in the viewer.
 * kifs_eval_trap writes u for n positions (host pointers, like kifs_eval_points) with the context's options; it reads and
 * validates only centre, axes and iterations.  It exists for parity tests and for choosing a range for scale and bias.
 * Every byte and every u equals the CPU restatement of the contract (tests/trap_reference.c), which is normative where
 * this text and it could be read differently. */
#define KIFS_MAX_TRAP_ITERATIONS 32
#define KIFS_MAX_TRAP_BATCH 64
typedef struct KifsOrbitTrap {      /* 56 bytes */
    float    centre[4];   /* the trap point a, in orbit space (x, y, z, w); finite */
    uint32_t axes;        /* bit i set: component i takes part in the distance; 1..15 */
    int32_t  iterations;  /* K: orbit points after z_0; 0..KIFS_MAX_TRAP_ITERATIONS */
    float    scale, bias; /* t = clamp(scale * u + bias); finite */
    float    mid[3];      /* linear RGB at t = 1/2; finite, >= 0 */
    float    far[3];      /* linear RGB at t = 1;   finite, >= 0 */
} KifsOrbitTrap;
int kifs_render_trapped_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras,
                              uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsOrbitTrap* trap,
                              const KifsLight* light /* NULL: the reference's light */,
                              const KifsAmbientOcclusion* ao /* may be NULL */, int y0, int y1, int encode);
int kifs_eval_trap(kifs_ctx* ctx, const KifsOrbitTrap* trap, const float* points_xyz, int n, float* u_out);

/* ---- extension: kaleidoscopic IFS scenes (not in the reference) -----------------------------------------------------
 * kifs_render_lit_async with the scene's distance estimate replaced by that of a base primitive seen through N rounds of
 * fold, rotate and scale: Menger sponges, octahedral and rotated tetrahedral flakes, kaleidoscoped tori and bunnies.  The
 * call is a render of its own (kifs_fold_kernels.hip); one fold system per call.  All f32 in the order written, fma only
 * where written, divide and square root correctly rounded, comparisons as C ternaries (a NaN compares false).
 *   host      k = scale - 1;  t_i = -(k * offset[i]);  h = 0.5 * t_z   (f32)
 *   estimate  at the position p: acc = 1; for j = 0 .. N-1, while sqrt(dot3(p,p)) < max_distance (the reference's
 *             r < options.max_distance, dot3(a,b) = fma(a.z,b.z, fma(a.y,b.y, a.x*b.x)); a position whose test fails
 *             stops for good and keeps its p and acc), the stages of `stages` in THIS order, whatever the mask:
 *               1 ABS       p = (|x|, |y|, |z|)
 *               2 SORT      if (x < y) swap(x, y);  if (x < z) swap(x, z);  if (y < z) swap(y, z)   (descending; a NaN
 *                           is not moved)
 *               3 TETRA     the reference's tetrahedral_fold (kifs.wgsl:56-66): for the pairs (x,y), (y,z), (x,z):
 *                           sd = (a + b) * fl(1/sqrt(2));  m = 2 * min(sd, 0);  a = fma(-m, fl(1/sqrt(2)), a), b likewise
 *               4 ROTATE    q.x = fma(R[2], p.z, fma(R[1], p.y, R[0]*p.x)), q.y with R[3..5], q.z with R[6..8];  p = q.
 *                           Without the bit the matrix is not read; there is no hidden test for the identity
 *                           (fma(0, y, x) loses the sign of a zero)
 *               5 scale     always: p_i = fma(scale, p_i, t_i)
 *               6 MIRROR_Z  p.z = |p.z - h| + h   (the Menger rule "subtract the z offset only beyond its half", written
 *                           as a mirror so that it stays continuous under any base shape; scale 3, offset (1,1,1),
 *                           ABS|SORT|MIRROR_Z and the box: the sponge)
 *               7 acc = acc * scale
 *             the estimate is base(p) / acc, base the KIFS group's estimate of options.primitive_id at the folded point
 *             -- sphere, cylinder, box, torus, the Sierpinski estimate with the context's fold iterations, the bunny,
 *             the constant 1 of an unknown id.  The normal is the reference's central differences with h = epsilon
 *             over this estimate.
 *   frame     exactly kifs_render_lit_async's with the folded estimate wherever that call evaluates the scene's: the
 *             primary march, the normal, the soft-shadow march towards the light and the occlusion probes.  light NULL:
 *             the light {(1,1,1), 0.1, 0.9, no highlight}.  A heatmap frame shows the counter.
 *   culls     none: a ray is a miss only if the march says so.  The bounding-sphere culls of the other calls stand on
 *             the base primitive's radius, which a folded scene leaves (offset (3,0,0): the shape sits around
 *             |x| = 1.5); the launch runs with all three off.
 *   samples, frames, ordering, launch: kifs_render_lit_async's -- supersampling honoured sample by sample; 1..
 *             KIFS_MAX_FOLD_BATCH frames, cameras NULL with count 1; bands bit-identical to the frame's rows and every
 *             frame of a batch to the lone call; not a feedback launch, the kifs_debug_last_* values left alone.
 *   identity  iterations == 0 with any stages, matrix, scale and offset in range writes the bytes of
 *             kifs_render_lit_async for the same light and term -- with light NULL those of kifs_render_batch_async, and
 *             with a term those of kifs_render_occlusion_async -- for every KIFS primitive, with soft shadows, heatmap
 *             and k > 1: x / 1.0f is x.  kifs_eval_fold then gives kifs_eval_points' values.
 *   refusals  a refused call launches nothing and writes nothing.  Everything kifs_render_lit_async refuses is refused
 *             with its status (a NULL light is not refused here).  KIFS_ERR_BAD_ARG also: a NULL fold; stages > 31;
 *             iterations outside 0..KIFS_MAX_FOLD_ITERATIONS; a scale that is not finite or outside [1, 16]; an offset
 *             component that is not finite; with KIFS_FOLD_ROTATE a matrix entry that is not finite (without the bit the
 *             matrix is not looked at); options.fractal_group_id != KIFS_GROUP_KIFS -- the two Julia pipelines have no
 *             folded form.  y1 == y0 returns KIFS_OK and enqueues nothing.
 *   scope     deliberately absent: per-frame systems (an animated fold is a sequence of calls); a form in the
 *             accumulate, animation, adaptive, geometry, ray-query and multi-GPU calls or in the viewer; negative scales
 *             (Mandelbox-style folds); a certified cull radius for folded scenes.  (No longer absent: a trap on a folded
 *             scene is kifs_render_folded_trapped_async, below.)
 * kifs_eval_fold writes the folded estimate and/or its normal for n positions (host pointers, either output may be NULL,
 * like kifs_eval_points) with the context's options.
 * Every byte, every estimate and every normal equals the CPU restatement of the contract (tests/fold_reference.c), which
 * is normative where this text and it could be read differently. */
#define KIFS_MAX_FOLD_ITERATIONS 24
#define KIFS_MAX_FOLD_BATCH 64
enum KifsFoldStage { KIFS_FOLD_ABS = 1, KIFS_FOLD_SORT = 2, KIFS_FOLD_TETRA = 4, KIFS_FOLD_ROTATE = 8, KIFS_FOLD_MIRROR_Z = 16 };
typedef struct KifsFoldSystem {   /* 60 bytes */
    uint32_t stages;       /* OR of KifsFoldStage, 0..31; the stages run in the order above whatever the mask */
    int32_t  iterations;   /* N: 0..KIFS_MAX_FOLD_ITERATIONS */
    float    scale;        /* s: finite, 1 <= s <= 16 (s^24 stays a normal f32) */
    float    offset[3];    /* c: the fixed point of the scaling; finite */
    float    rotation[9];  /* row-major 3x3, USED AS GIVEN (not checked for orthonormality); finite; read only with KIFS_FOLD_ROTATE */
} KifsFoldSystem;
int kifs_render_folded_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras,
                             uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsFoldSystem* fold,
                             const KifsLight* light /* NULL: the reference's light */,
                             const KifsAmbientOcclusion* ao /* may be NULL */, int y0, int y1, int encode);
int kifs_eval_fold(kifs_ctx* ctx, const KifsFoldSystem* fold, const float* points_xyz, int n,
                   float* sdf_out, float* normal_out_xyz);

/* ---- extension: orbit-trap colouring of folded scenes (not in the reference) ----------------------------------------
 * The two extensions above composed: kifs_render_folded_async with a colour per hit in the place of the one fractal
 * colour, from the orbit that the folded estimate already iterates -- the point after each round -- continued by the base
 * primitive's own.  The call is a render of its own (kifs_fold_trap_kernels.hip); one fold system and one trap per call.
 * All f32 in the order written, fma only where written, square root correctly rounded, comparisons as C ternaries (a NaN
 * compares false).  K is trap->iterations, N is fold->iterations.
 *   orbit     of a hit at the tested position p (the one the shading uses): z_0 = (p.x, p.y, p.z, 0).
 *               fold part   the folded estimate's loop exactly as kifs_render_folded_async states it: the same stop test
 *                           sqrt(dot3(p,p)) < max_distance, the same stages in the same order, the same scale step.
 *                           After each round j = 0..N-1 that ran for this position z_{j+1} = (p after MIRROR_Z, 0).  A
 *                           position whose stop test fails contributes no further fold points and keeps its p.  Fold
 *                           point k takes part only while k <= K.
 *               base part   K_b = max(K - N, 0), from N and not from the rounds that ran.  Base primitive Sierpinski:
 *                           the orbit goes on from the final folded p with the trapped call's rule, q = fma(2,
 *                           tetrahedral_fold(q), -1) per component, w stays 0, for K_b points; no stop rule.  Every other
 *                           primitive, the bunny and unknown primitive ids contribute nothing.
 *   distance  kifs_render_trapped_async's d(z) over `axes` in the order x, y, z, w;  m = d(z_0), then m = (d < m) ? d : m
 *             in orbit order (a NaN distance is never taken);  u = sqrt(m).
 *   colour    kifs_render_trapped_async's gradient at u with the stops fractal_color, mid and far, and its shading -- the
 *             colour in the place of fc in kifs_render_lit_async's, in that call's order.  light NULL: the light
 *             {(1,1,1), 0.1, 0.9, no highlight}.
 *   frame     the folded estimate stands wherever kifs_render_folded_async puts it: the primary march, the normal, the
 *             soft-shadow march and the occlusion probes.  No culls, as there.  A heatmap frame shows the counter.
 *   plane     dev_trap_u NULL, or one f32 per pixel laid out as kifs_render_occlusion_async's plane: row y of frame i at
 *             dev_trap_u + i * u_stride_bytes + (y - y0) * u_pitch_bytes; its alignment, pitch and stride rules.  A hit
 *             stores its u -- in heatmap mode too: with a plane u is evaluated for every hit whatever the mode, without
 *             one a heatmap frame evaluates none.  A miss stores +inf.  With supersampling k > 1 a plane is refused.
 *   samples, frames, ordering, launch: kifs_render_folded_async's -- supersampling honoured sample by sample; 1..
 *             KIFS_MAX_FOLD_TRAP_BATCH frames, cameras NULL with count 1; bands bit-identical to the frame's rows and
 *             every frame of a batch to the lone call; a caller's stream; not a feedback launch, the kifs_debug_last_*
 *             values left alone.  The two records travel in device memory, through a slot of the ring that
 *             kifs_render_animation_async's scene tables use (KIFS_ANIMATION_RING deep): the call may wait for the launch
 *             that read the slot KIFS_ANIMATION_RING calls ago.
 *   identity  each for every KIFS primitive, with soft shadows, heatmap and k > 1:  (a) scale = bias = 0, or mid = far =
 *             fractal_color, writes the bytes of kifs_render_folded_async for the same fold, light and term.  (b)
 *             fold->iterations == 0 writes the bytes of kifs_render_trapped_async for the same trap, light and term (K_b
 *             = K: the Sierpinski orbit is that call's), and kifs_eval_fold_trap gives kifs_eval_trap's values.  (c) the
 *             plane at a hit pixel equals kifs_eval_fold_trap at the hit position.
 *   refusals  a refused call launches nothing and writes nothing.  Everything kifs_render_folded_async refuses is refused
 *             with its status, the two Julia groups included; everything kifs_render_trapped_async refuses of a trap; a
 *             NULL fold or trap; kifs_render_occlusion_async's refusals of a plane.  A record that cannot be copied to
 *             the device returns KIFS_ERR_RUNTIME and launches nothing.  y1 == y0 returns KIFS_OK and enqueues nothing.
 *   scope     deliberately absent: per-frame systems or traps; a certified cull radius; folded forms of the other entry
 *             points.
 * kifs_eval_fold_trap writes u for n positions (host pointers, like kifs_eval_trap) with the context's options; it
 * validates the fold, and only centre, axes and iterations of the trap.
 * Every byte and every u equals the CPU restatement of the contract (tests/fold_trap_reference.c), which is normative
 * where this text and it could be read differently. */
#define KIFS_MAX_FOLD_TRAP_BATCH 64
int kifs_render_folded_trapped_async(kifs_ctx* ctx, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                     uint8_t* const* dev_outs_rgba8, size_t pitch_bytes, const KifsFoldSystem* fold,
                                     const KifsOrbitTrap* trap, const KifsLight* light /* NULL: the reference's light */,
                                     const KifsAmbientOcclusion* ao /* may be NULL */, float* dev_trap_u /* may be NULL */,
                                     size_t u_pitch_bytes, size_t u_stride_bytes, int y0, int y1, int encode);
int kifs_eval_fold_trap(kifs_ctx* ctx, const KifsFoldSystem* fold, const KifsOrbitTrap* trap, const float* points_xyz,
                        int n, float* u_out);

/* Contiguous row-band partition used for multi-GPU frames: rank r
 * of `world` owns rows [y0, y1); bands differ by at most one row. */
int kifs_band_range(int height, int rank, int world, int* y0, int* y1);

/* ---- row shards: load-balanced multi-GPU partition ----------------------------
 * Pixels are independent (entry.wgsl:49-59), so any set of rows can be rendered anywhere.  The
 * expensive rows of these scenes sit in the middle of the frame (the projected bounding sphere), so
 * contiguous bands leave the outer ranks idle.  A row SHARD is instead a list of 8-row stripes
 * (KIFS_STRIPE_ROWS = the height of the kernels' 32 x 8 pixel tiles) dealt to the ranks in turn:
 * stripe s covers frame rows [8 s, min(H, 8 s + 8)).
 *
 * kifs_shard_stripes: the stripes of `rank` when the frame's stripes are dealt to `world` ranks by
 * smooth weighted round robin -- weights NULL: equal shares, rank r gets stripes r, r + world, ..;
 * weights[r] >= 0: rank r gets weights[r] stripes in every sum(weights), spread evenly (a root that
 * receives everybody else's rows over point-to-point xGMI links can be given a larger share, so
 * that the peers' transfers take as long as the root's rendering).  Writes the ascending stripe
 * indices to stripes[0 .. *n_stripes) (stripes may be NULL to only count) and the shard's total row
 * count to *rows.  Every rank computes every rank's list from the same arguments.
 *
 * kifs_render_shard_async: kifs_render_batch_async for a shard.  Frame i (cameras[i]; cameras NULL
 * with count 1 = the context's camera) is rendered into dev_outs[i]:
 *   in_place == 0: a PACKED shard -- stripe k of the list occupies rows [8 k, 8 k + 8) of the
 *                  buffer (n_rows x pitch_bytes: what a peer sends to the root in one message);
 *   in_place != 0: dev_outs[i] is a whole frame and every row lands at its frame position (the
 *                  root's own shard needs no copy).
 * Pixel coordinates are global either way: shards are bit-identical to the frame's rows.
 *
 * kifs_unpack_shard_async: the root's side of the gather.  Copies `count` packed shards
 * (dev_shards + i * shard_stride, rows shard_pitch apart) into the frames dev_frames + i *
 * frame_stride (rows frame_pitch apart), stripe k to frame rows [8 stripes[k], ..).  Frame size from
 * the context's screen; all strides in bytes, multiples of 4.  count <= KIFS_MAX_SHARD_COUNT (the shard index is
 * one dimension of the launch grid): a larger one gives KIFS_ERR_BAD_SIZE and nothing is launched; the same holds
 * for kifs_fill_shard_async. */
#define KIFS_STRIPE_ROWS 8
#define KIFS_MAX_SHARD_COUNT 65535
int kifs_shard_stripes(int height, int world, const int* weights, int rank, int* stripes,
                       int max_stripes, int* n_stripes, int* rows);
int kifs_render_shard_async(kifs_ctx* ctx, void* hip_stream, int count,
                            const KifsCameraUniform* cameras, uint8_t* const* dev_outs_rgba8,
                            size_t pitch_bytes, const int* stripes, int n_stripes, int in_place,
                            int encode);
int kifs_unpack_shard_async(kifs_ctx* ctx, void* hip_stream, int count, uint8_t* dev_frames,
                            size_t frame_pitch, size_t frame_stride, const uint8_t* dev_shards,
                            size_t shard_pitch, size_t shard_stride, const int* stripes,
                            int n_stripes);

/* ---- sparse shards: a peer's rows without their background tiles -----------------------------
 * The root of a gather takes each peer's rows over ONE xGMI link (~19 Gpixel/s inbound per link), a
 * GPU renders several times faster, and nine tenths of a 1080p frame of these scenes are the
 * background colour (the clear colour of the reference's render pass, render.rs:300-330).  So a peer
 * sends only the 32 x 8 tiles of its packed shards that hold a pixel other than the background, and
 * the root writes the background itself.  Lossless for any frame: a frame with no background at
 * all costs 1.6 % more than its dense form.
 *
 * A RECORD is KIFS_SPARSE_RECORD_BYTES = 1040 bytes: uint32 tile id, three zero words, then the tile's
 * 8 rows of 32 RGBA8 pixels (pixels outside the frame hold the background).
 * Tile id = (shard i * n_stripes + stripe slot k) * tiles_x + tile column, tiles_x = ceil(W / 32).
 *
 * kifs_pack_sparse_async: appends one record per non-background tile of the `count` packed shards
 *   (layout as kifs_unpack_shard_async's dev_shards; `stripes` the shard's list) to dev_records
 *   (16-byte aligned, room for capacity_records >= count * n_stripes * tiles_x records), in no
 *   particular order, and leaves their number in *dev_n_records (zeroed by the call, on the
 *   stream); host_n_records, when not NULL (pinned host memory), receives an asynchronous copy of
 *   it -- valid once the stream has reached that point.  `encode` selects the background pixel
 *   (the context's options, encoded as the render would).
 * kifs_unpack_sparse_async: the root's side.  Writes records [0, n_records) to their rows of the
 *   frames dev_frames + i * frame_stride; records whose id is out of range are skipped.
 * kifs_fill_shard_async: the background over the rows of the listed stripes of `count` frames
 *   (what the records leave out; any order with kifs_unpack_sparse_async's stream, before it);
 *   count <= KIFS_MAX_SHARD_COUNT, otherwise KIFS_ERR_BAD_SIZE and nothing is written.
 * kifs_erase_sparse_async: the background over the tiles of records [0, n_records) only -- frame
 *   buffers that are reused need it back just where the previous frames' records went (2 % of the
 *   headline's tiles) instead of a fill of every row. */
#define KIFS_SPARSE_RECORD_BYTES 1040
int kifs_pack_sparse_async(kifs_ctx* ctx, void* hip_stream, int count, const uint8_t* dev_shards,
                           size_t shard_pitch, size_t shard_stride, const int* stripes, int n_stripes,
                           int encode, uint8_t* dev_records, size_t capacity_records,
                           uint32_t* dev_n_records, uint32_t* host_n_records);
int kifs_unpack_sparse_async(kifs_ctx* ctx, void* hip_stream, int count, uint8_t* dev_frames,
                             size_t frame_pitch, size_t frame_stride, const uint8_t* dev_records,
                             size_t n_records, const int* stripes, int n_stripes);
int kifs_fill_shard_async(kifs_ctx* ctx, void* hip_stream, int count, uint8_t* dev_frames,
                          size_t frame_pitch, size_t frame_stride, const int* stripes, int n_stripes,
                          int encode);
int kifs_erase_sparse_async(kifs_ctx* ctx, void* hip_stream, int count, uint8_t* dev_frames,
                            size_t frame_pitch, size_t frame_stride, const uint8_t* dev_records,
                            size_t n_records, const int* stripes, int n_stripes, int encode);

/* ---- single-process multi-GPU ------------------------------------------------------
 * For a host that drives all GPUs of a node from one process (the reference's host is one
 * process, application.rs:37-48).  A kifs_multi owns one context per listed device; a render deals
 * the frame's 8-row stripes to the devices (kifs_shard_stripes; equal shares unless
 * kifs_multi_set_weights says otherwise), launches every shard on its own device concurrently --
 * the ROOT device (the first one listed) straight into the frame -- and the root pulls the other
 * shards over xGMI (hipMemcpyPeerAsync) and moves their stripes to their frame rows.  The frame is
 * bit-identical to a single-GPU frame.  The multi-process form of the same sharding (one process
 * per GPU, RCCL point-to-point gather) lives above the ABI in kifs_raymarching_amd/bands.py.  A
 * device may be listed more than once (testing on one GPU). */
typedef struct kifs_multi kifs_multi;
kifs_multi* kifs_multi_create(const int* device_ordinals, int n_devices, int* status);
void kifs_multi_destroy(kifs_multi* m);
int kifs_multi_set_screen(kifs_multi* m, const KifsScreenUniform* screen);
int kifs_multi_set_camera(kifs_multi* m, const KifsCameraUniform* camera);
int kifs_multi_set_options(kifs_multi* m, const KifsOptionsUniform* options);
int kifs_multi_set_iters(kifs_multi* m, int sdf_iters, int normal_iters, int fold_iters);
int kifs_multi_set_extensions(kifs_multi* m, const KifsExtensions* ext);
int kifs_multi_set_supersampling(kifs_multi* m, int factor); /* kifs_set_supersampling on every device */
/* Shares of the devices, one integer per device in the order they were listed (NULL: equal). */
int kifs_multi_set_weights(kifs_multi* m, const int* weights);
/* `out_rgba8`: host memory or device memory of the root device; full frame, `pitch_bytes`
 * per row.  Returns when the frame is complete.  KIFS_ERR_COMM: a peer copy failed. */
int kifs_multi_render(kifs_multi* m, uint8_t* out_rgba8, size_t pitch_bytes, int encode);
/* Shard i of the configured screen: device ordinal, number of stripes, total rows. */
int kifs_multi_shard(kifs_multi* m, int i, int* device_ordinal, int* n_stripes, int* rows);
/* Kernel time of shard i in the last kifs_multi_render, ms (load balance across devices). */
double kifs_multi_shard_ms(kifs_multi* m, int i);

/* ---- batches of frames over several devices, gathered on the root (SURVEY 8b `kifs_render_multi`, 8e) ---------
 * The throughput form of kifs_multi_render for the one caller the reference has (one process, one thread:
 * application.rs:37-48, graphics.rs:310-325): `count` frames (cameras[i]; screen, options, iteration counts and
 * extensions as set) are rendered as ONE launch per device -- each device its row shard of every frame -- and
 * collected into `dev_frames` on the root device: frame i at dev_frames + i * frame_stride, rows frame_pitch
 * apart (caller-owned memory of the ROOT device, free to be overwritten when the call is made).
 *
 *   gather     KIFS_GATHER_SPARSE (default): the other devices send only the 32 x 8 tiles that hold a pixel
 *              other than the background (kifs_pack_sparse_async's records), the root writes the background
 *              under their rows itself and scatters the records over it.  KIFS_GATHER_DENSE: every row.
 *   transport  KIFS_TRANSPORT_RCCL: RCCL inside the library -- ncclCommInitAll over the listed devices once,
 *              then per step ONE group of point-to-point transfers, `ncclGroupStart(); every other device:
 *              ncclSend(its records, root); root: ncclRecv per device; ncclGroupEnd()` (RCCL has no gather;
 *              each sender -> root pair rides its own xGMI link).  librccl.so.1 is opened on first use; a
 *              device listed twice, a missing library or a failing call gives KIFS_ERR_COMM.
 *              KIFS_TRANSPORT_COPY: hipMemcpyPeerAsync per device (the copy engines; the only form that works
 *              with a device listed more than once, i.e. for testing on one GPU).
 *              KIFS_TRANSPORT_AUTO (default): RCCL when every listed device is distinct and there are at
 *              least two, else COPY.
 *
 * Asynchronous, two steps deep: kifs_multi_render_batch_async returns once the step's launches are enqueued
 * and writes the step's number to *step (0, 1, 2, ..).  A step's transfers are posted when the NEXT step has
 * been enqueued (their sizes are known on the host only once the senders have packed, and by then every device
 * is already rendering the next step), or by a wait.  kifs_multi_wait blocks until the frames of `step` are
 * complete in their dev_frames; kifs_multi_stream_wait makes a stream of the root device wait for them instead.
 * At most two steps are in flight: submitting step k first completes step k - 2.  A consumer therefore reads
 * the frames of step k after kifs_multi_wait(m, k) and before it hands the same buffer back in a later call.
 *
 * flags: KIFS_MULTI_FRAMES_UNTOUCHED -- dev_frames is the buffer of the submission two steps ago (same
 * pointer, pitch, stride, count, encoding) and nothing but this library has written to it since: with the sparse
 * gather the root then restores the background only under that step's records instead of under every row of
 * the other devices.  Without the flag (or when anything differs, the options' background included) every such
 * row is filled.  Each frame is bit-identical to the frame a single device renders.
 * kifs_multi_render_batch = submit + wait. */
typedef enum KifsGather { KIFS_GATHER_SPARSE = 0, KIFS_GATHER_DENSE = 1 } KifsGather;
typedef enum KifsTransport { KIFS_TRANSPORT_AUTO = 0, KIFS_TRANSPORT_RCCL = 1, KIFS_TRANSPORT_COPY = 2 } KifsTransport;
#define KIFS_MULTI_FRAMES_UNTOUCHED 1
int kifs_multi_set_gather(kifs_multi* m, int gather, int transport);
int kifs_multi_render_batch_async(kifs_multi* m, int count, const KifsCameraUniform* cameras, uint8_t* dev_frames,
                                  size_t frame_pitch, size_t frame_stride, int encode, int flags, uint64_t* step);
int kifs_multi_wait(kifs_multi* m, uint64_t step);
int kifs_multi_wait_all(kifs_multi* m);
int kifs_multi_stream_wait(kifs_multi* m, uint64_t step, void* hip_stream);
/* The counterpart of kifs_order_after for the frames a kifs_multi writes on its ROOT device: whatever the object
 * enqueues there from now on (the root's renders, the fill / erase and the scatter of the gather) runs after
 * everything `producer_stream` (a stream of the root device; NULL = the legacy default stream) holds now. */
int kifs_multi_order_after(kifs_multi* m, void* producer_stream);
int kifs_multi_render_batch(kifs_multi* m, int count, const KifsCameraUniform* cameras, uint8_t* dev_frames,
                            size_t frame_pitch, size_t frame_stride, int encode);
/* What the gather moved since creation (or the last call with reset != 0): steps completed, records received
 * and the tiles they stand for (sparse), payload bytes into the root, and the transport in use
 * (KIFS_TRANSPORT_RCCL / _COPY; AUTO until the first step decides). */
typedef struct KifsMultiStats {
    uint64_t steps;
    uint64_t records_received;
    uint64_t tiles_covered;
    uint64_t bytes_received;
    int32_t transport;
    int32_t gather;
    int32_t rccl_version; /* ncclGetVersion, 0 if RCCL was never opened */
    int32_t comm_ranks;   /* ranks of the communicator, 0 if none */
} KifsMultiStats;
int kifs_multi_stats(kifs_multi* m, KifsMultiStats* out, int reset);
/* Transport check: every other device sends `bytes` of a known pattern to the root through the configured
 * transport exactly as a step's gather would (with one device: the root sends to itself and receives from
 * itself in one group) and the root verifies what arrived.  KIFS_ERR_COMM on any mismatch or failing call. */
int kifs_multi_comm_selftest(kifs_multi* m, size_t bytes);

/* Device time of the most recent kifs_render on this context in ms (HIP events
 * on the launch stream), or a negative value if none completed. */
double kifs_last_kernel_ms(kifs_ctx* ctx);

/* Per-launch timing for benchmarks.  With enable != 0 every subsequent render launch is
 * bracketed by a pair of HIP events recorded on the launch stream immediately around the
 * render kernel (after any stream waits), kept in a ring of the latest 4096 launches;
 * enable = n > 1 times only every n-th launch (an event pair costs a few microseconds).
 * kifs_profile_read synchronises, reports how many launches were timed and their mean,
 * minimum and maximum kernel duration in ms, and clears the ring.  Timed are the launches of
 * kifs_render, kifs_render_async, kifs_render_batch_async, kifs_render_shard_async and
 * kifs_render_geometry_async, and of kifs_render_adaptive_async its first pass only (the plain frame
 * with its geometry; neither the classification nor the resolve of the edge pixels); a launch of
 * kifs_render_animation_async or kifs_render_accumulate_async is not timed and does not count towards every n-th. */
int kifs_set_profiling(kifs_ctx* ctx, int enable);
int kifs_profile_read(kifs_ctx* ctx, int* launches, double* mean_ms, double* min_ms, double* max_ms);

/* Scheduling hint.  n = how many frames the caller keeps in flight on this device at once
 * (several contexts, one stream each; the reference queues up to
 * desired_maximum_frame_latency = 2 frames, render.rs:108).  With n = 1 (default) a launch is
 * tuned for the latency of a lone frame: frames whose run time is the critical path of a few
 * long rays cap their own residency so that those rays have a SIMD to themselves.  With n > 1
 * the device is shared on purpose and the cap is dropped (throughput over latency).  Pixels do
 * not depend on it.  Returns KIFS_ERR_BAD_ARG for n < 1. */
int kifs_set_frames_in_flight(kifs_ctx* ctx, int n);

/* Blocks until everything the context enqueued on its own stream is done. */
int kifs_synchronize(kifs_ctx* ctx);

const char* kifs_strerror(int status);
int kifs_abi_version(void);

/* ---- point evaluation (parity tests and tooling) -----------------------------
 * Evaluates scene_SDF and get_normal of the current options at `n` points
 * (xyz triples, host pointers) on the device.  Either output may be NULL. */
int kifs_eval_points(kifs_ctx* ctx, const float* points_xyz, int n, float* sdf_out,
                     float* normal_out_xyz);

/* Evaluates one of the library's f32 elementary functions on the device over
 * `n` host values.  fn: 0 log, 1 log2, 2 exp2, 3 sin, 4 cos, 5 acos,
 * 6 pow(x, y) with y = `param`, 7 sRGB-encode (result as float code),
 * 8 UNORM-encode, 9 / 10 the mid-range reciprocal and square root of the generalised-Julia
 * step (correctly rounded for 2^-60 <= x < 2^60; tests check them exhaustively), 11 the branch-free
 * form of sin the bunny network uses (same values as 3), 12 / 13 / 14 / 15 / 16 the straight-line cores of the
 * generalised-Julia step -- exp2, log2, sin, cos, acos for ORDINARY arguments only (|x| < 128; 2^-60 <= x < 2^60;
 * |x| <= 2^20; |x| <= 1), where they must equal 2 / 1 / 3 / 4 / 5 bit for bit. */
int kifs_eval_math(kifs_ctx* ctx, int fn, const float* in, float param, float* out, int n);

/* Diagnostics: with enable != 0, subsequent Julia renders write one record per wave into a
 * device buffer sized for the current screen; each call zeroes the buffer (out[8] receives
 * the 8 reserved header words).  enable == 0 frees it.  Not for timed runs.
 * The buffer holds 4 records per tile of the screen that is current at the call and is never resized by a
 * launch.  A launch whose 4 * tiles * count wave records do not fit -- after kifs_set_screen to a larger frame,
 * or a batch of count > 1 -- runs as a normal launch with diagnostics off: its pixels and its kernel are those
 * of a context without diagnostics, and the records stay as they were.  Call again to size for a new screen. */
int kifs_debug_counters(kifs_ctx* ctx, int enable, unsigned long long out[8]);
/* Round length (march steps) of the ray re-queuing used by the context's latest launch; 0 = that
 * launch marched one wave per 8x8 block.  For tests. */
int kifs_debug_last_round_steps(kifs_ctx* ctx);
/* Shape of the throughput path in the context's latest launch: 0 = one single-wave workgroup per
 * tile (render_wave_kernel), 1 or 2 = tiles per 256-thread workgroup (render_group_kernel), -1 = the
 * launch did not re-queue rays at all.  For tests and bench.py's kernel name. */
int kifs_debug_last_group_tiles(kifs_ctx* ctx);
/* Which render kernel the context's latest launch used (-1 before the first).  For tests and bench.py. */
enum KifsKernel {
    KIFS_KERNEL_BLOCK = 0,       /* render_kernel: one wave per 8x8 block, whole rays (the latency path) */
    KIFS_KERNEL_GROUP = 1,       /* render_group_kernel: rays re-queued by a 256-thread workgroup */
    KIFS_KERNEL_WAVE = 2,        /* render_wave_kernel: rays re-queued, one wave per tile */
    KIFS_KERNEL_BUNNY_QUAD = 3,  /* render_bunny_quad_kernel: whole rays, four lanes per pixel */
    KIFS_KERNEL_BUNNY_COOP = 4,  /* render_bunny_coop_kernel: rays re-queued, four waves per 64 rays */
    KIFS_KERNEL_SSAA = 5,        /* ssaa::render_kernel: k x k supersampling (kifs_set_supersampling), every pipeline */
    KIFS_KERNEL_GEOMETRY = 6,    /* geom::render_kernel: colour plus the geometry plane (kifs_render_geometry_async) */
    KIFS_KERNEL_ADAPTIVE = 7,    /* adaptive::render_kernel: the edge pixels' k x k resolve (kifs_render_adaptive_async) */
    KIFS_KERNEL_ANIMATION = 8,   /* anim::render_kernel: a scene per view (kifs_render_animation_async) */
    KIFS_KERNEL_ACCUMULATE = 9   /* accum::render_kernel: the mean of a frame's sub-frames (kifs_render_accumulate_async) */
};
int kifs_debug_last_kernel(kifs_ctx* ctx);
/* The bunny's throughput form in the context's latest launch: 0 = four lanes per ray with every weight in VGPRs, 1 = four
 * waves per 64 rays, 2 = four lanes per ray with layer 2 of the network in LDS; -1 = not a re-queued bunny launch. */
int kifs_debug_last_bunny_form(kifs_ctx* ctx);
/* Tuning hooks: read / replace the order in which workgroups take the tiles of the full
 * frame (a permutation of (tile_x | tile_y << 16)); the order only affects speed. */
int kifs_debug_get_tile_order(kifs_ctx* ctx, uint32_t* order, size_t max_count, size_t* count);
int kifs_debug_set_tile_order(kifs_ctx* ctx, const uint32_t* order, size_t count);
/* The full frame's tile costs as the launches and sorts so far left them, for tests (after a synchronisation of the
 * device): `cost` -- what the latest recording launch wrote (row-major tile index; a sort clears it) -- and `seen` -- the
 * memory of a batch's sorts, (largest cost of the last few sorts) << 8 | sorts since it was recorded.  Either may be NULL;
 * `shift`, when given, receives the sort's shift for `cost`. */
int kifs_debug_get_tile_costs(kifs_ctx* ctx, uint32_t* cost, uint32_t* seen, size_t max_count, size_t* count, uint32_t* shift);
/* The tile-order sort on chosen costs, for tests: sorts the n host values `cost` (tile i = column i % tiles_x, row
 * i / tiles_x) exactly as a render's cost feedback would -- bin = 1023 - min(cost >> shift, 1023), lowest bin
 * (heaviest tiles) first, tile-index order inside a bin -- on scratch device buffers and the context's stream, and returns
 * the order (n words, tile_x | tile_y << 16) and the cost table as the kernel left it (n words, all zero).  None of
 * the context's own tile tables is read or written; no screen is needed.  n == 0, tiles_x == 0, tiles_x > 65536 or
 * more than 65536 tile rows give KIFS_ERR_BAD_SIZE; shift > 31 or a null pointer KIFS_ERR_BAD_ARG. */
int kifs_debug_sort_tiles(kifs_ctx* ctx, const uint32_t* cost, size_t n, uint32_t tiles_x, uint32_t shift,
                          uint32_t* order_out, uint32_t* cost_after_out);
/* Per-wave records of the last counted render: 4 words per wave (wave = 4 * workgroup + wave
 * in workgroup, workgroups in dispatch order): total s_memtime ticks, ticks in the long-ray
 * loop, long-ray steps | (entries << 32), general steps.  Copies up to max_waves records. */
int kifs_debug_wave_records(kifs_ctx* ctx, unsigned long long* out, size_t max_waves,
                            size_t* n_waves);

/* ---- host model: the reference's scene -> uniform packing --------------------
 * C++ restatement of the caller side of the boundary so a harness without the
 * Rust host produces the same 156 bytes.
 *   kifs_host_screen   ScreenData::into_buffer_data        data.rs:66-81
 *   kifs_host_camera   CameraData::into_buffer_data        data.rs:91-129
 *   kifs_host_options  OptionsData::from(GuiData) + pack   data.rs:176-220, packed.rs:116-139
 *   kifs_host_rotate   GraphicState::rotate_camera         graphics.rs:280-302
 *   kifs_host_zoom     GraphicState::zoom_camera           graphics.rs:268-278
 */
typedef struct KifsGuiData { /* GuiData, data.rs:131-143 */
    uint32_t max_iterations;
    float max_distance;
    float epsilon;
    uint8_t fractal_color[3];    /* sRGB bytes */
    uint8_t background_color[3]; /* sRGB bytes */
    uint8_t is_heatmap;
    uint8_t _reserved;
    uint32_t fractal_group;
    uint32_t primitive_shape;
    float power;
    float constant[4];
} KifsGuiData;

typedef struct KifsCameraData { /* CameraData, data.rs:83-88 */
    float origin_distance;
    float min_distance;
    float phi;   /* angles.0 */
    float theta; /* angles.1 */
} KifsCameraData;

void kifs_host_gui_default(KifsGuiData* out);       /* GuiData::default, data.rs:145-160 */
void kifs_host_camera_default(KifsCameraData* out); /* CameraData::default, data.rs:105-113 */
int kifs_host_screen(uint32_t width, uint32_t height, KifsScreenUniform* out);
int kifs_host_camera(const KifsCameraData* camera, KifsCameraUniform* out);
int kifs_host_options(const KifsGuiData* gui, KifsOptionsUniform* out);
int kifs_host_rotate(KifsCameraData* camera, float delta_phi, float delta_theta);
int kifs_host_zoom(KifsCameraData* camera, float distance);
/* Mouse semantics of render.rs:255-270 / :239-250: degrees = -dx/10, +dy/10. */
int kifs_host_mouse_motion(KifsCameraData* camera, double dx, double dy);
float kifs_host_radians_from_degrees(float degrees); /* math.rs:429-431 */
void kifs_host_camera_matrix(const KifsCameraData* camera, float m_colmajor[9]);
void kifs_host_rotation_matrix(int axis, float radians, float m_colmajor[9]); /* math.rs:386-416 */
void kifs_host_mat3_mul(const float a[9], const float b[9], float out[9]);    /* math.rs:326-353 */
void kifs_host_mat3_vec(const float a[9], const float v[3], float out[3]);    /* math.rs:355-367 */

/* The host model of the power-2 Julia pipeline's culls (no device needed).
 * kifs_host_julia_cull_radius: the certified radius rho of the set for this constant -- every point with |p| >= rho has
 * an estimate of at least *bound (may be NULL) >= 16 epsilon + 2^-14, so a ray whose closest approach to the origin is
 * >= rho never hits -- or 0 when there is none (|c| too large, a NaN, epsilon or max_distance out of range).
 * kifs_host_cull_thresholds: what a launch of `count` views of these uniforms would run with,
 *   out[0] cull_n2 (per-ray cull, squared radius; 0 = off)   out[1] quick_cull_n2 (wave-level exit)
 *   out[2] tile_cull_sqrtk, out[3] tile_cull_beta (tile-level exit; beta 0 = off)
 *   out[4] 1.1 (B + epsilon)^2 of the scene's bounding radius B: the sphere the launch-shape rules are written in.
 * KIFS_TUNING=1 KIFS_JULIA_CERT_CULL=0 keeps the Julia culls on the bounding sphere (A/B runs, tests). */
double kifs_host_julia_cull_radius(const float constant[4], float epsilon, float max_distance, int sdf_iters, double* bound);
int kifs_host_cull_thresholds(const KifsScreenUniform* screen, const KifsOptionsUniform* options, int sdf_iters,
                              const KifsCameraUniform* cameras, int count, float out[5]);

#ifdef __cplusplus
}
#endif
#endif /* KIFS_HIP_H */
