// kifs_accumulate_kernels.hip -- accumulated frames (kifs_render_accumulate_async, include/kifs_hip.h): every output
// frame is the mean of `samples` sub-frames that differ in camera, scene or both -- motion blur over a shutter interval,
// depth of field from a finite lens, the temporal anti-aliasing of a morph.  The mean is taken in linear colour, before
// the encode, and only a kernel holds that colour (kifs_ssaa_kernels.hip); no sub-frame ever reaches memory.
//
//   accum::render_kernel<GROUP, PRIM>  256 threads per 8 x 8 OUTPUT block and output frame: four workgroups share an
//                                      entry of the launch's tile order, one per 8-column block of the 32 x 8 tile.
//                                      Wave w marches sub-frames w, w + 4, .. of the block as whole rays, 64 lanes = the
//                                      block's 64 pixels, under the wave-level cull of that sub-frame's camera, and leaves
//                                      each lane's linear colour in LDS at [s][channel][lane].  After a barrier wave 0 adds
//                                      a pixel's sub-frames in the contract's order, divides, encodes and stores.
//   accum::jitter_render_kernel<GROUP, PRIM>  the same with a sub-pixel cell per sub-frame
//                                      (kifs_render_accumulate_jittered_async): sub-frame v's ray goes through cell (i, j)
//                                      of the g x g grid inside its pixel, pixel (g x + i, g y + j) of the virtual
//                                      g W x g H screen kifs_set_supersampling defines.  Both kernels are one body.
//   accum::carry_render_kernel<GROUP, PRIM>  one PASS of a progressive frame (kifs_render_accumulate_resume_async): the
//                                      jittered kernel's marches for every grid (g = 1: cell (0, 0), the pixel centre),
//                                      and a resolve that starts from the pixel's texel of a plane of f32 sums earlier
//                                      passes left -- (sum.r, sum.g, sum.b, float(total)), one 16-byte load per lane,
//                                      issued by wave 0 after its own last march and before the barrier, so that its
//                                      latency hides behind the other waves' marches -- adds the pass's sub-frames in the
//                                      contract's order, stores the texel with one 16-byte store and, when the pass has
//                                      destinations, encodes sum / float(total).  A texel is read and written by one
//                                      lane of one workgroup.  The same body again.
//   accum::converge_render_kernel<GROUP, PRIM>  one CONVERGING pass (kifs_render_accumulate_converge_async): the carried
//                                      pass for the pixels whose mean has not settled.  The texel's w word is the pixel's
//                                      own count n, a second plane holds q = the sum of its squared luminances, and a
//                                      pixel is ACTIVE unless n q - L^2 <= tol^2 n^2 (n - 1) at n >= min_samples (L the
//                                      luminance of the sum) or n could leave 2^24.  Every wave derives the block's
//                                      64-bit active mask from the planes itself (the same memory; nobody writes before
//                                      the resolve), a block without an active pixel leaves at once (wave 0 stays to
//                                      encode when the pass has a picture), an inactive lane is marched as a lane
//                                      beyond the frame's edge, and the resolve folds, stores and counts what is still
//                                      active for the active lanes alone.  The same body once more.
// Why not the supersampling kernel's shape (a lane marches all of its samples one after another): a launch is as long as
// its longest rays, and that shape makes a lone frame's critical ray `samples` rays long.  Here the
// sub-frames of a block run side by side on four waves, and the blocks of every output frame side by side on the device.
// (Measured: min(samples, 16) waves per workgroup, a wave per sub-frame up to 16, left the lone frame of 16 sub-frames
// where it was and cost six frames of eight 14 %: DESIGN 5.11.)
// No atomics and no sums across workgroups: the order of the additions is the contract's.
// A view of the launch is a SUB-FRAME: view f * samples + s, with its camera (inline up to MAX_BATCH_INLINE views,
// through the view-table ring beyond) and its scene record (anim::SceneView, always present: the host fills the table
// with the context's scene when the caller gives no options).  Both are read with scalar loads: the view index is
// wave-uniform and made so explicitly (readfirstlane of the wave's number).
// LDS: samples * 768 bytes of dynamic memory (48 KB at 64 sub-frames) beside the 1 KB sRGB table; lanes access
// consecutive words, no bank conflicts.  Stores: one 4-byte pixel per lane, eight 32-byte row segments per instruction,
// under the guards of a ragged frame edge and a band's last row.
// The entry point's host side is kifs_accumulate.cpp; it reaches the kernel through launch_accumulate_render at the end
// of this file (kifs_internal.hpp).
#include "kifs_render_common.hpp"

namespace kifs {
namespace accum {

constexpr int BLOCK_W = 8;                         // an output block: 8 x 8 pixels, one lane each
constexpr uint32_t BLOCKS = TILE_W / BLOCK_W;      // blocks per entry of the tile order
constexpr uint32_t WAVES = BLOCK / 64;             // sub-frames in flight per workgroup
constexpr uint32_t SLOT = 3 * 64;                  // floats per sub-frame in LDS: [channel][lane]

// View `view`'s scene over its frame constants, as anim::overlay_scene lays it (the encoded background is not used: a
// pixel every sub-frame misses is still the mean of the backgrounds, encoded like any other).
__device__ __forceinline__ void overlay_scene(FrameParams& P, const anim::SceneView* scenes, uint32_t view) {
    typedef const anim::SceneView __attribute__((address_space(4))) * ConstScene;
    const ConstScene s = (ConstScene)(scenes + view);
    P.c = V4{s->c.x, s->c.y, s->c.z, s->c.w};
    P.power = s->power;
    P.fractal_color = V3{s->fractal_color.x, s->fractal_color.y, s->fractal_color.z};
    P.background_color = V3{s->background_color.x, s->background_color.y, s->background_color.z};
}

// The kernel argument again, through a pointer the compiler cannot see through: inside the sub-frame loop every frame
// constant is then loaded where the march uses it (scalar loads from the argument segment, a few hundred bytes per ray
// march) instead of all of them being held in SGPRs across the loop beside the Julia march's pinned s74-s97 -- which
// cost 36 parked SGPRs, two spilled VGPRs and a private segment.
typedef const Params __attribute__((address_space(4))) * ConstParams;
__device__ __forceinline__ const Params& reloaded(ConstParams& kp) {
    asm volatile("" : "+s"(kp));
    return *(const Params*)kp;
}

// A jittered view's cell of the g x g grid inside a pixel (kifs_render_accumulate_jittered_async): pad[0] = i | j << 8 of
// its scene record, one more scalar load beside overlay_scene's.
__device__ __forceinline__ uint32_t cell_of(const anim::SceneView* scenes, uint32_t view) {
    typedef const anim::SceneView __attribute__((address_space(4))) * ConstScene;
    return ((ConstScene)(scenes + view))->pad[0];
}

// The body of both kernels: the operation order exists once.  JITTER: sub-frame v's ray goes through cell (i, j) of its
// pixel instead of the centre, i.e. through pixel (g x + i, g y + j) of the VIRTUAL g W x g H screen with the frame's
// aspect float, as ssaa::render_kernel's samples do (g = frame.ssaa, the virtual screen's 1 / height from the host).
// Only the wave-level cull is used, and its argument is per lane with the screen's own 1 / height: it holds on the
// virtual screen as it stands (cull_n2 and quick_cull_n2 are radii in scene space: fill_params).  `valid` and the store
// guards stay on OUTPUT coordinates.
// CARRY: the kernel argument is a CarryParams whose first member is A; the resolve starts from the plane's texel when
// earlier passes left one (prior > 0), writes the texel back and encodes only for a pass with destinations.
typedef float Texel __attribute__((ext_vector_type(4)));
typedef const CarryParams __attribute__((address_space(4))) * ConstCarry;
typedef const ConvergeParams __attribute__((address_space(4))) * ConstConverge;

// The stopping rule of kifs_render_accumulate_converge_async, stated once for the device (include/kifs_hip.h; the NumPy
// model is tests/converge_reference.py): all in f32, no fma (-ffp-contract=off), a NaN compares false.
__device__ __forceinline__ float luminance(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ bool is_active(float n, V3 sum, float q, float min_samples, float tol2, float samples) {
    const float L = luminance(sum);
    const float d = n * q - L * L;
    const float b = tol2 * ((n * n) * (n - 1.0f));
    const bool settled = (n >= min_samples) && (d <= b);
    return !settled && (n + samples <= 16777216.0f);
}

// The resolve of a converging pass, wave 0 (the other waves leave behind the barrier).  The lane's texel and moment are
// fetched as carry_render_kernel fetches its texel: after wave 0's last march, before the barrier, the wait behind it.
// An active lane folds colours and squared luminances in the contract's order and stores both; every guarded lane
// encodes its state as it stands after the pass; then the lanes still active under the same rule are counted, and one
// lane adds the block's count to the frame's word -- only when it is not zero: the blocks that are all settled must not
// queue up on one address.
__device__ __forceinline__ void converge_resolve(ConstParams kp, float* s_srgb, const float* s_colour, int tid, uint32_t wave,
                                                 uint32_t frame, uint32_t samples, int block_x, int tile_y, int frame_y,
                                                 uint64_t mask) {
    const ConstConverge K = (ConstConverge)kp;
    const uint32_t restart = K->restart;  // launch-uniform
    const uint32_t lane = uint32_t(tid) & 63u;
    const int ly = int(lane >> 3);
    const int x = block_x + int(lane & 7u), y = frame_y + ly;
    Texel texel{0.0f, 0.0f, 0.0f, 0.0f};
    float moment = 0.0f;
    Texel* cell = nullptr;
    float* word = nullptr;
    if (wave == 0u) {
        const FrameParams& C = reloaded(kp).B.frame;
        if (x < C.width && y < C.y1) {
            const size_t row = size_t(tile_y + ly);
            cell = reinterpret_cast<Texel*>(K->sums) + size_t(frame) * K->sums_stride_texels + row * K->sums_pitch_texels + uint32_t(x);
            word = K->moments + size_t(frame) * K->moments_stride_words + row * K->moments_pitch_words + uint32_t(x);
            if (restart == 0u) {
                texel = *cell;
                moment = *word;
            }
        }
    }
    if (mask != 0u) {  // uniform over the workgroup: every wave derived the same mask
        __syncthreads();  // every sub-frame's colours and s_srgb visible
    } else {           // wave 0 alone, nothing marched: the rest of the encode table is its own to fill
        const FrameParams& C = reloaded(kp).B.frame;
        if (C.encode == 1)
            for (uint32_t k = 64u; k < 256u; k += 64u) s_srgb[lane + k] = C.srgb_table[lane + k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // (the texel is first looked at here: the wait for the loads comes behind the barrier, not in front of it)
    asm volatile("" : "+v"(texel), "+v"(moment));
    if (wave != 0u) return;

    V3 acc{texel.x, texel.y, texel.z};
    float q = moment, n = texel.w;
    if ((mask >> lane) & 1u) {
        const float* at = s_colour + lane;
        V3 c{at[0], at[64], at[128]};
        float l = luminance(c);
        if (restart != 0u) {  // acc = c_0 itself (no 0 + c_0: -0)
            acc = c;
            q = l * l;
        } else {
            acc = V3{acc.x + c.x, acc.y + c.y, acc.z + c.z};
            q = q + l * l;
        }
        for (uint32_t s = 1; s < samples; ++s) {
            at += SLOT;
            c = V3{at[0], at[64], at[128]};
            acc = V3{acc.x + c.x, acc.y + c.y, acc.z + c.z};
            l = luminance(c);
            q = q + l * l;
        }
        n = n + float(samples);  // exact: at most 2^24 (is_active)
        *cell = Texel{acc.x, acc.y, acc.z, n};
        *word = q;
    }
    if (K->counts) {  // launch-uniform
        const bool still = cell && is_active(n, acc, q, float(K->min_samples), K->tol2, float(samples));
        const uint64_t left = __ballot(still);
        if (left != 0u && lane == 0u) atomicAdd(K->counts + frame, uint32_t(__popcll(left)));
    }
    if (K->picture == 0u) return;  // launch-uniform: the pass only advances the planes
    const FrameParams& C = reloaded(kp).B.frame;
    const uint32_t rgba = encode_rgba(V3{acc.x / n, acc.y / n, acc.z / n}, C.encode == 1, s_srgb);
    if (cell) {
        uint32_t* const out = batch_frame(reloaded(kp).B, frame * samples).out;
        out[out_row(C, y, tile_y + ly) * C.pitch_words + uint32_t(x)] = rgba;
    }
}

// CONVERGE: the kernel argument is a ConvergeParams whose first member is A.  `mask` holds the block's active lanes
// across the marches (two SGPRs); the resolve is converge_resolve above.
template <int GROUP, int PRIM, bool JITTER, bool CARRY = false, bool CONVERGE = false>
__device__ __forceinline__ void render_body(const Params& A, float* s_srgb, float* s_colour) {
    ConstParams kp = (ConstParams)__builtin_amdgcn_kernarg_segment_ptr();  // = &A
    int tid = threadIdx.x;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(tid >> 6));  // uniform, and known to be
    const uint32_t frames = uint32_t(A.frames), samples = uint32_t(A.samples);
    // workgroup b works on output frame b % frames, so the long rays of every frame start at t = 0 (launch_slot)
    const uint32_t frame = frames > 1 ? blockIdx.x % frames : 0u;
    const uint32_t index = frames > 1 ? blockIdx.x / frames : blockIdx.x;
    if (A.B.frame.encode == 1) s_srgb[tid] = A.B.frame.srgb_table[tid];
    const uint32_t tile = A.B.frame.tile_order[index / BLOCKS];
    const int block_x = int(tile & 0xffffu) * TILE_W + BLOCK_W * int(index % BLOCKS);
    if (block_x >= A.B.frame.width) return;  // uniform: a block beyond the frame's right edge (before any barrier)
    const int tile_y = int(tile >> 16) * TILE_H;
    const int frame_y = tile_frame_row(A.B.frame, tile >> 16);

    // A converging pass: the block's active lanes, derived by every wave from the state the planes hold (nothing of this
    // launch has written them: a texel belongs to one lane of one workgroup, whose stores come behind its barrier).
    [[maybe_unused]] uint64_t mask = 0u;
    if constexpr (CONVERGE) {
        const ConstConverge K = (ConstConverge)kp;
        const uint32_t lane = uint32_t(tid) & 63u;
        const int ly = int(lane >> 3);
        const int x = block_x + int(lane & 7u);
        bool active = (x < A.B.frame.width) && (frame_y + ly < A.B.frame.y1);
        if (K->restart == 0u) {  // launch-uniform: a scalar branch
            bool unsettled = false;
            if (active) {
                const size_t row = size_t(tile_y + ly);
                const Texel t = reinterpret_cast<const Texel*>(K->sums)[size_t(frame) * K->sums_stride_texels +
                                                                        row * K->sums_pitch_texels + uint32_t(x)];
                const float q = K->moments[size_t(frame) * K->moments_stride_words + row * K->moments_pitch_words + uint32_t(x)];
                unsettled = is_active(t.w, V3{t.x, t.y, t.z}, q, float(K->min_samples), K->tol2, float(samples));
            }
            active = unsettled;
        }
        mask = __ballot(active);
        if (mask == 0u && (K->picture == 0u || wave != 0u)) return;  // uniform, before any barrier: nothing to march
    }

    for (uint32_t s = wave; s < samples && (!CONVERGE || mask != 0u); s += WAVES) {  // scalar
        const Params& L = reloaded(kp);
        asm volatile("" : "+v"(tid));  // (and the lane's pixel from its number: one VGPR across the march, not four)
        const uint32_t lane = uint32_t(tid) & 63u;
        const int x = block_x + int(lane & 7u), y = frame_y + int(lane >> 3);
        const uint32_t view = frame * samples + s;
        FrameParams P = batch_frame(L.B, view);
        overlay_scene(P, L.scenes, view);
        bool valid = (x < P.width) && (y < P.y1);
        if constexpr (CONVERGE) valid = valid && ((mask >> lane) & 1u) != 0u;  // a settled pixel: a lane beyond the edge
        int px = x, py = y;  // the pixel the ray goes through: of the frame, or of the virtual screen
        if constexpr (JITTER) {
            const uint32_t cell = cell_of(L.scenes, view);  // wave-uniform
            const int g = P.ssaa;                           // 2..KIFS_MAX_JITTER_GRID
            px = g * x + int(cell & 0xffu);
            py = g * y + int((cell >> 8) & 0xffu);
            P.height = float(g) * P.height;  // exact: integers below 2^24
            P.inv_height = P.ssaa_inv_height;
        }
        V3 c = P.background_color;  // a ray the cull drops is a miss
        if (!wave_is_culled(P, px, py, valid)) {  // wave-uniform
            int steps = 0;
            const V3 dir = ray_direction(P, px, py);
            c = raymarch<GROUP, PRIM>(P, dir, valid, steps);
        }
        float* const slot = s_colour + s * SLOT + lane;
        slot[0] = c.x;
        slot[64] = c.y;
        slot[128] = c.z;
    }
    // A resumed pass: wave 0's lanes fetch their pixels' texels now, behind the marches the other waves are still in --
    // eight lanes of a block row read 128 contiguous bytes -- under the guard of the store below.
    if constexpr (CONVERGE) {
        converge_resolve(kp, s_srgb, s_colour, tid, wave, frame, samples, block_x, tile_y, frame_y, mask);
        return;
    }
    [[maybe_unused]] Texel texel{0.0f, 0.0f, 0.0f, 0.0f};
    [[maybe_unused]] Texel* cell = nullptr;
    [[maybe_unused]] uint32_t prior = 0u;
    if constexpr (CARRY) {
        prior = ((ConstCarry)kp)->prior;  // launch-uniform: a scalar
        if (wave == 0u) {
            const ConstCarry K = (ConstCarry)kp;
            const FrameParams& C = reloaded(kp).B.frame;
            const uint32_t lane = uint32_t(tid) & 63u;
            const int ly = int(lane >> 3);
            const int x = block_x + int(lane & 7u), y = frame_y + ly;
            if (x < C.width && y < C.y1) {
                cell = reinterpret_cast<Texel*>(K->sums) + size_t(frame) * K->sums_stride_texels +
                       size_t(tile_y + ly) * K->sums_pitch_texels + uint32_t(x);
                if (prior != 0u) texel = *cell;
            }
        }
    }
    __syncthreads();  // every sub-frame's colours and s_srgb visible
    // (the texel is first looked at here: the wait for the load comes behind the barrier, not in front of it)
    if constexpr (CARRY) asm volatile("" : "+v"(texel));
    if (wave != 0u) return;

    // The resolve of the contract, per channel in f32: acc = c_0, then acc + c_s in order (-ffp-contract=off: no fma),
    // mean = acc / samples correctly rounded, then the frame's encoder.
    const uint32_t lane = uint32_t(tid) & 63u;
    const float* at = s_colour + lane;
    V3 acc{at[0], at[64], at[128]};
    if constexpr (CARRY)  // acc = the texel's sum, then + c_0; a first pass starts from c_0 itself (no 0 + c_0: -0)
        if (prior != 0u) acc = V3{texel.x + acc.x, texel.y + acc.y, texel.z + acc.z};
    for (uint32_t s = 1; s < samples; ++s) {
        at += SLOT;
        acc = V3{acc.x + at[0], acc.y + at[64], acc.z + at[128]};
    }
    float n = float(samples);
    if constexpr (CARRY) {
        n = float(prior + samples);  // exact: at most 2^24 (KIFS_MAX_PROGRESSIVE_SAMPLES)
        if (cell) *cell = Texel{acc.x, acc.y, acc.z, n};
        if (((ConstCarry)kp)->picture == 0u) return;  // launch-uniform: the pass only advances the plane
    }
    const FrameParams& C = reloaded(kp).B.frame;  // what every view shares
    const uint32_t rgba = encode_rgba(V3{acc.x / n, acc.y / n, acc.z / n}, C.encode == 1, s_srgb);
    const int ly = int(lane >> 3);
    const int x = block_x + int(lane & 7u), y = frame_y + ly;
    if (x < C.width && y < C.y1) {
        uint32_t* const out = batch_frame(reloaded(kp).B, frame * samples).out;  // (every sub-frame of a frame carries it)
        out[out_row(C, y, tile_y + ly) * C.pitch_words + uint32_t(x)] = rgba;
    }
}

// (amdgpu_waves_per_eu: as ssaa::render_kernel, whose sample loop this one's sub-frame loop resembles)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const Params A) {
    __shared__ float s_srgb[256];
    extern __shared__ float s_colour[];  // [samples][3][64]
    render_body<GROUP, PRIM, false>(A, s_srgb, s_colour);
}

// The same with a sub-pixel cell per sub-frame (A.B.frame.ssaa = g > 1).  A kernel of its own, not a template parameter
// of the one above: the unjittered launch keeps its code and its name.
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void jitter_render_kernel(const Params A) {
    __shared__ float s_srgb[256];
    extern __shared__ float s_colour[];  // [samples][3][64]
    render_body<GROUP, PRIM, true>(A, s_srgb, s_colour);
}

// One pass of a progressive frame: the plane of sums carried across launches (CarryParams, kifs_params.hpp).  The marches
// are the jittered kernel's for every grid: at g = 1 the cell is (0, 0) and the virtual screen is the frame.
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void carry_render_kernel(const CarryParams K) {
    __shared__ float s_srgb[256];
    extern __shared__ float s_colour[];  // [samples][3][64]
    render_body<GROUP, PRIM, true, true>(K.A, s_srgb, s_colour);
}

// One converging pass: the planes and the rule in a ConvergeParams (kifs_params.hpp).
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void converge_render_kernel(const ConvergeParams K) {
    __shared__ float s_srgb[256];
    extern __shared__ float s_colour[];  // [samples][3][64]
    render_body<GROUP, PRIM, true, false, true>(K.A, s_srgb, s_colour);
}

// From 63 sub-frames the dynamic LDS and the 1 KB sRGB table together pass the default limit of 48 KB: the kernel then opts
// in, once per instantiation and device, as ensure_dynamic_lds does for the residency pad (kifs_render_common.hpp).
template <auto KERNEL>
static hipError_t ensure_lds(unsigned dynamic_bytes) {
    if (dynamic_bytes + 256u * unsigned(sizeof(float)) <= 48u * 1024u) return hipSuccess;
    static std::atomic<bool> opted_in[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    if (dev < 0 || dev >= 64 || !opted_in[dev].load(std::memory_order_acquire)) {
        hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (attr != hipSuccess) return attr;
        if (dev >= 0 && dev < 64) opted_in[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

// One launch of the family: KERNEL is the instantiation, K its argument, A the Params at K's head.
template <auto KERNEL, typename ARG>
static hipError_t launch(const ARG& K, const Params& A, hipStream_t stream) {
    const unsigned lds = unsigned(A.samples) * SLOT * unsigned(sizeof(float));  // at most 48 KB
    if (hipError_t e = ensure_lds<KERNEL>(lds); e != hipSuccess) return e;
    const dim3 grid(A.B.frame.tile_count * BLOCKS * uint32_t(A.frames));
    hipLaunchKernelGGL(KERNEL, grid, dim3(BLOCK), lds, stream, K);
    return hipGetLastError();
}

// What every launcher refuses of the Params: the views are frames x samples, the grid is 1..KIFS_MAX_JITTER_GRID.
static bool valid(const Params& A) {
    return A.frames >= 1 && A.samples >= 1 && A.samples <= 64 && A.B.count == A.frames * A.samples && A.B.frame.ssaa >= 1 &&
           A.B.frame.ssaa <= 8;
}

// The pipeline's instantiation of a launcher's kernel.  Julia: the short divide / square root by sdf_iters; the doubled
// orbit trip is the throughput kernels' only.  The bunny: per-lane bunny_sdf -- slow, correct.
template <typename F>
static hipError_t dispatch(const Params& A, uint32_t group, uint32_t primitive, F&& f) {
    return dispatch_pipeline<2>(group, primitive, uint32_t(A.B.frame.sdf_iters <= 24), f);
}

}  // namespace accum

hipError_t launch_accumulate_render(const accum::Params& A, uint32_t group, uint32_t primitive, hipStream_t stream) {
    if (!accum::valid(A)) return hipErrorInvalidValue;
    const bool jitter = A.B.frame.ssaa > 1;  // a cell per sub-frame in its scene record: jitter_render_kernel
    return accum::dispatch(A, group, primitive, [&](auto g, auto prim) {
        constexpr int G = decltype(g)::value, P = decltype(prim)::value;
        return jitter ? accum::launch<accum::jitter_render_kernel<G, P>>(A, A, stream) : accum::launch<accum::render_kernel<G, P>>(A, A, stream);
    });
}

hipError_t launch_accumulate_carry(const accum::CarryParams& K, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const accum::Params& A = K.A;
    if (!accum::valid(A) || !K.sums || (reinterpret_cast<uintptr_t>(K.sums) & 15u) != 0 || K.sums_pitch_texels < uint32_t(A.B.frame.width) ||
        uint64_t(K.prior) + uint64_t(A.samples) > (1ull << 24))
        return hipErrorInvalidValue;  // (refused by the API before it gets here)
    return accum::dispatch(A, group, primitive, [&](auto g, auto prim) {
        return accum::launch<accum::carry_render_kernel<decltype(g)::value, decltype(prim)::value>>(K, A, stream);
    });
}

hipError_t launch_accumulate_converge(const accum::ConvergeParams& K, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const accum::Params& A = K.A;
    if (!accum::valid(A) || !K.sums || (reinterpret_cast<uintptr_t>(K.sums) & 15u) != 0 || K.sums_pitch_texels < uint32_t(A.B.frame.width) ||
        !K.moments || (reinterpret_cast<uintptr_t>(K.moments) & 3u) != 0 || K.moments_pitch_words < uint32_t(A.B.frame.width) ||
        K.min_samples < 2u || K.min_samples > (1u << 24) || !(K.tol2 >= 0.0f))
        return hipErrorInvalidValue;  // (refused by the API before it gets here)
    return accum::dispatch(A, group, primitive, [&](auto g, auto prim) {
        return accum::launch<accum::converge_render_kernel<decltype(g)::value, decltype(prim)::value>>(K, A, stream);
    });
}

}  // namespace kifs
