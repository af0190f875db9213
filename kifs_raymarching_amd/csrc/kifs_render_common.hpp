// kifs_render_common.hpp -- what the render kernels of kifs_kernels.hip, kifs_bunny_kernels.hip, kifs_ssaa_kernels.hip
// and kifs_geometry_kernels.hip share.  Device side: a workgroup's place in the launch and its view's parameters
// (launch_slot, batch_frame), the tile <-> frame row mapping of bands and row shards, the tile and lane prologue of the
// whole-ray kernels (tile_origin, tile_frame), the wave- and tile-level forms of the bounding-sphere cull, a ray's
// position (ray_at), the guarded store of a staged tile (store_tile, store_tile_wave, store_group) and the cost
// write-back (tile_cost_slot, cost_from_cycles, cost_from_work, record_tile_cost).  Host side: the pipeline dispatch
// (dispatch_pipeline) and the opt-in to large dynamic LDS (ensure_dynamic_lds).
// render_wave_kernel and the Julia builds are at the edge of their register budgets (the hand-written loop pins v30-v63
// and s74-s97): where a helper cost one of them a register or a spill, that kernel keeps the text in place -- the
// wave kernel its scalar prologue, ray positions and cost write-back, the two queue kernels their round 0.
#pragma once

#include <atomic>
#include <type_traits>

#include "kifs_internal.hpp"
#include "kifs_scene.hpp"
#include "kifs_bunny.hpp"

namespace kifs {

constexpr int BLOCK = TILE_W * TILE_H;  // 256 threads = 4 waves

// Frame `view` of the batch: the common parameters with that view's camera and destination.
// Workgroup b of a launch works on view b % count and takes entry b / count of the tile order,
// so the expensive tiles of every frame of the batch start at t = 0.
__device__ __forceinline__ FrameParams batch_frame(const BatchParams& B, uint32_t view) {
    FrameParams P = B.frame;
    if (B.count > 1) {  // uniform; a batch of one carries its view in B.frame already
        if (B.table) {
            // a table in device memory, read through the constant address space: the index is uniform, so
            // these are scalar loads like the kernel argument's own (a generic pointer would cost VGPRs)
            typedef const BatchView __attribute__((address_space(4))) * ConstView;
            const ConstView v = (ConstView)(B.table + view);
            P.origin = V3{v->origin.x, v->origin.y, v->origin.z};
            P.m0 = V3{v->m0.x, v->m0.y, v->m0.z};
            P.m1 = V3{v->m1.x, v->m1.y, v->m1.z};
            P.m2 = V3{v->m2.x, v->m2.y, v->m2.z};
            P.out = v->out;
        } else {
            const BatchView& v = B.view[view];
            P.origin = v.origin;
            P.m0 = v.m0;
            P.m1 = v.m1;
            P.m2 = v.m2;
            P.out = v.out;
        }
    }
    return P;
}

// Where workgroup blockIdx.x stands in its launch: the launch's number of views, this one's view and its index among
// the view's workgroups (an entry of the tile order, or a group or a part of entries).  All uniform.
struct LaunchSlot {
    uint32_t batch, view, index;
};
__device__ __forceinline__ LaunchSlot launch_slot(const BatchParams& B) {
    const uint32_t batch = uint32_t(B.count);
    return LaunchSlot{batch, batch > 1 ? blockIdx.x % batch : 0u, batch > 1 ? blockIdx.x / batch : blockIdx.x};
}

// Frame row at which local tile row `tile_row` of the launch starts: a contiguous band counts on
// from y0, a row shard looks its stripe up (scalar load: tile_row is uniform per workgroup).
__device__ __forceinline__ int tile_frame_row(const FrameParams& P, uint32_t tile_row) {
    return P.stripe_rows ? int(P.stripe_rows[tile_row]) : P.y0 + int(tile_row) * TILE_H;
}
// Row of the destination for frame row `y` = row `local` of the launch's rows.
__device__ __forceinline__ size_t out_row(const FrameParams& P, int y, int local) {
    return size_t(P.out_frame_rows ? y : local);
}

// The tile a workgroup renders, or its part of one: the view's parameters, the tile-order entry (x | y << 16) and the
// first pixel's column, row within the launch's rows and row of the frame.  ROWS < TILE_H: TILE_H / ROWS workgroups
// share an entry, each with ROWS of its rows.  Scalar loads and scalar arithmetic throughout.
struct TileOrigin {
    FrameParams P;
    uint32_t batch, view, tile;  // views of the launch, this one, the entry
    int tile_x, tile_y, frame_y;
};
template <int ROWS = TILE_H>
__device__ __forceinline__ TileOrigin tile_origin(const FrameParams& P, const LaunchSlot& S) {
    constexpr uint32_t PARTS = TILE_H / ROWS;
    const uint32_t tile = P.tile_order[S.index / PARTS];
    const int first = ROWS * int(S.index % PARTS);
    return TileOrigin{P, S.batch, S.view, tile, int(tile & 0xffffu) * TILE_W, int(tile >> 16) * TILE_H + first,
                      tile_frame_row(P, tile >> 16) + first};
}
__device__ __forceinline__ TileOrigin tile_origin(const BatchParams& B) {
    const LaunchSlot S = launch_slot(B);
    return tile_origin(batch_frame(B, S.view), S);
}

// The whole-ray kernels' prologue, 256 threads: the sRGB table staged into `s_srgb` (256 floats of LDS, visible after
// the next barrier), the tile and this lane's pixel.  Wave w owns columns [8 w, 8 w + 8) of the tile; its lanes take
// the pixels of that block row by row, LPP lanes to a pixel, so a workgroup covers TILE_H / LPP rows.
struct TileFrame : TileOrigin {
    bool srgb;
    int lx, ly;  // pixel within the workgroup's rows
    int x, y;    // pixel of the frame
    bool valid;  // inside the frame and the launch's rows
};
template <int LPP = 1>
__device__ __forceinline__ TileFrame tile_frame(const BatchParams& B, float* s_srgb) {
    const LaunchSlot S = launch_slot(B);
    const FrameParams P = batch_frame(B, S.view);
    const int tid = threadIdx.x;
    const bool srgb = (P.encode == 1);
    if (srgb) s_srgb[tid] = P.srgb_table[tid];
    const int wave = tid >> 6, pixel = (tid & 63) / LPP;
    const int lx = (wave << 3) | (pixel & 7);
    const int ly = pixel >> 3;
    const TileOrigin O = tile_origin<TILE_H / LPP>(P, S);
    const int x = O.tile_x + lx;
    const int y = O.frame_y + ly;
    return TileFrame{O, srgb, lx, ly, x, y, (x < P.width) && (y < P.y1)};
}

// True when no pixel of this wave can ever be hit: every valid lane's ray passes the origin at more
// than sqrt(1.2) (B + epsilon), B the scene's bounding radius (fill_params).  Same geometry as
// ray_never_inside, but on the unnormalised direction and an approximate uv (28 instructions, no
// divide, no square root): closest approach c^2 = |o|^2 - (o.d)^2 / |d|^2 > K  <=>
// (|o|^2 - K) |d|^2 > (o.d)^2.  K is 9 % above the radius the exact cull uses, five orders of
// magnitude more than the rounding of this arithmetic, so a wave that leaves here would have had
// all its lanes culled at ray set-up anyway and its pixels are the background colour either way.
// In a 1080p frame nine waves in ten leave here without setting up a single ray.
__device__ __forceinline__ bool wave_is_culled(const FrameParams& P, int x, int y, bool valid) {
    if (!(P.quick_cull_n2 > 0.0f)) return false;  // uniform
    const float px = float(x) + 0.5f, py = float(y) + 0.5f;
    const float ux = (2.0f * px) * P.inv_height - P.aspect;
    const float uy = (2.0f * py) * P.inv_height - 1.0f;
    const V3 d{(ux * P.m1.x - uy * P.m2.x) - P.m0.x, (ux * P.m1.y - uy * P.m2.y) - P.m0.y,
               (ux * P.m1.z - uy * P.m2.z) - P.m0.z};
    const float s = -dot(P.origin, d);  // > 0: the ray approaches the origin
    const float dd = dot(d, d);
    const float room = dot(P.origin, P.origin) - P.quick_cull_n2;
    const bool never = (s <= 0.0f) ? (room > 0.0f) : (room * dd > s * s);
    return __builtin_amdgcn_ballot_w64(valid && !never) == 0ull;
}

// The same exit for a whole 32 x 8 tile, before anything else is computed: the quick test at the
// tile's centre against a sphere grown by what the tile subtends.  With theta the angle between a ray
// and the direction to the origin, the ray's line passes the origin at |o| sin(theta) (theta < 90
// degrees; beyond that the ray moves away and never enters as long as the camera is outside).  Every ray
// of the tile is within beta = P.tile_cull_beta of the ray through the tile's centre (fill_params), and
// sin is 1-Lipschitz and increasing up to 90 degrees, so all of them pass at more than sqrt(K) if the
// centre's ray passes at more than T = sqrt(K) + |o| beta -- or points away while |o| > T, which also
// covers the rays of such a tile that still approach: theirs is |o| cos(beta) >= |o| (1 - beta) > sqrt(K).
// K = quick_cull_n2 as in wave_is_culled, with the same 9 % of room over the exact cull for the
// rounding of this arithmetic and of hardware sqrt.  In a 1080p frame 89 tiles in 100 leave here; the
// ring of tiles within half a tile's diagonal of the projected sphere goes on to the per-block tests.
__device__ __forceinline__ bool tile_is_culled(const FrameParams& P, int tile_x, int frame_y) {
    if (!(P.tile_cull_beta > 0.0f)) return false;  // uniform
    const float oo = dot(P.origin, P.origin);
    const float T = fmaf_(1.01f * P.tile_cull_beta, __builtin_amdgcn_sqrtf(oo), P.tile_cull_sqrtk);
    const float room = oo - T * T;
    // pixel centres x + 0.5 .. x + 31.5 and y + 0.5 .. y + 7.5: the tile's centre is (x + 16, y + 4)
    const float ux = (2.0f * (float(tile_x) + 16.0f)) * P.inv_height - P.aspect;
    const float uy = (2.0f * (float(frame_y) + 4.0f)) * P.inv_height - 1.0f;
    const V3 d{(ux * P.m1.x - uy * P.m2.x) - P.m0.x, (ux * P.m1.y - uy * P.m2.y) - P.m0.y,
               (ux * P.m1.z - uy * P.m2.z) - P.m0.z};
    const float s = -dot(P.origin, d);
    const float dd = dot(d, d);
    const bool never = (room > 0.0f) && ((s <= 0.0f) || (room * dd > s * s));
    return __builtin_amdgcn_readfirstlane(int(never)) != 0;  // every lane holds the same value
}
__device__ __forceinline__ bool tile_is_whole(const FrameParams& P, int tile_x, int frame_y) {
    return tile_x + TILE_W <= P.width && frame_y + TILE_H <= P.y1;
}
// The background over the row pairs [k0, k1) of a whole tile (pair k = rows 2k, 2k + 1: one wave's
// 64 lanes), straight from registers: one address, one store per pair.  (Only render_wave_kernel uses
// the tile-level exit: a 256-thread workgroup's empty tile costs its four wave launches, whatever they
// execute -- 8 frames per launch: 50.3 Gpixel/s with, 51.1 without.)
__device__ __forceinline__ void store_background(const FrameParams& P, int tile_x, int tile_y, int frame_y,
                                                 uint32_t lane, int k0, int k1) {
    uint32_t* row = P.out + (out_row(P, frame_y, tile_y) + size_t(2 * k0)) * P.pitch_words + uint32_t(tile_x);
    const uint32_t at = (lane >> 5) * P.pitch_words + (lane & 31u);
    for (int k = k0; k < k1; ++k) {
        row[at] = P.background_rgba;
        row += 2u * P.pitch_words;
    }
}

// A linear colour as the frame's RGBA8 pixel: the colour target of the reference (render.rs:72-80, graphics.rs:87-91:
// sRGB or UNORM format, alpha 1.0), `table` = the sRGB thresholds (LDS or memory).
__device__ __forceinline__ uint32_t encode_rgba(V3 colour, bool srgb, const float* __restrict__ table) {
    uint32_t r, g, b;
    if (srgb) {
        r = srgb8(colour.x, table);
        g = srgb8(colour.y, table);
        b = srgb8(colour.z, table);
    } else {
        r = unorm8(colour.x);
        g = unorm8(colour.y);
        b = unorm8(colour.z);
    }
    return r | (g << 8) | (b << 16) | 0xff000000u;  // alpha = 1.0 -> 255
}

// Where a ray stands after it has advanced by t: what the march last computed.  The callers choose when the origin's
// own bits stand in for it, and the two conditions in use are not interchangeable: a hit list's entry asks its own
// `t == 0` (per lane), a queue's round the uniform `trips == 0` (every ray of round 0 stands at the origin, every ray
// of a later round has advanced).
__device__ __forceinline__ V3 ray_at(const FrameParams& P, float t, V3 dir) {
    return V3{fmaf_(t, dir.x, P.origin.x), fmaf_(t, dir.y, P.origin.y), fmaf_(t, dir.z, P.origin.z)};
}

// A lane's output pixel in the kernels whose phases read the kernel argument anew (occl::render_kernel,
// light::render_kernel): the view's parameters and the pixel, made from the argument and the workgroup's tile alone.
struct TilePixel {
    FrameParams P;  // the view's parameters
    uint32_t view;
    int tile_x, tile_y, frame_y;  // the OUTPUT tile, as TileOrigin's
    int lx, ly, x, y;             // this lane's output pixel: within the tile, of the frame
    bool valid;                   // inside the frame and the launch's rows
};
// `at`: the kernel argument (occl::ConstParams, light::ConstParams: a BatchParams B first; anew is the namespace's own);
// `tile`: the workgroup's entry of the tile order (x | y << 16), the one scalar the phases hand on.
template <class Args>
__device__ __forceinline__ TilePixel tile_pixel(Args at, uint32_t tile) {
    const Args K = anew(at);
    const BatchParams& B = *(const BatchParams*)&K->B;
    const LaunchSlot S = launch_slot(B);
    const FrameParams P = batch_frame(B, S.view);
    const int tile_x = int(tile & 0xffffu) * TILE_W, tile_y = int(tile >> 16) * TILE_H;
    const int frame_y = tile_frame_row(P, tile >> 16);
    // wave w owns columns [8 w, 8 w + 8) of the tile, its lanes the pixels of that block row by row (tile_frame)
    const int tid = threadIdx.x, wave = tid >> 6, pixel = tid & 63;
    const int lx = (wave << 3) | (pixel & 7), ly = pixel >> 3;
    const int x = tile_x + lx, y = frame_y + ly;
    return TilePixel{P, S.view, tile_x, tile_y, frame_y, lx, ly, x, y, (x < P.width) && (y < P.y1)};
}

// The staged tile to the destination, 256 threads: thread -> (tid & 31, tid >> 5), linear rows of 128 bytes, the first
// ROWS rows of `s_tile`, under the guards of a ragged frame edge and a band's last row.
template <int ROWS = TILE_H>
__device__ __forceinline__ void store_tile(const FrameParams& P, int tile_x, int tile_y, int frame_y,
                                           const uint32_t (*s_tile)[TILE_W], int tid) {
    if (ROWS < TILE_H && tid >= ROWS * TILE_W) return;
    const int sx = tid & (TILE_W - 1), sy = tid >> 5;
    const int ox = tile_x + sx;
    if (ox < P.width && (frame_y + sy) < P.y1)
        P.out[out_row(P, frame_y + sy, tile_y + sy) * P.pitch_words + ox] = s_tile[sy][sx];
}
// The same with one wave: two full 128-byte rows per instruction, from the staged tile or, BACKGROUND, the background
// colour straight from a register (`s_tile` is not read then).
template <bool BACKGROUND = false>
__device__ __forceinline__ void store_tile_wave(const FrameParams& P, int tile_x, int tile_y, int frame_y, uint32_t lane,
                                                const uint32_t (*s_tile)[TILE_W]) {
#pragma unroll
    for (int r = 0; r < TILE_H; r += 2) {
        const int sx = int(lane & 31u), sy = r + int(lane >> 5);
        const int ox = tile_x + sx;
        if (ox < P.width && (frame_y + sy) < P.y1)
            P.out[out_row(P, frame_y + sy, tile_y + sy) * P.pitch_words + uint32_t(ox)] =
                BACKGROUND ? P.background_rgba : s_tile[sy][sx];
    }
}

// Cost of a tile for the next frame's tile order (tile_order_kernel).  render_kernel and the bunny's kernels: the run time
// of the wave or workgroup that rendered it in units of 1024 cycles, minus a floor that maps culled / instant ones to 0
// (march steps alone are too coarse there: hundreds of tiles tie at max_iterations).  The throughput kernels
// (render_wave_kernel, render_group_kernel): the WORK of the tile's wave or workgroup, a count it holds anyway -- the march
// steps of every chunk-round it ran (render_group_kernel, whose chunks are drawn by ticket: a round of several chunks
// counts in full), plus WORK_PER_SHADED_CHUNK for every chunk of hits it shaded.  A run time depends on
// who shared the SIMD and on when in the launch the wave ran, and it saturated the sort's 1024 bins from 1.05 M cycles,
// which one tile in ten of a 48-frame launch exceeds; the count is the same whenever the same views are rendered, and
// work_cost_shift() (kifs_schedule.cpp) fits its range -- 4 chunks per tile x max_iterations -- to the bins.
constexpr uint32_t WORK_PER_SHADED_CHUNK = 8u;  // (a hit's normal and shading: about eight march steps' instructions)
__device__ __forceinline__ uint32_t* tile_cost_slot(const FrameParams& P, uint32_t tile) {
    const uint32_t tiles_x = uint32_t(P.width + TILE_W - 1) / TILE_W;
    return &P.tile_cost[(tile >> 16) * tiles_x + (tile & 0xffffu)];
}
__device__ __forceinline__ uint32_t cost_from_cycles(unsigned long long cycles) {
    return uint32_t(min(cycles > 4096ull ? (cycles - 4096ull) >> 10 : 0ull, 1ull << 20));
}
__device__ __forceinline__ uint32_t cost_from_work(uint32_t march_steps, uint32_t hits) {
    return min(march_steps + WORK_PER_SHADED_CHUNK * ((hits + 63u) >> 6), 1u << 20);  // (saturates)
}
__device__ __forceinline__ void record_tile_cost(uint32_t* slot, uint32_t cost, uint32_t batch) {
    if (batch > 1) atomicMax(slot, cost);  // the batch's views share the table (the sort clears it)
    else *slot = cost;
}

// The end of the two queue kernels, 256 threads: the T staged tiles of the group to the destination; cost of each of
// them: the workgroup's, `cost`.
template <int T>
__device__ __forceinline__ void store_group(const FrameParams& P, const uint32_t* s_tiles, const int* s_rows,
                                            const uint32_t (*s_tile)[TILE_H][TILE_W], int tid, uint32_t batch, bool feedback,
                                            uint32_t cost) {
    for (int j = 0; j < T; ++j) {
        const uint32_t tile = s_tiles[j];
        if (tile == 0xffffffffu) break;
        store_tile(P, int(tile & 0xffffu) * TILE_W, int(tile >> 16) * TILE_H, s_rows[j], s_tile[j], tid);
        if (tid == 0 && feedback) record_tile_cost(tile_cost_slot(P, tile), cost, batch);
    }
}

// Pipeline selection: the reference keeps three render pipelines and picks one per frame by fractal_group
// (graphics.rs:310-321); the KIFS shader then switches on primitive_id per SDF call (kifs.wgsl:139-155).  Here both are
// template parameters: launch(integral_constant<int, GROUP>, integral_constant<int, PRIM>) is called with the pair
// that (group, primitive) stand for.  The Julia pipeline's PRIM slot is the build of its long-ray loop (see
// KIFS_DIVSQRT_ORDINARY and KIFS_FAST_TRIP_X2_ in kifs_scene.hpp), `julia_slot` < JULIA_SLOTS, chosen by the caller;
// slots at and above JULIA_SLOTS are not instantiated.
template <int JULIA_SLOTS, class Launch>
hipError_t dispatch_pipeline(uint32_t group, uint32_t primitive, uint32_t julia_slot, Launch&& launch) {
    using std::integral_constant;
    static_assert(JULIA_SLOTS == 2 || JULIA_SLOTS == 4, "sdf_iters <= 24, and the doubled orbit trip above it");
    switch (group) {
    case GROUP_JULIA:
        if constexpr (JULIA_SLOTS == 4) {
            if (julia_slot == 2) return launch(integral_constant<int, GROUP_JULIA>{}, integral_constant<int, 2>{});
            if (julia_slot == 3) return launch(integral_constant<int, GROUP_JULIA>{}, integral_constant<int, 3>{});
        }
        if (julia_slot == 0) return launch(integral_constant<int, GROUP_JULIA>{}, integral_constant<int, 0>{});
        if (julia_slot == 1) return launch(integral_constant<int, GROUP_JULIA>{}, integral_constant<int, 1>{});
        return hipErrorInvalidValue;
    case GROUP_GENJULIA: return launch(integral_constant<int, GROUP_GENJULIA>{}, integral_constant<int, 0>{});
    case GROUP_KIFS:
        switch (primitive) {
        case PRIM_SPHERE: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_SPHERE>{});
        case PRIM_CYLINDER: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_CYLINDER>{});
        case PRIM_BOX: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_BOX>{});
        case PRIM_TORUS: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_TORUS>{});
        case PRIM_SIERPINSKI: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_SIERPINSKI>{});
        case PRIM_BUNNY: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_BUNNY>{});
        default: return launch(integral_constant<int, GROUP_KIFS>{}, integral_constant<int, PRIM_OTHER>{});  // kifs.wgsl:154
        }
    default: return hipErrorInvalidValue;
    }
}

// Before a launch of KERNEL with `bytes` of dynamic LDS: beyond the default limit of 48 KB the kernel has to opt in,
// once per kernel AND per device (the attribute belongs to the device's copy of the code object).
// (two contexts on two threads may come through here at once -- the header allows one caller thread per context --
// hence atomics; setting the attribute twice is harmless, a torn flag would not be)
template <void (*KERNEL)(const BatchParams)>
hipError_t ensure_dynamic_lds(unsigned bytes) {
    if (bytes <= 48 * 1024) return hipSuccess;
    static std::atomic<bool> opted_in[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    if (dev < 0 || dev >= 64 || !opted_in[dev].load(std::memory_order_acquire)) {
        hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (attr != hipSuccess) return attr;
        if (dev >= 0 && dev < 64) opted_in[dev].store(true, std::memory_order_release);
    }
    return hipSuccess;
}

// the bunny's kernels (kifs_bunny_kernels.hip), launched from launch_render's dispatch in kifs_kernels.hip
hipError_t launch_bunny_coop(const BatchParams& B, hipStream_t stream);        // four waves per 64 rays, re-queued
hipError_t launch_bunny_whole_rays(const BatchParams& B, hipStream_t stream);  // four lanes per pixel, start to finish
// k x k supersampling (FrameParams::ssaa > 1), every pipeline (kifs_ssaa_kernels.hip)
hipError_t launch_ssaa(const BatchParams& B, uint32_t group, uint32_t primitive, hipStream_t stream);
// the geometry output (FrameParams::geom non-null), every pipeline (kifs_geometry_kernels.hip)
hipError_t launch_geometry(const BatchParams& B, uint32_t group, uint32_t primitive, hipStream_t stream);
// dynamic LDS that caps how many workgroups share a CU (kifs_kernels.hip)
unsigned residency_pad_bytes(int workgroups_per_cu);

}  // namespace kifs
