// kifs_internal.hpp -- launcher prototypes shared by the host code and the kernel files (kifs_kernels.hip,
// kifs_support_kernels.hip, kifs_adaptive_kernels.hip, kifs_animation_kernels.hip, kifs_accumulate_kernels.hip,
// kifs_rays_kernels.hip, kifs_occlusion_kernels.hip, kifs_lighting_kernels.hip, kifs_trap_kernels.hip, kifs_fold_kernels.hip,
// kifs_fold_trap_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "kifs_params.hpp"

namespace kifs {

hipError_t launch_render(const BatchParams& B, uint32_t group, uint32_t primitive,
                         hipStream_t stream);
// Adaptive anti-aliasing (kifs_adaptive_kernels.hip; the host side is kifs_adaptive.cpp).  Pass B: the edge pixels of
// `count` planes of `stride_texels` texels each (rows of `width`) by the pair rule, appended to view i's queue at
// queues + i * stride_texels and counted in counts[i] (zero beforehand).  Pass C: the queued pixels' k x k resolves,
// `groups_per_view` workgroups per view.
hipError_t launch_adaptive_classify(const float* planes, uint32_t stride_texels, int width, int height, int count,
                                    float normal_cos, float depth_rel, uint32_t* queues, uint32_t* counts, hipStream_t stream);
hipError_t launch_adaptive_render(const adaptive::Params& A, uint32_t group, uint32_t primitive, uint32_t groups_per_view,
                                  hipStream_t stream);
// Animated batches (kifs_animation_kernels.hip; the host side is kifs_animation.cpp): launch_render's whole-ray form
// with view i's scene record laid over the frame constants.
hipError_t launch_animation_render(const anim::Params& A, uint32_t group, uint32_t primitive, hipStream_t stream);
// Accumulated frames (kifs_accumulate_kernels.hip; the host side is kifs_accumulate.cpp): every output frame the mean of
// its sub-frames' linear colours, one workgroup per 8 x 8 output block and output frame.
hipError_t launch_accumulate_render(const accum::Params& A, uint32_t group, uint32_t primitive, hipStream_t stream);
// One pass of a progressive frame (kifs_render_accumulate_resume_async; the host side is kifs_progressive.cpp): the same
// launch with the resolve started from, and written back to, a plane of f32 sums (accum::carry_render_kernel).
hipError_t launch_accumulate_carry(const accum::CarryParams& K, uint32_t group, uint32_t primitive, hipStream_t stream);
// One converging pass (kifs_render_accumulate_converge_async; the host side is kifs_converge.cpp): the same launch again,
// marching only the pixels whose mean has not settled (accum::converge_render_kernel).
hipError_t launch_accumulate_converge(const accum::ConvergeParams& K, uint32_t group, uint32_t primitive, hipStream_t stream);
// Ray queries (kifs_trace_rays_async; kifs_rays_kernels.hip, the host side is kifs_rays.cpp): one caller-supplied ray per
// lane, ceil(n / 256) workgroups (rays::trace_render_kernel).
hipError_t launch_trace_rays(const rays::Params& R, uint32_t group, uint32_t primitive, hipStream_t stream);
// Ambient occlusion (kifs_render_occlusion_async; kifs_occlusion_kernels.hip, the host side is kifs_occlusion.cpp): the
// supersampled launch's shape from k = 1 up, every hit attenuated by its own factor (occl::render_kernel).
hipError_t launch_occlusion(const occl::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream);
// A configurable light (kifs_render_lit_async; kifs_lighting_kernels.hip, the host side is kifs_lighting.cpp): the same
// shape, every hit shaded by the launch's light and, with a term, attenuated by its factor (light::render_kernel).
hipError_t launch_lit(const light::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream);
// Orbit-trap surface colouring (kifs_render_trapped_async; kifs_trap_kernels.hip, the host side is kifs_trap.cpp): the
// lit launch with every hit's colour from the launch's trap (trap::render_kernel); and kifs_eval_trap's u of E.n
// positions, one per lane (trap::eval_kernel).
hipError_t launch_trapped(const trap::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream);
hipError_t launch_eval_trap(const trap::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream);
// Kaleidoscopic IFS scenes (kifs_render_folded_async; kifs_fold_kernels.hip, the host side is kifs_fold.cpp): the lit
// launch with the folded estimate in the place of the scene's (fold::render_kernel); and kifs_eval_fold's estimate and
// normal at E.n positions, one per lane (fold::eval_kernel).  KIFS group only.
hipError_t launch_folded(const fold::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream);
hipError_t launch_eval_fold(const fold::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream);
// Orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async; kifs_fold_trap_kernels.hip, the host side is
// kifs_fold_trap.cpp): the folded launch with every hit's colour from the orbit of the fold and the launch's trap, both
// read from O.record in device memory, and the optional plane of u (foldorbit::render_kernel); and kifs_eval_fold_trap's u
// of E.n positions, one per lane (foldorbit::eval_kernel).  KIFS group only.
hipError_t launch_folded_trapped(const foldorbit::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream);
hipError_t launch_eval_fold_trap(const foldorbit::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream);
// Device-side counting sort: order[] = tile ids (x | y << 16) by descending cost[] >> shift (1024 bins);
// clears cost[].
hipError_t launch_tile_order(uint32_t* cost, uint32_t* order, uint32_t tile_count,
                             uint32_t tiles_x, uint32_t shift, hipStream_t stream);
// The same for a batch's costs, with a memory: seen[] (tile_count words, zero at first) keeps every tile's largest cost
// of the last `window` (1..255) calls, and the order is made from that.  window 1: the order of cost[] alone.
hipError_t launch_tile_order_remembering(uint32_t* cost, uint32_t* seen, uint32_t* order, uint32_t tile_count,
                                         uint32_t tiles_x, uint32_t shift, uint32_t window, hipStream_t stream);
// Packed row shards -> frame rows: stripe s of shard f (8 rows at src + f * src_shard_stride + 8 s *
// src_pitch) goes to frame rows stripe_rows[s].. of dst + f * dst_frame_stride.
hipError_t launch_unpack_stripes(uint8_t* dst, size_t dst_pitch, size_t dst_frame_stride, const uint8_t* src,
                                 size_t src_pitch, size_t src_shard_stride, const uint32_t* stripe_rows,
                                 int n_stripes, int count, int width, int height, hipStream_t stream);
// Sparse shards (see pack_sparse_kernel): records of SPARSE_RECORD_WORDS words for the tiles of packed shards
// that hold a pixel other than `background`; *n_records must be zero beforehand.  And back: records -> frame
// rows; the background over the rows of the listed stripes.
constexpr int SPARSE_RECORD_WORDS_HOST = 260;
hipError_t launch_pack_sparse(const uint8_t* src, size_t src_pitch, size_t src_shard_stride, const uint32_t* stripe_rows,
                              int n_stripes, int count, int width, int height, uint32_t background, uint32_t* records,
                              uint32_t* n_records, hipStream_t stream);
hipError_t launch_unpack_sparse(uint8_t* dst, size_t dst_pitch, size_t dst_frame_stride, const uint32_t* records,
                                uint32_t n_records, const uint32_t* stripe_rows, int n_stripes, int count, int width,
                                int height, int erase, uint32_t background, hipStream_t stream);
hipError_t launch_fill_stripes(uint8_t* dst, size_t dst_pitch, size_t dst_frame_stride, const uint32_t* stripe_rows,
                               int n_stripes, int count, int width, int height, uint32_t background, hipStream_t stream);
hipError_t launch_eval_points(const FrameParams& P, uint32_t group, uint32_t primitive,
                              const float* pts, int n, float* sdf, float* nrm,
                              hipStream_t stream);
hipError_t launch_eval_math(int fn, const float* in, float param, const float* srgb_table,
                            float* out, int n, hipStream_t stream);

// Workgroup tile geometry of render_kernel (shared with the host-side tile ordering).
constexpr int TILE_W = 32;
constexpr int TILE_H = 8;

// 256 sRGB thresholds: t[k] = smallest f32 whose ideal sRGB UNORM8 encoding is >= k.
void build_srgb_thresholds(float t[256]);

}  // namespace kifs
