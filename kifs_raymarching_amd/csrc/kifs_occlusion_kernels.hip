// kifs_occlusion_kernels.hip -- ambient occlusion (kifs_render_occlusion_async, include/kifs_hip.h): the frame of
// kifs_render_batch_async with every hit's colour attenuated by how closed the surface is around it, and optionally the
// factors themselves as a plane of one f32 per pixel.  The term needs the hit position and the normal, which only the
// kernel holds; it travels in an argument of its own (occl::Params), so FrameParams and every other kernel stay as they
// are.
//
//   occl::render_kernel<GROUP, PRIM>  ssaa::render_kernel's shape, widened to k = 1: 256 threads per 32 x 8 OUTPUT tile
//                                     of the launch's tile order, wave w owns 8 x 8 output block w, a lane owns one
//                                     output pixel and marches its k^2 samples one after another, whole rays
//                                     (raymarch_occluded, kifs_scene.hpp), summing their linear colours in its LDS
//                                     slots; the mean is encoded and stored through the LDS tile.  The plane (k = 1
//                                     only) is one dword store per lane: the eight lanes of a block row write 32
//                                     contiguous bytes.
// Sample (i, j) of output pixel (x, y) is pixel (k x + i, k y + j) of the virtual screen k W x k H, as in
// kifs_ssaa_kernels.hip; with k = 1 that is the frame itself.  A miss -- culled waves included -- is the background and
// stores 1.0f.
#include "kifs_render_common.hpp"

namespace kifs {
namespace occl {

// The kernel has three phases -- the prologue, a sample's march and shading, the store -- and each reads what it needs
// of the kernel argument anew (scalar loads of uniform addresses, a handful of cycles against a march's thousands).
// Held in SGPRs from the kernel's start, the frame constants, the term and the plane would stay live across the sample
// loop's back edge and across the march, whose hand-written loops pin s74-s97: that cost the Julia builds spill slots
// for whole SGPR tuples and the bunny's two dozen parked registers.  occl::anew (kifs_scene.hpp) ties a phase's loads to its place.
// A phase's view of the lane's pixel is tile_pixel (kifs_render_common.hpp).

// (amdgpu_waves_per_eu: as ssaa::render_kernel)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const Params O) {
    __shared__ float s_srgb[256];
    __shared__ uint32_t s_tile[TILE_H][TILE_W];
    __shared__ float s_acc[3][BLOCK];  // per lane: the running sums of its samples' linear colours

    // the argument is this kernel's one parameter, at the start of the segment
    const ConstParams K = (ConstParams)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x;
    // (from the argument as the compiler sees it: the entry's load stays a scalar one)
    const uint32_t tile = O.B.frame.tile_order[launch_slot(O.B).index];
    {
        const TilePixel F = tile_pixel(K, tile);
        if (F.P.encode == 1) s_srgb[tid] = F.P.srgb_table[tid];  // visible after the next barrier
    }
    // The resolve of kifs_set_supersampling, per channel in f32: acc = c(0,0), then acc + c(i,j) with j outer and i
    // inner, mean = acc / k^2 correctly rounded (k = 1: c / 1 = c).  A culled sample is the background colour.
    float a = 1.0f;  // the plane's value: the factor of the (one) sample's hit, 1 on a miss
    for (int s = 0;; ++s) {
        const TilePixel F = tile_pixel(K, tile);
        const int k = F.P.ssaa;  // uniform, 1..KIFS_MAX_SUPERSAMPLING
        if (s >= k * k || __ballot(F.valid) == 0ull) break;  // wave-uniform; a wave without a pixel in the frame marches nothing
        // The virtual screen, as ssaa::render_kernel's: height k H, same aspect float, its own 1 / height for the
        // wave-level cull (k = 1: the frame's own values, bit for bit).
        FrameParams V = F.P;
        V.height = float(k) * V.height;  // exact: integers below 2^24
        V.inv_height = V.ssaa_inv_height;
        V.counters = nullptr;
        const int j = s / k, i = s - j * k;  // scalar
        const int vx = k * F.x + i, vy = k * F.y + j;
        V3 c = V.background_color;
        if (!wave_is_culled(V, vx, vy, F.valid)) {  // wave-uniform
            const V3 dir = ray_direction(V, vx, vy);
            const Occluded r = raymarch_occluded<GROUP, PRIM>(V, K, dir, F.valid);
            c = r.colour;
            a = r.a;
        }
        s_acc[0][tid] = s == 0 ? c.x : s_acc[0][tid] + c.x;
        s_acc[1][tid] = s == 0 ? c.y : s_acc[1][tid] + c.y;
        s_acc[2][tid] = s == 0 ? c.z : s_acc[2][tid] + c.z;
    }
    const TilePixel F = tile_pixel(K, tile);
    // the factor of pixel (x, y): row y - y0 of view `view`'s plane (rows of a band are packed, as the colour's)
    const ConstParams L = anew(K);
    float* const plane = L->plane;
    if (plane && F.valid) plane[size_t(F.view) * L->stride_words + size_t(F.tile_y + F.ly) * L->pitch_words + size_t(F.x)] = a;
    const float n = float(F.P.ssaa * F.P.ssaa);
    const V3 mean{s_acc[0][tid] / n, s_acc[1][tid] / n, s_acc[2][tid] / n};  // (a lane outside the frame: not stored)
    __syncthreads();  // s_srgb visible
    s_tile[F.ly][F.lx] = encode_rgba(mean, F.P.encode == 1, s_srgb);
    __syncthreads();
    store_tile(F.P, F.tile_x, F.tile_y, F.frame_y, s_tile, tid);
}

template <int GROUP, int PRIM>
static hipError_t launch(const Params& O, hipStream_t stream) {
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(O.B.frame.tile_count * uint32_t(O.B.count)), dim3(BLOCK), 0, stream,
                       O);
    return hipGetLastError();
}

}  // namespace occl

hipError_t launch_occlusion(const occl::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = O.B.frame;
    // (refused by the API before it gets here)
    if (P.ssaa < 1 || P.ssaa > 4 || O.ao.samples < 1 || O.ao.samples > 16 || (O.plane && P.ssaa > 1) || P.stripe_rows || O.B.table ||
        O.B.count < 1 || O.B.count > MAX_BATCH_INLINE)
        return hipErrorInvalidValue;
    // the ten instantiations, picked as launch_ssaa picks them
    return dispatch_pipeline<2>(group, primitive, uint32_t(P.sdf_iters <= 24), [&](auto g, auto prim) {
        return occl::launch<decltype(g)::value, decltype(prim)::value>(O, stream);
    });
}

}  // namespace kifs
