// kifs_ssaa_kernels.hip -- k x k supersampling with the resolve fused into the render (kifs_set_supersampling,
// include/kifs_hip.h).  Only the kernel holds a pixel's linear colour before the encode, so only here can its samples
// be averaged in the right space.
//
//   ssaa::render_kernel<GROUP, PRIM>  256 threads per 32 x 8 OUTPUT tile of the launch's tile order, exactly as
//                                     kifs::render_kernel takes them: wave w owns 8 x 8 output block w, a lane owns one
//                                     output pixel and marches its k^2 samples one after another, whole rays, summing
//                                     their linear colours in VGPRs; then the mean is encoded and stored through the
//                                     LDS tile as everywhere else.
// Sample (i, j) of output pixel (x, y) is pixel (k x + i, k y + j) of a VIRTUAL screen k W x k H with the frame's
// aspect ratio: the same fs_main (ray_direction) at the same kind of fragment centre, so every sample is a pixel of a
// plain frame of that size.  The output geometry -- tile table, stripes, bands, views, order -- is the plain launch's.
#include "kifs_render_common.hpp"

namespace kifs {
namespace ssaa {

// (amdgpu_waves_per_eu: around the sample loop the compiler otherwise keeps more of the Julia march's constants in
// VGPRs than kifs::render_kernel does -- 84, five waves per SIMD; asked for six it fits them in 80 without spilling)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const BatchParams B) {
    __shared__ float s_srgb[256];
    __shared__ uint32_t s_tile[TILE_H][TILE_W];
    __shared__ float s_acc[3][BLOCK];  // per lane: the running sums of its samples' linear colours

    const TileFrame F = tile_frame(B, s_srgb);  // the OUTPUT tile and this lane's output pixel
    const FrameParams& P = F.P;
    const int tid = threadIdx.x;
    const int x = F.x, y = F.y;
    const bool valid = F.valid;
    // The virtual screen: height k H, same aspect float.  Only the wave-level quick cull is valid on it (with ITS
    // 1 / height); the tile-level cull's margin belongs to the pixel centres of a plain 32 x 8 tile.
    const int k = P.ssaa;  // uniform, 2..KIFS_MAX_SUPERSAMPLING
    FrameParams V = P;
    V.height = float(k) * P.height;  // exact: integers below 2^24
    V.inv_height = P.ssaa_inv_height;
    V.counters = nullptr;  // (the per-wave diagnostics describe one march per wave)

    // The resolve of the contract, per channel in f32: acc = c(0,0), then acc + c(i,j) with j outer and i inner
    // (-ffp-contract=off: no fma), mean = acc / k^2 correctly rounded.  A culled sample is the background colour.
    // The sums live in the lane's own LDS slots, not in VGPRs: three more registers held across the Julia march
    // (whose hand-written loop pins v30-v63) cost its sixth wave per SIMD.
    // One loop over s = j k + i rather than two nested ones: nothing of a sample's ray set-up is invariant across
    // the loop, so the compiler keeps none of it in registers through the march.
    if (__ballot(valid) != 0ull) {  // wave-uniform
        for (int s = 0; s < k * k; ++s) {
            const int j = s / k, i = s - j * k;  // scalar
            const int vx = k * x + i, vy = k * y + j;
            V3 c = P.background_color;
            if (!wave_is_culled(V, vx, vy, valid)) {  // wave-uniform
                int steps = 0;
                const V3 dir = ray_direction(V, vx, vy);
                c = raymarch<GROUP, PRIM>(V, dir, valid, steps);
            }
            s_acc[0][tid] = s == 0 ? c.x : s_acc[0][tid] + c.x;
            s_acc[1][tid] = s == 0 ? c.y : s_acc[1][tid] + c.y;
            s_acc[2][tid] = s == 0 ? c.z : s_acc[2][tid] + c.z;
        }
    }
    const float n = float(k * k);
    const V3 mean{s_acc[0][tid] / n, s_acc[1][tid] / n, s_acc[2][tid] / n};  // (a lane outside the frame: not stored)
    __syncthreads();  // s_srgb visible
    s_tile[F.ly][F.lx] = encode_rgba(mean, F.srgb, s_srgb);
    __syncthreads();
    store_tile(P, F.tile_x, F.tile_y, F.frame_y, s_tile, tid);
}

template <int GROUP, int PRIM>
static hipError_t launch(const BatchParams& B, hipStream_t stream) {
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(B.frame.tile_count * uint32_t(B.count)), dim3(BLOCK), 0, stream,
                       B);
    return hipGetLastError();
}

}  // namespace ssaa

hipError_t launch_ssaa(const BatchParams& B, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = B.frame;
    if (P.ssaa < 2 || P.ssaa > 4) return hipErrorInvalidValue;
    // Julia: the short divide / square root by sdf_iters; the doubled orbit trip is the throughput kernels' only
    // (launch_variant's LPRIM).  The bunny: per-lane bunny_sdf -- slow, correct.
    return dispatch_pipeline<2>(group, primitive, uint32_t(P.sdf_iters <= 24), [&](auto g, auto prim) {
        return ssaa::launch<decltype(g)::value, decltype(prim)::value>(B, stream);
    });
}

}  // namespace kifs
