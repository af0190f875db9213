// kifs_trap_kernels.hip -- orbit-trap surface colouring (kifs_render_trapped_async, include/kifs_hip.h): the frame of
// kifs_render_lit_async with every hit's colour taken from a gradient over how close the hit point's orbit comes to a
// trap -- a point, a line or a plane of orbit space -- in the place of the one fractal colour.  The light, the optional
// occlusion term and the trap travel in an argument of its own (trap::Params), so FrameParams and every other kernel stay
// as they are.
//
//   trap::render_kernel<GROUP, PRIM>  light::render_kernel's shape: 256 threads per 32 x 8 OUTPUT tile of the launch's
//                                     tile order, wave w owns 8 x 8 output block w, a lane owns one output pixel and
//                                     marches its k^2 samples one after another, whole rays (raymarch_trapped,
//                                     kifs_scene.hpp), summing their linear colours in its LDS slots; the mean is
//                                     encoded and stored through the LDS tile.
//   trap::eval_kernel<GROUP, PRIM>    kifs_eval_trap: u of one caller-supplied position per lane (orbit_trap).
// Sample (i, j) of output pixel (x, y) is pixel (k x + i, k y + j) of the virtual screen k W x k H, as in
// kifs_ssaa_kernels.hip; with k = 1 that is the frame itself.  A miss -- culled waves included -- is the background.
#include "../../include/kifs_hip.h"
#include "kifs_render_common.hpp"

namespace kifs {
namespace trap {

// The phases read what they need of the kernel argument anew, as light::render_kernel's do and for its reasons
// (trap::anew, kifs_scene.hpp; tile_pixel, kifs_render_common.hpp); the trap itself is read where the shading asks for a
// hit's colour, after the march and the shadow ray.

// The virtual screen of sample s of the launch's k^2 and the sample's pixel on it, as light::render_kernel's.
struct Sample {
    FrameParams V;
    int vx, vy;
};
__device__ __forceinline__ Sample sample_of(const TilePixel& F, int s) {
    const int k = F.P.ssaa;  // uniform, 1..KIFS_MAX_SUPERSAMPLING
    Sample r{F.P, 0, 0};
    r.V.height = float(k) * r.V.height;  // exact: integers below 2^24
    r.V.inv_height = r.V.ssaa_inv_height;
    r.V.counters = nullptr;
    const int j = s / k, i = s - j * k;  // scalar
    r.vx = k * F.x + i;
    r.vy = k * F.y + j;
    return r;
}

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
    for (int s = 0;; ++s) {
        const TilePixel F = tile_pixel(K, tile);
        const int k = F.P.ssaa;
        if (s >= k * k || __ballot(F.valid) == 0ull) break;  // wave-uniform; a wave without a pixel in the frame marches nothing
        const Sample a = sample_of(F, s);
        V3 c = a.V.background_color;
        if (!wave_is_culled(a.V, a.vx, a.vy, F.valid)) {  // wave-uniform
            const V3 dir = ray_direction(a.V, a.vx, a.vy);
            c = raymarch_trapped<GROUP, PRIM>(a.V, K, dir, F.valid, [&]() __attribute__((always_inline)) {
                const Sample b = sample_of(tile_pixel(K, tile), s);
                return ray_direction(b.V, b.vx, b.vy);
            });
        }
        s_acc[0][tid] = s == 0 ? c.x : s_acc[0][tid] + c.x;
        s_acc[1][tid] = s == 0 ? c.y : s_acc[1][tid] + c.y;
        s_acc[2][tid] = s == 0 ? c.z : s_acc[2][tid] + c.z;
    }
    const TilePixel F = tile_pixel(K, tile);
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

// One position per lane, 256 lanes per workgroup; a lane past the end leaves before the orbit (its wave's trip count is
// that of the lanes that stay).
template <int GROUP, int PRIM>
__global__ __launch_bounds__(256) void eval_kernel(const EvalParams E) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= E.n) return;
    const V3 p{E.points[3 * i], E.points[3 * i + 1], E.points[3 * i + 2]};
    E.u[i] = orbit_trap<GROUP, PRIM>(E.frame, E.trap, p);
}

template <int GROUP, int PRIM>
static hipError_t launch_eval(const EvalParams& E, hipStream_t stream) {
    hipLaunchKernelGGL((eval_kernel<GROUP, PRIM>), dim3((uint32_t(E.n) + 255u) / 256u), dim3(256), 0, stream, E);
    return hipGetLastError();
}

static bool trap_in_range(const Trap& T) {
    return T.axes >= 1u && T.axes <= 15u && T.iterations >= 0 && T.iterations <= KIFS_MAX_TRAP_ITERATIONS;
}

}  // namespace trap

hipError_t launch_trapped(const trap::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = O.B.frame;
    // (refused by the API before it gets here)
    if (P.ssaa < 1 || P.ssaa > KIFS_MAX_SUPERSAMPLING || O.light.shininess_log2 < 0 || O.light.shininess_log2 > KIFS_MAX_SHININESS_LOG2 ||
        (O.has_ao && (O.ao.samples < 1 || O.ao.samples > KIFS_MAX_AO_SAMPLES)) || !trap::trap_in_range(O.trap) || P.stripe_rows ||
        O.B.table || O.B.count < 1 || O.B.count > MAX_BATCH_INLINE)
        return hipErrorInvalidValue;
    // the ten instantiations, picked as launch_lit picks them
    return dispatch_pipeline<2>(group, primitive, uint32_t(P.sdf_iters <= 24), [&](auto g, auto prim) {
        return trap::launch<decltype(g)::value, decltype(prim)::value>(O, stream);
    });
}

hipError_t launch_eval_trap(const trap::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream) {
    if (E.n <= 0) return hipSuccess;
    if (!trap::trap_in_range(E.trap) || !E.points || !E.u) return hipErrorInvalidValue;
    // (the Julia slot picks a form of the march's loop, which no orbit here runs: one instantiation serves both)
    return dispatch_pipeline<2>(group, primitive, 0u, [&](auto g, auto prim) {
        constexpr int G = decltype(g)::value;
        constexpr int PR = G == GROUP_JULIA ? 0 : decltype(prim)::value;
        return trap::launch_eval<G, PR>(E, stream);
    });
}

}  // namespace kifs
