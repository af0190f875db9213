// kifs_fold_kernels.hip -- kaleidoscopic IFS scenes (kifs_render_folded_async, include/kifs_hip.h): the frame of
// kifs_render_lit_async with the scene's estimate replaced by that of a base primitive seen through N rounds of fold,
// rotate and scale (folded_sdf, kifs_scene.hpp) -- in the march, the normal, the shadow ray and the occlusion probes.
// The light, the optional occlusion term and the fold system travel in an argument of its own (fold::Params), so
// FrameParams and every other kernel stay as they are.
//
//   fold::render_kernel<GROUP, PRIM>  trap::render_kernel's shape: 256 threads per 32 x 8 OUTPUT tile of the launch's tile
//                                     order, wave w owns 8 x 8 output block w, a lane owns one output pixel and
//                                     marches its k^2 samples one after another, whole rays (raymarch_folded), summing
//                                     their linear colours in its LDS slots; the mean is encoded and stored through the
//                                     LDS tile.
//   fold::eval_kernel<GROUP, PRIM>    kifs_eval_fold: the folded estimate and/or its normal at one caller-supplied
//                                     position per lane.
// Only the KIFS group has a folded form (GROUP is in the name as in every render kernel's, and is GROUP_KIFS): seven
// instantiations each, the six primitives and the unknown id.  The launch
// carries no cull (kifs_fold.cpp zeroes all three): wave_is_culled then answers false and a miss is what the march says.
#include <cstddef>

#include "../../include/kifs_hip.h"
#include "kifs_render_common.hpp"

namespace kifs {
namespace fold {

static_assert(offsetof(Params, light) == offsetof(light::Params, light) && offsetof(Params, ao) == offsetof(light::Params, ao) &&
                  offsetof(Params, has_ao) == offsetof(light::Params, has_ao),
              "lit_shade reads the argument as light::Params");

// The virtual screen of sample s of the launch's k^2 and the sample's pixel on it, as trap::render_kernel's.
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
    static_assert(GROUP == GROUP_KIFS, "the two Julia pipelines have no folded form");
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
    // inner, mean = acc / k^2 correctly rounded (k = 1: c / 1 = c).
    for (int s = 0;; ++s) {
        const TilePixel F = tile_pixel(K, tile);
        const int k = F.P.ssaa;
        if (s >= k * k || __ballot(F.valid) == 0ull) break;  // wave-uniform; a wave without a pixel in the frame marches nothing
        const Sample a = sample_of(F, s);
        V3 c = a.V.background_color;
        if (!wave_is_culled(a.V, a.vx, a.vy, F.valid)) {  // wave-uniform; the launch's culls are off: always marched
            const V3 dir = ray_direction(a.V, a.vx, a.vy);
            c = raymarch_folded<PRIM>(a.V, K, dir, F.valid, [&]() __attribute__((always_inline)) {
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
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(O.B.frame.tile_count * uint32_t(O.B.count)), dim3(BLOCK), 0, stream, O);
    return hipGetLastError();
}

// One position per lane, 256 lanes per workgroup; a lane past the end leaves before the estimate (its wave's trip count
// is that of the lanes that stay).
template <int GROUP, int PRIM>
__global__ __launch_bounds__(256) void eval_kernel(const EvalParams E) {
    static_assert(GROUP == GROUP_KIFS, "the two Julia pipelines have no folded form");
    typedef const EvalParams __attribute__((address_space(4))) * ConstEval;
    const ConstEval K = (ConstEval)__builtin_amdgcn_kernarg_segment_ptr();
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= E.n) return;
    const V3 p{E.points[3 * i], E.points[3 * i + 1], E.points[3 * i + 2]};
    if (E.sdf) E.sdf[i] = folded_sdf<PRIM>(E.frame, &K->fold, p, ~0ull);
    if (E.normal) {
        const V3 v = normal_fd(E.frame.epsilon, p, [&](V3 e) __attribute__((always_inline)) { return folded_sdf<PRIM>(E.frame, &K->fold, e, ~0ull); });
        E.normal[3 * i] = v.x;
        E.normal[3 * i + 1] = v.y;
        E.normal[3 * i + 2] = v.z;
    }
}

template <int GROUP, int PRIM>
static hipError_t launch_eval(const EvalParams& E, hipStream_t stream) {
    hipLaunchKernelGGL((eval_kernel<GROUP, PRIM>), dim3((uint32_t(E.n) + 255u) / 256u), dim3(256), 0, stream, E);
    return hipGetLastError();
}

static bool fold_in_range(const Fold& F) {
    return F.stages <= 31u && F.iterations >= 0 && F.iterations <= KIFS_MAX_FOLD_ITERATIONS && F.scale >= 1.0f && F.scale <= 16.0f;
}

}  // namespace fold

hipError_t launch_folded(const fold::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = O.B.frame;
    // (refused by the API before it gets here)
    if (group != uint32_t(GROUP_KIFS) || P.ssaa < 1 || P.ssaa > KIFS_MAX_SUPERSAMPLING || O.light.shininess_log2 < 0 ||
        O.light.shininess_log2 > KIFS_MAX_SHININESS_LOG2 || (O.has_ao && (O.ao.samples < 1 || O.ao.samples > KIFS_MAX_AO_SAMPLES)) ||
        !fold::fold_in_range(O.fold) || P.stripe_rows || O.B.table || O.B.count < 1 || O.B.count > MAX_BATCH_INLINE)
        return hipErrorInvalidValue;
    // the seven instantiations: the six primitives and the unknown id
    return dispatch_pipeline<2>(group, primitive, 0u, [&](auto g, auto prim) {
        if constexpr (decltype(g)::value == GROUP_KIFS) return fold::launch<GROUP_KIFS, decltype(prim)::value>(O, stream);
        else return hipErrorInvalidValue;
    });
}

hipError_t launch_eval_fold(const fold::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream) {
    if (E.n <= 0) return hipSuccess;
    if (group != uint32_t(GROUP_KIFS) || !fold::fold_in_range(E.fold) || !E.points || (!E.sdf && !E.normal)) return hipErrorInvalidValue;
    return dispatch_pipeline<2>(group, primitive, 0u, [&](auto g, auto prim) {
        if constexpr (decltype(g)::value == GROUP_KIFS) return fold::launch_eval<GROUP_KIFS, decltype(prim)::value>(E, stream);
        else return hipErrorInvalidValue;
    });
}

}  // namespace kifs
