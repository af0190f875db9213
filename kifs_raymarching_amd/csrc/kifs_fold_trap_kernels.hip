// kifs_fold_trap_kernels.hip -- orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async,
// include/kifs_hip.h): the frame of kifs_render_folded_async with every hit's colour taken from a gradient over how close
// the hit point's orbit -- the point after each round of the fold, continued by the base primitive's own -- comes to a
// trap.  The light and the optional occlusion term travel in the kernel argument at light::Params' offsets; the fold
// system and the trap do not fit beside them and are read from a 128-byte record in device memory (foldorbit::Record),
// through a pointer cast to the constant address space, so that FrameParams, BatchParams and every other kernel stay as
// they are.
//
//   foldorbit::render_kernel<GROUP, PRIM>  fold::render_kernel's shape: 256 threads per 32 x 8 OUTPUT tile of the launch's
//                                         tile order, wave w owns 8 x 8 output block w, a lane owns one output pixel and
//                                         marches its k^2 samples one after another, whole rays
//                                         (raymarch_folded_trapped, kifs_scene.hpp), summing their linear colours in its
//                                         LDS slots; the mean is encoded and stored through the LDS tile.  The plane of u
//                                         (k = 1 only) is the occlusion kernel's store: one dword per lane, the eight
//                                         lanes of a block row write 32 contiguous bytes.  A miss stores +inf.
//   foldorbit::eval_kernel<PRIM>           kifs_eval_fold_trap: u of one caller-supplied position per lane
//                                         (folded_orbit_trap).  The orbit alone: no base estimate is taken, and only the
//                                         Sierpinski primitive continues the orbit, so there are two instantiations.
// Only the KIFS group has a folded form: seven render instantiations, the six primitives and the unknown id.  The launch
// carries no cull (kifs_fold_trap.cpp zeroes all three), as the folded call's.
#include <cmath>
#include <cstddef>

#include "../../include/kifs_hip.h"
#include "kifs_render_common.hpp"

namespace kifs {
namespace foldorbit {

static_assert(offsetof(Params, light) == offsetof(light::Params, light) && offsetof(Params, ao) == offsetof(light::Params, ao) &&
                  offsetof(Params, has_ao) == offsetof(light::Params, has_ao),
              "the argument is light::Params' fields at their offsets");
static_assert(offsetof(Params, light) == offsetof(trap::Params, light) && offsetof(Params, ao) == offsetof(trap::Params, ao) &&
                  offsetof(Params, has_ao) == offsetof(trap::Params, has_ao),
              "trapped_shade reads the argument as trap::Params");
static_assert(offsetof(Params, record) == sizeof(light::Params) && offsetof(Params, plane) == sizeof(light::Params) + 8 &&
                  offsetof(Params, pitch_words) == sizeof(light::Params) + 16 && offsetof(Params, stride_words) == sizeof(light::Params) + 20,
              "behind them: the record, the plane, its pitch and stride");
static_assert(offsetof(Record, fold) == 0 && offsetof(Record, trap) == 64, "the record: fold::Fold, trap::Trap, padding");

// The virtual screen of sample s of the launch's k^2 and the sample's pixel on it, as fold::render_kernel's.
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
    float u = INFINITY;  // the plane's value: u of the (one) sample's hit, +inf on a miss
    for (int s = 0;; ++s) {
        const TilePixel F = tile_pixel(K, tile);
        const int k = F.P.ssaa;
        if (s >= k * k || __ballot(F.valid) == 0ull) break;  // wave-uniform; a wave without a pixel in the frame marches nothing
        const Sample a = sample_of(F, s);
        V3 c = a.V.background_color;
        if (!wave_is_culled(a.V, a.vx, a.vy, F.valid)) {  // wave-uniform; the launch's culls are off: always marched
            const V3 dir = ray_direction(a.V, a.vx, a.vy);
            c = raymarch_folded_trapped<PRIM>(a.V, K, dir, F.valid, u, [&]() __attribute__((always_inline)) {
                const Sample b = sample_of(tile_pixel(K, tile), s);
                return ray_direction(b.V, b.vx, b.vy);
            });
        }
        s_acc[0][tid] = s == 0 ? c.x : s_acc[0][tid] + c.x;
        s_acc[1][tid] = s == 0 ? c.y : s_acc[1][tid] + c.y;
        s_acc[2][tid] = s == 0 ? c.z : s_acc[2][tid] + c.z;
    }
    const TilePixel F = tile_pixel(K, tile);
    // u of pixel (x, y): row y - y0 of view `view`'s plane (rows of a band are packed, as the colour's)
    const ConstParams L = anew(K);
    float* const plane = L->plane;
    if (plane && F.valid) plane[size_t(F.view) * L->stride_words + size_t(F.tile_y + F.ly) * L->pitch_words + size_t(F.x)] = u;
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

// One position per lane, 256 lanes per workgroup; a lane past the end leaves before the orbit (its wave's trip count is
// that of the lanes that stay).  The two records are read from the kernel argument, which is constant address space.
template <int PRIM>
__global__ __launch_bounds__(256) void eval_kernel(const EvalParams E) {
    typedef const EvalParams __attribute__((address_space(4))) * ConstEval;
    const ConstEval K = (ConstEval)__builtin_amdgcn_kernarg_segment_ptr();
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= E.n) return;
    const V3 p{E.points[3 * i], E.points[3 * i + 1], E.points[3 * i + 2]};
    E.u[i] = folded_orbit_trap<PRIM>(E.frame, &K->fold, &K->trap, p);
}

template <int PRIM>
static hipError_t launch_eval(const EvalParams& E, hipStream_t stream) {
    hipLaunchKernelGGL((eval_kernel<PRIM>), dim3((uint32_t(E.n) + 255u) / 256u), dim3(256), 0, stream, E);
    return hipGetLastError();
}

}  // namespace foldorbit

hipError_t launch_folded_trapped(const foldorbit::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = O.B.frame;
    // (refused by the API before it gets here; the record's ranges are the API's to check: it lies in device memory)
    if (group != uint32_t(GROUP_KIFS) || P.ssaa < 1 || P.ssaa > KIFS_MAX_SUPERSAMPLING || O.light.shininess_log2 < 0 ||
        O.light.shininess_log2 > KIFS_MAX_SHININESS_LOG2 || (O.has_ao && (O.ao.samples < 1 || O.ao.samples > KIFS_MAX_AO_SAMPLES)) ||
        !O.record || (O.plane && P.ssaa > 1) || P.stripe_rows || O.B.table || O.B.count < 1 || O.B.count > MAX_BATCH_INLINE)
        return hipErrorInvalidValue;
    // the seven instantiations: the six primitives and the unknown id
    return dispatch_pipeline<2>(group, primitive, 0u, [&](auto g, auto prim) {
        if constexpr (decltype(g)::value == GROUP_KIFS) return foldorbit::launch<GROUP_KIFS, decltype(prim)::value>(O, stream);
        else return hipErrorInvalidValue;
    });
}

hipError_t launch_eval_fold_trap(const foldorbit::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream) {
    if (E.n <= 0) return hipSuccess;
    const fold::Fold& F = E.fold;
    if (group != uint32_t(GROUP_KIFS) || F.stages > 31u || F.iterations < 0 || F.iterations > KIFS_MAX_FOLD_ITERATIONS ||
        !(F.scale >= 1.0f && F.scale <= 16.0f) || E.trap.axes < 1u || E.trap.axes > 15u || E.trap.iterations < 0 ||
        E.trap.iterations > KIFS_MAX_TRAP_ITERATIONS || !E.points || !E.u)
        return hipErrorInvalidValue;
    // the orbit alone: the Sierpinski primitive continues it, every other id does not
    return primitive == uint32_t(PRIM_SIERPINSKI) ? foldorbit::launch_eval<PRIM_SIERPINSKI>(E, stream)
                                                  : foldorbit::launch_eval<PRIM_SPHERE>(E, stream);
}

}  // namespace kifs
