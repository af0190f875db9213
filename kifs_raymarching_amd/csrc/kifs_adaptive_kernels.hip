// kifs_adaptive_kernels.hip -- adaptive anti-aliasing (kifs_render_adaptive_async, include/kifs_hip.h): the frame is
// rendered once with its geometry, the pixels whose geometry differs from a 4-neighbour's are marked, and only those are
// supersampled k x k with the resolve of kifs_set_supersampling; every other pixel keeps the plain launch's bytes.
// Three passes on one stream, over scratch memory the context owns (planes | queues | counters):
//   A  the geometry launch (geom::render_kernel through host::enqueue_batch): the plain frame into the caller's
//      destination, the texels (n.x, n.y, n.z, t) into the scratch planes.
//   B  adaptive::classify_kernel       one thread per pixel: its texel and up to four neighbours' -> E(p); the edge
//                                      pixels (x | y << 16) are appended to the view's queue, one atomicAdd per wave.
//   C  adaptive::render_kernel<GROUP, PRIM>  sample rays drawn from the queue fill a wave's lanes: 64 / k^2 entries per
//                                      trip (16, 7 or 4), lane l = sample l % k^2 of entry l / k^2, whole rays on the virtual
//                                      k W x k H screen exactly as ssaa::render_kernel marches them; the samples' linear
//                                      colours meet in LDS, where the lane of sample 0 adds them in the contract's order,
//                                      encodes the mean and overwrites the pixel.  Workgroups stride over the queue; the
//                                      grid comes from the device's CU count, never from the frame or a counter read back.
// The entry point's host side is kifs_adaptive.cpp; it reaches passes B and C through the two launchers at the end of
// this file (kifs_internal.hpp).
#include "kifs_render_common.hpp"

namespace kifs {
namespace adaptive {

typedef float Texel __attribute__((ext_vector_type(4)));

constexpr int CLASSIFY_W = 64, CLASSIFY_H = 4;  // a wave takes 64 pixels of a row: 1 KB of texels per load
constexpr uint32_t MISS_T = 0x7f800000u;        // the miss texel's t: +inf

// The pair rule of the contract, f32 without fma (-ffp-contract=off): hit against miss, or two hits whose normals or
// depths are too far apart.
__device__ __forceinline__ bool pair(Texel p, Texel q, float normal_cos, float depth_rel) {
    const bool hp = __float_as_uint(p.w) != MISS_T, hq = __float_as_uint(q.w) != MISS_T;
    if (hp != hq) return true;
    if (!hp) return false;
    const float d = (p.x * q.x + p.y * q.y) + p.z * q.z;
    return !(d >= normal_cos) || __builtin_fabsf(p.w - q.w) > depth_rel * __builtin_fminf(p.w, q.w);
}

// Pass B.  Grid (ceil(W / 64), ceil(H / 4), views); planes of `stride` texels per view, rows of `width` texels.
__global__ __launch_bounds__(CLASSIFY_W* CLASSIFY_H) void classify_kernel(const Texel* __restrict__ planes, uint32_t stride,
                                                                         int width, int height, float normal_cos,
                                                                         float depth_rel, uint32_t* __restrict__ queues,
                                                                         uint32_t capacity, uint32_t* __restrict__ counts) {
    const int x = int(blockIdx.x) * CLASSIFY_W + int(threadIdx.x & 63u);
    const int y = int(blockIdx.y) * CLASSIFY_H + int(threadIdx.x >> 6);
    const uint32_t view = blockIdx.z;
    bool edge = false;
    if (x < width && y < height) {
        const Texel* const at = planes + size_t(view) * stride + size_t(y) * size_t(width) + size_t(x);
        const Texel p = at[0];
        if (x > 0) edge = edge || pair(p, at[-1], normal_cos, depth_rel);
        if (x + 1 < width) edge = edge || pair(p, at[1], normal_cos, depth_rel);
        if (y > 0) edge = edge || pair(p, at[-width], normal_cos, depth_rel);
        if (y + 1 < height) edge = edge || pair(p, at[width], normal_cos, depth_rel);
    }
    // the wave's edge pixels take consecutive slots: one atomicAdd for all of them, each lane's slot by prefix count
    const unsigned long long lanes = __ballot(edge);  // (every lane of the wave gets here)
    if (lanes == 0ull) return;
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(&counts[view], uint32_t(__popcll(lanes)));
    base = uint32_t(__builtin_amdgcn_readfirstlane(int(base)));
    const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi(uint32_t(lanes >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(lanes), 0u));
    if (edge && slot < capacity) queues[size_t(view) * capacity + slot] = uint32_t(x) | (uint32_t(y) << 16);
}

// Pass C.  Grid: a multiple of the views; workgroup b works on view b % count as group b / count of gridDim.x / count.
// (amdgpu_waves_per_eu: as ssaa::render_kernel)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const Params A) {
    __shared__ float s_srgb[256];
    __shared__ float s_sample[3][BLOCK];  // per lane: its sample's linear colour

    const LaunchSlot S = launch_slot(A.B);
    const FrameParams P = batch_frame(A.B, S.view);
    const int tid = threadIdx.x;
    const bool srgb = (P.encode == 1);
    if (srgb) s_srgb[tid] = P.srgb_table[tid];
    __syncthreads();  // s_srgb visible; the only barrier: from here on every wave goes its own way

    // The virtual screen, as ssaa::render_kernel builds it: height k H, same aspect float, its own 1 / height.
    const int k = P.ssaa;  // uniform, 2..KIFS_MAX_SUPERSAMPLING
    const int kk = k * k;
    FrameParams V = P;
    V.height = float(k) * P.height;  // exact: integers below 2^24
    V.inv_height = P.ssaa_inv_height;
    V.counters = nullptr;

    const uint32_t per_trip = 64u / uint32_t(kk);  // entries a wave takes at once: 16, 7 or 4
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(tid >> 6));
    const uint32_t waves = (gridDim.x / S.batch) * uint32_t(BLOCK / 64);  // of this view
    const uint32_t n = min(A.counts[S.view], A.capacity);
    const uint32_t* const queue = A.queues + size_t(S.view) * A.capacity;
    const uint32_t lane = uint32_t(tid) & 63u;
    const uint32_t e = lane / uint32_t(kk);                // the lane's entry of the trip
    const int s = int(lane - e * uint32_t(kk));            // and its sample, s = j k + i
    const int j = s / k, i = s - j * k;

    for (uint32_t first = (S.index * uint32_t(BLOCK / 64) + wave) * per_trip; first < n; first += waves * per_trip) {  // scalar
        const bool valid = e < per_trip && first + e < n;  // (the spare lanes of k = 3, the queue's ragged end)
        const uint32_t entry = valid ? queue[first + e] : 0u;
        const int x = int(entry & 0xffffu), y = int(entry >> 16);
        const int vx = k * x + i, vy = k * y + j;
        V3 c = P.background_color;  // a culled sample
        if (!wave_is_culled(V, vx, vy, valid)) {  // wave-uniform
            int steps = 0;
            const V3 dir = ray_direction(V, vx, vy);
            c = raymarch<GROUP, PRIM>(V, dir, valid, steps);
        }
        s_sample[0][tid] = c.x;
        s_sample[1][tid] = c.y;
        s_sample[2][tid] = c.z;
        // the samples of a pixel sit in one wave: LDS serves a wave's accesses in order, the fences keep the compiler to it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (valid && s == 0) {
            // The resolve of the contract, per channel in f32: acc = c(0,0), then acc + c(i,j) with j outer and i inner
            // (s ascending; no fma), mean = acc / k^2 correctly rounded.
            V3 acc = c;
            for (int o = 1; o < kk; ++o) {
                acc.x = acc.x + s_sample[0][tid + o];
                acc.y = acc.y + s_sample[1][tid + o];
                acc.z = acc.z + s_sample[2][tid + o];
            }
            const float d = float(kk);
            P.out[size_t(y) * P.pitch_words + uint32_t(x)] = encode_rgba(V3{acc.x / d, acc.y / d, acc.z / d}, srgb, s_srgb);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the sums are read before the next trip's colours land
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int GROUP, int PRIM>
static hipError_t launch(const Params& A, uint32_t groups_per_view, hipStream_t stream) {
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(groups_per_view * uint32_t(A.B.count)), dim3(BLOCK), 0, stream, A);
    return hipGetLastError();
}

}  // namespace adaptive

hipError_t launch_adaptive_classify(const float* planes, uint32_t stride_texels, int width, int height, int count,
                                    float normal_cos, float depth_rel, uint32_t* queues, uint32_t* counts, hipStream_t stream) {
    using namespace adaptive;
    const dim3 grid(uint32_t(width + CLASSIFY_W - 1) / CLASSIFY_W, uint32_t(height + CLASSIFY_H - 1) / CLASSIFY_H, uint32_t(count));
    hipLaunchKernelGGL(classify_kernel, grid, dim3(CLASSIFY_W * CLASSIFY_H), 0, stream, reinterpret_cast<const Texel*>(planes),
                       stride_texels, width, height, normal_cos, depth_rel, queues, stride_texels, counts);
    return hipGetLastError();
}

hipError_t launch_adaptive_render(const adaptive::Params& A, uint32_t group, uint32_t primitive, uint32_t groups_per_view,
                                  hipStream_t stream) {
    // Julia: the short divide / square root by sdf_iters.  The bunny: per-lane bunny_sdf -- slow, correct.
    return dispatch_pipeline<2>(group, primitive, uint32_t(A.B.frame.sdf_iters <= 24), [&](auto g, auto prim) {
        return adaptive::launch<decltype(g)::value, decltype(prim)::value>(A, groups_per_view, stream);
    });
}

}  // namespace kifs
