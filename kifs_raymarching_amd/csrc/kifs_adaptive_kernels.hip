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
// This file also holds the entry point's host side: the sanitizer build of the host units (make asan) links against a
// stand-in that knows no launcher of this file, so none of those units refers to one.
#include <cmath>

#include "kifs_context.hpp"
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

// Pass C's argument: the launch's frame constants and views as every render kernel takes them (frame.ssaa = k,
// frame.out / view[i].out = the destinations pass A wrote), and the queues pass B filled.
struct Params {
    BatchParams B;
    const uint32_t* queues;  // view i's entries at queues + i * capacity
    const uint32_t* counts;  // view i's number of entries
    uint32_t capacity;
};
static_assert(sizeof(Params) <= 4096, "the kernel argument is limited to 4 KB");

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

static hipError_t launch_classify(const float* planes, uint32_t stride_texels, int width, int height, int count,
                                  const KifsAdaptiveAA& aa, uint32_t* queues, uint32_t* counts, hipStream_t stream) {
    const dim3 grid(uint32_t(width + CLASSIFY_W - 1) / CLASSIFY_W, uint32_t(height + CLASSIFY_H - 1) / CLASSIFY_H, uint32_t(count));
    hipLaunchKernelGGL(classify_kernel, grid, dim3(CLASSIFY_W * CLASSIFY_H), 0, stream, reinterpret_cast<const Texel*>(planes),
                       stride_texels, width, height, aa.normal_cos, aa.depth_rel, queues, stride_texels, counts);
    return hipGetLastError();
}

static hipError_t launch_render(const Params& A, uint32_t group, uint32_t primitive, uint32_t groups_per_view, hipStream_t stream) {
    // Julia: the short divide / square root by sdf_iters.  The bunny: per-lane bunny_sdf -- slow, correct.
    return dispatch_pipeline<2>(group, primitive, uint32_t(A.B.frame.sdf_iters <= 24), [&](auto g, auto prim) {
        return launch<decltype(g)::value, decltype(prim)::value>(A, groups_per_view, stream);
    });
}

// ---- host side --------------------------------------------------------------------------------------------------
// Views per round of the three passes: what the kernel argument holds inline, and at most SCRATCH_CAP bytes of planes and
// queues (20 B per pixel per view; 1080p: 51 views).  A larger batch takes several rounds over the same scratch memory,
// which the stream keeps in order.
constexpr size_t SCRATCH_CAP = size_t(2) << 30;
constexpr size_t PLANE_BYTES = 16, QUEUE_BYTES = 4;
// Pass C's workgroups per CU, all views together: four waves each, so six fill the six waves per SIMD every
// instantiation is built for (measured against four per CU: DESIGN 5.9).
constexpr int GROUPS_PER_CU = 6;

// The device's CU count, asked once per device (two contexts on two threads may come through here at once: atomics).
static int cu_count(int device) {
    static std::atomic<int> known[64];
    if (device >= 0 && device < 64)
        if (const int n = known[device].load(std::memory_order_acquire); n > 0) return n;
    int cus = 0;
    if (!host::hip_ok(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device), "CU count") || cus < 1) return 0;
    if (device >= 0 && device < 64) known[device].store(cus, std::memory_order_release);
    return cus;
}

// The scratch block belongs to the context, not to a stream: a call on another stream than the previous call's waits for
// that call's last pass before it touches the block (as feedback_before does for the tile tables), and every call leaves
// the event behind its pass C.
static int order_after_previous_call(kifs_ctx* c, hipStream_t stream) {
    if (!c->adaptive_done) return KIFS_OK;  // the first call
    if (c->adaptive_stream != stream && !host::hip_ok(hipStreamWaitEvent(stream, c->adaptive_done, 0), "wait(adaptive scratch)"))
        return KIFS_ERR_RUNTIME;
    return KIFS_OK;
}
static int mark_call_end(kifs_ctx* c, hipStream_t stream) {
    if (!c->adaptive_done && !host::hip_ok(hipEventCreateWithFlags(&c->adaptive_done, hipEventDisableTiming), "hipEventCreate(adaptive)"))
        return KIFS_ERR_RUNTIME;
    if (!host::hip_ok(hipEventRecord(c->adaptive_done, stream), "record(adaptive scratch)")) return KIFS_ERR_RUNTIME;
    c->adaptive_stream = stream;
    return KIFS_OK;
}

static int check(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, size_t pitch,
                 const KifsAdaptiveAA* aa, int encode, int* w, int* h) {
    if (!c || !outs || !aa) return KIFS_ERR_BAD_ARG;
    if (!cameras && count != 1) return KIFS_ERR_BAD_ARG;  // NULL: the context's camera, one frame
    if (count < 1 || count > MAX_BATCH) return KIFS_ERR_BAD_ARG;
    if (aa->factor < 2 || aa->factor > KIFS_MAX_SUPERSAMPLING) return KIFS_ERR_BAD_ARG;
    if (std::isnan(aa->normal_cos) || std::isnan(aa->depth_rel) || aa->depth_rel < 0.0f) return KIFS_ERR_BAD_ARG;
    if (c->supersampling > 1) return KIFS_ERR_BAD_ARG;  // the mask is the primary ray's: one sample per pixel in pass A
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    if (const int st = host::frame_dims(c, w, h); st != KIFS_OK) return st;
    if (pitch < size_t(*w) * 4 || (pitch & 3u) != 0 || (pitch >> 2) > 0xffffffffull) return KIFS_ERR_BAD_ARG;
    if (int64_t(*w) * aa->factor > 65536 || int64_t(*h) * aa->factor > 65536) return KIFS_ERR_BAD_SIZE;
    return KIFS_OK;
}

// One round: `count` <= MAX_BATCH_INLINE views through the three passes.
static int enqueue_round(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras, uint8_t* const* outs,
                         size_t pitch, int w, int h, const KifsAdaptiveAA& aa, uint32_t* dev_edge_counts, int encode, int cus) {
    const size_t pixels = size_t(w) * size_t(h);
    float* const planes = reinterpret_cast<float*>(c->d_adaptive);
    uint32_t* const queues = reinterpret_cast<uint32_t*>(c->d_adaptive + size_t(count) * pixels * PLANE_BYTES);
    uint32_t* const counts = queues + size_t(count) * pixels;
    // A: the plain frame and its texels
    int st = host::enqueue_batch(c, stream, count, cameras, outs, pitch, 0, h, encode, nullptr, 0, 0, planes,
                                 size_t(w) * PLANE_BYTES, pixels * PLANE_BYTES);
    if (st != KIFS_OK) return st;
    // B: the edge pixels of every view, queued
    if (!host::hip_ok(hipMemsetAsync(counts, 0, size_t(count) * sizeof(uint32_t), stream), "memset(edge counts)") ||
        !host::hip_ok(launch_classify(planes, uint32_t(pixels), w, h, count, aa, queues, counts, stream), "classify_kernel launch"))
        return KIFS_ERR_RUNTIME;
    if (dev_edge_counts &&
        !host::hip_ok(hipMemcpyAsync(dev_edge_counts, counts, size_t(count) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream),
                      "copy(edge counts)"))
        return KIFS_ERR_RUNTIME;
    // C: their k x k resolves over pass A's pixels
    Params A;
    FrameParams& P = A.B.frame;
    if ((st = host::fill_params(c, &P)) != KIFS_OK) return st;
    A.B.count = count;
    A.B.table = nullptr;
    host::fill_views(c, P, A.B.view, count, cameras, outs);
    P.encode = encode;
    P.background_rgba = host::background_pixel(c, P.background_color, encode);
    P.pitch_words = uint32_t(pitch >> 2);
    P.out = reinterpret_cast<uint32_t*>(outs[0]);
    P.counters = nullptr;
    P.round_steps = 0;
    P.ssaa = aa.factor;
    P.ssaa_inv_height = 1.0f / (float(aa.factor) * c->screen.height);  // as fill_params computes a supersampled launch's
    A.queues = queues;
    A.counts = counts;
    A.capacity = uint32_t(pixels);
    const uint32_t groups_per_view = uint32_t(std::max(1, (cus * GROUPS_PER_CU + count - 1) / count));
    if (!host::hip_ok(launch_render(A, c->options.fractal_group_id, c->options.primitive_id, groups_per_view, stream),
                      "adaptive render_kernel launch"))
        return KIFS_ERR_RUNTIME;
    c->last_kernel = KIFS_KERNEL_ADAPTIVE;
    return KIFS_OK;
}

}  // namespace adaptive
}  // namespace kifs

extern "C" int kifs_render_adaptive_async(kifs_ctx* c, void* hip_stream, int count, const KifsCameraUniform* cameras,
                                          uint8_t* const* dev_outs, size_t pitch, const KifsAdaptiveAA* aa,
                                          uint32_t* dev_edge_counts, int encode) {
    using namespace kifs;
    int w = 0, h = 0;
    if (const int st = adaptive::check(c, count, cameras, dev_outs, pitch, aa, encode, &w, &h); st != KIFS_OK) return st;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const int cus = adaptive::cu_count(c->device);
    if (cus < 1) return KIFS_ERR_RUNTIME;
    // rounds of equal size, each within the inline views and the scratch cap
    const size_t per_view = size_t(w) * size_t(h) * (adaptive::PLANE_BYTES + adaptive::QUEUE_BYTES);
    const int fit = int(std::min<size_t>(size_t(MAX_BATCH_INLINE), std::max<size_t>(1, adaptive::SCRATCH_CAP / per_view)));
    const int rounds = (count + fit - 1) / fit;
    const int per_round = (count + rounds - 1) / rounds;
    const size_t need = size_t(per_round) * per_view + size_t(per_round) * sizeof(uint32_t);
    // (growing frees the old block, which waits for the launches that still use it)
    if (!host::grow(c->d_adaptive, c->adaptive_bytes, need, "hipMalloc(adaptive scratch)")) return KIFS_ERR_RUNTIME;
    if (const int st = adaptive::order_after_previous_call(c, s); st != KIFS_OK) return st;
    int st = KIFS_OK;
    for (int done = 0; done < count && st == KIFS_OK; done += per_round) {
        const int n = std::min(per_round, count - done);
        st = adaptive::enqueue_round(c, s, n, cameras ? cameras + done : nullptr, dev_outs + done, pitch, w, h, *aa,
                                     dev_edge_counts ? dev_edge_counts + done : nullptr, encode, cus);
    }
    // (also after a failed round: whatever it did enqueue uses the block)
    const int marked = adaptive::mark_call_end(c, s);
    return st != KIFS_OK ? st : marked;
}
