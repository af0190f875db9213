// kifs_adaptive.cpp -- the host side of adaptive anti-aliasing (kifs_render_adaptive_async, include/kifs_hip.h): the
// argument checks, the scratch block the context owns (planes | queues | counters), the split of a batch into rounds and
// the three passes of a round on one stream -- A the geometry launch (host::enqueue_batch), B and C the launchers of
// kifs_adaptive_kernels.hip -- and the event that hands the block from one stream to the next.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "kifs_context.hpp"

namespace kifs {
namespace adaptive {

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
    if (!host::hip_ok(hipEventRecord(c->adaptive_done, stream), "record(adaptive scratch)")) {
        // Nothing marks the end of this call's passes, and the event may never have been recorded at all (a wait for it
        // would be over at once): the passes are waited for here, and the next call starts as the first one does.
        (void)hipStreamSynchronize(stream);
        (void)hipEventDestroy(c->adaptive_done);
        c->adaptive_done = nullptr;
        c->adaptive_stream = nullptr;
        return KIFS_ERR_RUNTIME;
    }
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
        !host::hip_ok(launch_adaptive_classify(planes, uint32_t(pixels), w, h, count, aa.normal_cos, aa.depth_rel, queues, counts, stream), "classify_kernel launch"))
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
    if (!host::hip_ok(launch_adaptive_render(A, c->options.fractal_group_id, c->options.primitive_id, groups_per_view, stream),
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
