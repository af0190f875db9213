// host_driver.cpp -- TEST INFRASTRUCTURE: drives the C ABI of include/kifs_hip.h against tests/hip_stub/hip_stub.cpp
// under AddressSanitizer + UndefinedBehaviorSanitizer (make -C kifs_raymarching_amd/csrc asan; tests/
// test_host_sanitizers.py).  The scenarios are the ones tests/test_gpu_multi_batch.py, test_gpu_shards.py and
// test_gpu_api.py run on the GPU -- here what is checked is the HOST side: every frame gathered from four "devices"
// must equal the frame one context renders (the stub's pixels depend on camera and frame coordinates only), one
// long-lived context must keep rendering exact frames across evictions, feedback transitions, resizes and diagnostics
// (context_lifecycle), every launch-shape rule must pick what it picked when the table was written (launch_shapes),
// nothing may touch memory it does not own, every failure that is injected must leave the object usable, and after the last
// destroy the stub must hold no allocation, stream or event.  The adaptive and the animated entry points
// (kifs_adaptive.cpp, kifs_animation.cpp; tests/test_gpu_adaptive.py, test_gpu_animation.py) come last, so that the
// call trace of everything before them stays what it was: their frames are compared with the stand-in's patterns as
// this file restates them (namespace model).  Prints "host_driver: N checks ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/kifs_hip.h"

struct StubRenderLaunch {  // hip_stub.cpp: what the latest render launch was told
    int count;
    unsigned tile_count;
    int round_steps, group_tiles, bunny_coop, workgroups_per_cu;
    int tile_cost, counters, geom, stripe_rows, table;
    int ssaa, encode, y0, y1;
    int cull, quick_cull, tile_cull;
    int order;
    int orbit_x2;
};

extern "C" {
void stub_last_render(StubRenderLaunch* out);
void stub_fail_in(long n);
void stub_trace_mark(const char* what);
long stub_launches();
long stub_calls();
long stub_device_synchronizes();
size_t stub_live_device_allocations();
size_t stub_live_streams_and_events();
long stub_stream_waits();
long stub_event_synchronizes();
long stub_device_frees();
int stub_events_created();
long stub_stream_waits_on(int event_ordinal);
long stub_event_synchronizes_on(int event_ordinal);
int stub_has_device_allocation_of(size_t bytes);
int stub_adaptive_rounds(int* out, int max);
}

static long g_checks = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            std::fprintf(stderr, "host_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                  \
        }                                                                                  \
    } while (0)

namespace {

struct Scene {
    KifsScreenUniform screen;
    KifsOptionsUniform options;
    int w, h;
};

Scene scene(int w, int h, uint8_t bg = 0) {
    Scene s{};
    s.w = w;
    s.h = h;
    CHECK(kifs_host_screen(uint32_t(w), uint32_t(h), &s.screen) == KIFS_OK);
    KifsGuiData gui;
    kifs_host_gui_default(&gui);
    gui.fractal_group = 1;  // Julia
    gui.background_color[0] = bg;
    gui.background_color[1] = uint8_t(bg / 2);
    CHECK(kifs_host_options(&gui, &s.options) == KIFS_OK);
    return s;
}

std::vector<KifsCameraUniform> cameras(int n, int first) {
    std::vector<KifsCameraUniform> out(static_cast<size_t>(n), KifsCameraUniform{});
    for (int i = 0; i < n; ++i) {
        KifsCameraData c;
        kifs_host_camera_default(&c);
        c.origin_distance = 3.0f + 0.25f * float((first + i) % 7);
        c.phi = 0.37f * float(first + i);
        c.theta = 0.2f * float((first + i) % 5) - 0.4f;
        CHECK(kifs_host_camera(&c, &out[size_t(i)]) == KIFS_OK);
    }
    return out;
}

uint8_t* dev_alloc(size_t bytes) {
    void* p = nullptr;
    CHECK(hipMalloc(&p, bytes) == hipSuccess);
    return static_cast<uint8_t*>(p);
}

// The frames one context renders, one kifs_render each, into host memory.
std::vector<uint8_t> single_frames(const Scene& s, const std::vector<KifsCameraUniform>& cams, int encode = 1) {
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK && kifs_set_options(c, &s.options) == KIFS_OK);
    const size_t fb = size_t(s.w) * s.h * 4;
    std::vector<uint8_t> out(fb * cams.size());
    for (size_t i = 0; i < cams.size(); ++i) {
        CHECK(kifs_set_camera(c, &cams[i]) == KIFS_OK);
        CHECK(kifs_render(c, out.data() + i * fb, size_t(s.w) * 4, 0, s.h, encode) == KIFS_OK);
    }
    kifs_destroy(c);
    return out;
}

bool equal_dev(const uint8_t* dev, const std::vector<uint8_t>& want) { return std::memcmp(dev, want.data(), want.size()) == 0; }

kifs_multi* multi(const std::vector<int>& devs, const Scene& s, int gather, int transport = KIFS_TRANSPORT_COPY) {
    int st = 0;
    kifs_multi* m = kifs_multi_create(devs.data(), int(devs.size()), &st);
    CHECK(m && st == KIFS_OK);
    CHECK(kifs_multi_set_screen(m, &s.screen) == KIFS_OK && kifs_multi_set_options(m, &s.options) == KIFS_OK);
    auto cam = cameras(1, 0);
    CHECK(kifs_multi_set_camera(m, &cam[0]) == KIFS_OK);
    CHECK(kifs_multi_set_gather(m, gather, transport) == KIFS_OK);
    return m;
}

// ---- scenarios -----------------------------------------------------------------------------------------------

void null_and_argument_checks() {
    stub_trace_mark("null_and_argument_checks");
    CHECK(kifs_abi_version() == KIFS_ABI_VERSION);
    CHECK(kifs_set_screen(nullptr, nullptr) == KIFS_ERR_BAD_ARG && kifs_render(nullptr, nullptr, 0, 0, 0, 0) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_order_after(nullptr, nullptr, nullptr) == KIFS_ERR_BAD_ARG && kifs_multi_order_after(nullptr, nullptr) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_multi_wait_all(nullptr) == KIFS_ERR_BAD_ARG && kifs_multi_stats(nullptr, nullptr, 0) == KIFS_ERR_BAD_ARG);
    int st = 0;
    CHECK(kifs_create(99, &st) == nullptr && st == KIFS_ERR_NO_DEVICE);
    CHECK(kifs_multi_create(nullptr, 2, &st) == nullptr && st == KIFS_ERR_BAD_ARG);
    int bad[2] = {0, 77};
    CHECK(kifs_multi_create(bad, 2, &st) == nullptr && st == KIFS_ERR_NO_DEVICE);
    kifs_destroy(nullptr);
    kifs_multi_destroy(nullptr);
    kifs_ctx* c = kifs_create(1, &st);
    CHECK(c && st == KIFS_OK);
    uint8_t px[64];
    CHECK(kifs_render(c, px, 16, 0, 1, 1) == KIFS_ERR_UNCONFIGURED);
    Scene s = scene(4, 4);
    KifsScreenUniform zero = s.screen;
    zero.width = 0.0f;
    CHECK(kifs_set_screen(c, &zero) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK && kifs_set_options(c, &s.options) == KIFS_OK);
    KifsOptionsUniform o = s.options;
    o.fractal_group_id = 9;
    CHECK(kifs_set_options(c, &o) == KIFS_ERR_BAD_ARG && kifs_set_iters(c, -1, 0, 0) == KIFS_ERR_BAD_ARG);
    auto cam = cameras(1, 0);
    CHECK(kifs_set_camera(c, &cam[0]) == KIFS_OK);
    CHECK(kifs_render(c, px, 16, 0, 4, 1) == KIFS_OK && kifs_render(c, px, 16, 0, 5, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_render(c, px, 12, 0, 4, 1) == KIFS_ERR_BAD_SIZE && kifs_render(c, px, 16, 0, 4, 2) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_render(c, px, 16, 2, 2, 1) == KIFS_OK);
    CHECK(kifs_order_after(c, nullptr, nullptr) == KIFS_OK);
    int y0, y1, n, rows;
    CHECK(kifs_band_range(1080, 3, 8, &y0, &y1) == KIFS_OK && y0 == 405 && y1 == 540);
    CHECK(kifs_band_range(10, 8, 8, &y0, &y1) == KIFS_ERR_BAD_ARG);
    int stripes[200];
    int wts[3] = {3, 1, 1};
    CHECK(kifs_shard_stripes(1080, 3, wts, 0, stripes, 200, &n, &rows) == KIFS_OK && n == 81 && rows == 648);
    CHECK(kifs_shard_stripes(1080, 3, wts, 0, stripes, 10, &n, &rows) == KIFS_ERR_BAD_ARG);
    // the tile-order sort on chosen costs: scratch buffers only, freed on every path
    uint32_t cost[5] = {0, 900, 0, 7, 900}, order[5], after[5];
    CHECK(kifs_debug_sort_tiles(c, cost, 5, 2, 0, order, after) == KIFS_OK);
    CHECK(order[0] == (1u | 0u << 16) && order[1] == (0u | 2u << 16) && order[2] == (1u | 1u << 16) && after[1] == 0 && after[4] == 0);
    CHECK(kifs_debug_sort_tiles(c, cost, 0, 2, 0, order, after) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_debug_sort_tiles(c, cost, 5, 0, 0, order, after) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_debug_sort_tiles(c, cost, 5, 65537, 0, order, after) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_debug_sort_tiles(c, cost, 5, 2, 32, order, after) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_debug_sort_tiles(c, nullptr, 5, 2, 0, order, after) == KIFS_ERR_BAD_ARG);
    // more shards than a launch grid has rows: refused before anything is looked at
    int one = 0;
    CHECK(kifs_unpack_shard_async(c, nullptr, KIFS_MAX_SHARD_COUNT + 1, px, 16, 64, px, 16, 64, &one, 1) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_fill_shard_async(c, nullptr, KIFS_MAX_SHARD_COUNT + 1, px, 16, 64, &one, 1, 1) == KIFS_ERR_BAD_SIZE);
    kifs_destroy(c);
}

// One context: bands, batches (inline and through the view table), shards packed and in place, the sparse round trip.
void single_context(int w, int h) {
    stub_trace_mark("single_context");
    Scene s = scene(w, h, 40);
    const size_t fb = size_t(w) * h * 4;
    auto cams = cameras(70, 3);
    auto want = single_frames(s, cams);
    int st = 0;
    kifs_ctx* c = kifs_create(2, &st);
    CHECK(c != nullptr);
    CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK && kifs_set_options(c, &s.options) == KIFS_OK && kifs_set_camera(c, &cams[0]) == KIFS_OK);
    CHECK(kifs_set_profiling(c, 1) == KIFS_OK);
    // a frame in three bands with a padded pitch, into device memory
    const size_t pitch = size_t(w) * 4 + 32;
    uint8_t* d = dev_alloc(pitch * h);
    const int cuts[4] = {0, h / 3, h / 3 + 5 < h ? h / 3 + 5 : h, h};
    for (int b = 0; b < 3; ++b)
        CHECK(kifs_render_async(c, nullptr, d + size_t(cuts[b]) * pitch, pitch, cuts[b], cuts[b + 1], 1) == KIFS_OK);
    CHECK(kifs_synchronize(c) == KIFS_OK);
    for (int y = 0; y < h; ++y) CHECK(std::memcmp(d + y * pitch, want.data() + size_t(y) * w * 4, size_t(w) * 4) == 0);
    CHECK(hipFree(d) == hipSuccess);
    // batches of 5 and of 70 (beyond the kernel argument: the device view table, four times round its ring)
    uint8_t* frames = dev_alloc(fb * 70);
    std::vector<uint8_t*> outs(70);
    for (int i = 0; i < 70; ++i) outs[size_t(i)] = frames + fb * i;
    CHECK(kifs_render_batch_async(c, nullptr, 5, cams.data(), outs.data(), size_t(w) * 4, 0, h, 1) == KIFS_OK);
    CHECK(std::memcmp(frames, want.data(), fb * 5) == 0);
    {   // a big batch that is rejected takes no slot of the view ring (none exists yet: taking one would allocate it)
        const long calls = stub_calls();
        CHECK(kifs_render_batch_async(c, nullptr, 70, cams.data(), outs.data(), size_t(w) * 4, 0, h + 1, 1) == KIFS_ERR_BAD_ARG);
        CHECK(kifs_render_batch_async(c, nullptr, 70, cams.data(), outs.data(), size_t(w) * 4 - 4, 0, h, 1) == KIFS_ERR_BAD_SIZE);
        CHECK(stub_calls() == calls);
    }
    for (int round = 0; round < 6; ++round) {
        std::memset(frames, 0xEE, fb * 70);
        CHECK(kifs_render_batch_async(c, nullptr, 70, cams.data(), outs.data(), size_t(w) * 4, 0, h, 1) == KIFS_OK);
        CHECK(equal_dev(frames, want));
    }
    CHECK(kifs_render_batch_async(c, nullptr, 0, cams.data(), outs.data(), size_t(w) * 4, 0, h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_render_batch_async(c, nullptr, 513, cams.data(), outs.data(), size_t(w) * 4, 0, h, 1) == KIFS_ERR_BAD_ARG);
    int launches = 0;
    double mean = 0, lo = 0, hi = 0;
    CHECK(kifs_profile_read(c, &launches, &mean, &lo, &hi) == KIFS_OK && launches >= 7);
    // three ranks' shards of 6 frames: packed + unpack, in place, and the sparse form; every partition's union = the frames
    const int B = 6, world = 3;
    const int all = (h + 7) / 8;
    uint8_t* gathered = dev_alloc(fb * B);
    for (int mode = 0; mode < 3; ++mode) {  // 0 dense packed, 1 in place, 2 sparse
        std::memset(gathered, 0x11, fb * B);
        std::vector<int> peer_stripes;
        for (int r = 0; r < world; ++r) {
            std::vector<int> st_(static_cast<size_t>(all), 0);
            int n = 0, rows = 0;
            CHECK(kifs_shard_stripes(h, world, nullptr, r, st_.data(), all, &n, &rows) == KIFS_OK);
            st_.resize(size_t(n));
            if (n == 0) continue;
            if (mode == 1) {
                std::vector<uint8_t*> fo(B);
                for (int i = 0; i < B; ++i) fo[size_t(i)] = gathered + fb * i;
                CHECK(kifs_render_shard_async(c, nullptr, B, cams.data(), fo.data(), size_t(w) * 4, st_.data(), n, 1, 1) == KIFS_OK);
                continue;
            }
            const size_t sb = size_t(rows) * w * 4;
            uint8_t* shard = dev_alloc(sb * B);
            std::vector<uint8_t*> so(B);
            for (int i = 0; i < B; ++i) so[size_t(i)] = shard + sb * i;
            CHECK(kifs_render_shard_async(c, nullptr, B, cams.data(), so.data(), size_t(w) * 4, st_.data(), n, 0, 1) == KIFS_OK);
            if (mode == 0) {
                CHECK(kifs_unpack_shard_async(c, nullptr, B, gathered, size_t(w) * 4, fb, shard, size_t(w) * 4, sb, st_.data(), n) == KIFS_OK);
            } else {
                const size_t cap = size_t(B) * n * ((w + 31) / 32);
                uint8_t* rec = dev_alloc(cap * KIFS_SPARSE_RECORD_BYTES);
                uint32_t* cnt = reinterpret_cast<uint32_t*>(dev_alloc(4));
                void* pinned = nullptr;
                CHECK(hipHostMalloc(&pinned, 4, 0) == hipSuccess);
                CHECK(kifs_pack_sparse_async(c, nullptr, B, shard, size_t(w) * 4, sb, st_.data(), n, 1, rec, cap, cnt,
                                             static_cast<uint32_t*>(pinned)) == KIFS_OK);
                const uint32_t nrec = *static_cast<uint32_t*>(pinned);
                CHECK(nrec == *cnt && nrec <= cap && nrec > 0 && nrec < cap);  // (some tiles hold something, some do not)
                CHECK(kifs_pack_sparse_async(c, nullptr, B, shard, size_t(w) * 4, sb, st_.data(), n, 1, rec, cap - 1, cnt, nullptr) == KIFS_ERR_BAD_SIZE);
                CHECK(kifs_fill_shard_async(c, nullptr, B, gathered, size_t(w) * 4, fb, st_.data(), n, 1) == KIFS_OK);
                CHECK(kifs_unpack_sparse_async(c, nullptr, B, gathered, size_t(w) * 4, fb, rec, nrec, st_.data(), n) == KIFS_OK);
                // erase + scatter again: the same frames
                CHECK(kifs_erase_sparse_async(c, nullptr, B, gathered, size_t(w) * 4, fb, rec, nrec, st_.data(), n, 1) == KIFS_OK);
                CHECK(kifs_unpack_sparse_async(c, nullptr, B, gathered, size_t(w) * 4, fb, rec, nrec, st_.data(), n) == KIFS_OK);
                CHECK(hipFree(rec) == hipSuccess && hipFree(cnt) == hipSuccess && hipHostFree(pinned) == hipSuccess);
            }
            CHECK(hipFree(shard) == hipSuccess);
        }
        CHECK(std::memcmp(gathered, want.data(), fb * B) == 0);
    }
    // stripe lists the library must refuse
    {
        int desc[2] = {1, 0}, beyond[1] = {all}, neg[1] = {-1};
        uint8_t* o1[1] = {gathered};
        CHECK(kifs_render_shard_async(c, nullptr, 1, cams.data(), o1, size_t(w) * 4, desc, 2, 1, 1) == KIFS_ERR_BAD_ARG);
        CHECK(kifs_render_shard_async(c, nullptr, 1, cams.data(), o1, size_t(w) * 4, beyond, 1, 1, 1) == KIFS_ERR_BAD_ARG);
        CHECK(kifs_render_shard_async(c, nullptr, 1, cams.data(), o1, size_t(w) * 4, neg, 1, 1, 1) == KIFS_ERR_BAD_ARG);
    }
    CHECK(hipFree(gathered) == hipSuccess && hipFree(frames) == hipSuccess);
    kifs_destroy(c);
}

// kifs_multi: batches on four devices, both gathers, against single frames; the lone-frame form; weights.
void multi_batches(int w, int h, int gather) {
    stub_trace_mark("multi_batches");
    Scene s = scene(w, h, 90);
    const size_t fb = size_t(w) * h * 4;
    const int B = 9;
    auto cams = cameras(B, 11);
    auto want = single_frames(s, cams);
    kifs_multi* m = multi({0, 1, 2, 3}, s, gather);
    uint8_t* frames = dev_alloc(fb * B);
    std::memset(frames, 0x5A, fb * B);
    CHECK(kifs_multi_render_batch(m, B, cams.data(), frames, size_t(w) * 4, fb, 1) == KIFS_OK);
    CHECK(equal_dev(frames, want));
    KifsMultiStats st{};
    CHECK(kifs_multi_stats(m, &st, 0) == KIFS_OK && st.steps == 1 && st.transport == KIFS_TRANSPORT_COPY && st.gather == gather);
    CHECK(st.bytes_received > 0);
    if (gather == KIFS_GATHER_SPARSE) CHECK(st.records_received > 0 && st.records_received < st.tiles_covered);
    // the lone-frame form: device destination, host destination
    CHECK(kifs_multi_set_camera(m, &cams[4]) == KIFS_OK);
    std::memset(frames, 0, fb);
    CHECK(kifs_multi_render(m, frames, size_t(w) * 4, 1) == KIFS_OK);
    CHECK(std::memcmp(frames, want.data() + 4 * fb, fb) == 0);
    std::vector<uint8_t> host(fb);
    CHECK(kifs_multi_render(m, host.data(), size_t(w) * 4, 1) == KIFS_OK);
    CHECK(std::memcmp(host.data(), want.data() + 4 * fb, fb) == 0);
    for (int i = 0; i < 4; ++i) CHECK(kifs_multi_shard_ms(m, i) >= 0.0);
    // other shares, a device with no share at all
    int wts[4] = {2, 0, 5, 1};
    CHECK(kifs_multi_set_weights(m, wts) == KIFS_OK);
    int dev = 0, n = 0, rows = 0, total = 0;
    for (int i = 0; i < 4; ++i) {
        CHECK(kifs_multi_shard(m, i, &dev, &n, &rows) == KIFS_OK && dev == i);
        total += rows;
        if (i == 1) CHECK(n == 0 && rows == 0);
    }
    CHECK(total == h);
    std::memset(frames, 0xA5, fb * B);
    uint64_t step = 0;
    CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &step) == KIFS_OK);
    CHECK(kifs_multi_order_after(m, nullptr) == KIFS_OK);
    CHECK(kifs_multi_wait(m, step) == KIFS_OK && equal_dev(frames, want));
    int zero[4] = {0, 0, 0, 0}, neg[4] = {1, -1, 1, 1};
    CHECK(kifs_multi_set_weights(m, zero) == KIFS_ERR_BAD_ARG && kifs_multi_set_weights(m, neg) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_multi_set_weights(m, nullptr) == KIFS_OK);
    // the root alone, and a root with no share
    int root_only[4] = {1, 0, 0, 0}, no_root[4] = {0, 1, 1, 1};
    for (int* wt : {root_only, no_root}) {
        CHECK(kifs_multi_set_weights(m, wt) == KIFS_OK);
        std::memset(frames, 0x3C, fb * B);
        CHECK(kifs_multi_render_batch(m, B, cams.data(), frames, size_t(w) * 4, fb, 1) == KIFS_OK && equal_dev(frames, want));
    }
    // argument checks of the batched form
    CHECK(kifs_multi_render_batch_async(m, 0, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &step) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4 - 4, fb, 1, 0, &step) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb - 4, 1, 0, &step) == KIFS_ERR_BAD_SIZE);
    CHECK(kifs_multi_render_batch_async(m, B, cams.data(), host.data(), size_t(w) * 4, fb, 1, 0, &step) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_multi_wait(m, 1000) == KIFS_ERR_BAD_ARG && kifs_multi_stream_wait(m, 0, nullptr) == KIFS_ERR_BAD_ARG);
    CHECK(hipFree(frames) == hipSuccess);
    kifs_multi_destroy(m);
}

// Pipelined steps: two buffers handed back untouched; ONE buffer for every step; a lone render in between; overlapping
// buffers; a change of options / partition / gather under the untouched flag; destroy with steps in flight.
void multi_pipeline(int w, int h) {
    stub_trace_mark("multi_pipeline");
    Scene s = scene(w, h, 0);
    const size_t fb = size_t(w) * h * 4;
    const int B = 5;
    kifs_multi* m = multi({0, 1, 2}, s, KIFS_GATHER_SPARSE);
    uint8_t* buf[2] = {dev_alloc(fb * B), dev_alloc(fb * B)};
    uint64_t steps[9];
    std::vector<std::vector<uint8_t>> wants;
    for (int k = 0; k < 9; ++k) wants.push_back(single_frames(s, cameras(B, 10 * k)));
    for (int k = 0; k < 9; ++k) {
        if (k >= 2) {
            CHECK(kifs_multi_wait(m, steps[k - 2]) == KIFS_OK);
            CHECK(equal_dev(buf[k % 2], wants[size_t(k - 2)]));
        }
        auto cams = cameras(B, 10 * k);
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[k % 2], size_t(w) * 4, fb, 1, k >= 2 ? KIFS_MULTI_FRAMES_UNTOUCHED : 0,
                                            &steps[k]) == KIFS_OK && steps[k] == uint64_t(k));
    }
    CHECK(kifs_multi_wait_all(m) == KIFS_OK && equal_dev(buf[1], wants[7]) && equal_dev(buf[0], wants[8]));
    KifsMultiStats st{};
    CHECK(kifs_multi_stats(m, &st, 1) == KIFS_OK && st.steps == 9);
    // the flag with the other encoding: black is the same pixel both ways and everything else matches the slot's record,
    // but "anything differs" means a fill -- it repairs rows that (against the flag's promise) do not hold the background
    {
        auto cams = cameras(B, 77);
        uint64_t sn = 0;
        std::memset(buf[1], 0x11, fb * B);
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[1], size_t(w) * 4, fb, 0, KIFS_MULTI_FRAMES_UNTOUCHED, &sn) == KIFS_OK);
        CHECK(kifs_multi_wait(m, sn) == KIFS_OK && equal_dev(buf[1], single_frames(s, cams, 0)));
    }
    // ONE buffer for every step, the flag always set: step k - 1's tiles must not survive under step k's background
    for (int k = 0; k < 6; ++k) {
        auto cams = cameras(B, 100 + 13 * k);
        uint64_t sn = 0;
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[0], size_t(w) * 4, fb, 1, KIFS_MULTI_FRAMES_UNTOUCHED, &sn) == KIFS_OK);
        CHECK(kifs_multi_wait(m, sn) == KIFS_OK && equal_dev(buf[0], single_frames(s, cams)));
        if (k == 3) {  // a lone frame into the middle of the buffer between two steps
            auto lone = cameras(1, 999);
            CHECK(kifs_multi_set_camera(m, &lone[0]) == KIFS_OK && kifs_multi_render(m, buf[0] + 2 * fb, size_t(w) * 4, 1) == KIFS_OK);
        }
    }
    // overlapping buffers: frames 0..3 and 1..4 of one allocation, alternating
    for (int k = 0; k < 4; ++k) {
        auto cams = cameras(B - 1, 300 + 7 * k);
        uint8_t* view = buf[1] + (k % 2) * fb;
        uint64_t sn = 0;
        CHECK(kifs_multi_render_batch_async(m, B - 1, cams.data(), view, size_t(w) * 4, fb, 1, KIFS_MULTI_FRAMES_UNTOUCHED, &sn) == KIFS_OK);
        CHECK(kifs_multi_wait(m, sn) == KIFS_OK && equal_dev(view, single_frames(s, cams)));
    }
    // another background colour, another partition, the dense gather and back -- the flag stays set throughout
    Scene red = scene(w, h, 200);
    auto cams = cameras(B, 5);
    CHECK(kifs_multi_set_options(m, &red.options) == KIFS_OK);
    for (int k = 0; k < 3; ++k) {
        uint64_t sn = 0;
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[k % 2], size_t(w) * 4, fb, 1, KIFS_MULTI_FRAMES_UNTOUCHED, &sn) == KIFS_OK);
    }
    CHECK(kifs_multi_wait_all(m) == KIFS_OK);
    auto want_red = single_frames(red, cams);
    CHECK(equal_dev(buf[0], want_red) && equal_dev(buf[1], want_red));
    int wts[3] = {1, 3, 2};
    CHECK(kifs_multi_set_weights(m, wts) == KIFS_OK);
    for (int k = 0; k < 2; ++k) {
        uint64_t sn = 0;
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[k], size_t(w) * 4, fb, 1, KIFS_MULTI_FRAMES_UNTOUCHED, &sn) == KIFS_OK);
    }
    CHECK(kifs_multi_set_gather(m, KIFS_GATHER_DENSE, KIFS_TRANSPORT_COPY) == KIFS_OK);  // (drains the two steps)
    CHECK(equal_dev(buf[0], want_red) && equal_dev(buf[1], want_red));
    for (int k = 0; k < 3; ++k) {
        uint64_t sn = 0;
        std::memset(buf[k % 2], 0x77, fb * B);
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[k % 2], size_t(w) * 4, fb, 1, KIFS_MULTI_FRAMES_UNTOUCHED, &sn) == KIFS_OK);
        CHECK(kifs_multi_wait(m, sn) == KIFS_OK && equal_dev(buf[k % 2], want_red));
    }
    CHECK(kifs_multi_set_gather(m, KIFS_GATHER_SPARSE, KIFS_TRANSPORT_AUTO) == KIFS_OK);
    CHECK(kifs_multi_set_gather(m, 7, 0) == KIFS_ERR_BAD_ARG && kifs_multi_set_gather(m, 0, 7) == KIFS_ERR_BAD_ARG);
    // a device listed twice cannot have RCCL: explicit RCCL is an error there, AUTO means peer copies
    {
        int st_ = 0;
        int twice[3] = {0, 1, 1};
        kifs_multi* m2 = kifs_multi_create(twice, 3, &st_);
        CHECK(m2 != nullptr);
        CHECK(kifs_multi_set_screen(m2, &s.screen) == KIFS_OK && kifs_multi_set_options(m2, &s.options) == KIFS_OK);
        CHECK(kifs_multi_set_gather(m2, KIFS_GATHER_SPARSE, KIFS_TRANSPORT_RCCL) == KIFS_ERR_COMM);
        CHECK(kifs_multi_set_gather(m2, KIFS_GATHER_SPARSE, KIFS_TRANSPORT_AUTO) == KIFS_OK);
        auto c2 = cameras(B, 40);
        CHECK(kifs_multi_render_batch(m2, B, c2.data(), buf[0], size_t(w) * 4, fb, 1) == KIFS_OK && equal_dev(buf[0], single_frames(s, c2)));
        CHECK(kifs_multi_stats(m2, &st, 0) == KIFS_OK && st.transport == KIFS_TRANSPORT_COPY);
        kifs_multi_destroy(m2);
    }
    // destroy with two steps in flight
    CHECK(kifs_multi_set_gather(m, KIFS_GATHER_SPARSE, KIFS_TRANSPORT_COPY) == KIFS_OK);
    for (int k = 0; k < 2; ++k) {
        uint64_t sn = 0;
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), buf[k], size_t(w) * 4, fb, 1, 0, &sn) == KIFS_OK);
    }
    kifs_multi_destroy(m);
    CHECK(equal_dev(buf[0], want_red) && equal_dev(buf[1], want_red));  // (destroy completes what is in flight)
    CHECK(hipFree(buf[0]) == hipSuccess && hipFree(buf[1]) == hipSuccess);
}

// Every HIP call and launch of a submit / wait cycle -- and of a lone frame, an explicit transport, the self-test --
// fails once, in turn: the call reports an error (or absorbs it), the object stays usable, the next steps are exact,
// and nothing leaks.
void injected_failures(int w, int h) {
    stub_trace_mark("injected_failures");
    Scene s = scene(w, h, 10);
    const size_t fb = size_t(w) * h * 4;
    const int B = 4;
    auto cams = cameras(B, 21);
    auto want = single_frames(s, cams);
    uint8_t* frames = dev_alloc(fb * B * 2);  // (the second half: a second step's frames, or a lone frame)
    int failed_calls = 0;
    for (int gather : {KIFS_GATHER_SPARSE, KIFS_GATHER_DENSE}) {
        for (long n = 1; n < 400; ++n) {
            kifs_multi* m = multi({0, 1, 2}, s, gather);
            uint64_t s0 = 0, s1 = 0;
            // a clean first step, so that the failure lands in a steady-state submit (buffers exist) for small n as well
            CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &s0) == KIFS_OK);
            const long before = stub_calls();
            stub_fail_in(n);
            int st = kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &s1);
            int sw = st == KIFS_OK ? kifs_multi_wait(m, s1) : KIFS_OK;
            const bool reached = stub_calls() - before >= n;
            stub_fail_in(-1);
            if (st != KIFS_OK || sw != KIFS_OK) ++failed_calls;
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME || st == KIFS_ERR_COMM);
            CHECK(sw == KIFS_OK || sw == KIFS_ERR_RUNTIME || sw == KIFS_ERR_COMM);
            // whatever happened: the object renders exact frames afterwards (a failed wait may need a second one to drain)
            (void)kifs_multi_wait_all(m);
            std::memset(frames, 0x42, fb * B);
            uint64_t s2 = 0;
            CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &s2) == KIFS_OK);
            CHECK(kifs_multi_wait(m, s2) == KIFS_OK && equal_dev(frames, want));
            kifs_multi_destroy(m);
            if (!reached) break;  // the cycle has fewer than n calls: every one has had its turn
        }
    }
    CHECK(failed_calls > 10);
    // the same for the other calls that enqueue or allocate: a lone frame (device and host destination), an explicit
    // transport on a fresh object, the transport self-test -- each with a batched step in flight where one can be
    std::vector<uint8_t> host(fb);
    const auto lone_want = single_frames(s, cameras(1, 0));  // (the camera multi() sets)
    for (int call = 0; call < 4; ++call) {
        failed_calls = 0;
        for (long n = 1; n < 400; ++n) {
            kifs_multi* m = nullptr;
            uint64_t s0 = 0;
            if (call == 2) {
                int st0 = 0;
                const int devs[3] = {0, 1, 2};
                m = kifs_multi_create(devs, 3, &st0);
                CHECK(m && kifs_multi_set_screen(m, &s.screen) == KIFS_OK && kifs_multi_set_options(m, &s.options) == KIFS_OK);
            } else {
                m = multi({0, 1, 2}, s, KIFS_GATHER_SPARSE);
                CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &s0) == KIFS_OK);
            }
            uint8_t* lone_dst = call == 0 ? frames + fb * B : host.data();
            const long before = stub_calls();
            stub_fail_in(n);
            const int st = call <= 1   ? kifs_multi_render(m, lone_dst, size_t(w) * 4, 1)
                           : call == 2 ? kifs_multi_set_gather(m, KIFS_GATHER_SPARSE, KIFS_TRANSPORT_COPY)
                                       : kifs_multi_comm_selftest(m, 4096);
            const bool reached = stub_calls() - before >= n;
            stub_fail_in(-1);
            if (st != KIFS_OK) ++failed_calls;
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME || st == KIFS_ERR_COMM);
            if (call <= 1 && st == KIFS_OK) CHECK(std::memcmp(lone_dst, lone_want.data(), fb) == 0);
            (void)kifs_multi_wait_all(m);
            std::memset(frames, 0x42, fb * B);
            uint64_t s2 = 0;
            CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &s2) == KIFS_OK);
            CHECK(kifs_multi_wait(m, s2) == KIFS_OK && equal_dev(frames, want));
            kifs_multi_destroy(m);
            if (!reached) break;
        }
        CHECK(failed_calls > 2);
    }
    // A flush that fails inside a submit leaves the older step unflushed beside the new one: kifs_multi_stream_wait for
    // the newer step posts the older one first (the gather stream runs them in order), so the wait for the older one
    // that follows has nothing left to launch.
    hipStream_t consumer = nullptr;
    CHECK(hipStreamCreateWithFlags(&consumer, hipStreamNonBlocking) == hipSuccess);
    int older_first = 0;
    for (long n = 1; n < 400; ++n) {
        kifs_multi* m = multi({0, 1, 2}, s, KIFS_GATHER_SPARSE);
        uint64_t s0 = 0, s1 = ~uint64_t(0);
        CHECK(kifs_multi_render_batch_async(m, B, cams.data(), frames, size_t(w) * 4, fb, 1, 0, &s0) == KIFS_OK);
        const long before = stub_calls();
        stub_fail_in(n);
        const int st = kifs_multi_render_batch_async(m, B, cams.data(), frames + fb * B, size_t(w) * 4, fb, 1, 0, &s1);
        const bool reached = stub_calls() - before >= n;
        stub_fail_in(-1);
        if (st != KIFS_OK && s1 == s0 + 1) {  // the new step exists; what failed is the flush of the one before it
            ++older_first;
            CHECK(kifs_multi_stream_wait(m, s1, consumer) == KIFS_OK);
            const long launches = stub_launches();
            CHECK(kifs_multi_wait(m, s0) == KIFS_OK && stub_launches() == launches);
            CHECK(kifs_multi_wait(m, s1) == KIFS_OK && equal_dev(frames, want) && equal_dev(frames + fb * B, want));
        }
        kifs_multi_destroy(m);
        if (!reached) break;
    }
    CHECK(older_first > 0);
    CHECK(hipStreamDestroy(consumer) == hipSuccess);
    // a context whose creation fails half way
    for (long n = 1; n < 12; ++n) {
        stub_fail_in(n);
        int st = 0;
        kifs_ctx* c = kifs_create(0, &st);
        stub_fail_in(-1);
        if (c) kifs_destroy(c);
        else CHECK(st == KIFS_ERR_DEVICE_INIT);
    }
    CHECK(hipFree(frames) == hipSuccess);
}


// ---- one long-lived context: tile-table eviction, the feedback state machine at every phase, resizes, diagnostics ----
struct Lifecycle {
    kifs_ctx* c = nullptr;
    Scene s{};
    std::vector<KifsCameraUniform> cams;
    std::vector<uint8_t> want;  // single_frames(s, cams)
    uint8_t* dev = nullptr;     // room for 70 frames of the largest size
    size_t dev_bytes = 0;
    int next_band = 0, next_cam = 0;

    size_t fb() const { return size_t(s.w) * s.h * 4; }
    const uint8_t* expect(int cam, int y0 = 0) const { return want.data() + size_t(cam) * fb() + size_t(y0) * s.w * 4; }
    void use(const Scene& sc) {
        s = sc;
        want = single_frames(s, cams);
        CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK && kifs_set_options(c, &s.options) == KIFS_OK);
    }
    // one lone launch of rows [y0, y1) into a sentinel-filled device band, on `stream` (null: the context's)
    void lone(int y0 = 0, int y1 = -1, hipStream_t stream = nullptr) {
        if (y1 < 0) y1 = s.h;
        const int cam = next_cam++ % int(cams.size());
        const size_t bytes = size_t(y1 - y0) * s.w * 4;
        std::memset(dev, 0xEE, bytes + 64);
        CHECK(kifs_set_camera(c, &cams[size_t(cam)]) == KIFS_OK);
        CHECK(kifs_render_async(c, stream, dev, size_t(s.w) * 4, y0, y1, 1) == KIFS_OK);
        CHECK(std::memcmp(dev, expect(cam, y0), bytes) == 0 && dev[bytes] == 0xEE && dev[bytes + 63] == 0xEE);
    }
    void batch(int n) {
        std::vector<KifsCameraUniform> v(static_cast<size_t>(n));
        std::vector<uint8_t*> outs(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) {
            v[size_t(i)] = cams[size_t(i) % cams.size()];
            outs[size_t(i)] = dev + fb() * size_t(i);
        }
        std::memset(dev, 0xEE, fb() * size_t(n));
        CHECK(kifs_render_batch_async(c, nullptr, n, v.data(), outs.data(), size_t(s.w) * 4, 0, s.h, 1) == KIFS_OK);
        for (int i = 0; i < n; ++i) CHECK(std::memcmp(outs[size_t(i)], expect(i % int(cams.size())), fb()) == 0);
    }
    // a band geometry this context has never rendered: always a miss in the tile-table cache
    void new_band() {
        const int n = next_band++;
        const int y0 = 8 * (n % 61), y1 = y0 + 8 + n / 61;
        CHECK(y1 <= s.h);
        lone(y0, y1);
    }
    std::vector<uint32_t> order() {
        std::vector<uint32_t> o(size_t((s.w + 31) / 32) * size_t((s.h + 7) / 8));
        size_t n = 0;
        CHECK(kifs_debug_get_tile_order(c, o.data(), o.size(), &n) == KIFS_OK && n == o.size());
        return o;
    }
};

// The centre-first order of a context that has rendered nothing.
std::vector<uint32_t> fresh_order(const Scene& s) {
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK && kifs_set_screen(c, &s.screen) == KIFS_OK);
    std::vector<uint32_t> o(size_t((s.w + 31) / 32) * size_t((s.h + 7) / 8));
    size_t n = 0;
    CHECK(kifs_debug_get_tile_order(c, o.data(), o.size(), &n) == KIFS_OK && n == o.size());
    kifs_destroy(c);
    return o;
}

void context_lifecycle() {
    stub_trace_mark("context_lifecycle");
    Lifecycle L;
    int st = 0;
    L.c = kifs_create(0, &st);
    CHECK(L.c && st == KIFS_OK);
    L.cams = cameras(4, 50);
    const Scene full = scene(1024, 512, 40);     // 32 x 64 = 2048 tiles: the >= edge of FEEDBACK_MIN_TILES
    const Scene ragged = scene(1056, 516, 40);   // 33 x 65 tiles, the last column and row partial
    L.dev_bytes = size_t(1056) * 516 * 4 * 70 + 64;
    L.dev = dev_alloc(L.dev_bytes);
    kifs_ctx* const c = L.c;

    for (const Scene& sc : {full, ragged}) {
        L.use(sc);
        L.next_band = 0;
        const std::vector<uint32_t> centre_first = fresh_order(sc);
        for (int i = 0; i < 8; ++i) L.new_band();  // every slot of the cache is in use from here on
        // ---- eviction: the full-frame table at phase k of the lone period, eight other geometries, and back
        for (int k = 0; k < 4; ++k) {
            for (int i = 0; i < 8; ++i) L.new_band();  // (the full-frame table is rebuilt below: phase 0)
            for (int i = 0; i < k; ++i) L.lone();
            long syncs = stub_device_synchronizes();
            for (int i = 0; i < 8; ++i) L.new_band();
            CHECK(stub_device_synchronizes() - syncs == 8);  // one drain per eviction, nothing else drains
            L.lone();
            CHECK(stub_device_synchronizes() - syncs == 9);
            for (int i = 0; i < 6; ++i) L.lone();
            CHECK(stub_device_synchronizes() - syncs == 9);  // a cached geometry drains nothing
            // a pinned order survives seven other geometries and is gone after eight
            std::vector<uint32_t> pin = L.order();
            std::reverse(pin.begin(), pin.end());
            CHECK(pin != centre_first);
            CHECK(kifs_debug_set_tile_order(c, pin.data(), pin.size()) == KIFS_OK);
            L.lone();
            for (int i = 0; i < 7; ++i) L.new_band();
            CHECK(L.order() == pin);
            L.lone();
            for (int i = 0; i < 8; ++i) L.new_band();
            CHECK(L.order() == centre_first);
            for (int i = 0; i < 6; ++i) L.lone();  // (feedback is on again: the sixth launch has adopted a sorted order)
            CHECK(L.order() != centre_first);  // (the stub's costs are a hash of the tile index: their sort is not centre-first)
        }
        // ---- transitions: from phase k, one transition, then six lone launches
        hipStream_t caller = nullptr;
        CHECK(hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) == hipSuccess);
        const size_t texels = size_t(sc.w) * sc.h;
        float* geom = reinterpret_cast<float*>(dev_alloc(texels * 16));
        Scene sphere = sc;
        {
            KifsGuiData gui;
            kifs_host_gui_default(&gui);
            gui.fractal_group = 0;  // KIFS, sphere: no feedback below 16384 tiles
            gui.background_color[0] = 40;
            gui.background_color[1] = 20;
            CHECK(kifs_host_options(&gui, &sphere.options) == KIFS_OK);
        }
        for (int transition = 0; transition < 8; ++transition)
            for (int k = 0; k < 4; ++k) {
                for (int i = 0; i < 8; ++i) L.new_band();  // evicts the full-frame table: the next launch is phase 0
                for (int i = 0; i < k; ++i) L.lone();
                switch (transition) {
                case 0: L.batch(3); break;
                case 1: L.batch(70); break;
                case 2:
                    CHECK(kifs_set_frames_in_flight(c, 3) == KIFS_OK);
                    L.lone();
                    L.lone();
                    CHECK(kifs_set_frames_in_flight(c, 1) == KIFS_OK);
                    break;
                case 3: L.lone(0, -1, caller); L.lone(0, -1, caller); break;
                case 4:
                    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
                    L.lone();
                    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
                    break;
                case 5: {
                    const std::vector<uint32_t> before = L.order();
                    uint8_t* outs[1] = {L.dev};
                    std::memset(L.dev, 0xEE, L.fb());
                    std::memset(geom, 0xEE, texels * 16);
                    CHECK(kifs_render_geometry_async(c, nullptr, 1, &L.cams[1], outs, size_t(sc.w) * 4, geom, size_t(sc.w) * 16,
                                                     texels * 16, 0, sc.h, 1) == KIFS_OK);
                    CHECK(std::memcmp(L.dev, L.expect(1), L.fb()) == 0);
                    for (size_t i = 0; i < texels; i += 997) CHECK(geom[4 * i] == float(i % size_t(sc.w)) && geom[4 * i + 1] == float(i / size_t(sc.w)));
                    CHECK(geom[4 * (texels - 1)] == float(sc.w - 1) && geom[4 * (texels - 1) + 1] == float(sc.h - 1));
                    CHECK(L.order() == before);
                    break;
                }
                case 6:
                    CHECK(kifs_set_options(c, &sphere.options) == KIFS_OK);
                    L.lone();
                    CHECK(kifs_set_options(c, &sc.options) == KIFS_OK);
                    break;
                case 7: L.lone(0, 504); break;  // 63 tile rows: 2016 tiles at 1024 (no feedback), 2079 at 1056
                }
                for (int i = 0; i < 6; ++i) L.lone();
                (void)L.order();  // (the stub has checked the permutation at every launch; this drains like a caller would)
            }
        CHECK(hipFree(geom) == hipSuccess && hipStreamDestroy(caller) == hipSuccess);
    }

    // ---- resizes: host and device destinations interleaved, stripe lists cached at a tall size refused at a short one
    {
        const int sizes[5][2] = {{1024, 512}, {330, 149}, {64, 40}, {1056, 516}, {1024, 512}};
        const int tall[2] = {3, 64}, mid[2] = {0, 18};  // stripe 64: rows 512..515 of 516; stripe 18: rows 144..148 of 149
        for (int i = 0; i < 5; ++i) {
            const Scene sc = scene(sizes[i][0], sizes[i][1], 40);
            L.use(sc);
            std::vector<uint8_t> host(L.fb(), 0xEE);
            for (int rep = 0; rep < 3; ++rep) {
                const int cam = L.next_cam++ % 4;
                CHECK(kifs_set_camera(c, &L.cams[size_t(cam)]) == KIFS_OK);
                if (rep % 2 == i % 2) {
                    CHECK(kifs_render(c, host.data(), size_t(sc.w) * 4, 0, sc.h, 1) == KIFS_OK);
                    CHECK(std::memcmp(host.data(), L.expect(cam), L.fb()) == 0);
                } else {
                    L.lone();
                    L.lone(sc.h / 3, sc.h - 3);
                }
            }
            uint8_t* outs[1] = {L.dev};
            auto shard = [&](const int* stripes) {
                return kifs_render_shard_async(c, nullptr, 1, &L.cams[0], outs, size_t(sc.w) * 4, stripes, 2, 1, 1);
            };
            std::memset(L.dev, 0xEE, L.fb());
            if (sc.h == 516) {
                CHECK(shard(tall) == KIFS_OK);
                for (int y : {24, 31, 512, 515}) CHECK(std::memcmp(L.dev + size_t(y) * sc.w * 4, L.expect(0, y), size_t(sc.w) * 4) == 0);
                CHECK(L.dev[size_t(32) * sc.w * 4] == 0xEE);
            } else {
                CHECK(shard(tall) == KIFS_ERR_BAD_ARG);  // (on the last visit it sits in the cache)
            }
            if (sc.h == 149) CHECK(shard(mid) == KIFS_OK);
            if (sc.h == 40) CHECK(shard(mid) == KIFS_ERR_BAD_ARG);
        }
    }

    // ---- diagnostics: the buffer is sized by the call, a launch with more waves than it holds runs without it
    {
        const Scene small = scene(330, 149, 40);  // 11 x 19 tiles
        L.use(small);
        unsigned long long head[8];
        size_t n = 0;
        std::vector<unsigned long long> rec(size_t(4) * 4 * 2048), zero(rec.size(), 0ull);
        CHECK(kifs_debug_wave_records(c, rec.data(), 1, &n) == KIFS_ERR_UNCONFIGURED);
        CHECK(kifs_debug_counters(c, 1, head) == KIFS_OK);
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK && n == size_t(4) * 11 * 19);
        CHECK(std::memcmp(rec.data(), zero.data(), n * 32) == 0);
        L.lone();
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK && n == size_t(4) * 11 * 19);
        CHECK(rec[0] == 1000 && rec[4 * (n - 1)] == 1000 + 11 * 19 - 1);
        CHECK(kifs_debug_counters(c, 1, head) == KIFS_OK);
        L.lone(16, 56);  // five tile rows: 55 workgroups
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK);
        CHECK(rec[4 * (4 * 55 - 1)] == 1000 + 54 && std::memcmp(rec.data() + 16 * 55, zero.data(), (n - 4 * 55) * 32) == 0);
        CHECK(kifs_debug_counters(c, 1, head) == KIFS_OK);
        L.batch(3);  // 3 x 209 workgroups: three times the buffer
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK && std::memcmp(rec.data(), zero.data(), n * 32) == 0);
        L.use(full);
        L.lone();    // 2048 workgroups after the resize
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK && n == size_t(4) * 11 * 19);
        CHECK(std::memcmp(rec.data(), zero.data(), n * 32) == 0);
        CHECK(kifs_debug_counters(c, 1, head) == KIFS_OK);  // re-enabling sizes for the new screen
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK && n == size_t(4) * 2048);
        L.lone();
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_OK && rec[4 * (n - 1)] == 1000 + 2047);
        CHECK(kifs_debug_counters(c, 0, head) == KIFS_OK);
        CHECK(kifs_debug_wave_records(c, rec.data(), rec.size() / 4, &n) == KIFS_ERR_UNCONFIGURED);
        L.lone();
    }
    CHECK(hipFree(L.dev) == hipSuccess);
    kifs_destroy(c);
}

// ---- the launch-shape rules (namespace rules of kifs_schedule.cpp), from both sides of every threshold --------------
// One context, no tuning knobs.  A case is a scene, a frame of tx x ty whole tiles, a camera distance, a number of views
// and of frames in flight; after its launch the kernel, the round length, the tiles per workgroup, the bunny's form, the
// residency cap, whether costs were recorded and which culls were on must equal the literals beside it.  THE LITERALS
// WERE TAKEN FROM A RUN OF THIS SCENARIO AGAINST THE kifs_schedule.cpp OF COMMIT aa8491c, before that file's
// enqueue_batch was split up; whoever changes a rule changes its line here on purpose, never by copying what the changed
// code reports.  A camera at distance 0.5 is inside every scene's bounding sphere: the rules' `load` is then the exact
// integer tiles x views, and a case can sit ON a threshold.  Where REQUEUE_MIN_WORKGROUPS (4096 workgroups) keeps such a
// launch from having rounds at all, the camera stands outside and the pair of cases brackets the threshold within 5 %
// (load = views x pi (H/2)^2 R^2 / (d^2 - R^2) / 256 for a frame of H rows, R = B + epsilon: disc_tiles(); at 1080 rows
// 14315.4 / (d^2 - 4.0004) a view for the Julia set, 3579.2 / (d^2 - 1.0002) for the bunny).
enum : int { HEATMAP = 1, EPS_ZERO = 2, DIAGNOSTICS = 4, GEOMETRY = 8, SSAA2 = 16, FAR_ORIGIN = 32, NAN_ORIGIN = 64, SKEWED = 128 };
enum : int { JULIA = 1, GENJULIA = 2, KIFS = 0, SPHERE = 0, SIERPINSKI = 4, BUNNY = 5 };
struct ShapeCase {
    const char* what;
    int group, prim, tx, ty;
    float distance;
    int views, in_flight, max_iterations, flags;
    // expected: KifsKernel; FrameParams round_steps, group_tiles, bunny_coop, workgroups_per_cu; costs recorded; culls as
    // three digits (bounding sphere, wave-level, tile-level)
    int kernel, rounds, group_tiles, bunny, per_cu, costs, culls;
};
const float IN = 0.5f;
const ShapeCase SHAPE_CASES[] = {
    // REQUEUE_MIN_WORKGROUPS = 4096
    {"requeue: lone, on the edge", JULIA, 0, 64, 64, IN, 1, 1, 256, 0, /**/ 1, 32, 1, 0, 0, 1, 111},
    {"requeue: lone, one tile short", JULIA, 0, 63, 65, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 0, 1, 111},
    {"requeue: 8 x 512", JULIA, 0, 16, 32, IN, 8, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 0, 111},
    {"requeue: 8 x 511", JULIA, 0, 7, 73, IN, 8, 1, 256, 0, /**/ 0, 0, 2, 0, 0, 0, 111},
    // max_iterations < 2 x rounds; the generalised Julia under 32 steps
    {"steps: Julia 32", JULIA, 0, 16, 32, IN, 8, 1, 32, 0, /**/ 1, 16, 2, 0, 0, 0, 111},
    {"steps: Julia 31", JULIA, 0, 16, 32, IN, 8, 1, 31, 0, /**/ 0, 0, 2, 0, 0, 0, 111},
    {"steps: sphere 16", KIFS, SPHERE, 16, 32, IN, 8, 1, 16, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"steps: sphere 15", KIFS, SPHERE, 16, 32, IN, 8, 1, 15, 0, /**/ 0, 0, 1, 0, 0, 0, 111},
    {"steps: gen-Julia 32", GENJULIA, 0, 16, 32, IN, 8, 1, 32, 0, /**/ 1, 16, 1, 0, 0, 0, 111},
    {"steps: gen-Julia 31", GENJULIA, 0, 16, 32, IN, 8, 1, 31, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"steps: gen-Julia 16", GENJULIA, 0, 16, 32, IN, 8, 1, 16, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"steps: gen-Julia 15", GENJULIA, 0, 16, 32, IN, 8, 1, 15, 0, /**/ 0, 0, 1, 0, 0, 0, 111},
    // heatmap, epsilon <= 0, diagnostics (a batch's records do not fit the buffer: it is dropped BEFORE it stops the rounds)
    {"heatmap", JULIA, 0, 16, 32, IN, 8, 1, 256, HEATMAP, /**/ 0, 0, 2, 0, 0, 0, 100},
    {"epsilon 0", JULIA, 0, 16, 32, IN, 8, 1, 256, EPS_ZERO, /**/ 0, 0, 2, 0, 0, 0, 111},
    {"diagnostics: lone", JULIA, 0, 64, 64, IN, 1, 1, 256, DIAGNOSTICS, /**/ 0, 0, 1, 0, 0, 0, 111},
    {"diagnostics: batch", JULIA, 0, 64, 64, IN, 2, 1, 256, DIAGNOSTICS, /**/ 1, 16, 2, 0, 0, 0, 111},
    // ROUND_STEPS_LONE_JULIA: 64+ steps, uncapped, one view
    {"lone Julia: 64 steps", JULIA, 0, 64, 64, IN, 1, 1, 64, 0, /**/ 1, 32, 1, 0, 0, 0, 111},
    {"lone Julia: 63 steps", JULIA, 0, 64, 64, IN, 1, 1, 63, 0, /**/ 1, 16, 1, 0, 0, 1, 111},
    {"lone Julia: two views", JULIA, 0, 64, 64, IN, 2, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 0, 111},
    {"lone Julia: two frames in flight", JULIA, 0, 64, 64, IN, 1, 2, 256, 0, /**/ 1, 32, 2, 0, 0, 0, 111},
    {"lone gen-Julia", GENJULIA, 0, 64, 64, IN, 1, 1, 256, 0, /**/ 1, 16, 1, 0, 0, 0, 111},
    // RESIDENCY_ONE_PER_CU = 1024, RESIDENCY_TWO_PER_CU = 2048: lone Julia frames only
    {"residency: 1024", JULIA, 0, 32, 32, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 1, 0, 111},
    {"residency: 1025", JULIA, 0, 25, 41, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 2, 0, 111},
    {"residency: 2048", JULIA, 0, 32, 64, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 2, 1, 111},
    {"residency: 2049", JULIA, 0, 3, 683, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 0, 1, 111},
    {"residency: 1024, two frames in flight", JULIA, 0, 32, 32, IN, 1, 2, 256, 0, /**/ 0, 0, 1, 0, 0, 0, 111},
    {"residency: 1024, gen-Julia", GENJULIA, 0, 32, 32, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 0, 0, 111},
    {"residency: 1024, sphere", KIFS, SPHERE, 32, 32, IN, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 0, 0, 111},
    // (a capped launch has no rounds.  1080p = 60 x 135 tiles; heavy tiles: 2020 and 2078)
    {"residency: 1080p, 1.4 % under 2048", JULIA, 0, 60, 135, 3.33f, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 2, 1, 111},
    {"residency: 1080p, 1.5 % over 2048", JULIA, 0, 60, 135, 3.30f, 1, 1, 256, 0, /**/ 1, 32, 1, 0, 0, 0, 111},
    {"residency: 1080p at distance 5", JULIA, 0, 60, 135, 5.0f, 1, 1, 256, 0, /**/ 0, 0, 1, 0, 1, 0, 111},
    {"residency: 1080p at distance 5, two in flight", JULIA, 0, 60, 135, 5.0f, 1, 2, 256, 0, /**/ 1, 32, 1, 0, 0, 0, 111},
    // WAVE_FROM_JULIA = 12500, with its `count >= 3 || load >= WAVE_FROM_LONE` clause
    {"wave: Julia 4 x 3125", JULIA, 0, 25, 125, IN, 4, 1, 256, 0, /**/ 2, 16, 0, 0, 0, 1, 111},
    {"wave: Julia 4 x 3124", JULIA, 0, 44, 71, IN, 4, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 1, 111},
    {"wave: Julia 3 x 4167", JULIA, 0, 9, 463, IN, 3, 1, 256, 0, /**/ 2, 16, 0, 0, 0, 1, 111},
    {"wave: Julia 2 x 6250", JULIA, 0, 50, 125, IN, 2, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 1, 111},
    {"wave: Julia 2 x 15000", JULIA, 0, 100, 150, IN, 2, 1, 256, 0, /**/ 2, 16, 0, 0, 0, 1, 111},
    {"wave: Julia 2 x 14999", JULIA, 0, 53, 283, IN, 2, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 1, 111},
    // WAVE_FROM_OTHER = 32000 (KIFS on one wave per tile: rounds of 4); the generalised Julia never
    {"wave: sphere 4 x 8000", KIFS, SPHERE, 80, 100, IN, 4, 1, 256, 0, /**/ 2, 4, 0, 0, 0, 0, 111},
    {"wave: sphere 4 x 7999", KIFS, SPHERE, 19, 421, IN, 4, 1, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    {"wave: gen-Julia 4 x 8000", GENJULIA, 0, 80, 100, IN, 4, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 1, 111},
    // WAVE_FROM_LONE = 30000
    {"wave: lone Julia 30000", JULIA, 0, 150, 200, IN, 1, 1, 256, 0, /**/ 2, 32, 0, 0, 0, 1, 111},
    {"wave: lone Julia 29999", JULIA, 0, 131, 229, IN, 1, 1, 256, 0, /**/ 1, 32, 1, 0, 0, 1, 111},
    {"wave: lone Sierpinski 30000", KIFS, SIERPINSKI, 150, 200, IN, 1, 1, 256, 0, /**/ 2, 4, 0, 0, 0, 0, 111},
    {"wave: lone Sierpinski 29999", KIFS, SIERPINSKI, 131, 229, IN, 1, 1, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    {"wave: Julia 30000, two in flight", JULIA, 0, 150, 200, IN, 1, 2, 256, 0, /**/ 2, 32, 0, 0, 0, 0, 111},
    {"wave: Julia 29999, two in flight", JULIA, 0, 131, 229, IN, 1, 2, 256, 0, /**/ 1, 32, 2, 0, 0, 0, 111},
    // PAIR_FROM_BATCH = 3500 (1080p x 8, load 3579 and 3423), PAIR_FROM_GENJULIA = 5000,
    // PAIR_FROM_BATCH_KIFS = 7000, PAIR_FROM_LONE_KIFS = 12000
    {"pair: Julia, 2.3 % over 3500", JULIA, 0, 60, 135, 6.00f, 8, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 1, 111},
    {"pair: Julia, 2.2 % under 3500", JULIA, 0, 60, 135, 6.12f, 8, 1, 256, 0, /**/ 1, 16, 1, 0, 0, 0, 111},
    {"pair: gen-Julia 8 x 625", GENJULIA, 0, 25, 25, IN, 8, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 0, 111},
    {"pair: gen-Julia 8 x 624", GENJULIA, 0, 24, 26, IN, 8, 1, 256, 0, /**/ 1, 16, 1, 0, 0, 0, 111},
    {"pair: sphere 8 x 875", KIFS, SPHERE, 25, 35, IN, 8, 1, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    {"pair: sphere 8 x 874", KIFS, SPHERE, 23, 38, IN, 8, 1, 256, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"pair: lone Sierpinski 12000", KIFS, SIERPINSKI, 100, 120, IN, 1, 1, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    {"pair: lone Sierpinski 11999", KIFS, SIERPINSKI, 13, 923, IN, 1, 1, 256, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"pair: Sierpinski 12000, two in flight", KIFS, SIERPINSKI, 100, 120, IN, 1, 2, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    // the bunny at 1080p: a lone frame takes the quad kernel; BUNNY_ROUNDS_FROM = 450 (load 465 and 437), BUNNY_PAIR_FROM = 1600
    // (1637 and 1567), BUNNY_W2LDS_FROM = 2600 (2660 and 2545), BUNNY_COOP_FROM = 5000
    {"bunny: lone", KIFS, BUNNY, 64, 64, IN, 1, 1, 256, 0, /**/ 3, 0, 2, 2, 0, 0, 111},
    {"bunny: lone, two in flight", KIFS, BUNNY, 64, 64, IN, 1, 2, 256, 0, /**/ 3, 0, 2, 2, 0, 0, 111},
    {"bunny: 3.3 % over 450", KIFS, BUNNY, 60, 135, 4.05f, 2, 1, 256, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"bunny: 2.9 % under 450", KIFS, BUNNY, 60, 135, 4.17f, 2, 1, 256, 0, /**/ 3, 0, 1, 0, 0, 0, 111},
    {"bunny: 2.3 % over 1600", KIFS, BUNNY, 60, 135, 4.30f, 8, 1, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    {"bunny: 2.1 % under 1600", KIFS, BUNNY, 60, 135, 4.39f, 8, 1, 256, 0, /**/ 1, 8, 1, 0, 0, 0, 111},
    {"bunny: 2.3 % over 2600", KIFS, BUNNY, 60, 135, 3.43f, 8, 1, 256, 0, /**/ 1, 8, 2, 2, 0, 0, 111},
    {"bunny: 2.1 % under 2600", KIFS, BUNNY, 60, 135, 3.50f, 8, 1, 256, 0, /**/ 1, 8, 2, 0, 0, 0, 111},
    {"bunny: 8 x 625", KIFS, BUNNY, 25, 25, IN, 8, 1, 256, 0, /**/ 4, 4, 2, 1, 0, 0, 111},
    {"bunny: 8 x 624", KIFS, BUNNY, 24, 26, IN, 8, 1, 256, 0, /**/ 1, 8, 2, 2, 0, 0, 111},
    // the geometry and the supersampled launch: one tuple each, the geometry launch with the lone frame's residency
    {"geometry: lone 1024", JULIA, 0, 32, 32, IN, 1, 1, 256, GEOMETRY, /**/ 6, 0, 1, 0, 1, 0, 111},
    {"geometry: 1025", JULIA, 0, 25, 41, IN, 1, 1, 256, GEOMETRY, /**/ 6, 0, 1, 0, 2, 0, 111},
    {"geometry: 1024, two in flight", JULIA, 0, 32, 32, IN, 1, 2, 256, GEOMETRY, /**/ 6, 0, 1, 0, 0, 0, 111},
    {"geometry: lone 4096", JULIA, 0, 64, 64, IN, 1, 1, 256, GEOMETRY, /**/ 6, 0, 1, 0, 0, 0, 111},
    {"supersampled: lone 1024", JULIA, 0, 32, 32, IN, 1, 1, 256, SSAA2, /**/ 5, 0, 1, 0, 0, 0, 111},
    {"supersampled: lone 4096", JULIA, 0, 64, 64, IN, 1, 1, 256, SSAA2, /**/ 5, 0, 1, 0, 0, 0, 111},
    {"supersampled: 8 x 512", JULIA, 0, 16, 32, IN, 8, 1, 256, SSAA2, /**/ 5, 0, 1, 0, 0, 0, 111},
    // the culls: off for a far or NaN origin (every tile then counts as heavy), the tile-level one for a skewed matrix
    {"culls: far origin", JULIA, 0, 32, 32, IN, 1, 1, 256, FAR_ORIGIN, /**/ 0, 0, 1, 0, 0, 0, 0},
    {"culls: NaN origin", JULIA, 0, 32, 32, IN, 1, 1, 256, NAN_ORIGIN, /**/ 0, 0, 1, 0, 0, 0, 0},
    {"culls: skewed matrix", JULIA, 0, 32, 32, IN, 1, 1, 256, SKEWED, /**/ 0, 0, 1, 0, 1, 0, 110},
    {"culls: far origin in a batch", JULIA, 0, 60, 135, 6.12f, 8, 1, 256, FAR_ORIGIN, /**/ 2, 16, 0, 0, 0, 1, 0},
    {"culls: 32 rows", JULIA, 0, 128, 4, IN, 8, 1, 256, 0, /**/ 1, 16, 2, 0, 0, 0, 110},
};

void launch_shapes() {
    stub_trace_mark("launch_shapes");
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    const size_t pixels = size_t(32 * 150) * (8 * 200);  // the largest frame of the table
    uint8_t* frame = dev_alloc(pixels * 4);  // every view of a batch writes this one frame
    float* geom = reinterpret_cast<float*>(dev_alloc(size_t(32 * 64) * (8 * 64) * 16));
    for (const ShapeCase& k : SHAPE_CASES) {
        const int w = 32 * k.tx, h = 8 * k.ty;
        CHECK(size_t(w) * h <= pixels && size_t(w) * h * k.views <= 40u * 1000 * 1000);
        KifsScreenUniform screen;
        KifsOptionsUniform options;
        KifsGuiData gui;
        kifs_host_gui_default(&gui);
        gui.fractal_group = uint32_t(k.group);
        gui.primitive_shape = uint32_t(k.prim);
        gui.max_iterations = uint32_t(k.max_iterations);
        gui.is_heatmap = (k.flags & HEATMAP) ? 1 : 0;
        if (k.flags & EPS_ZERO) gui.epsilon = 0.0f;
        CHECK(kifs_host_screen(uint32_t(w), uint32_t(h), &screen) == KIFS_OK && kifs_host_options(&gui, &options) == KIFS_OK);
        KifsCameraData cd;
        kifs_host_camera_default(&cd);
        cd.origin_distance = k.distance;
        KifsCameraUniform cam;
        CHECK(kifs_host_camera(&cd, &cam) == KIFS_OK);
        if (k.flags & FAR_ORIGIN) cam.origin[1] = 2.0e15f;
        if (k.flags & NAN_ORIGIN) cam.origin[2] = std::nanf("");
        if (k.flags & SKEWED) cam.matrix[1][0] += 0.01f;
        CHECK(kifs_set_screen(c, &screen) == KIFS_OK && kifs_set_options(c, &options) == KIFS_OK && kifs_set_camera(c, &cam) == KIFS_OK);
        CHECK(kifs_set_frames_in_flight(c, k.in_flight) == KIFS_OK);
        CHECK(kifs_set_supersampling(c, (k.flags & SSAA2) ? 2 : 1) == KIFS_OK);
        unsigned long long head[8];
        if (k.flags & DIAGNOSTICS) CHECK(kifs_debug_counters(c, 1, head) == KIFS_OK);
        const std::vector<KifsCameraUniform> cams(size_t(k.views), cam);
        const std::vector<uint8_t*> outs(size_t(k.views), frame);
        if (k.flags & GEOMETRY)
            CHECK(kifs_render_geometry_async(c, nullptr, 1, nullptr, outs.data(), size_t(w) * 4, geom, size_t(w) * 16, 0, 0, h, 1) == KIFS_OK);
        else if (k.views == 1)
            CHECK(kifs_render_async(c, nullptr, frame, size_t(w) * 4, 0, h, 1) == KIFS_OK);
        else
            CHECK(kifs_render_batch_async(c, nullptr, k.views, cams.data(), outs.data(), size_t(w) * 4, 0, h, 1) == KIFS_OK);
        if (k.flags & DIAGNOSTICS) CHECK(kifs_debug_counters(c, 0, head) == KIFS_OK);
        StubRenderLaunch got;
        stub_last_render(&got);
        const int culls = 100 * got.cull + 10 * got.quick_cull + got.tile_cull;
        const bool same = kifs_debug_last_kernel(c) == k.kernel && got.round_steps == k.rounds && got.group_tiles == k.group_tiles &&
                          got.bunny_coop == k.bunny && got.workgroups_per_cu == k.per_cu && got.tile_cost == k.costs && culls == k.culls;
        if (!same)
            std::fprintf(stderr, "launch_shapes: %s: kernel %d, rounds %d, group_tiles %d, bunny %d, per CU %d, costs %d, culls %03d\n", k.what,
                         kifs_debug_last_kernel(c), got.round_steps, got.group_tiles, got.bunny_coop, got.workgroups_per_cu, got.tile_cost, culls);
        CHECK(same);
        // the report the library gives of the same launch
        const bool rounds = got.round_steps > 0;
        CHECK(got.count == k.views && got.tile_count == unsigned(k.tx * k.ty) && kifs_debug_last_round_steps(c) == got.round_steps);
        CHECK(kifs_debug_last_group_tiles(c) == (rounds ? got.group_tiles : -1));
        CHECK(kifs_debug_last_bunny_form(c) == (rounds && k.group == KIFS && k.prim == BUNNY ? got.bunny_coop : -1));
    }
    CHECK(hipFree(frame) == hipSuccess && hipFree(geom) == hipSuccess);
    kifs_destroy(c);
}

// ---- the option gates (fill_params' `sane` and rounds, orbit_x2_eligible, set_culls, fill_views), from both sides --------
// kifs_set_options refuses nothing but a group id above 2, so these values reach the gates.  A case is an options image
// written field by field, a frame of w x h pixels, a number of views and, for fill_views, the |origin| of one view (on the
// x axis); after its launch the culls' three digits, FrameParams::orbit_x2 and round_steps must equal the literals beside
// it.  THE LITERALS WERE WRITTEN FROM THE GATES' DEFINITIONS (the comments name the comparison each pair brackets), not
// from a run.  Neighbours are nextafterf of the constant.  512 x 256 pixels x 8 views = 4096 workgroups: a batch with
// rounds; a lone frame of that size has none.  tests/option_gates.py holds the same cases for the GPU.
const float F_NAN = std::nanf(""), F_INF = INFINITY;
const float E15 = 1.0e15f, E15_BELOW = std::nextafterf(1.0e15f, 0.0f), E15_ABOVE = std::nextafterf(1.0e15f, F_INF);
const float X_LO = 0x1p-14f, X_LO_BELOW = std::nextafterf(0x1p-14f, 0.0f), X_HI = 0x1p10f, X_HI_ABOVE = std::nextafterf(0x1p10f, F_INF);
const float X_FAR = 0x1p60f, X_FAR_ABOVE = std::nextafterf(0x1p60f, F_INF);
struct GateCase {
    const char* what;
    int group, prim;
    float epsilon, max_distance;
    float c[4];
    int max_iterations, heatmap;
    int w, h, views;
    float origin;    // 0: every view from inside the bounding sphere; else |origin| of view `far_view` (of every view: -1)
    int far_view;
    int culls, orbit_x2, rounds;  // expected
};
#define C_IN {-0.2f, 0.6f, 0.2f, 0.2f}  /* every |c_i| far inside the doubled trip's window */
const GateCase GATE_CASES[] = {
    // E: `epsilon >= 0` for the culls, `epsilon > 0` for the rounds; bound_n2 = +inf for a NaN epsilon closes the doubled trip
    {"E: epsilon 1e-6", JULIA, 0, 1.0e-6f, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    {"E: epsilon +0", JULIA, 0, 0.0f, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 0},
    {"E: epsilon -0", JULIA, 0, -0.0f, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 0},
    {"E: epsilon -1e-3", JULIA, 0, -1.0e-3f, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 0},
    {"E: epsilon NaN", JULIA, 0, F_NAN, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 0, 0},
    {"E: sphere, epsilon +0", KIFS, SPHERE, 0.0f, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 0},
    {"E: sphere, epsilon NaN", KIFS, SPHERE, F_NAN, 1000.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 0, 0},
    // R: `B + epsilon < 1e6` in f32 -- B = 1: 999999 and 1000001; B = 2: 999999 and 1000000
    {"R: sphere, epsilon 999998", KIFS, SPHERE, 999998.0f, 1.0e8f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 8},
    {"R: sphere, epsilon 1e6", KIFS, SPHERE, 1.0e6f, 1.0e8f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 8},
    {"R: Julia, epsilon 999997", JULIA, 0, 999997.0f, 1.0e8f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    {"R: Julia, epsilon 999998", JULIA, 0, 999998.0f, 1.0e8f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 16},
    {"R: Sierpinski, epsilon 999997", KIFS, SIERPINSKI, 999997.0f, 1.0e8f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 8},
    {"R: Sierpinski, epsilon 999998", KIFS, SIERPINSKI, 999998.0f, 1.0e8f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 8},
    // D: `max_distance < 1e15f`, a batch and a lone frame; the doubled trip wants 0 < max_distance <= 2^60
    {"D: below 1e15", JULIA, 0, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    {"D: 1e15", JULIA, 0, 1.0e-4f, E15, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 16},
    {"D: below 1e15, lone", JULIA, 0, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 1, 0, 0, /**/ 111, 1, 0},
    {"D: 1e15, lone", JULIA, 0, 1.0e-4f, E15, C_IN, 256, 0, 512, 256, 1, 0, 0, /**/ 0, 1, 0},
    {"D: sphere, below 1e15", KIFS, SPHERE, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 8},
    {"D: sphere, 1e15", KIFS, SPHERE, 1.0e-4f, E15, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 8},
    {"D: infinity", JULIA, 0, 1.0e-4f, F_INF, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 0, 16},
    {"D: NaN", JULIA, 0, 1.0e-4f, F_NAN, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 0, 16},
    {"D: 0", JULIA, 0, 1.0e-4f, 0.0f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 0, 16},
    {"D: the GUI's 1e4", JULIA, 0, 1.0e-4f, 1.0e4f, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    // X: every |c_i| in [2^-14, 2^10], max_distance in (0, 2^60] -- where the culls are already off
    {"X: c.x = 2^-14", JULIA, 0, 1.0e-4f, 1000.0f, {X_LO, 0.6f, 0.2f, 0.2f}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    {"X: c.x below 2^-14", JULIA, 0, 1.0e-4f, 1000.0f, {X_LO_BELOW, 0.6f, 0.2f, 0.2f}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 0, 16},
    {"X: c.w = -2^-14", JULIA, 0, 1.0e-4f, 1000.0f, {-0.2f, 0.6f, 0.2f, -X_LO}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    {"X: c.w above -2^-14", JULIA, 0, 1.0e-4f, 1000.0f, {-0.2f, 0.6f, 0.2f, -X_LO_BELOW}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 0, 16},
    {"X: c.y = 2^10", JULIA, 0, 1.0e-4f, 1000.0f, {-0.2f, X_HI, 0.2f, 0.2f}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 16},
    {"X: c.y above 2^10", JULIA, 0, 1.0e-4f, 1000.0f, {-0.2f, X_HI_ABOVE, 0.2f, 0.2f}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 0, 16},
    {"X: c.z = +0", JULIA, 0, 1.0e-4f, 1000.0f, {-0.2f, 0.6f, 0.0f, 0.2f}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 0, 16},
    {"X: c.z = -0", JULIA, 0, 1.0e-4f, 1000.0f, {-0.2f, 0.6f, -0.0f, 0.2f}, 256, 0, 512, 256, 8, 0, 0, /**/ 111, 0, 16},
    {"X: max_distance 2^60", JULIA, 0, 1.0e-4f, X_FAR, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 1, 16},
    {"X: max_distance above 2^60", JULIA, 0, 1.0e-4f, X_FAR_ABOVE, C_IN, 256, 0, 512, 256, 8, 0, 0, /**/ 0, 0, 16},
    // M: the quick cull (and with it the tile cull) wants max_iterations > 0; the round thresholds are in SHAPE_CASES
    {"M: 1 step", JULIA, 0, 1.0e-4f, 1000.0f, C_IN, 1, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 0},
    {"M: 0 steps", JULIA, 0, 1.0e-4f, 1000.0f, C_IN, 0, 0, 512, 256, 8, 0, 0, /**/ 100, 1, 0},
    {"M: -5 steps", JULIA, 0, 1.0e-4f, 1000.0f, C_IN, -5, 0, 512, 256, 8, 0, 0, /**/ 100, 1, 0},
    {"M: 0 steps, heatmap", JULIA, 0, 1.0e-4f, 1000.0f, C_IN, 0, 1, 512, 256, 8, 0, 0, /**/ 100, 1, 0},
    {"M: sphere, 1 step", KIFS, SPHERE, 1.0e-4f, 1000.0f, C_IN, 1, 0, 512, 256, 8, 0, 0, /**/ 111, 1, 0},
    {"M: sphere, 0 steps", KIFS, SPHERE, 1.0e-4f, 1000.0f, C_IN, 0, 0, 512, 256, 8, 0, 0, /**/ 100, 1, 0},
    {"M: sphere, -5 steps", KIFS, SPHERE, 1.0e-4f, 1000.0f, C_IN, -5, 0, 512, 256, 8, 0, 0, /**/ 100, 1, 0},
    // O: `|origin|^2 < 1e30` in double -- f32(1e15)^2 = 9.9999997e29, its neighbour's 1.0000001e30; lone, and one view of a batch
    {"O: origin 1e15, lone", JULIA, 0, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 1, E15, -1, /**/ 111, 1, 0},
    {"O: origin above 1e15, lone", JULIA, 0, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 1, E15_ABOVE, -1, /**/ 0, 1, 0},
    {"O: one view at 1e15", JULIA, 0, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 8, E15, 5, /**/ 111, 1, 16},
    {"O: one view above 1e15", JULIA, 0, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 8, E15_ABOVE, 5, /**/ 0, 1, 16},
    {"O: sphere, one view at 1e15", KIFS, SPHERE, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 8, E15, 5, /**/ 111, 1, 8},
    {"O: sphere, one view above 1e15", KIFS, SPHERE, 1.0e-4f, E15_BELOW, C_IN, 256, 0, 512, 256, 8, E15_ABOVE, 5, /**/ 0, 1, 8},
    // H: the tile cull from 64 rows (512 x 64 x 64 views = 8192 workgroups)
    {"H: 63 rows", JULIA, 0, 1.0e-4f, 1000.0f, C_IN, 256, 0, 512, 63, 64, 0, 0, /**/ 110, 1, 16},
    {"H: 64 rows", JULIA, 0, 1.0e-4f, 1000.0f, C_IN, 256, 0, 512, 64, 64, 0, 0, /**/ 111, 1, 16},
};
#undef C_IN

void option_gates() {
    stub_trace_mark("option_gates");
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    uint8_t* frame = dev_alloc(size_t(512) * 256 * 4);  // every view of a batch writes this one frame
    for (const GateCase& k : GATE_CASES) {
        CHECK(k.w <= 512 && k.h <= 256 && k.views <= 64 && std::abs(k.max_iterations) <= 256);
        KifsScreenUniform screen;
        KifsOptionsUniform options;
        KifsGuiData gui;
        kifs_host_gui_default(&gui);
        gui.fractal_group = uint32_t(k.group);
        gui.primitive_shape = uint32_t(k.prim);
        CHECK(kifs_host_screen(uint32_t(k.w), uint32_t(k.h), &screen) == KIFS_OK && kifs_host_options(&gui, &options) == KIFS_OK);
        options.max_iterations = k.max_iterations;  // (written into the image: the GUI type holds none of these)
        options.max_distance = k.max_distance;
        options.epsilon = k.epsilon;
        options.is_heatmap = uint32_t(k.heatmap);
        for (int i = 0; i < 4; ++i) options.constant[i] = k.c[i];
        KifsCameraData cd;
        kifs_host_camera_default(&cd);
        cd.origin_distance = IN;
        KifsCameraUniform cam;
        CHECK(kifs_host_camera(&cd, &cam) == KIFS_OK);
        std::vector<KifsCameraUniform> cams(size_t(k.views), cam);
        if (k.origin != 0.0f)
            for (int v = 0; v < k.views; ++v)
                if (k.far_view < 0 || v == k.far_view) {
                    cams[size_t(v)].origin[0] = k.origin;
                    cams[size_t(v)].origin[1] = cams[size_t(v)].origin[2] = 0.0f;
                }
        CHECK(kifs_set_screen(c, &screen) == KIFS_OK && kifs_set_options(c, &options) == KIFS_OK && kifs_set_camera(c, &cams[0]) == KIFS_OK);
        const std::vector<uint8_t*> outs(size_t(k.views), frame);
        if (k.views == 1)
            CHECK(kifs_render_async(c, nullptr, frame, size_t(k.w) * 4, 0, k.h, 1) == KIFS_OK);
        else
            CHECK(kifs_render_batch_async(c, nullptr, k.views, cams.data(), outs.data(), size_t(k.w) * 4, 0, k.h, 1) == KIFS_OK);
        StubRenderLaunch got;
        stub_last_render(&got);
        const int culls = 100 * got.cull + 10 * got.quick_cull + got.tile_cull;
        const bool same = culls == k.culls && got.orbit_x2 == k.orbit_x2 && got.round_steps == k.rounds;
        if (!same)
            std::fprintf(stderr, "option_gates: %s: culls %03d, orbit_x2 %d, rounds %d\n", k.what, culls, got.orbit_x2, got.round_steps);
        CHECK(same);
        CHECK(got.count == k.views && kifs_debug_last_round_steps(c) == got.round_steps);
    }
    // julia_cull_radius repeats `sane` for the certified radius.  Its own range checks (16 epsilon of room below the bound,
    // trips x log2(4 max_distance) <= 100, the escape radius inside the shell) already refuse both neighbours of every
    // constant, so the repeat can only agree: a radius inside the GUI's ranges, none next to any gate.
    const float c_in[4] = {-0.2f, 0.6f, 0.2f, 0.2f}, c_hi[4] = {-0.2f, X_HI, 0.2f, 0.2f}, c_hi_above[4] = {-0.2f, X_HI_ABOVE, 0.2f, 0.2f};
    const double rho = kifs_host_julia_cull_radius(c_in, 1.0e-4f, 1000.0f, 24, nullptr);
    CHECK(rho > 1.0 && rho < 2.0);
    CHECK(kifs_host_julia_cull_radius(c_in, 1.0e-4f, 1.0e4f, 24, nullptr) > 1.0);
    for (float eps : {999997.0f, 999998.0f, -1.0e-3f, -0.0f - 1.0e-30f, F_NAN}) CHECK(kifs_host_julia_cull_radius(c_in, eps, 1000.0f, 24, nullptr) == 0.0);
    for (float md : {E15_BELOW, E15, F_INF, F_NAN}) CHECK(kifs_host_julia_cull_radius(c_in, 1.0e-4f, md, 24, nullptr) == 0.0);
    CHECK(kifs_host_julia_cull_radius(c_hi, 1.0e-4f, 1000.0f, 24, nullptr) == 0.0);
    CHECK(kifs_host_julia_cull_radius(c_hi_above, 1.0e-4f, 1000.0f, 24, nullptr) == 0.0);
    CHECK(hipFree(frame) == hipSuccess);
    kifs_destroy(c);
}


// ---- the adaptive and the animated entry points ----------------------------------------------------------------------
// What the stand-in's launchers write, restated from its documentation (hip_stub.cpp: stub_key, stub_hit, stub_depth,
// stub_adaptive_pixel, stub_scene_key, stub_sampled_tile): the driver computes every expected frame from these alone.
namespace model {

uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
uint32_t key(const KifsCameraUniform& c) {
    return fbits(c.origin[0]) * 2654435761u ^ fbits(c.origin[1]) * 40503u ^ fbits(c.origin[2]) * 69069u ^ fbits(c.matrix[1][0]);
}
bool hit(uint32_t k, int x, int y) { return (((unsigned(x) >> 5) + 3u * (unsigned(y) >> 3) + (k >> 7)) & 3u) == 0u; }
struct Texel { float nx, ny, nz, t; };
Texel texel(const KifsCameraUniform& c, int x, int y) {
    return Texel{float(x), float(y), c.origin[0], hit(key(c), x, y) ? c.origin[2] + 0.25f * float((x + 2 * y) & 3) : INFINITY};
}
// include/kifs_hip.h, "pair"
bool pair(const Texel& p, const Texel& q, const KifsAdaptiveAA& aa) {
    const bool hp = fbits(p.t) != 0x7f800000u, hq = fbits(q.t) != 0x7f800000u;
    if (hp != hq) return true;
    if (!hp) return false;
    const float d = (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz;
    return !(d >= aa.normal_cos) || std::fabs(p.t - q.t) > aa.depth_rel * std::fmin(p.t, q.t);
}
uint32_t adaptive_pixel(const KifsCameraUniform& c, int x, int y, int k) {
    return (unsigned(x) * 2246822519u ^ unsigned(y) * 3266489917u ^ key(c) * 668265263u ^ unsigned(k) * 374761393u) | 0xff000000u;
}
uint32_t scene_key(const KifsOptionsUniform& o) {
    const float f[11] = {o.constant[0], o.constant[1], o.constant[2], o.constant[3], o.power, o.fractal_color[0], o.fractal_color[1],
                         o.fractal_color[2], o.background_color[0], o.background_color[1], o.background_color[2]};
    uint32_t k = 2166136261u;
    for (float v : f) k = (k ^ fbits(v)) * 16777619u;
    return k & 0x00ffffffu;
}
// A frame of more than 2^23 pixels: the stand-in writes and classifies this sample of its 32 x 8 tiles only, and a
// neighbour outside the sample does not exist.
bool sampled(int w, int h, int x, int y) {
    if (size_t(w) * size_t(h) <= (size_t(1) << 23)) return true;
    const int tiles_x = (w + 31) / 32, tiles_y = (h + 7) / 8, tx = x / 32, tj = y / 8;
    return (tx % 32 <= 1 || tx == tiles_x - 1) && (tj % 64 == 0 || tj == tiles_y - 1);
}
bool edge(const KifsCameraUniform& c, int w, int h, int x, int y, const KifsAdaptiveAA& aa) {
    const Texel p = texel(c, x, y);
    const int nb[4][2] = {{x - 1, y}, {x + 1, y}, {x, y - 1}, {x, y + 1}};
    for (const auto& q : nb)
        if (q[0] >= 0 && q[1] >= 0 && q[0] < w && q[1] < h && sampled(w, h, q[0], q[1]) && pair(p, texel(c, q[0], q[1]), aa)) return true;
    return false;
}

}  // namespace model

// The plain frames of (camera i, options i) as one context renders them one by one, into host memory.
std::vector<uint8_t> plain_frames(const Scene& s, const std::vector<KifsCameraUniform>& cams, const std::vector<KifsOptionsUniform>& opts, int encode) {
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK && kifs_set_screen(c, &s.screen) == KIFS_OK);
    const size_t fb = size_t(s.w) * s.h * 4;
    std::vector<uint8_t> out(fb * cams.size());
    for (size_t i = 0; i < cams.size(); ++i) {
        CHECK(kifs_set_camera(c, &cams[i]) == KIFS_OK && kifs_set_options(c, &opts[i % opts.size()]) == KIFS_OK);
        CHECK(kifs_render(c, out.data() + i * fb, size_t(s.w) * 4, 0, s.h, encode) == KIFS_OK);
    }
    kifs_destroy(c);
    return out;
}

// The frames kifs_render_adaptive_async owes for `cams`: the plain frame with every edge pixel replaced; counts[i] = frame
// i's edge pixels.  (A frame above the sampling threshold: only model::sampled pixels mean anything.)
std::vector<uint8_t> adaptive_frames(const Scene& s, const std::vector<KifsCameraUniform>& cams, const KifsAdaptiveAA& aa, int encode,
                                     std::vector<uint32_t>* counts) {
    std::vector<uint8_t> want = plain_frames(s, cams, {s.options}, encode);
    const size_t fb = size_t(s.w) * s.h * 4;
    counts->assign(cams.size(), 0u);
    for (size_t i = 0; i < cams.size(); ++i)
        for (int y = 0; y < s.h; ++y)
            for (int x = 0; x < s.w; ++x) {
                if (!model::edge(cams[i], s.w, s.h, x, y, aa)) continue;
                const uint32_t px = model::adaptive_pixel(cams[i], x, y, aa.factor);
                std::memcpy(want.data() + i * fb + (size_t(y) * s.w + size_t(x)) * 4, &px, 4);
                ++(*counts)[i];
            }
    return want;
}

// Rows of `w` pixels, `pitch` bytes apart, equal to the packed frame `want`, and the bytes between them still 0xEE.
bool rows_equal(const uint8_t* dev, size_t pitch, const uint8_t* want, int w, int y0, int y1) {
    for (int y = y0; y < y1; ++y) {
        if (std::memcmp(dev + size_t(y - y0) * pitch, want + size_t(y) * w * 4, size_t(w) * 4) != 0) return false;
        for (size_t b = size_t(w) * 4; b < pitch; ++b)
            if (dev[size_t(y - y0) * pitch + b] != 0xEE) return false;
    }
    return true;
}

kifs_ctx* context_for(const Scene& s, const KifsCameraUniform* cam, bool options = true, int device = 0) {
    int st = 0;
    kifs_ctx* c = kifs_create(device, &st);
    CHECK(c && st == KIFS_OK && kifs_set_screen(c, &s.screen) == KIFS_OK);
    if (options) CHECK(kifs_set_options(c, &s.options) == KIFS_OK);
    if (cam) CHECK(kifs_set_camera(c, cam) == KIFS_OK);
    return c;
}

// One adaptive call of `count` frames (first camera cams[first]; lone: cameras NULL, the context's camera must be
// cams[first]) into sentinel-filled device frames `pitch` apart in rows, with or without counts.  Returns the status; on
// KIFS_OK with `want` given, every frame, every byte between the rows and every count has been compared.
struct AdaptiveCall {
    const Scene& s;
    const std::vector<KifsCameraUniform>& cams;
    KifsAdaptiveAA aa;
    int encode = 1;
    size_t pad = 0;  // bytes between rows
    uint8_t* dev = nullptr;       // room for cams.size() frames of the padded pitch
    uint32_t* dev_counts = nullptr;  // cams.size() + 2 words: a sentinel before and behind

    size_t pitch() const { return size_t(s.w) * 4 + pad; }
    size_t frame_bytes() const { return pitch() * size_t(s.h); }
    void alloc() {
        dev = dev_alloc(frame_bytes() * cams.size());
        dev_counts = reinterpret_cast<uint32_t*>(dev_alloc((cams.size() + 2) * 4));
    }
    void release() { CHECK(hipFree(dev) == hipSuccess && hipFree(dev_counts) == hipSuccess); }
    int run(kifs_ctx* c, hipStream_t stream, int first, int count, bool lone, bool with_counts, const std::vector<uint8_t>* want,
            const std::vector<uint32_t>* want_counts) {
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        for (int i = 0; i < count; ++i) outs[size_t(i)] = dev + frame_bytes() * size_t(i);
        std::memset(dev, 0xEE, frame_bytes() * size_t(count));
        std::memset(dev_counts, 0xEE, (cams.size() + 2) * 4);
        const int st = kifs_render_adaptive_async(c, stream, count, lone ? nullptr : cams.data() + first, outs.data(), pitch(), &aa,
                                                  with_counts ? dev_counts + 1 : nullptr, encode);
        if (st != KIFS_OK || !want) return st;
        const size_t fb = size_t(s.w) * s.h * 4;
        for (int i = 0; i < count; ++i) CHECK(rows_equal(outs[size_t(i)], pitch(), want->data() + fb * size_t(first + i), s.w, 0, s.h));
        CHECK(dev_counts[0] == 0xEEEEEEEEu);
        for (int i = 0; i < count; ++i) CHECK(dev_counts[1 + i] == (with_counts ? (*want_counts)[size_t(first + i)] : 0xEEEEEEEEu));
        CHECK(dev_counts[1 + count] == 0xEEEEEEEEu);
        CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ADAPTIVE);
        return st;
    }
};

// The view counts of the adaptive render launches since the last question.
std::vector<int> adaptive_rounds() {
    int r[16];
    const int n = stub_adaptive_rounds(r, 16);
    return std::vector<int>(r, r + std::min(n, 16));  // (more than 16: nobody compares such a run)
}

void adaptive_batches(int w, int h) {
    stub_trace_mark("adaptive_batches");
    const Scene s = scene(w, h, 40);
    const auto cams = cameras(70, 5);
    const size_t pixels = size_t(w) * h;
    // two hits' normals (x, y, origin.x): an edge inside a circle about the frame's corner; depths 0.25 .. 0.75 apart
    AdaptiveCall A{s, cams, KifsAdaptiveAA{2, 0.35f * float(w) * float(w), 0.1f}};
    std::vector<uint32_t> counts;
    const auto want = adaptive_frames(s, cams, A.aa, 1, &counts);
    {   // the mask is neither empty nor everything, and it differs between the views
        size_t total = 0;
        for (uint32_t n : counts) { CHECK(n > 0 && n < pixels); total += n; }
        CHECK(total != counts[0] * counts.size());
        CHECK(want != single_frames(s, cams));
    }
    A.alloc();
    kifs_ctx* c = context_for(s, &cams[0]);
    (void)adaptive_rounds();
    // the lone frame of the context's camera, without and with its count; batches within and beyond the kernel argument
    CHECK(A.run(c, nullptr, 0, 1, true, false, &want, &counts) == KIFS_OK);
    CHECK(A.run(c, nullptr, 0, 1, true, true, &want, &counts) == KIFS_OK);
    CHECK(A.run(c, nullptr, 2, 3, false, true, &want, &counts) == KIFS_OK);
    CHECK(A.run(c, nullptr, 2, 3, false, false, &want, &counts) == KIFS_OK);
    CHECK(adaptive_rounds() == (std::vector<int>{1, 1, 3, 3}));
    CHECK(A.run(c, nullptr, 0, 70, false, true, &want, &counts) == KIFS_OK);  // two rounds: the second's counts at + 35
    CHECK(adaptive_rounds() == (std::vector<int>{35, 35}));
    CHECK(A.run(c, nullptr, 0, 70, false, false, &want, &counts) == KIFS_OK);
    CHECK(A.run(c, nullptr, 3, 67, false, true, &want, &counts) == KIFS_OK);  // rounds of unequal size over one block
    CHECK(adaptive_rounds() == (std::vector<int>{35, 35, 34, 33}));
    CHECK(A.run(c, nullptr, 1, 64, false, true, &want, &counts) == KIFS_OK && A.run(c, nullptr, 1, 65, false, true, &want, &counts) == KIFS_OK);
    CHECK(adaptive_rounds() == (std::vector<int>{64, 33, 32}));
    A.release();
    // a padded pitch, the other encoding, another factor and thresholds at which only hit against miss is an edge
    AdaptiveCall B{s, cams, KifsAdaptiveAA{3, -INFINITY, INFINITY}, 0, 48};
    const std::vector<KifsCameraUniform> few(cams.begin(), cams.begin() + 4);
    const auto want_b = adaptive_frames(s, few, B.aa, 0, &counts);
    B.alloc();
    CHECK(B.run(c, nullptr, 0, 4, false, true, &want_b, &counts) == KIFS_OK);
    CHECK(B.run(c, nullptr, 0, 1, true, true, &want_b, &counts) == KIFS_OK);
    B.release();
    kifs_destroy(c);
}

// The scratch block over sizes and counts that shrink and grow: freed and allocated anew exactly when a call needs more
// than every call before it, and then of exactly the bytes the layout asks for.
void adaptive_scratch() {
    stub_trace_mark("adaptive_scratch");
    const auto cams = cameras(6, 9);
    const int calls[][3] = {{64, 40, 1}, {333, 211, 3}, {64, 40, 5}, {333, 211, 3}, {340, 211, 3}, {64, 8, 6}, {333, 211, 6}, {340, 211, 1}};
    kifs_ctx* c = context_for(scene(64, 40, 40), &cams[0]);
    size_t have = 0;
    for (const auto& k : calls) {
        const Scene s = scene(k[0], k[1], 40);
        CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK);
        AdaptiveCall A{s, cams, KifsAdaptiveAA{2, 5000.0f, 0.1f}};
        std::vector<uint32_t> counts;
        const auto want = adaptive_frames(s, cams, A.aa, 1, &counts);
        A.alloc();
        const size_t need = size_t(k[2]) * (size_t(k[0]) * size_t(k[1]) * 20 + 4);
        const long frees = stub_device_frees(), syncs = stub_device_synchronizes();
        CHECK(A.run(c, nullptr, 0, k[2], false, true, &want, &counts) == KIFS_OK);
        CHECK(stub_device_frees() - frees == (need > have && have > 0 ? 1 : 0));
        CHECK(stub_device_synchronizes() == syncs);  // (hipFree itself waits for the launches that use the block)
        if (need > have) have = need;
        CHECK(stub_has_device_allocation_of(have));
        A.release();
    }
    kifs_destroy(c);
    CHECK(!stub_has_device_allocation_of(have));
}

// Calls of one context on two streams and its own: the library waits for the previous call's event exactly when the
// stream is another one than that call's.
void adaptive_streams() {
    stub_trace_mark("adaptive_streams");
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(3, 1);
    AdaptiveCall A{s, cams, KifsAdaptiveAA{2, 5000.0f, 0.1f}};
    std::vector<uint32_t> counts;
    const auto want = adaptive_frames(s, cams, A.aa, 1, &counts);
    A.alloc();
    kifs_ctx* c = context_for(s, &cams[0]);
    hipStream_t a = nullptr, b = nullptr;
    CHECK(hipStreamCreateWithFlags(&a, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&b, hipStreamNonBlocking) == hipSuccess);
    CHECK(A.run(c, a, 0, 3, false, true, &want, &counts) == KIFS_OK);
    const int done = stub_events_created();  // (the call's last act was to create and record adaptive_done)
    CHECK(stub_stream_waits_on(done) == 0);
    hipStream_t order[] = {a, b, b, a, nullptr, nullptr, b, a, a};
    hipStream_t previous = a;
    long waits = 0;
    for (hipStream_t st : order) {
        CHECK(A.run(c, st, 0, 3, false, true, &want, &counts) == KIFS_OK);
        if (st != previous) ++waits;
        CHECK(stub_stream_waits_on(done) == waits);
        previous = st;
    }
    kifs_destroy(c);
    CHECK(hipStreamDestroy(a) == hipSuccess && hipStreamDestroy(b) == hipSuccess);
    A.release();
}

// A round count that the 2 GiB cap on the scratch block decides: 4096 x 4096, 20 bytes a pixel and view -- six views fit,
// seven take two rounds of 4 and 3.  (Above the stand-in's sampling threshold: model::sampled.)
void adaptive_scratch_cap() {
    stub_trace_mark("adaptive_scratch_cap");
    const int w = 4096, h = 4096, views = 7;
    const Scene s = scene(w, h, 40);
    const auto cams = cameras(views, 2);
    const KifsAdaptiveAA aa{2, 3.0e6f, 0.1f};
    const size_t fb = size_t(w) * h * 4;
    uint8_t* dev = dev_alloc(fb * views);
    uint32_t* dev_counts = reinterpret_cast<uint32_t*>(dev_alloc((views + 2) * 4));
    std::memset(dev_counts, 0xEE, (views + 2) * 4);
    std::vector<uint8_t*> outs(views);
    for (int i = 0; i < views; ++i) outs[size_t(i)] = dev + fb * size_t(i);
    kifs_ctx* c = context_for(s, &cams[0]);
    (void)adaptive_rounds();
    CHECK(kifs_render_adaptive_async(c, nullptr, views, cams.data(), outs.data(), size_t(w) * 4, &aa, dev_counts + 1, 1) == KIFS_OK);
    CHECK(adaptive_rounds() == (std::vector<int>{4, 3}));
    CHECK(stub_has_device_allocation_of(size_t(4) * (size_t(w) * h * 20 + 4)));
    CHECK(dev_counts[0] == 0xEEEEEEEEu && dev_counts[views + 1] == 0xEEEEEEEEu);
    // the sample of every frame against the plain frame of a second context and the model's mask
    kifs_ctx* plain = context_for(s, &cams[0]);
    uint8_t* one = dev_alloc(fb);
    for (int i = 0; i < views; ++i) {
        CHECK(kifs_set_camera(plain, &cams[size_t(i)]) == KIFS_OK && kifs_render_async(plain, nullptr, one, size_t(w) * 4, 0, h, 1) == KIFS_OK);
        uint32_t edges = 0;
        bool same = true;
        for (int y = 0; y < h; ++y) {
            if (!model::sampled(w, h, 0, y)) { y |= 7; continue; }  // (tile column 0 is in the sample wherever the tile row is)
            for (int x = 0; x < w; ++x) {
                if (!model::sampled(w, h, x, y)) { x |= 31; continue; }
                uint32_t px;
                std::memcpy(&px, one + (size_t(y) * w + size_t(x)) * 4, 4);
                if (model::edge(cams[size_t(i)], w, h, x, y, aa)) { px = model::adaptive_pixel(cams[size_t(i)], x, y, aa.factor); ++edges; }
                same = same && std::memcmp(&px, outs[size_t(i)] + (size_t(y) * w + size_t(x)) * 4, 4) == 0;
            }
        }
        CHECK(same && edges > 0 && dev_counts[1 + i] == edges);
    }
    kifs_destroy(plain);
    kifs_destroy(c);
    CHECK(hipFree(one) == hipSuccess && hipFree(dev) == hipSuccess && hipFree(dev_counts) == hipSuccess);
}

// Every refusal of include/kifs_hip.h for the adaptive call: the status, no HIP call, no launch, nothing written.
void adaptive_refusals() {
    stub_trace_mark("adaptive_refusals");
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(3, 1);
    const size_t pitch = size_t(s.w) * 4, fb = pitch * s.h;
    uint8_t* dev = dev_alloc(fb * 3);
    uint32_t* dev_counts = reinterpret_cast<uint32_t*>(dev_alloc(12));
    std::memset(dev, 0xEE, fb * 3);
    std::memset(dev_counts, 0xEE, 12);
    uint8_t* outs[3] = {dev, dev + fb, dev + 2 * fb};
    kifs_ctx* c = context_for(s, &cams[0]);
    const KifsAdaptiveAA good{2, 0.9f, 0.1f};
    auto call = [&](kifs_ctx* ctx, int count, const KifsCameraUniform* cm, uint8_t* const* o, size_t p, const KifsAdaptiveAA* aa, int encode) {
        const long calls = stub_calls(), launches = stub_launches();  // a refused call makes no HIP call and launches nothing
        const int st = kifs_render_adaptive_async(ctx, nullptr, count, cm, o, p, aa, dev_counts, encode);
        CHECK(st != KIFS_OK && stub_calls() == calls && stub_launches() == launches);
        return st;
    };
    CHECK(call(nullptr, 3, cams.data(), outs, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), nullptr, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), outs, pitch, nullptr, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, nullptr, outs, pitch, &good, 1) == KIFS_ERR_BAD_ARG);  // the context's camera is one frame's
    CHECK(call(c, 0, cams.data(), outs, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 513, cams.data(), outs, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    for (int factor : {-1, 0, 1, KIFS_MAX_SUPERSAMPLING + 1}) {
        const KifsAdaptiveAA aa{factor, 0.9f, 0.1f};
        CHECK(call(c, 3, cams.data(), outs, pitch, &aa, 1) == KIFS_ERR_BAD_ARG);
    }
    const KifsAdaptiveAA nan_cos{2, std::nanf(""), 0.1f}, nan_depth{2, 0.9f, std::nanf("")}, neg_depth{2, 0.9f, -0.5f};
    CHECK(call(c, 3, cams.data(), outs, pitch, &nan_cos, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), outs, pitch, &nan_depth, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), outs, pitch, &neg_depth, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), outs, pitch, &good, 2) == KIFS_ERR_BAD_ARG);
    uint8_t* null_out[3] = {dev, nullptr, dev}, *odd_out[3] = {dev, dev + 2, dev};
    CHECK(call(c, 3, cams.data(), null_out, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), odd_out, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), outs, pitch - 4, &good, 1) == KIFS_ERR_BAD_ARG);  // a bad pitch: short, unaligned
    CHECK(call(c, 3, cams.data(), outs, pitch + 2, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
    CHECK(call(c, 3, cams.data(), outs, pitch, &good, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    {   // k W above 65536
        const Scene wide = scene(16400, 8, 40);
        CHECK(kifs_set_screen(c, &wide.screen) == KIFS_OK);
        const KifsAdaptiveAA four{4, 0.9f, 0.1f}, five{5, 0.9f, 0.1f};
        CHECK(KIFS_MAX_SUPERSAMPLING < 5 || call(c, 1, cams.data(), outs, size_t(16400) * 4, &five, 1) == KIFS_ERR_BAD_SIZE);
        CHECK(KIFS_MAX_SUPERSAMPLING < 4 || call(c, 1, cams.data(), outs, size_t(16400) * 4, &four, 1) == KIFS_ERR_BAD_SIZE);
        const Scene tall = scene(8, 16400, 40);
        CHECK(kifs_set_screen(c, &tall.screen) == KIFS_OK);
        CHECK(KIFS_MAX_SUPERSAMPLING < 4 || call(c, 1, cams.data(), outs, 32, &four, 1) == KIFS_ERR_BAD_SIZE);
        CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK);
    }
    {   // unconfigured: no options, no camera
        kifs_ctx* bare = context_for(s, nullptr, false);
        CHECK(call(bare, 3, cams.data(), outs, pitch, &good, 1) == KIFS_ERR_UNCONFIGURED);
        CHECK(kifs_set_options(bare, &s.options) == KIFS_OK);
        CHECK(call(bare, 1, nullptr, outs, pitch, &good, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
    }
    for (size_t i = 0; i < fb * 3; ++i)
        if (dev[i] != 0xEE) CHECK(false);
    CHECK(dev_counts[0] == 0xEEEEEEEEu && dev_counts[2] == 0xEEEEEEEEu);
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess && hipFree(dev_counts) == hipSuccess);
}

// ---- animated batches
// Frame i's options: the constant, the power and both colours move, the pipeline and the march budget stay.
std::vector<KifsOptionsUniform> morph(const KifsOptionsUniform& base, int n, int first) {
    std::vector<KifsOptionsUniform> out(static_cast<size_t>(n), base);
    for (int i = 0; i < n; ++i) {
        KifsOptionsUniform& o = out[size_t(i)];
        const float t = float(first + i);
        o.constant[0] += 0.01f * t;
        o.constant[3] -= 0.02f * t;
        o.power = 2.0f + 0.125f * float((first + i) % 9);
        o.fractal_color[1] = 0.1f + 0.01f * t;
        o.background_color[0] = 0.002f * t;
        o.background_color[2] = 0.5f - 0.004f * t;
    }
    return out;
}

// The frames kifs_render_animation_async owes: frame i as a plain render with (cams[i], opts[i]) writes it, every pixel
// that is not background also a function of opts[i]'s scene.
std::vector<uint8_t> animation_frames(const Scene& s, const std::vector<KifsCameraUniform>& cams, const std::vector<KifsOptionsUniform>& opts, int encode) {
    std::vector<uint8_t> want = plain_frames(s, cams, opts, encode);
    const size_t fb = size_t(s.w) * s.h * 4;
    for (size_t i = 0; i < cams.size(); ++i) {
        const uint32_t k = model::key(cams[i]), sk = model::scene_key(opts[i % opts.size()]);
        for (int y = 0; y < s.h; ++y)
            for (int x = 0; x < s.w; ++x) {
                if (!model::hit(k, x, y)) continue;
                uint32_t px;
                uint8_t* at = want.data() + i * fb + (size_t(y) * s.w + size_t(x)) * 4;
                std::memcpy(&px, at, 4);
                px ^= sk;
                std::memcpy(at, &px, 4);
            }
    }
    return want;
}

struct AnimationCall {
    const Scene& s;
    const std::vector<KifsCameraUniform>& cams;
    const std::vector<KifsOptionsUniform>& opts;
    int encode = 1;
    size_t pad = 0;
    uint8_t* dev = nullptr;

    size_t pitch() const { return size_t(s.w) * 4 + pad; }
    size_t frame_bytes() const { return pitch() * size_t(s.h); }
    void alloc() { dev = dev_alloc(frame_bytes() * cams.size() + 64); }
    void release() { CHECK(hipFree(dev) == hipSuccess); }
    // `shared_camera`: cameras NULL, every frame with the context's camera (which must be cams[first] = ... = the same)
    int run(kifs_ctx* c, hipStream_t stream, int first, int count, int y0, int y1, bool shared_camera, const std::vector<uint8_t>* want) {
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        const size_t band = pitch() * size_t(y1 - y0);
        for (int i = 0; i < count; ++i) outs[size_t(i)] = dev + band * size_t(i);
        std::memset(dev, 0xEE, frame_bytes() * cams.size() + 64);
        const int st = kifs_render_animation_async(c, stream, count, shared_camera ? nullptr : cams.data() + first, opts.data() + first,
                                                   outs.data(), pitch(), y0, y1, encode);
        if (st != KIFS_OK || !want) return st;
        const size_t fb = size_t(s.w) * s.h * 4;
        for (int i = 0; i < count; ++i) CHECK(rows_equal(outs[size_t(i)], pitch(), want->data() + fb * size_t(first + i), s.w, y0, y1));
        for (size_t b = band * size_t(count); b < band * size_t(count) + 64; ++b) CHECK(dev[b] == 0xEE);
        if (y1 > y0) CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ANIMATION && kifs_debug_last_round_steps(c) == 0);
        return st;
    }
};

void animation_batches(int w, int h) {
    stub_trace_mark("animation_batches");
    const Scene s = scene(w, h, 40);
    const auto cams = cameras(70, 7);
    const auto opts = morph(s.options, 70, 0);
    AnimationCall A{s, cams, opts};
    const auto want = animation_frames(s, cams, opts, 1);
    CHECK(want != plain_frames(s, cams, opts, 1));
    A.alloc();
    // a context that never had kifs_set_options: it has none afterwards either
    kifs_ctx* c = context_for(s, nullptr, false);
    uint8_t* plain = dev_alloc(size_t(w) * h * 4);
    for (int count : {1, 5, 70}) {
        CHECK(A.run(c, nullptr, 0, count, 0, h, false, &want) == KIFS_OK);
        CHECK(A.run(c, nullptr, 70 - count, count, 0, h, false, &want) == KIFS_OK);
    }
    CHECK(A.run(c, nullptr, 0, 1, 0, h, true, nullptr) == KIFS_ERR_UNCONFIGURED);  // no camera yet
    CHECK(kifs_set_camera(c, &cams[4]) == KIFS_OK);
    CHECK(kifs_render_async(c, nullptr, plain, size_t(w) * 4, 0, h, 1) == KIFS_ERR_UNCONFIGURED);
    {   // the context's camera for every frame
        const std::vector<KifsCameraUniform> same(70, cams[4]);
        AnimationCall S{s, same, opts};
        const auto want_same = animation_frames(s, same, opts, 1);
        S.alloc();
        for (int count : {1, 5, 70}) CHECK(S.run(c, nullptr, 3, std::min(count, 67), 0, h, true, &want_same) == KIFS_OK);
        S.release();
    }
    CHECK(kifs_render_async(c, nullptr, plain, size_t(w) * 4, 0, h, 1) == KIFS_ERR_UNCONFIGURED);
    // with options of its own: a plain frame before and after a call with other options is that of its own
    const Scene other = scene(w, h, 200);
    CHECK(kifs_set_options(c, &other.options) == KIFS_OK);
    const auto own = single_frames(other, {cams[4]});
    CHECK(own != single_frames(s, {cams[4]}));
    CHECK(kifs_render_async(c, nullptr, plain, size_t(w) * 4, 0, h, 1) == KIFS_OK && equal_dev(plain, own));
    CHECK(A.run(c, nullptr, 10, 5, 0, h, false, &want) == KIFS_OK);
    CHECK(kifs_render_async(c, nullptr, plain, size_t(w) * 4, 0, h, 1) == KIFS_OK && equal_dev(plain, own));
    CHECK(A.run(c, nullptr, 0, 70, 0, h, false, &want) == KIFS_OK);
    CHECK(kifs_render_async(c, nullptr, plain, size_t(w) * 4, 0, h, 1) == KIFS_OK && equal_dev(plain, own));
    A.release();
    // bands with a padded pitch, the other encoding; an empty band enqueues nothing
    AnimationCall B{s, cams, opts, 0, 80};
    const auto want_b = animation_frames(s, cams, opts, 0);
    B.alloc();
    for (int count : {1, 5, 70}) {
        CHECK(B.run(c, nullptr, 70 - count, count, h / 3, h - 3, false, &want_b) == KIFS_OK);
        CHECK(B.run(c, nullptr, 0, count, 0, std::min(h, 9), false, &want_b) == KIFS_OK);
        const long calls = stub_calls(), launches = stub_launches();
        CHECK(B.run(c, nullptr, 0, count, h / 2, h / 2, false, &want_b) == KIFS_OK);
        CHECK(stub_launches() == launches && stub_calls() == calls);
    }
    B.release();
    CHECK(hipFree(plain) == hipSuccess);
    kifs_destroy(c);
}

// The rings: a call waits on the host for the launch that read its scene table four calls ago, not sooner; the view
// ring is the one kifs_render_batch_async uses; a call on another stream than the tile table's follows it once.
void animation_rings() {
    stub_trace_mark("animation_rings");
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(70, 7);
    const auto opts = morph(s.options, 70, 3);
    AnimationCall A{s, cams, opts};
    const auto want = animation_frames(s, cams, opts, 1);
    const auto want_plain = single_frames(s, cams);
    A.alloc();
    kifs_ctx* c = context_for(s, &cams[0]);
    const size_t fb = size_t(s.w) * s.h * 4;
    uint8_t* frames = dev_alloc(fb * 70);
    std::vector<uint8_t*> outs(70);
    for (int i = 0; i < 70; ++i) outs[size_t(i)] = frames + fb * size_t(i);
    CHECK(kifs_render_async(c, nullptr, frames, size_t(s.w) * 4, 0, s.h, 1) == KIFS_OK);  // (the tile table and its events exist)
    // six calls, no wait between them: slots 0..3 new, then slot 0's event, then slot 1's
    int slot_event[KIFS_ANIMATION_RING];
    for (int k = 0; k < 6; ++k) {
        const int events = stub_events_created();
        const long syncs = stub_event_synchronizes();
        CHECK(A.run(c, nullptr, k, 5, 0, s.h, false, &want) == KIFS_OK);
        if (k < KIFS_ANIMATION_RING) {
            CHECK(stub_events_created() == events + 1 && stub_event_synchronizes() == syncs);
            slot_event[k] = events + 1;
        } else {
            CHECK(stub_events_created() == events && stub_event_synchronizes() == syncs + 1);
            CHECK(stub_event_synchronizes_on(slot_event[k - KIFS_ANIMATION_RING]) == 1);
        }
    }
    // animated calls of 70 frames between batches of 70: one view ring, every slot waited for before it is rewritten
    for (int k = 0; k < 10; ++k) {
        const long syncs = stub_event_synchronizes();
        if (k % 3 == 1) {
            std::memset(frames, 0xEE, fb * 70);
            CHECK(kifs_render_batch_async(c, nullptr, 70, cams.data(), outs.data(), size_t(s.w) * 4, 0, s.h, 1) == KIFS_OK);
            CHECK(equal_dev(frames, want_plain));
            CHECK(stub_event_synchronizes() - syncs == (k >= 4 ? 1 : 0));  // its view slot's previous launch
        } else {
            CHECK(A.run(c, nullptr, 0, 70, 0, s.h, false, &want) == KIFS_OK);
            CHECK(stub_event_synchronizes() - syncs == (k >= 4 ? 2 : 1));  // the scene slot's, and the view slot's
        }
    }
    // the caller's stream after the context's, and back: one record on the stream left and one wait, once per change
    hipStream_t caller = nullptr;
    CHECK(hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) == hipSuccess);
    hipStream_t order[] = {nullptr, caller, caller, nullptr, nullptr, caller};
    hipStream_t previous = nullptr;
    CHECK(A.run(c, nullptr, 0, 5, 0, s.h, false, &want) == KIFS_OK);
    for (hipStream_t st : order) {
        const long waits = stub_stream_waits();
        CHECK(A.run(c, st, 0, 5, 0, s.h, false, &want) == KIFS_OK);
        CHECK(stub_stream_waits() - waits == (st != previous ? 1 : 0));
        previous = st;
    }
    CHECK(hipStreamDestroy(caller) == hipSuccess);
    kifs_destroy(c);
    CHECK(hipFree(frames) == hipSuccess);
    A.release();
}

void animation_refusals() {
    stub_trace_mark("animation_refusals");
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(3, 1);
    auto opts = morph(s.options, 3, 0);
    const size_t pitch = size_t(s.w) * 4, fb = pitch * s.h;
    uint8_t* dev = dev_alloc(fb * 3);
    std::memset(dev, 0xEE, fb * 3);
    uint8_t* outs[3] = {dev, dev + fb, dev + 2 * fb};
    kifs_ctx* c = context_for(s, &cams[0]);
    auto call = [&](kifs_ctx* ctx, int count, const KifsCameraUniform* cm, const KifsOptionsUniform* o, uint8_t* const* out, size_t p, int y0, int y1,
                    int encode) {
        const long calls = stub_calls(), launches = stub_launches();  // a refused call makes no HIP call and launches nothing
        const int st = kifs_render_animation_async(ctx, nullptr, count, cm, o, out, p, y0, y1, encode);
        CHECK(st != KIFS_OK && stub_calls() == calls && stub_launches() == launches);
        return st;
    };
    CHECK(call(nullptr, 3, cams.data(), opts.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), nullptr, outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), nullptr, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    uint8_t* null_out[3] = {dev, nullptr, dev}, *odd_out[3] = {dev, dev, dev + 1};
    CHECK(call(c, 3, cams.data(), opts.data(), null_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), odd_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 0, cams.data(), opts.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 513, cams.data(), opts.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch, 0, s.h, 2) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch, -1, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch, 0, s.h + 1, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch, 9, 8, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch - 4, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch + 2, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    {   // a pipeline that does not exist; frames that differ where they may not -- by bit pattern, padding apart
        auto o = opts;
        for (auto& f : o) f.fractal_group_id = 3;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o = opts; o[2].max_iterations += 1;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o = opts; o[1].max_distance *= 2.0f;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o = opts; o[1].is_heatmap = 1;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o = opts; o[2].fractal_group_id = 2;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o = opts; o[2].primitive_id = 3;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o = opts;
        for (auto& f : o) f.epsilon = 0.0f;
        o[1].epsilon = -0.0f;
        CHECK(call(c, 3, cams.data(), o.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
    CHECK(call(c, 3, cams.data(), opts.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    {   // no camera with cameras NULL; no screen
        kifs_ctx* bare = context_for(s, nullptr, false);
        CHECK(call(bare, 3, nullptr, opts.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
        int st = 0;
        bare = kifs_create(0, &st);
        CHECK(bare && call(bare, 3, cams.data(), opts.data(), outs, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
    }
    for (size_t i = 0; i < fb * 3; ++i)
        if (dev[i] != 0xEE) CHECK(false);
    // junk in the padding words is no difference: accepted, and the frames are those of the clean images
    auto junk = opts;
    junk[1]._padding1 = 0xdeadbeefu;
    junk[2]._padding2 = 0x12345678u;
    junk[0]._padding3 = 0xffffffffu;
    AnimationCall A{s, cams, junk};
    const auto want = animation_frames(s, cams, opts, 1);
    A.alloc();
    CHECK(A.run(c, nullptr, 0, 3, 0, s.h, false, &want) == KIFS_OK);
    A.release();
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess);
}

// Every HIP call and launch of an adaptive call of 70 views and of animated calls of 5 and of 70 frames fails once, in
// turn, on a fresh context and on a warm one (scratch, rings and tables allocated): the call reports KIFS_ERR_RUNTIME or
// absorbs the failure; KIFS_ANIMATION_RING + 1 more calls of its kind and a batch of 70 each return a status -- the rings
// come round to whatever slot the failure left half made -- and from the first that succeeds on every frame is exact;
// the destroy leaves nothing behind.
void extension_injected_failures(int w, int h) {
    stub_trace_mark("extension_injected_failures");
    const Scene s = scene(w, h, 10);
    const auto cams = cameras(70, 13);
    const auto opts = morph(s.options, 70, 1);
    AdaptiveCall A{s, cams, KifsAdaptiveAA{2, 5000.0f, 0.1f}};
    AnimationCall M{s, cams, opts};
    std::vector<uint32_t> counts;
    const auto want_adaptive = adaptive_frames(s, cams, A.aa, 1, &counts);
    const auto want_animation = animation_frames(s, cams, opts, 1);
    const auto want_plain = single_frames(s, cams);
    A.alloc();
    M.alloc();
    const size_t fb = size_t(w) * h * 4;
    uint8_t* frames = dev_alloc(fb * 70);
    std::vector<uint8_t*> outs(70);
    for (int i = 0; i < 70; ++i) outs[size_t(i)] = frames + fb * size_t(i);
    const size_t own_allocations = stub_live_device_allocations(), own_handles = stub_live_streams_and_events();
    for (int kind = 0; kind < 3; ++kind) {  // adaptive 70, animated 5, animated 70
        auto call = [&](kifs_ctx* c) {
            return kind == 0 ? A.run(c, nullptr, 0, 70, false, true, &want_adaptive, &counts)
                             : M.run(c, nullptr, 0, kind == 1 ? 5 : 70, 0, h, false, &want_animation);
        };
        for (int warm = 0; warm < 2; ++warm) {
            int failed = 0;
            for (long n = 1; n < 400; ++n) {
                kifs_ctx* c = context_for(s, &cams[0]);
                if (warm)
                    for (int k = 0; k < KIFS_ANIMATION_RING; ++k) CHECK(call(c) == KIFS_OK);
                const long before = stub_calls();
                stub_fail_in(n);
                const int st = call(c);  // (KIFS_OK: the frames have been compared)
                const bool reached = stub_calls() - before >= n;
                stub_fail_in(-1);
                CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
                if (st != KIFS_OK) ++failed;
                bool ok_seen = false;
                for (int k = 0; k < KIFS_ANIMATION_RING + 2; ++k) {
                    int again;
                    if (k == 2) {
                        std::memset(frames, 0xEE, fb * 70);
                        again = kifs_render_batch_async(c, nullptr, 70, cams.data(), outs.data(), size_t(w) * 4, 0, h, 1);
                        if (again == KIFS_OK) CHECK(equal_dev(frames, want_plain));
                    } else {
                        again = call(c);
                    }
                    CHECK(again == KIFS_OK || (again == KIFS_ERR_RUNTIME && !ok_seen));
                    ok_seen = ok_seen || again == KIFS_OK;
                }
                CHECK(ok_seen);
                kifs_destroy(c);
                CHECK(stub_live_device_allocations() == own_allocations && stub_live_streams_and_events() == own_handles);
                if (!reached) break;
            }
            CHECK(failed >= 3);  // (a warm animated call of 5 frames: the copy, the launch, the record)
        }
    }
    CHECK(hipFree(frames) == hipSuccess);
    M.release();
    A.release();
}

}  // namespace

int main() {
    null_and_argument_checks();
    single_context(333, 211);  // neither dimension a multiple of the 32 x 8 tile
    single_context(64, 8);
    for (int gather : {KIFS_GATHER_SPARSE, KIFS_GATHER_DENSE}) {
        multi_batches(333, 211, gather);
        multi_batches(96, 20, gather);
    }
    multi_pipeline(320, 200);
    multi_pipeline(70, 37);
    injected_failures(100, 50);
    context_lifecycle();
    launch_shapes();
    option_gates();
    adaptive_batches(333, 211);  // neither dimension a multiple of the 32 x 8 tile
    adaptive_batches(96, 20);  // (every camera sees a tile that holds something)
    adaptive_scratch();
    adaptive_streams();
    adaptive_scratch_cap();
    adaptive_refusals();
    animation_batches(333, 211);
    animation_batches(64, 8);
    animation_rings();
    animation_refusals();
    extension_injected_failures(100, 50);
    CHECK(stub_live_device_allocations() == 0);
    CHECK(stub_live_streams_and_events() == 0);
    std::printf("host_driver: %ld checks ok\n", g_checks);
    return 0;
}
