// accumulate_driver.cpp -- TEST INFRASTRUCTURE: drives the host side of kifs_render_accumulate_async
// (kifs_accumulate.cpp, with the seven other host units) against tests/hip_stub/hip_stub.cpp and accumulate_family_stub.cpp under
// AddressSanitizer + UndefinedBehaviorSanitizer (`make asan-accumulate`; tests/test_accumulate_host_sanitizers.py).
// A stand-alone CPU program: 1 x 1, 6 x 8, 8 x 64 (the view-table path) and 13 x 5 views, options NULL and given, bands
// with a padded pitch, two streams, the rings, every refusal, a failure injected into every HIP call and into the launch
// of an 8 x 64 call, and a final census of what is still alive.  The expected pixels are restated here from
// accumulate_model.hpp.  Prints "accumulate_driver: N checks ok".
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/kifs_hip.h"
#include "accumulate_model.hpp"

static long g_checks = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        ++g_checks;                                                                              \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "accumulate_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

#include "accumulate_driver_common.hpp"

namespace {

// One call's destinations, expectation and checks.  `opts` empty: options NULL, the context's options for every view.
struct Call {
    const Scene& s;
    int count, samples;
    const std::vector<KifsCameraUniform>& cams;
    const std::vector<KifsOptionsUniform>& opts;
    size_t pad = 0;
    uint8_t* dev = nullptr;

    size_t pitch() const { return size_t(s.w) * 4 + pad; }
    size_t bytes() const { return pitch() * size_t(s.h) * size_t(count) + 64; }
    void alloc() { dev = dev_alloc(bytes()); }
    void release() { CHECK(hipFree(dev) == hipSuccess); }
    uint32_t expected(int f, int x, int y) const {
        uint32_t acc = 0;
        for (int k = 0; k < samples; ++k) {
            const size_t v = size_t(f) * size_t(samples) + size_t(k);
            const uint32_t one = accumulate_model::sample(view_of(cams[v]), scene_of(opts.empty() ? s.options : opts[v]), x, y);
            acc = k == 0 ? one : accumulate_model::fold(acc, one);
        }
        return accumulate_model::pixel(acc, samples);
    }
    int run(kifs_ctx* c, hipStream_t stream, int y0, int y1, int encode = 1, bool compare = true) {
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        const size_t band = pitch() * size_t(y1 - y0);
        for (int f = 0; f < count; ++f) outs[size_t(f)] = dev + band * size_t(f);
        std::memset(dev, 0xEE, bytes());
        const long launches = family_stub_launches();
        const int st = kifs_render_accumulate_async(c, stream, count, samples, cams.data(), opts.empty() ? nullptr : opts.data(), outs.data(),
                                                    pitch(), y0, y1, encode);
        if (st != KIFS_OK || !compare) return st;
        if (y1 == y0) {
            CHECK(family_stub_launches() == launches);
        } else {
            CHECK(family_stub_launches() == launches + 1);
            CHECK(family_stub_last_params().B.count == count * samples && (family_stub_last_params().B.table ? 1 : 0) == (count * samples > 64 ? 1 : 0));
            CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ACCUMULATE && kifs_debug_last_round_steps(c) == 0);
            CHECK(kifs_debug_last_group_tiles(c) == -1 && kifs_debug_last_bunny_form(c) == -1);
        }
        for (int f = 0; f < count; ++f)
            for (int y = y0; y < y1; ++y) {
                const uint8_t* row = outs[size_t(f)] + pitch() * size_t(y - y0);
                for (int x = 0; x < s.w; ++x) {
                    uint32_t px;
                    std::memcpy(&px, row + 4 * size_t(x), 4);
                    if (px != expected(f, x, y)) CHECK(false);
                }
                for (size_t b = size_t(s.w) * 4; b < pitch(); ++b)
                    if (row[b] != 0xEE) CHECK(false);
            }
        ++g_checks;
        for (size_t b = band * size_t(count); b < bytes(); ++b)
            if (dev[b] != 0xEE) CHECK(false);
        return st;
    }
};

const int SHAPES[4][2] = {{1, 1}, {6, 8}, {8, 64}, {13, 5}};

void shapes(int w, int h) {
    const Scene s = scene(w, h, 40);
    const std::vector<KifsOptionsUniform> none;
    for (const auto& shape : SHAPES) {
        const int count = shape[0], samples = shape[1], views = count * samples;
        const auto cams = cameras(views, 3);
        const auto opts = morph(s.options, views, true);
        for (int given = 0; given < 2; ++given) {
            // options given: a context that never had kifs_set_options, and has none afterwards either
            kifs_ctx* c = context_for(s, !given);
            Call A{s, count, samples, cams, given ? opts : none};
            A.alloc();
            CHECK(A.run(c, nullptr, 0, h) == KIFS_OK);
            CHECK(A.run(c, nullptr, 0, h, 0) == KIFS_OK);
            A.release();
            Call B{s, count, samples, cams, given ? opts : none, 48};  // a band, a padded pitch
            B.alloc();
            CHECK(B.run(c, nullptr, h / 3, h - 3) == KIFS_OK);
            CHECK(B.run(c, nullptr, 0, std::min(h, 9)) == KIFS_OK);
            const long calls = stub_calls();
            CHECK(B.run(c, nullptr, h / 2, h / 2) == KIFS_OK && stub_calls() == calls);  // an empty band: nothing enqueued
            B.release();
            if (given) {
                std::vector<uint8_t> px(size_t(w) * 4);
                CHECK(kifs_set_camera(c, &cams[0]) == KIFS_OK);
                CHECK(kifs_render(c, px.data(), px.size(), 0, 1, 1) == KIFS_ERR_UNCONFIGURED);  // its options are still unset
            }
            kifs_destroy(c);
        }
    }
}

// Two streams and the rings: the scene ring is the animated call's (a call waits on the host for the launch that read its
// table KIFS_ANIMATION_RING calls ago), beyond 64 views the view ring too; a call on another stream than the tile table's
// follows it once per change.
void streams_and_rings() {
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(512, 1);
    const auto opts = morph(s.options, 512, true);
    kifs_ctx* c = context_for(s, true);
    Call A{s, 3, 4, cams, opts}, T{s, 8, 64, cams, opts};
    A.alloc();
    T.alloc();
    CHECK(A.run(c, nullptr, 0, s.h) == KIFS_OK);
    for (int k = 1; k < 7; ++k) {
        const long syncs = stub_event_synchronizes();
        CHECK(A.run(c, nullptr, 0, s.h) == KIFS_OK);
        CHECK(stub_event_synchronizes() - syncs == (k >= KIFS_ANIMATION_RING ? 1 : 0));
    }
    for (int k = 0; k < 6; ++k) {
        const long syncs = stub_event_synchronizes();
        CHECK(T.run(c, nullptr, 0, s.h) == KIFS_OK);
        CHECK(stub_event_synchronizes() - syncs == (k >= 4 ? 2 : 1));  // the scene slot's, and from the fifth the view slot's
    }
    // a mix with the animated call itself: one ring
    {
        std::vector<uint8_t*> outs(12);
        uint8_t* frames = dev_alloc(size_t(s.w) * s.h * 4 * 12);
        for (int i = 0; i < 12; ++i) outs[size_t(i)] = frames + size_t(s.w) * s.h * 4 * size_t(i);
        for (int k = 0; k < 6; ++k) {
            const long syncs = stub_event_synchronizes();
            CHECK(kifs_render_animation_async(c, nullptr, 12, cams.data(), opts.data(), outs.data(), size_t(s.w) * 4, 0, s.h, 1) == KIFS_OK);
            CHECK(stub_event_synchronizes() - syncs == 1);
            CHECK(A.run(c, nullptr, 0, s.h) == KIFS_OK);
        }
        CHECK(hipFree(frames) == hipSuccess);
    }
    hipStream_t one = nullptr, two = nullptr;
    CHECK(hipStreamCreateWithFlags(&one, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&two, hipStreamNonBlocking) == hipSuccess);
    hipStream_t order[] = {nullptr, one, one, two, nullptr, two, one};
    hipStream_t previous = nullptr;
    for (hipStream_t st : order) {
        const long waits = stub_stream_waits();
        CHECK((st == two ? T : A).run(c, st, 0, s.h) == KIFS_OK);
        CHECK(stub_stream_waits() - waits == (st != previous ? 1 : 0));
        previous = st;
    }
    CHECK(kifs_order_after(c, one, two) == KIFS_OK);
    CHECK(A.run(c, one, 0, s.h) == KIFS_OK);
    CHECK(hipStreamDestroy(one) == hipSuccess && hipStreamDestroy(two) == hipSuccess);
    kifs_destroy(c);
    A.release();
    T.release();
}

void refusals() {
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(513, 1);
    auto opts = morph(s.options, 513, true);
    const size_t pitch = size_t(s.w) * 4, fb = pitch * s.h;
    uint8_t* dev = dev_alloc(fb * 3);
    std::memset(dev, 0xEE, fb * 3);
    std::vector<uint8_t*> outs(513, dev);
    outs[1] = dev + fb;
    outs[2] = dev + 2 * fb;
    kifs_ctx* c = context_for(s, true);
    auto call = [&](kifs_ctx* ctx, int count, int samples, const KifsCameraUniform* cm, const KifsOptionsUniform* o, uint8_t* const* out, size_t p,
                    int y0, int y1, int encode) {
        const long calls = stub_calls(), launches = stub_launches() + family_stub_launches();  // a refused call makes no HIP call
        const int st = kifs_render_accumulate_async(ctx, nullptr, count, samples, cm, o, out, p, y0, y1, encode);
        CHECK(st != KIFS_OK && stub_calls() == calls && stub_launches() + family_stub_launches() == launches);
        return st;
    };
    const KifsCameraUniform* cm = cams.data();
    const KifsOptionsUniform* op = opts.data();
    uint8_t* const* out = outs.data();
    CHECK(call(nullptr, 3, 2, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, nullptr, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, nullptr, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    uint8_t* null_out[3] = {dev, nullptr, dev}, *odd_out[3] = {dev, dev, dev + 1};
    CHECK(call(c, 3, 2, cm, op, null_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, odd_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 0, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, -1, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, KIFS_MAX_ACCUMULATE + 1, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 0, 2, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, -3, 2, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 513, 1, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 9, 57, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);                 // 513 views
    CHECK(call(c, 0x7fffffff, 64, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);        // (no overflow on the way)
    CHECK(call(c, 3, 2, cm, op, out, pitch, 0, s.h, 2) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, out, pitch, -1, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, out, pitch, 0, s.h + 1, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, out, pitch, 9, 8, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, out, pitch - 4, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    CHECK(call(c, 3, 2, cm, op, out, pitch + 2, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    {   // a pipeline that does not exist; images that differ where they may not -- by bit pattern, padding apart
        std::vector<KifsOptionsUniform> o(opts.begin(), opts.begin() + 6);
        for (auto& f : o) f.fractal_group_id = 3;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o.assign(opts.begin(), opts.begin() + 6); o[4].max_iterations += 1;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o.assign(opts.begin(), opts.begin() + 6); o[5].max_distance *= 2.0f;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o.assign(opts.begin(), opts.begin() + 6); o[1].is_heatmap = 1;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o.assign(opts.begin(), opts.begin() + 6); o[2].fractal_group_id = 2;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o.assign(opts.begin(), opts.begin() + 6); o[3].primitive_id = 3;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        o.assign(opts.begin(), opts.begin() + 6);
        for (auto& f : o) f.epsilon = 0.0f;
        o[4].epsilon = -0.0f;
        CHECK(call(c, 3, 2, cm, o.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
    CHECK(call(c, 3, 2, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    {   // no options with options NULL; no screen
        kifs_ctx* bare = context_for(s, false);
        CHECK(call(bare, 3, 2, cm, nullptr, out, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
        int st = 0;
        bare = kifs_create(0, &st);
        CHECK(bare && call(bare, 3, 2, cm, op, out, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
    }
    for (size_t i = 0; i < fb * 3; ++i)
        if (dev[i] != 0xEE) CHECK(false);
    // junk in the padding words is no difference: accepted, and the frames are those of the clean images
    std::vector<KifsOptionsUniform> junk(opts.begin(), opts.begin() + 6);
    junk[1]._padding1 = 0xdeadbeefu;
    junk[2]._padding2 = 0x12345678u;
    junk[5]._padding3 = 0xffffffffu;
    Call A{s, 3, 2, cams, junk};
    A.alloc();
    CHECK(A.run(c, nullptr, 0, s.h) == KIFS_OK);
    A.release();
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess);
}

// Every HIP call of an 8 x 64 call fails once, in turn, and then its launch, on a fresh context and on a warm one (rings
// and tables allocated): the call reports KIFS_ERR_RUNTIME or absorbs the failure; KIFS_ANIMATION_RING + 1 more calls each
// return a status -- the rings come round to whatever slot the failure left half made -- and from the first that succeeds
// on every frame is exact; the destroy leaves nothing behind.
void injected_failures() {
    const Scene s = scene(40, 13, 10);
    const auto cams = cameras(512, 13);
    const auto opts = morph(s.options, 512, true);
    Call T{s, 8, 64, cams, opts};
    T.alloc();
    const size_t own_allocations = stub_live_device_allocations(), own_handles = stub_live_streams_and_events();
    for (int warm = 0; warm < 2; ++warm) {
        int failed = 0;
        for (long n = 0; n < 400; ++n) {  // n == 0: the launch itself
            kifs_ctx* c = context_for(s, true);
            if (warm)
                for (int k = 0; k < KIFS_ANIMATION_RING; ++k) CHECK(T.run(c, nullptr, 0, s.h) == KIFS_OK);
            const long before = stub_calls();
            if (n == 0) family_stub_fail_next();
            else stub_fail_in(n);
            const int st = T.run(c, nullptr, 0, s.h);  // (KIFS_OK: the frames have been compared)
            const bool reached = n == 0 || stub_calls() - before >= n;
            stub_fail_in(-1);
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
            if (n == 0) CHECK(st == KIFS_ERR_RUNTIME);
            if (st != KIFS_OK) ++failed;
            bool ok_seen = false;
            for (int k = 0; k < KIFS_ANIMATION_RING + 1; ++k) {
                const int again = T.run(c, nullptr, 0, s.h);
                CHECK(again == KIFS_OK || (again == KIFS_ERR_RUNTIME && !ok_seen));
                ok_seen = ok_seen || again == KIFS_OK;
            }
            CHECK(ok_seen);
            kifs_destroy(c);
            CHECK(stub_live_device_allocations() == own_allocations && stub_live_streams_and_events() == own_handles);
            if (!reached) break;
        }
        CHECK(failed >= 5);  // (a warm call: two copies, the launch, two records)
    }
    T.release();
}

}  // namespace

int main() {
    family_stub_expect_grid(1);  // the unjittered call: a launch with any other grid aborts in the stand-in
    shapes(74, 45);  // neither dimension a multiple of the 32 x 8 tile
    shapes(64, 8);
    streams_and_rings();
    refusals();
    injected_failures();
    CHECK(stub_live_device_allocations() == 0);
    CHECK(stub_live_streams_and_events() == 0);
    std::printf("accumulate_driver: %ld checks ok\n", g_checks);
    return 0;
}
