// accumulate_jitter_driver.cpp -- TEST INFRASTRUCTURE: drives the host side of kifs_render_accumulate_jittered_async
// (kifs_accumulate.cpp, with the seven other host units) against tests/hip_stub/hip_stub.cpp and
// accumulate_family_stub.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan-jitter`;
// tests/test_jitter_host_sanitizers.py).  A stand-alone CPU program: 1 x 1, 6 x 8, 8 x 64 (the view-table path), 13 x 5
// and 2 x 9 views at grids 1, 3 and 8, cells given and NULL (where samples == grid^2), options given and NULL, bands with
// a padded pitch; after every launch the recorded Params and scene table are checked view by view (pad[0], ssaa,
// ssaa_inv_height); unjittered calls between jittered ones (zero pad words, ssaa 1); every refusal; a failure injected
// into every HIP call and into the launch of an 8 x 64 call; and a final census of what is still alive.  The expected
// pixels are restated here from accumulate_model.hpp.  Prints "accumulate_jitter_driver: N checks ok".
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
#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        ++g_checks;                                                                                     \
        if (!(cond)) {                                                                                  \
            std::fprintf(stderr, "accumulate_jitter_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                               \
        }                                                                                               \
    } while (0)

#include "accumulate_driver_common.hpp"

namespace {

// One call's destinations, expectation and checks.  `opts` empty: options NULL.  grid 0: the UNJITTERED entry point.
// `cells` empty: cells NULL.
struct Call {
    const Scene& s;
    int count, samples;
    const std::vector<KifsCameraUniform>& cams;
    const std::vector<KifsOptionsUniform>& opts;
    int grid;
    std::vector<KifsSubpixel> cells;
    size_t pad = 0;
    uint8_t* dev = nullptr;

    size_t pitch() const { return size_t(s.w) * 4 + pad; }
    size_t bytes() const { return pitch() * size_t(s.h) * size_t(count) + 64; }
    void alloc() { dev = dev_alloc(bytes()); }
    void release() { CHECK(hipFree(dev) == hipSuccess); }
    int g() const { return grid > 0 ? grid : 1; }
    KifsSubpixel cell(size_t v) const {
        if (grid <= 1) return KifsSubpixel{0, 0};
        const int n = int(v % size_t(samples));
        return cells.empty() ? KifsSubpixel{uint8_t(n % grid), uint8_t(n / grid)} : cells[v];
    }
    uint32_t expected(int f, int x, int y) const {
        uint32_t acc = 0;
        for (int k = 0; k < samples; ++k) {
            const size_t v = size_t(f) * size_t(samples) + size_t(k);
            const KifsSubpixel at = cell(v);
            const uint32_t one = accumulate_model::sample(view_of(cams[v]), scene_of(opts.empty() ? s.options : opts[v]), g() * x + at.i,
                                                          g() * y + at.j);
            acc = k == 0 ? one : accumulate_model::fold(acc, one);
        }
        return accumulate_model::pixel(acc, samples);
    }
    int call(kifs_ctx* c, uint8_t* const* outs, int y0, int y1, int encode) const {
        const KifsOptionsUniform* o = opts.empty() ? nullptr : opts.data();
        if (grid == 0) return kifs_render_accumulate_async(c, nullptr, count, samples, cams.data(), o, outs, pitch(), y0, y1, encode);
        return kifs_render_accumulate_jittered_async(c, nullptr, count, samples, cams.data(), o, grid, cells.empty() ? nullptr : cells.data(),
                                                     outs, pitch(), y0, y1, encode);
    }
    int run(kifs_ctx* c, int y0, int y1, int encode = 1) {
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        const size_t band = pitch() * size_t(y1 - y0);
        for (int f = 0; f < count; ++f) outs[size_t(f)] = dev + band * size_t(f);
        std::memset(dev, 0xEE, bytes());
        const long launches = family_stub_launches();
        const int st = call(c, outs.data(), y0, y1, encode);
        if (st != KIFS_OK) return st;
        if (y1 == y0) {
            CHECK(family_stub_launches() == launches);
        } else {
            CHECK(family_stub_launches() == launches + 1);
            CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ACCUMULATE && kifs_debug_last_round_steps(c) == 0);
            CHECK(kifs_debug_last_group_tiles(c) == -1 && kifs_debug_last_bunny_form(c) == -1);
            // what the launch carried: the grid, the virtual screen's 1 / height, a cell per view
            const kifs::accum::Params& A = family_stub_last_params();
            const std::vector<kifs::anim::SceneView>& scenes = family_stub_last_scenes();
            const int views = count * samples;
            CHECK(A.frames == count && A.samples == samples && A.B.count == views && int(scenes.size()) == views);
            CHECK(A.B.frame.ssaa == g());
            CHECK(A.B.frame.ssaa_inv_height == 1.0f / (float(g()) * float(s.h)));
            CHECK(A.B.frame.height == float(s.h) && A.B.frame.inv_height == 1.0f / float(s.h));  // the OUTPUT frame's stay
            for (int v = 0; v < views; ++v) {
                const KifsSubpixel at = cell(size_t(v));
                if (scenes[size_t(v)].pad[0] != (uint32_t(at.i) | uint32_t(at.j) << 8)) CHECK(false);
                if (scenes[size_t(v)].pad[1] || scenes[size_t(v)].pad[2] || scenes[size_t(v)].pad[3]) CHECK(false);
            }
            ++g_checks;
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

const int SHAPES[5][2] = {{1, 1}, {6, 8}, {8, 64}, {13, 5}, {2, 9}};
const int GRIDS[3] = {1, 3, 8};

void shapes(int w, int h) {
    const Scene s = scene(w, h, 40);
    const std::vector<KifsOptionsUniform> none;
    int null_cells = 0;
    for (const auto& shape : SHAPES) {
        const int count = shape[0], samples = shape[1], views = count * samples;
        const auto cams = cameras(views, 3);
        const auto opts = morph(s.options, views);
        for (int given = 0; given < 2; ++given) {
            // options given: a context that never had kifs_set_options
            kifs_ctx* c = context_for(s, !given);
            Call plain{s, count, samples, cams, given ? opts : none, 0, {}};
            plain.alloc();
            for (const int g : GRIDS) {
                for (int with_cells = 1; with_cells >= 0; --with_cells) {
                    if (!with_cells && samples != g * g) continue;  // (refusals(): NULL with another number of samples)
                    null_cells += !with_cells;
                    Call A{s, count, samples, cams, given ? opts : none, g, with_cells ? cells_for(views, g) : std::vector<KifsSubpixel>()};
                    A.alloc();
                    CHECK(A.run(c, 0, h) == KIFS_OK);
                    CHECK(A.run(c, 0, h, 0) == KIFS_OK);
                    A.release();
                    // an unjittered call between jittered ones: zero pad words, a grid of 1
                    CHECK(plain.run(c, 0, h) == KIFS_OK);
                    Call B{s, count, samples, cams, given ? opts : none, g, with_cells ? cells_for(views, g) : std::vector<KifsSubpixel>(), 48};
                    B.alloc();
                    CHECK(B.run(c, h / 3, h - 3) == KIFS_OK);  // a band, a padded pitch: coordinates stay the frame's
                    const long calls = stub_calls();
                    CHECK(B.run(c, h / 2, h / 2) == KIFS_OK && stub_calls() == calls);  // an empty band: nothing enqueued
                    B.release();
                }
            }
            plain.release();
            kifs_destroy(c);
        }
    }
    CHECK(null_cells == 2 * 3);  // 1 x 1 at grid 1, 2 x 9 at grid 3, 8 x 64 at grid 8, with and without options
}

void refusals() {
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(513, 1);
    const auto opts = morph(s.options, 513);
    const size_t pitch = size_t(s.w) * 4, fb = pitch * s.h;
    uint8_t* dev = dev_alloc(fb * 3);
    std::memset(dev, 0xEE, fb * 3);
    std::vector<uint8_t*> outs(513, dev);
    outs[1] = dev + fb;
    outs[2] = dev + 2 * fb;
    kifs_ctx* c = context_for(s, true);
    const KifsCameraUniform* cm = cams.data();
    const KifsOptionsUniform* op = opts.data();
    uint8_t* const* out = outs.data();
    std::vector<KifsSubpixel> zero(513, KifsSubpixel{0, 0}), in3 = cells_for(6, 3);
    auto call = [&](kifs_ctx* ctx, int count, int samples, const KifsCameraUniform* cam, const KifsOptionsUniform* o, int grid,
                    const KifsSubpixel* cells, uint8_t* const* to, size_t p, int y0, int y1, int encode) {
        const long calls = stub_calls(), launches = stub_launches() + family_stub_launches();  // a refused call makes no HIP call
        const int st = kifs_render_accumulate_jittered_async(ctx, nullptr, count, samples, cam, o, grid, cells, to, p, y0, y1, encode);
        CHECK(st != KIFS_OK && stub_calls() == calls && stub_launches() + family_stub_launches() == launches);
        return st;
    };
    // the jittered call's own
    for (const int grid : {0, -1, KIFS_MAX_JITTER_GRID + 1, 0x7fffffff})
        CHECK(call(c, 3, 2, cm, op, grid, zero.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    for (int v = 0; v < 6; ++v) {  // a cell on the grid's edge, in either coordinate, at every view
        auto bad = in3;
        bad[size_t(v)].i = 3;
        CHECK(call(c, 3, 2, cm, op, 3, bad.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        bad = in3;
        bad[size_t(v)].j = 255;
        CHECK(call(c, 3, 2, cm, op, 3, bad.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    {
        auto one = zero;
        one[5].j = 1;  // grid 1: cells are (0, 0)
        CHECK(call(c, 3, 2, cm, op, 1, one.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    CHECK(call(c, 3, 2, cm, op, 3, nullptr, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);   // NULL: samples != 9
    CHECK(call(c, 3, 2, cm, op, 1, nullptr, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);   // NULL: samples != 1
    CHECK(call(c, 3, 8, cm, op, 3, nullptr, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 4, cm, op, 2, nullptr, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    // the unjittered call's, with their statuses
    CHECK(call(nullptr, 3, 2, cm, op, 3, in3.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, nullptr, op, 3, in3.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), nullptr, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    uint8_t* null_out[3] = {dev, nullptr, dev}, *odd_out[3] = {dev, dev, dev + 1};
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), null_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), odd_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 0, cm, op, 1, zero.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, KIFS_MAX_ACCUMULATE + 1, cm, op, 1, zero.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 0, 2, cm, op, 1, zero.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 513, 1, cm, op, 1, zero.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 0x7fffffff, 64, cm, op, 8, nullptr, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // (no overflow on the way)
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), out, pitch, 0, s.h, 2) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), out, pitch, -1, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), out, pitch, 0, s.h + 1, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), out, pitch - 4, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), out, pitch + 2, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    {
        std::vector<KifsOptionsUniform> o(opts.begin(), opts.begin() + 6);
        o[4].max_iterations += 1;
        CHECK(call(c, 3, 2, cm, o.data(), 3, in3.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    {   // no options with options NULL; no screen
        kifs_ctx* bare = context_for(s, false);
        CHECK(call(bare, 3, 2, cm, nullptr, 3, in3.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
        int st = 0;
        bare = kifs_create(0, &st);
        CHECK(bare && call(bare, 3, 2, cm, op, 3, in3.data(), out, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
    }
    {   // the virtual screen above 65536 in either dimension, as for supersampling
        const Scene wide = scene(8200, 1, 40), tall = scene(1, 8200, 40);
        for (const Scene* big : {&wide, &tall}) {
            kifs_ctx* b = context_for(*big, true);
            const size_t p = size_t(big->w) * 4;
            std::vector<KifsSubpixel> c8(2, KifsSubpixel{7, 7});
            CHECK(call(b, 1, 2, cm, nullptr, 8, c8.data(), out, p, 0, big->h, 1) == KIFS_ERR_BAD_SIZE);
            CHECK(call(b, 1, 64, cm, nullptr, 8, nullptr, out, p, 0, big->h, 1) == KIFS_ERR_BAD_SIZE);
            kifs_destroy(b);
        }
    }
    for (size_t i = 0; i < fb * 3; ++i)
        if (dev[i] != 0xEE) CHECK(false);
    // and the same arguments unrefused
    Call A{s, 3, 2, cams, opts, 3, in3};
    A.alloc();
    CHECK(A.run(c, 0, s.h) == KIFS_OK);
    A.release();
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess);
}

// Every HIP call of an 8 x 64 call at grid 8 fails once, in turn, and then its launch, on a fresh context and on a warm
// one: the call reports KIFS_ERR_RUNTIME or absorbs the failure; KIFS_ANIMATION_RING + 1 more calls each return a status and
// from the first that succeeds on every frame is exact; the destroy leaves nothing behind.
void injected_failures() {
    const Scene s = scene(40, 13, 10);
    const auto cams = cameras(512, 13);
    const auto opts = morph(s.options, 512);
    Call T{s, 8, 64, cams, opts, 8, cells_for(512, 8)};
    T.alloc();
    const size_t own_allocations = stub_live_device_allocations(), own_handles = stub_live_streams_and_events();
    for (int warm = 0; warm < 2; ++warm) {
        int failed = 0;
        for (long n = 0; n < 400; ++n) {  // n == 0: the launch itself
            kifs_ctx* c = context_for(s, true);
            if (warm)
                for (int k = 0; k < KIFS_ANIMATION_RING; ++k) CHECK(T.run(c, 0, s.h) == KIFS_OK);
            const long before = stub_calls();
            if (n == 0) family_stub_fail_next();
            else stub_fail_in(n);
            const int st = T.run(c, 0, s.h);  // (KIFS_OK: the frames have been compared)
            const bool reached = n == 0 || stub_calls() - before >= n;
            stub_fail_in(-1);
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
            if (n == 0) CHECK(st == KIFS_ERR_RUNTIME);
            if (st != KIFS_OK) ++failed;
            bool ok_seen = false;
            for (int k = 0; k < KIFS_ANIMATION_RING + 1; ++k) {
                const int again = T.run(c, 0, s.h);
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
    shapes(74, 45);  // neither dimension a multiple of the 32 x 8 tile
    shapes(64, 8);
    refusals();
    injected_failures();
    CHECK(stub_live_device_allocations() == 0);
    CHECK(stub_live_streams_and_events() == 0);
    std::printf("accumulate_jitter_driver: %ld checks ok\n", g_checks);
    return 0;
}
