// converge_driver.cpp -- TEST INFRASTRUCTURE: drives the host side of kifs_render_accumulate_converge_async
// (kifs_converge.cpp on top of kifs_accumulate.cpp, with kifs_progressive.cpp and the seven other host units) against
// tests/hip_stub/hip_stub.cpp and accumulate_family_stub.cpp under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make asan-converge`; tests/test_converge_host_sanitizers.py).  A stand-alone CPU program: frames of 1 x 2, 6 x 8,
// 8 x 64 and 13 x 5 views per pass (8 x 64 and 13 x 5: the view-table path) as sequences of three passes over one pair
// of planes, the first restarting over planes of 0xEE bytes or continuing from seeded planes; a picture from every pass,
// the last or none; counts given (pre-filled with garbage: the stand-in refuses a word the library did not zero before
// the launch) or NULL; bands with padded pitches on all three destinations; passes alternating between two streams and
// two contexts that share the planes; the tolerance tightened between passes; after every pass the recorded
// ConvergeParams, both planes, the picture and the counts are checked against converge_model.hpp restated here, and an
// existing resume call and an existing jittered call on the same context still give their texels and pixels; every
// refusal, with nothing launched and no HIP call made; a failure injected into every HIP call and into the launch of an
// 8 x 64 pass; the animated call and the four accumulated ones in one sequence on one context (shared_launch_path: the
// only driver that links them all), with a failure injected at every HIP call of it; and a final census of what is
// still alive.  Prints "converge_driver: N checks ok".
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/kifs_hip.h"
#include "converge_model.hpp"

static long g_checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        ++g_checks;                                                                                  \
        if (!(cond)) {                                                                               \
            std::fprintf(stderr, "converge_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

#include "accumulate_driver_common.hpp"

namespace {

enum Picture { EVERY, LAST, NEVER };

// A converging frame: `count` frames of three passes of `n` sub-frames, view f * 3 n + k the k-th sub-frame of frame f.
// `opts` empty: options NULL.
struct Frame {
    const Scene& s;
    int count, n;
    const std::vector<KifsCameraUniform>& cams;
    const std::vector<KifsOptionsUniform>& opts;
    int grid;
    std::vector<KifsSubpixel> cells;
    size_t pad = 0;        // bytes behind a picture row; 4 x and 1 x as many behind a row of the sums and of the moments
    uint8_t* dev = nullptr;      // the pictures
    uint8_t* plane = nullptr;    // the sums
    uint8_t* moments = nullptr;  // the moments
    uint32_t* counts = nullptr;  // count + 2 words: a guard on either side
    uint8_t* side = nullptr;     // what the existing calls made between the passes write: a picture and a plane

    size_t pitch() const { return size_t(s.w) * 4 + pad; }
    size_t plane_pitch() const { return size_t(s.w) * 16 + 4 * pad; }
    size_t moments_pitch() const { return size_t(s.w) * 4 + pad; }
    size_t bytes() const { return pitch() * size_t(s.h) * size_t(count) + 64; }
    size_t plane_bytes() const { return (plane_pitch() * size_t(s.h) + 4 * pad) * size_t(count) + 64; }
    size_t moments_bytes() const { return (moments_pitch() * size_t(s.h) + pad) * size_t(count) + 64; }
    void alloc() {
        dev = dev_alloc(bytes());
        plane = dev_alloc(plane_bytes());
        moments = dev_alloc(moments_bytes());
        counts = reinterpret_cast<uint32_t*>(dev_alloc(size_t(count + 2) * 4));
        side = dev_alloc(size_t(s.w) * 20 * size_t(s.h) * size_t(count));
    }
    void release() {
        CHECK(hipFree(dev) == hipSuccess && hipFree(plane) == hipSuccess && hipFree(moments) == hipSuccess);
        CHECK(hipFree(counts) == hipSuccess && hipFree(side) == hipSuccess);
    }
    uint32_t sample(size_t v, int x, int y) const {
        const KifsSubpixel at = cells[v];
        return accumulate_model::sample(view_of(cams[v]), scene_of(opts.empty() ? s.options : opts[v]), grid * x + at.i, grid * y + at.j);
    }
    // An existing resume call (a plane of its own, prior 0) and an existing jittered call on the same context between two
    // passes: the pass's own views.
    void existing_calls(kifs_ctx* c, const std::vector<KifsCameraUniform>& pc, const std::vector<KifsOptionsUniform>& po,
                        const std::vector<KifsSubpixel>& pcells, int first) {
        const size_t sp = size_t(s.w) * 4, tp = size_t(s.w) * 16;
        uint8_t* const texels = side;  // (16-byte aligned: the pictures come behind it)
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        for (int f = 0; f < count; ++f) outs[size_t(f)] = side + tp * size_t(s.h) * size_t(count) + sp * size_t(s.h) * size_t(f);
        const KifsOptionsUniform* o = po.empty() ? nullptr : po.data();
        const long converges = family_stub_converges(), carries = family_stub_carries(), launches = family_stub_launches();
        CHECK(kifs_render_accumulate_resume_async(c, nullptr, count, n, pc.data(), o, grid, pcells.data(), reinterpret_cast<float*>(texels), tp,
                                                  tp * size_t(s.h), 0, nullptr, 0, 0, s.h, 1) == KIFS_OK);
        CHECK(kifs_render_accumulate_jittered_async(c, nullptr, count, n, pc.data(), o, grid, pcells.data(), outs.data(), sp, 0, s.h, 1) == KIFS_OK);
        CHECK(family_stub_converges() == converges && family_stub_carries() == carries + 1 && family_stub_launches() == launches + 2);
        for (int f = 0; f < count; ++f)
            for (int y = 0; y < s.h; y += 3)
                for (int x = 0; x < s.w; x += 5) {
                    uint32_t px, t[4], acc = 0;
                    std::memcpy(&px, outs[size_t(f)] + sp * size_t(y) + 4 * size_t(x), 4);
                    std::memcpy(t, texels + tp * size_t(s.h) * size_t(f) + tp * size_t(y) + 16 * size_t(x), 16);
                    for (int k = 0; k < n; ++k) {
                        const uint32_t one = sample(size_t(f) * size_t(3 * n) + size_t(first + k), x, y);
                        acc = k == 0 ? one : accumulate_model::fold(acc, one);
                    }
                    if (px != accumulate_model::pixel(acc, n) || t[0] != acc || t[3] != accumulate_model::bits(float(n))) CHECK(false);
                }
        ++g_checks;
    }
    // Three passes in turn on ctxs[p % size] and streams[p % size] (null: the context's stream) under rules[p].  `seeded`:
    // the planes hold a state before pass 0, which then does not restart; otherwise they hold 0xEE bytes and it does.
    // Returns the first status that is not KIFS_OK, or KIFS_OK with everything checked after every pass.
    int run(const std::vector<kifs_ctx*>& ctxs, const std::vector<hipStream_t>& streams, int y0, int y1, bool seeded, Picture picture,
            bool with_counts, const KifsConvergence (&rules)[3], int encode = 1, bool between = false) {
        const int rows = y1 - y0;
        const size_t band = pitch() * size_t(rows), stride = plane_pitch() * size_t(rows) + 4 * pad,
                     mstride = moments_pitch() * size_t(rows) + pad;
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        for (int f = 0; f < count; ++f) outs[size_t(f)] = dev + band * size_t(f);
        std::memset(dev, 0xEE, bytes());
        std::memset(plane, 0xEE, plane_bytes());
        std::memset(moments, 0xEE, moments_bytes());
        // the model's copy of the state, and whether a pixel has been written at all
        std::vector<converge_model::Pixel> state(size_t(count) * size_t(rows) * size_t(s.w));
        std::vector<char> written(state.size(), 0);
        auto at = [&](int f, int y, int x) { return (size_t(f) * size_t(rows) + size_t(y - y0)) * size_t(s.w) + size_t(x); };
        if (seeded)
            for (int f = 0; f < count; ++f)
                for (int y = y0; y < y1; ++y)
                    for (int x = 0; x < s.w; ++x) {
                        converge_model::Pixel& p = state[at(f, y, x)];
                        p.acc = 0x9e3779b9u * uint32_t(f + 1) ^ uint32_t(x) * 2654435761u ^ uint32_t(y) * 40503u;
                        p.q = p.acc * 13u + 5u;
                        p.n = (x + y) % 11 == 0 ? 16777216.0f - float(n) - float((x / 11) % 2) : float(2 + (x * 7 + y) % 9);
                        uint8_t* t = plane + stride * size_t(f) + plane_pitch() * size_t(y - y0) + 16 * size_t(x);
                        const uint32_t words[3] = {p.acc, 0x11111111u, 0x22222222u};
                        std::memcpy(t, words, 12);
                        std::memcpy(t + 12, &p.n, 4);
                        std::memcpy(moments + mstride * size_t(f) + moments_pitch() * size_t(y - y0) + 4 * size_t(x), &p.q, 4);
                    }
        int last_picture = -1;
        std::vector<uint32_t> shown(state.size(), 0xEEEEEEEEu);
        for (int p = 0; p < 3; ++p) {
            std::vector<KifsCameraUniform> pc;
            std::vector<KifsOptionsUniform> po;
            std::vector<KifsSubpixel> pcells;
            for (int f = 0; f < count; ++f)
                for (int k = 0; k < n; ++k) {
                    const size_t v = size_t(f) * size_t(3 * n) + size_t(p * n + k);
                    pc.push_back(cams[v]);
                    if (!opts.empty()) po.push_back(opts[v]);
                    pcells.push_back(cells[v]);
                }
            kifs_ctx* c = ctxs[size_t(p) % ctxs.size()];
            hipStream_t stream = streams[size_t(p) % streams.size()];
            if (p > 0 && streams.size() > 1)  // the caller orders passes on different streams
                CHECK(kifs_order_after(c, stream, streams[size_t(p - 1) % streams.size()]) == KIFS_OK);
            const bool with_picture = picture == EVERY || (picture == LAST && p == 2);
            const bool restart = p == 0 && !seeded;
            for (int f = 0; f < count + 2; ++f) counts[f] = 0xEEEEEEEEu;  // garbage: the library zeroes its words
            const long converges = family_stub_converges(), launches = family_stub_launches(), calls = stub_calls();
            const int st = kifs_render_accumulate_converge_async(
                c, stream, count, n, pc.data(), po.empty() ? nullptr : po.data(), grid, pcells.data(), reinterpret_cast<float*>(plane),
                plane_pitch(), stride, reinterpret_cast<float*>(moments), moments_pitch(), mstride, restart ? 7 : 0, &rules[p],
                with_counts ? counts + 1 : nullptr, with_picture ? outs.data() : nullptr, with_picture ? pitch() : 1, y0, y1, encode);
            if (st != KIFS_OK) return st;
            CHECK(counts[0] == 0xEEEEEEEEu && counts[count + 1] == 0xEEEEEEEEu);
            if (rows == 0) {  // an empty band: nothing enqueued, the counts untouched
                CHECK(family_stub_launches() == launches && stub_calls() == calls);
                for (int f = 0; f < count; ++f) CHECK(counts[f + 1] == 0xEEEEEEEEu);
                continue;
            }
            CHECK(family_stub_converges() == converges + 1 && family_stub_launches() == launches + 1);
            CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ACCUMULATE && kifs_debug_last_round_steps(c) == 0);
            const kifs::accum::ConvergeParams& K = family_stub_last_converge();
            CHECK(K.sums == reinterpret_cast<float*>(plane) && K.sums_pitch_texels == plane_pitch() / 16 && K.sums_stride_texels == stride / 16);
            CHECK(K.moments == reinterpret_cast<float*>(moments) && K.moments_pitch_words == moments_pitch() / 4 && K.moments_stride_words == mstride / 4);
            CHECK(K.restart == (restart ? 1u : 0u) && K.picture == (with_picture ? 1u : 0u) && K.min_samples == rules[p].min_samples);
            CHECK(accumulate_model::bits(K.tol2) == accumulate_model::bits(rules[p].tolerance * rules[p].tolerance));
            CHECK(K.counts == (with_counts ? counts + 1 : nullptr));
            CHECK(K.A.frames == count && K.A.samples == n && K.A.B.count == count * n && K.A.B.frame.ssaa == grid);
            CHECK(K.A.B.frame.y0 == y0 && K.A.B.frame.y1 == y1 && K.A.B.frame.encode == encode);
            CHECK(with_picture ? K.A.B.frame.pitch_words == pitch() / 4 && K.A.B.frame.out == reinterpret_cast<uint32_t*>(outs[0])
                               : K.A.B.frame.pitch_words == 0 && K.A.B.frame.out == nullptr);
            // the model's pass, then everything against it
            const float tol2 = rules[p].tolerance * rules[p].tolerance;
            std::vector<uint32_t> left(size_t(count), 0u);
            for (int f = 0; f < count; ++f)
                for (int y = y0; y < y1; ++y)
                    for (int x = 0; x < s.w; ++x) {
                        converge_model::Pixel& px = state[at(f, y, x)];
                        if (restart || converge_model::active(px, rules[p].min_samples, tol2, n)) {
                            if (restart) px = converge_model::Pixel{};
                            for (int k = 0; k < n; ++k)
                                converge_model::add(px, sample(size_t(f) * size_t(3 * n) + size_t(p * n + k), x, y), k == 0 && restart);
                            px.n += float(n);
                            written[at(f, y, x)] = 1;
                        }
                        if (converge_model::active(px, rules[p].min_samples, tol2, n)) ++left[size_t(f)];
                        if (with_picture) shown[at(f, y, x)] = accumulate_model::pixel(px.acc, int(px.n));
                    }
            if (with_picture) last_picture = p;
            for (int f = 0; f < count; ++f) {
                if (with_counts) CHECK(counts[f + 1] == left[size_t(f)]);
                else CHECK(counts[f + 1] == 0xEEEEEEEEu);
                for (int y = y0; y < y1; ++y) {
                    const uint8_t* trow = plane + stride * size_t(f) + plane_pitch() * size_t(y - y0);
                    const uint8_t* mrow = moments + mstride * size_t(f) + moments_pitch() * size_t(y - y0);
                    const uint8_t* row = outs[size_t(f)] + pitch() * size_t(y - y0);
                    for (int x = 0; x < s.w; ++x) {
                        const converge_model::Pixel& px = state[at(f, y, x)];
                        uint32_t t[4], q, shade;
                        std::memcpy(t, trow + 16 * size_t(x), 16);
                        std::memcpy(&q, mrow + 4 * size_t(x), 4);
                        std::memcpy(&shade, row + 4 * size_t(x), 4);
                        if (written[at(f, y, x)]) {
                            if (t[0] != px.acc || t[1] != ~px.acc || t[2] != px.acc * 3u) CHECK(false);
                        } else if (seeded) {  // never active: the seeded words, all of them
                            if (t[0] != px.acc || t[1] != 0x11111111u || t[2] != 0x22222222u) CHECK(false);
                        }
                        if (t[3] != accumulate_model::bits(px.n) || q != px.q || shade != shown[at(f, y, x)]) CHECK(false);
                    }
                    for (size_t b = size_t(s.w) * 16; b < plane_pitch(); ++b)
                        if (trow[b] != 0xEE) CHECK(false);
                    for (size_t b = size_t(s.w) * 4; b < moments_pitch(); ++b)
                        if (mrow[b] != 0xEE || row[b] != 0xEE) CHECK(false);
                }
            }
            ++g_checks;
            if (between) existing_calls(c, pc, po, pcells, p * n);
        }
        (void)last_picture;
        for (int f = 0; f < count && rows > 0; ++f) {  // behind every frame's rows, and behind the last frame
            for (size_t b = stride * size_t(f) + plane_pitch() * size_t(rows); b < (f + 1 < count ? stride * size_t(f + 1) : plane_bytes()); ++b)
                if (plane[b] != 0xEE) CHECK(false);
            for (size_t b = mstride * size_t(f) + moments_pitch() * size_t(rows); b < (f + 1 < count ? mstride * size_t(f + 1) : moments_bytes()); ++b)
                if (moments[b] != 0xEE) CHECK(false);
        }
        for (size_t b = band * size_t(count); b < bytes(); ++b)
            if (dev[b] != 0xEE) CHECK(false);
        return KIFS_OK;
    }
};

const float INF = std::numeric_limits<float>::infinity();
const KifsConvergence LOOSE[3] = {{0.5f, 4u}, {0.5f, 4u}, {0.5f, 4u}};
const KifsConvergence TIGHTENED[3] = {{0.75f, 2u}, {0.25f, 2u}, {0.0f, 2u}};
const KifsConvergence NEVER_SETTLES[3] = {{0.5f, 1u << 24}, {INF, 1u << 24}, {0.5f, 1u << 24}};
const KifsConvergence ALL_AT_ONCE[3] = {{INF, 2u}, {INF, 2u}, {INF, 2u}};

// {frames, sub-frames per pass}
const int SHAPES[4][2] = {{1, 2}, {6, 8}, {8, 64}, {13, 5}};

void shapes(int w, int h) {
    const Scene s = scene(w, h, 40);
    const std::vector<KifsOptionsUniform> none;
    hipStream_t extra[2] = {nullptr, nullptr};
    for (hipStream_t& e : extra) CHECK(hipStreamCreateWithFlags(&e, hipStreamNonBlocking) == hipSuccess);
    for (const auto& shape : SHAPES) {
        const int count = shape[0], n = shape[1], views = count * 3 * n;
        const auto cams = cameras(views, 3);
        const auto opts = morph(s.options, views);
        for (int given = 0; given < 2; ++given) {
            kifs_ctx* a = context_for(s, !given);  // options given: contexts that never had kifs_set_options
            kifs_ctx* b = context_for(s, !given);
            const std::vector<kifs_ctx*> one = {a}, two = {a, b};
            const std::vector<hipStream_t> own = {nullptr}, both = {extra[0], extra[1]};
            for (const int g : {1, 3, 8}) {
                Frame F{s, count, n, cams, given ? opts : none, g, g == 1 ? std::vector<KifsSubpixel>(size_t(views), KifsSubpixel{0, 0}) : cells_for(views, g, false)};
                F.alloc();
                CHECK(F.run(one, own, 0, h, false, EVERY, true, LOOSE, 1, g == 3) == KIFS_OK);
                CHECK(F.run(one, own, 0, h, true, LAST, true, TIGHTENED, 0) == KIFS_OK);
                CHECK(F.run(one, own, 0, h, false, NEVER, false, NEVER_SETTLES) == KIFS_OK);
                CHECK(F.run(one, own, 0, h, false, EVERY, true, ALL_AT_ONCE) == KIFS_OK);  // passes 2 and 3: nothing active
                CHECK(F.run(two, own, 0, h, false, LAST, true, LOOSE) == KIFS_OK);         // two contexts on one pair of planes
                CHECK(F.run(one, both, 0, h, true, EVERY, false, LOOSE) == KIFS_OK);       // two streams
                CHECK(F.run(two, both, 0, h, false, NEVER, true, TIGHTENED, 1, g == 8 && n == 5) == KIFS_OK);
                F.release();
                Frame B{s, count, n, cams, given ? opts : none, g, F.cells, 12};
                B.alloc();
                CHECK(B.run(one, own, h / 3, h - 3, false, LAST, true, LOOSE) == KIFS_OK);  // a band, padded pitches on all three
                CHECK(B.run(two, both, h / 3, h - 3, true, EVERY, true, TIGHTENED, 0) == KIFS_OK);
                CHECK(B.run(one, own, h / 2, h / 2, false, EVERY, true, LOOSE) == KIFS_OK);  // an empty band: nothing enqueued
                B.release();
            }
            kifs_destroy(a);
            kifs_destroy(b);
        }
    }
    for (hipStream_t e : extra) CHECK(hipStreamDestroy(e) == hipSuccess);
}

void refusals() {
    const Scene s = scene(100, 50, 40);
    const auto cams = cameras(513, 1);
    const auto opts = morph(s.options, 513);
    const size_t pitch = size_t(s.w) * 4, fb = pitch * s.h, pp = size_t(s.w) * 16, pb = pp * s.h, mp = pitch, mb = fb;
    uint8_t* dev = dev_alloc(fb * 3);
    uint8_t* plane = dev_alloc(pb * 3 + 64);
    uint8_t* mom = dev_alloc(mb * 3 + 64);
    uint32_t* counts = reinterpret_cast<uint32_t*>(dev_alloc(12));
    std::memset(dev, 0xEE, fb * 3);
    std::memset(plane, 0xEE, pb * 3 + 64);
    std::memset(mom, 0xEE, mb * 3 + 64);
    std::memset(counts, 0xEE, 12);
    std::vector<uint8_t*> outs(513, dev);
    outs[1] = dev + fb;
    outs[2] = dev + 2 * fb;
    kifs_ctx* c = context_for(s, true);
    const KifsCameraUniform* cm = cams.data();
    const KifsOptionsUniform* op = opts.data();
    uint8_t* const* out = outs.data();
    float* sums = reinterpret_cast<float*>(plane);
    float* q = reinterpret_cast<float*>(mom);
    const KifsConvergence good{0.25f, 4u};
    std::vector<KifsSubpixel> zero(513, KifsSubpixel{0, 0}), in3 = cells_for(6, 3, false);
    struct Args {
        kifs_ctx* ctx;
        int count, samples;
        const KifsCameraUniform* cam;
        const KifsOptionsUniform* o;
        int grid;
        const KifsSubpixel* cells;
        float* sums;
        size_t sp, ss;
        float* q;
        size_t qp, qs;
        int restart;
        const KifsConvergence* rule;
        uint32_t* counts;
        uint8_t* const* to;
        size_t p;
        int y0, y1, encode;
    };
    const Args ok{c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, q, mp, mb, 0, &good, counts, out, pitch, 0, s.h, 1};
    auto call = [&](const Args& a) {
        const long calls = stub_calls(), launches = stub_launches() + family_stub_launches();  // a refused call makes no HIP call
        const int st = kifs_render_accumulate_converge_async(a.ctx, nullptr, a.count, a.samples, a.cam, a.o, a.grid, a.cells, a.sums, a.sp, a.ss, a.q,
                                                             a.qp, a.qs, a.restart, a.rule, a.counts, a.to, a.p, a.y0, a.y1, a.encode);
        CHECK(st != KIFS_OK && stub_calls() == calls && stub_launches() + family_stub_launches() == launches);
        return st;
    };
    auto with = [&](auto change) {
        Args a = ok;
        change(a);
        return call(a);
    };
    // the resume call's, with their statuses
    for (const int grid : {0, -1, KIFS_MAX_JITTER_GRID + 1, 0x7fffffff})
        CHECK(with([&](Args& a) { a.grid = grid; a.cells = zero.data(); }) == KIFS_ERR_BAD_ARG);
    for (int v = 0; v < 6; ++v) {
        auto bad = in3;
        bad[size_t(v)].i = 3;
        CHECK(with([&](Args& a) { a.cells = bad.data(); }) == KIFS_ERR_BAD_ARG);
    }
    CHECK(with([&](Args& a) { a.cells = nullptr; }) == KIFS_ERR_BAD_ARG);  // NULL: samples != 9
    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
    CHECK(call(ok) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    CHECK(with([&](Args& a) { a.ctx = nullptr; }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.cam = nullptr; }) == KIFS_ERR_BAD_ARG);
    uint8_t* null_out[3] = {dev, nullptr, dev}, *odd_out[3] = {dev, dev, dev + 1};
    CHECK(with([&](Args& a) { a.to = null_out; }) == KIFS_ERR_BAD_ARG);  // an ENTRY of a given array
    CHECK(with([&](Args& a) { a.to = odd_out; }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.samples = 0; a.grid = 1; a.cells = zero.data(); }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.samples = KIFS_MAX_ACCUMULATE + 1; a.grid = 1; a.cells = zero.data(); }) == KIFS_ERR_BAD_ARG);  // per pass
    CHECK(with([&](Args& a) { a.count = 0; }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.count = 513; a.samples = 1; a.grid = 1; a.cells = zero.data(); }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.encode = 2; }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.y0 = -1; }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.y1 = s.h + 1; a.to = nullptr; }) == KIFS_ERR_BAD_ARG);
    CHECK(with([&](Args& a) { a.p = pitch - 4; }) == KIFS_ERR_BAD_SIZE);
    CHECK(with([&](Args& a) { a.p = pitch - 4; a.q = nullptr; a.rule = nullptr; }) == KIFS_ERR_BAD_SIZE);  // the shared checks come first
    {
        std::vector<KifsOptionsUniform> o(opts.begin(), opts.begin() + 6);
        o[4].max_iterations += 1;
        CHECK(with([&](Args& a) { a.o = o.data(); }) == KIFS_ERR_BAD_ARG);
    }
    {
        kifs_ctx* bare = context_for(s, false);
        CHECK(with([&](Args& a) { a.ctx = bare; a.o = nullptr; }) == KIFS_ERR_UNCONFIGURED);
        CHECK(with([&](Args& a) { a.ctx = bare; a.o = nullptr; a.rule = nullptr; }) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
    }
    // the call's own, with a picture and without, restarting and not
    for (int variant = 0; variant < 4; ++variant) {
        auto own = [&](auto change) {
            return with([&](Args& a) {
                if (variant & 1) a.to = nullptr;
                if (variant & 2) a.restart = 1;
                change(a);
            });
        };
        CHECK(own([&](Args& a) { a.sums = nullptr; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.sums = reinterpret_cast<float*>(plane + 8); }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.sp = pp - 16; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.ss = pb - 16; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.q = nullptr; }) == KIFS_ERR_BAD_ARG);
        for (const size_t off : {size_t(1), size_t(2), size_t(3)})
            CHECK(own([&](Args& a) { a.q = reinterpret_cast<float*>(mom + off); }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.qp = mp - 4; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.qp = mp + 2; a.qs = mb + 2 * s.h; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.qp = 0; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.qs = mb + 2; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.qs = mb - 4; }) == KIFS_ERR_BAD_ARG);  // frames would overlap
        CHECK(own([&](Args& a) { a.qs = 0; }) == KIFS_ERR_BAD_ARG);
        CHECK(own([&](Args& a) { a.rule = nullptr; }) == KIFS_ERR_BAD_ARG);
        for (const KifsConvergence bad : {KifsConvergence{std::nanf(""), 4u}, KifsConvergence{-0.25f, 4u}, KifsConvergence{-INF, 4u},
                                          KifsConvergence{0.25f, 1u}, KifsConvergence{0.25f, 0u}, KifsConvergence{0.25f, (1u << 24) + 1u},
                                          KifsConvergence{0.25f, 0xffffffffu}})
            CHECK(own([&](Args& a) { a.rule = &bad; }) == KIFS_ERR_BAD_ARG);
    }
    for (size_t i = 0; i < fb * 3; ++i)
        if (dev[i] != 0xEE) CHECK(false);
    for (size_t i = 0; i < pb * 3 + 64; ++i)
        if (plane[i] != 0xEE) CHECK(false);
    for (size_t i = 0; i < mb * 3 + 64; ++i)
        if (mom[i] != 0xEE) CHECK(false);
    CHECK(counts[0] == 0xEEEEEEEEu && counts[1] == 0xEEEEEEEEu && counts[2] == 0xEEEEEEEEu);
    CHECK(hipFree(dev) == hipSuccess && hipFree(plane) == hipSuccess && hipFree(mom) == hipSuccess && hipFree(counts) == hipSuccess);
    // and the same arguments unrefused, the rule at its limits
    const KifsConvergence limits[3] = {{0.0f, 2u}, {INF, 1u << 24}, {0.0f, 2u}};
    Frame A{s, 3, 2, cams, opts, 3, cells_for(18, 3, false)};
    A.alloc();
    CHECK(A.run({c}, {nullptr}, 0, s.h, false, LAST, true, limits) == KIFS_OK);
    A.release();
    kifs_destroy(c);
}

// Every HIP call of an 8 x 64 pass fails once, in turn, and then its launch, on a fresh context and on a warm one: the call
// reports KIFS_ERR_RUNTIME or absorbs the failure; KIFS_ANIMATION_RING + 1 more runs each return a status and from the
// first that succeeds on everything is exact; the destroy leaves nothing behind.
void injected_failures() {
    const Scene s = scene(40, 13, 10);
    const auto cams = cameras(8 * 3 * 64, 13);
    const auto opts = morph(s.options, 8 * 3 * 64);
    Frame T{s, 8, 64, cams, opts, 8, cells_for(8 * 3 * 64, 8, false)};
    T.alloc();
    const size_t own_allocations = stub_live_device_allocations(), own_handles = stub_live_streams_and_events();
    for (int warm = 0; warm < 2; ++warm) {
        int failed = 0;
        for (long n = 0; n < 400; ++n) {  // n == 0: the launch itself
            kifs_ctx* c = context_for(s, true);
            if (warm) CHECK(T.run({c}, {nullptr}, 0, s.h, false, LAST, true, LOOSE) == KIFS_OK);
            const long before = stub_calls();
            if (n == 0) family_stub_fail_next();
            else stub_fail_in(n);
            const int st = T.run({c}, {nullptr}, 0, s.h, false, LAST, true, LOOSE);  // (KIFS_OK: everything has been compared)
            const bool reached = n == 0 || stub_calls() - before >= n;
            stub_fail_in(-1);
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
            if (n == 0) CHECK(st == KIFS_ERR_RUNTIME);
            if (st != KIFS_OK) ++failed;
            bool ok_seen = false;
            for (int k = 0; k < KIFS_ANIMATION_RING + 1; ++k) {
                const int again = T.run({c}, {nullptr}, 0, s.h, false, LAST, true, LOOSE);
                CHECK(again == KIFS_OK || (again == KIFS_ERR_RUNTIME && !ok_seen));
                ok_seen = ok_seen || again == KIFS_OK;
            }
            CHECK(ok_seen);
            kifs_destroy(c);
            CHECK(stub_live_device_allocations() == own_allocations && stub_live_streams_and_events() == own_handles);
            if (!reached) break;
        }
        CHECK(failed >= 6);  // (a warm call: two copies, the memset, the launch, two records)
    }
    T.release();
}

// Where the animated call and the four accumulated ones meet (launch_scenes, kifs_animation.cpp): one context, two streams
// in turn, nine calls -- animation, accumulate, jittered, resume, converge, animation, accumulate, resume, animation: more
// than two laps of the scene ring -- of 3 and 65 views in turn (65: the view ring, on every other call), a 45 x 19 frame's
// rows 3..17, every call into a region of its own of one arena.
struct Mixed {
    enum Kind { ANIMATION, ACCUMULATE, JITTERED, RESUME, CONVERGE };
    static constexpr int CALLS = 9, W = 45, H = 19, Y0 = 3, Y1 = 17, ROWS = Y1 - Y0, GRID = 3;
    static constexpr size_t PITCH = size_t(W) * 4, SUMS_PITCH = size_t(W) * 16;
    const Kind kinds[CALLS] = {ANIMATION, ACCUMULATE, JITTERED, RESUME, CONVERGE, ANIMATION, ACCUMULATE, RESUME, ANIMATION};
    const Scene s = scene(W, H, 40);
    const std::vector<KifsCameraUniform> cams = cameras(65, 5);
    const std::vector<KifsOptionsUniform> opts = morph(s.options, 65);
    const std::vector<KifsSubpixel> cells = cells_for(65, GRID);
    std::vector<uint32_t> animated;  // the animated call's 65 whole frames, by the stand-in's model
    size_t pictures[CALLS], sums[CALLS], moments = 0, counts = 0, bytes = 0;  // offsets into the arena
    uint8_t* arena = nullptr;
    std::vector<uint8_t> first;  // the arena after the first clean sequence

    int views(int k) const { return k % 2 ? 65 : 3; }
    int frames(int k) const { return kinds[k] == ANIMATION ? views(k) : views(k) == 3 ? 1 : 5; }
    int samples(int k) const { return views(k) / frames(k); }
    size_t take(size_t n) {
        const size_t at = bytes;
        bytes += (n + 15) & ~size_t(15);
        return at;
    }
    // hip_stub.cpp's model of an animated frame (stub_key, stub_hit, stub_scene_key), restated: a plain render of the
    // frame's camera and options, every pixel that is not background also a function of the frame's scene.
    void model_animation() {
        int st = 0;
        kifs_ctx* c = kifs_create(0, &st);
        CHECK(c && st == KIFS_OK && kifs_set_screen(c, &s.screen) == KIFS_OK);
        animated.resize(size_t(65) * W * H);
        for (size_t f = 0; f < 65; ++f) {
            uint32_t* frame = animated.data() + f * W * H;
            CHECK(kifs_set_camera(c, &cams[f]) == KIFS_OK && kifs_set_options(c, &opts[f]) == KIFS_OK);
            CHECK(kifs_render(c, reinterpret_cast<uint8_t*>(frame), PITCH, 0, H, 1) == KIFS_OK);
            const KifsCameraUniform& cam = cams[f];
            const uint32_t key = accumulate_model::bits(cam.origin[0]) * 2654435761u ^ accumulate_model::bits(cam.origin[1]) * 40503u ^
                                 accumulate_model::bits(cam.origin[2]) * 69069u ^ accumulate_model::bits(cam.matrix[1][0]);
            const kifs::anim::SceneView sc = scene_of(opts[f]);
            uint32_t scene_key = 2166136261u;
            for (float v : {sc.c.x, sc.c.y, sc.c.z, sc.c.w, sc.power, sc.fractal_color.x, sc.fractal_color.y, sc.fractal_color.z,
                            sc.background_color.x, sc.background_color.y, sc.background_color.z})
                scene_key = (scene_key ^ accumulate_model::bits(v)) * 16777619u;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if ((((unsigned(x) >> 5) + 3u * (unsigned(y) >> 3) + (key >> 7)) & 3u) == 0u) frame[y * W + x] ^= scene_key & 0x00ffffffu;
        }
        kifs_destroy(c);
    }
    uint32_t expected(int k, int f, int x, int y) const {
        if (kinds[k] == ANIMATION) return animated[(size_t(f) * H + size_t(y)) * W + size_t(x)];
        const int g = kinds[k] == ACCUMULATE ? 1 : GRID;
        uint32_t acc = 0;
        for (int n = 0; n < samples(k); ++n) {
            const size_t v = size_t(f) * size_t(samples(k)) + size_t(n);
            const KifsSubpixel at = g == 1 ? KifsSubpixel{0, 0} : cells[v];
            const uint32_t one = accumulate_model::sample(view_of(cams[v]), scene_of(opts[v]), g * x + at.i, g * y + at.j);
            acc = n == 0 ? one : accumulate_model::fold(acc, one);
        }
        return accumulate_model::pixel(acc, samples(k));
    }
    void alloc() {
        for (int k = 0; k < CALLS; ++k) {
            pictures[k] = take(PITCH * ROWS * size_t(frames(k)));
            sums[k] = kinds[k] >= RESUME ? take(SUMS_PITCH * ROWS * size_t(frames(k))) : 0;
        }
        moments = take(PITCH * ROWS);
        counts = take(4);
        arena = dev_alloc(bytes);
        model_animation();
    }
    // The nine calls; status[k]: call k's, fired[k]: whether an injected failure (the `fail_at`-th HIP call from the start;
    // `fail_launch` >= 0: that call's accumulate launch) struck during it.
    void sequence(kifs_ctx* c, hipStream_t (&streams)[2], long fail_at, int fail_launch, int (&status)[CALLS], bool (&fired)[CALLS]) {
        std::memset(arena, 0xEE, bytes);
        const KifsConvergence rule{0.25f, 2u};
        const long start = stub_calls();
        if (fail_at > 0) stub_fail_in(fail_at);
        for (int k = 0; k < CALLS; ++k) {
            const int count = frames(k), n = samples(k);
            std::vector<uint8_t*> outs(static_cast<size_t>(count));
            for (int f = 0; f < count; ++f) outs[size_t(f)] = arena + pictures[k] + PITCH * ROWS * size_t(f);
            float* const plane = reinterpret_cast<float*>(arena + sums[k]);
            hipStream_t stream = streams[k % 2];
            const long before = stub_calls() - start;
            if (k == fail_launch) family_stub_fail_next();
            switch (kinds[k]) {
            case ANIMATION:
                status[k] = kifs_render_animation_async(c, stream, count, cams.data(), opts.data(), outs.data(), PITCH, Y0, Y1, 1);
                break;
            case ACCUMULATE:
                status[k] = kifs_render_accumulate_async(c, stream, count, n, cams.data(), opts.data(), outs.data(), PITCH, Y0, Y1, 1);
                break;
            case JITTERED:
                status[k] = kifs_render_accumulate_jittered_async(c, stream, count, n, cams.data(), opts.data(), GRID, cells.data(), outs.data(),
                                                                  PITCH, Y0, Y1, 1);
                break;
            case RESUME:
                status[k] = kifs_render_accumulate_resume_async(c, stream, count, n, cams.data(), opts.data(), GRID, cells.data(), plane, SUMS_PITCH,
                                                                SUMS_PITCH * ROWS, 0, outs.data(), PITCH, Y0, Y1, 1);
                break;
            case CONVERGE:
                status[k] = kifs_render_accumulate_converge_async(c, stream, count, n, cams.data(), opts.data(), GRID, cells.data(), plane, SUMS_PITCH,
                                                                  SUMS_PITCH * ROWS, reinterpret_cast<float*>(arena + moments), PITCH, PITCH * ROWS, 1,
                                                                  &rule, reinterpret_cast<uint32_t*>(arena + counts), outs.data(), PITCH, Y0, Y1, 1);
                break;
            }
            fired[k] = k == fail_launch || (fail_at > 0 && before < fail_at && stub_calls() - start >= fail_at);
            if (status[k] == KIFS_OK)
                CHECK(kifs_debug_last_kernel(c) == (kinds[k] == ANIMATION ? KIFS_KERNEL_ANIMATION : KIFS_KERNEL_ACCUMULATE));
        }
        stub_fail_in(-1);
    }
    // A clean sequence: every call succeeds, every picture is the model's, and the arena is the first clean sequence's.
    void clean(kifs_ctx* c, hipStream_t (&streams)[2]) {
        int status[CALLS];
        bool fired[CALLS];
        const long launches = family_stub_launches(), carries = family_stub_carries(), converges = family_stub_converges();
        sequence(c, streams, 0, -1, status, fired);
        for (int k = 0; k < CALLS; ++k) CHECK(status[k] == KIFS_OK);
        CHECK(family_stub_launches() == launches + 6 && family_stub_carries() == carries + 2 && family_stub_converges() == converges + 1);
        for (int k = 0; k < CALLS; ++k) {
            for (int f = 0; f < frames(k); ++f)
                for (int y = Y0; y < Y1; ++y)
                    for (int x = 0; x < W; ++x) {
                        uint32_t px;
                        std::memcpy(&px, arena + pictures[k] + PITCH * (size_t(ROWS) * size_t(f) + size_t(y - Y0)) + 4 * size_t(x), 4);
                        if (px != expected(k, f, x, y)) CHECK(false);
                    }
            ++g_checks;
        }
        if (first.empty()) first.assign(arena, arena + bytes);
        CHECK(std::memcmp(first.data(), arena, bytes) == 0);
    }
};

// The sequence clean on a fresh context, twice; then a failure injected at every HIP call of the sequence in turn and at
// each of its six accumulate launches, on a fresh context and on a warm one: a call returns KIFS_ERR_RUNTIME only if the
// failure struck during it, the launch's own always, and the next clean sequence on the same context gives the same bytes.
void shared_launch_path() {
    Mixed M;
    M.alloc();
    hipStream_t streams[2] = {nullptr, nullptr};
    CHECK(hipStreamCreateWithFlags(&streams[0], hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&streams[1], hipStreamNonBlocking) == hipSuccess);
    const size_t own_allocations = stub_live_device_allocations(), own_handles = stub_live_streams_and_events();
    {
        kifs_ctx* c = context_for(M.s, true);
        M.clean(c, streams);
        const long syncs = stub_event_synchronizes();
        M.clean(c, streams);
        // a warm lap: every call waits for its scene slot's last reader, every 65-view call for its view slot's as well
        CHECK(stub_event_synchronizes() - syncs == Mixed::CALLS + 4);
        kifs_destroy(c);
    }
    for (int warm = 0; warm < 2; ++warm) {
        int failed = 0;
        for (long n = 1 - Mixed::CALLS; n < 2000; ++n) {  // n <= 0: the accumulate launch of call -n (an animated call's is a HIP call)
            if (n <= 0 && M.kinds[-n] == Mixed::ANIMATION) continue;
            kifs_ctx* c = context_for(M.s, true);
            if (warm) M.clean(c, streams);
            int status[Mixed::CALLS];
            bool fired[Mixed::CALLS];
            const long before = stub_calls();
            M.sequence(c, streams, n > 0 ? n : 0, n > 0 ? -1 : int(-n), status, fired);
            const bool reached = n <= 0 || stub_calls() - before >= n;
            for (int k = 0; k < Mixed::CALLS; ++k) {
                CHECK(status[k] == KIFS_OK || (status[k] == KIFS_ERR_RUNTIME && fired[k]));
                if (n <= 0 && fired[k]) CHECK(status[k] == KIFS_ERR_RUNTIME);
                if (status[k] != KIFS_OK) ++failed;
            }
            M.clean(c, streams);
            kifs_destroy(c);
            CHECK(stub_live_device_allocations() == own_allocations && stub_live_streams_and_events() == own_handles);
            if (!reached) break;
        }
        CHECK(failed >= 6 + 2 * Mixed::CALLS);  // (the six launches; of every call at least the scene table's copy and record)
    }
    CHECK(hipStreamDestroy(streams[0]) == hipSuccess && hipStreamDestroy(streams[1]) == hipSuccess);
    CHECK(hipFree(M.arena) == hipSuccess);
}

}  // namespace

int main() {
    shapes(74, 45);  // neither dimension a multiple of the 32 x 8 tile
    shapes(64, 8);
    refusals();
    injected_failures();
    shared_launch_path();
    CHECK(stub_live_device_allocations() == 0);
    CHECK(stub_live_streams_and_events() == 0);
    std::printf("converge_driver: %ld checks ok\n", g_checks);
    return 0;
}
