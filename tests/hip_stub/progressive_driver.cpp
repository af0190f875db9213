// progressive_driver.cpp -- TEST INFRASTRUCTURE: drives the host side of kifs_render_accumulate_resume_async
// (kifs_progressive.cpp and kifs_accumulate.cpp, with the seven other host units) against tests/hip_stub/hip_stub.cpp and
// accumulate_family_stub.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan-progressive`;
// tests/test_progressive_host_sanitizers.py).  A stand-alone CPU program: frames of 1 x 1, 6 x 8, 8 x 64 and 13 x 5 views per
// pass (8 x 64 and 13 x 5: the view-table path) as sequences of passes over one plane, started from prior 0, 1 and
// 2^24 - the frame's sub-frames; a picture from every pass, from the last one, from none; bands with padded pitches on
// both destinations; passes alternating between two streams and between two contexts that share the plane; after every
// pass the recorded CarryParams and scene table are checked, and an existing jittered and an existing unjittered call on
// the same context still give their pixels; every refusal, with nothing launched and no HIP call made; a failure
// injected into every HIP call and into the launch of an 8 x 64 pass; and a final census of what is still alive.  The
// expected pixels and texels are restated here from accumulate_model.hpp.  Prints "progressive_driver: N checks ok".
#include <hip/hip_runtime_api.h>

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
            std::fprintf(stderr, "progressive_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                               \
        }                                                                                               \
    } while (0)

#include "accumulate_driver_common.hpp"

namespace {

constexpr uint32_t LIMIT = KIFS_MAX_PROGRESSIVE_SAMPLES;

uint32_t seed_of(int f, int x, int y) { return 0x9e3779b9u * uint32_t(f + 1) ^ uint32_t(x) * 2654435761u ^ uint32_t(y) * 40503u; }

enum Picture { EVERY, LAST, NEVER };

// A progressive frame: `count` frames of sum(splits) sub-frames each, view f * total + k the k-th sub-frame of frame f.
// `opts` empty: options NULL.
struct Frame {
    const Scene& s;
    int count;
    std::vector<int> splits;
    const std::vector<KifsCameraUniform>& cams;
    const std::vector<KifsOptionsUniform>& opts;
    int grid;
    std::vector<KifsSubpixel> cells;
    size_t pad = 0, plane_pad = 0;
    uint8_t* dev = nullptr;    // the pictures
    uint8_t* plane = nullptr;  // the sums
    uint8_t* side = nullptr;   // the destination of the existing calls made between the passes

    int total() const {
        int n = 0;
        for (const int k : splits) n += k;
        return n;
    }
    size_t pitch() const { return size_t(s.w) * 4 + pad; }
    size_t plane_pitch() const { return size_t(s.w) * 16 + plane_pad; }
    size_t bytes() const { return pitch() * size_t(s.h) * size_t(count) + 64; }
    size_t plane_bytes() const { return (plane_pitch() * size_t(s.h) + plane_pad) * size_t(count) + 64; }
    void alloc() {
        dev = dev_alloc(bytes());
        plane = dev_alloc(plane_bytes());
        side = dev_alloc(size_t(s.w) * 4 * size_t(s.h) * size_t(count));
    }
    void release() {
        CHECK(hipFree(dev) == hipSuccess && hipFree(plane) == hipSuccess && hipFree(side) == hipSuccess);
    }
    uint32_t sample(size_t v, int x, int y) const {
        const KifsSubpixel at = cells[v];
        return accumulate_model::sample(view_of(cams[v]), scene_of(opts.empty() ? s.options : opts[v]), grid * x + at.i, grid * y + at.j);
    }
    // the fold of sub-frames [k0, k1) of frame f; `from`: the texel it starts from, or null
    uint32_t folded(int f, int x, int y, int k0, int k1, const uint32_t* from) const {
        uint32_t acc = from ? *from : 0u;
        for (int k = k0; k < k1; ++k) {
            const uint32_t one = sample(size_t(f) * size_t(total()) + size_t(k), x, y);
            acc = (k == k0 && !from) ? one : accumulate_model::fold(acc, one);
        }
        return acc;
    }
    // An existing call on the same context after a pass: the pass's own views, jittered (grid as the pass) or not.
    void existing_call(kifs_ctx* c, const std::vector<KifsCameraUniform>& pc, const std::vector<KifsOptionsUniform>& po,
                       const std::vector<KifsSubpixel>& pcells, int n, int first, bool jittered) {
        const size_t sp = size_t(s.w) * 4;
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        for (int f = 0; f < count; ++f) outs[size_t(f)] = side + sp * size_t(s.h) * size_t(f);
        const long carries = family_stub_carries(), launches = family_stub_launches();
        const KifsOptionsUniform* o = po.empty() ? nullptr : po.data();
        const int st = jittered ? kifs_render_accumulate_jittered_async(c, nullptr, count, n, pc.data(), o, grid, pcells.data(), outs.data(), sp, 0, s.h, 1)
                                : kifs_render_accumulate_async(c, nullptr, count, n, pc.data(), o, outs.data(), sp, 0, s.h, 1);
        CHECK(st == KIFS_OK && family_stub_carries() == carries && family_stub_launches() == launches + 1);
        for (int f = 0; f < count; ++f)
            for (int y = 0; y < s.h; y += 3)
                for (int x = 0; x < s.w; x += 5) {
                    uint32_t px, acc = 0;
                    std::memcpy(&px, outs[size_t(f)] + sp * size_t(y) + 4 * size_t(x), 4);
                    for (int k = 0; k < n; ++k) {
                        const size_t v = size_t(f) * size_t(total()) + size_t(first + k);
                        const KifsSubpixel at = jittered ? cells[v] : KifsSubpixel{0, 0};
                        const int g = jittered ? grid : 1;
                        const uint32_t one = accumulate_model::sample(view_of(cams[v]), scene_of(opts.empty() ? s.options : opts[v]),
                                                                      g * x + at.i, g * y + at.j);
                        acc = k == 0 ? one : accumulate_model::fold(acc, one);
                    }
                    if (px != accumulate_model::pixel(acc, n)) CHECK(false);
                }
        ++g_checks;
    }
    // The passes in turn on ctxs[p % ctxs.size()] and streams[p % streams.size()] (null: the context's stream), the plane
    // holding `prior` sub-frames at the start (a seeded word 0) or nothing the call may read (prior == 0: 0xEE bytes).
    // Returns the first status that is not KIFS_OK (the caller re-runs from the start), or KIFS_OK with everything checked.
    int run(const std::vector<kifs_ctx*>& ctxs, const std::vector<hipStream_t>& streams, int y0, int y1, uint32_t prior, Picture picture,
            int encode = 1, bool between = true) {
        const int rows = y1 - y0, n_total = total();
        const size_t band = pitch() * size_t(rows), stride = plane_pitch() * size_t(rows) + plane_pad;
        std::vector<uint8_t*> outs(static_cast<size_t>(count));
        for (int f = 0; f < count; ++f) outs[size_t(f)] = dev + band * size_t(f);
        std::memset(dev, 0xEE, bytes());
        std::memset(plane, 0xEE, plane_bytes());
        if (prior)
            for (int f = 0; f < count; ++f)
                for (int y = y0; y < y1; ++y)
                    for (int x = 0; x < s.w; ++x) {
                        const uint32_t seed = seed_of(f, x, y);
                        std::memcpy(plane + stride * size_t(f) + plane_pitch() * size_t(y - y0) + 16 * size_t(x), &seed, 4);
                    }
        int done = 0;
        uint32_t in_plane = prior;
        int last_picture = -1;
        for (size_t p = 0; p < splits.size(); ++p) {
            const int n = splits[p];
            std::vector<KifsCameraUniform> pc;
            std::vector<KifsOptionsUniform> po;
            std::vector<KifsSubpixel> pcells;
            for (int f = 0; f < count; ++f)
                for (int k = 0; k < n; ++k) {
                    const size_t v = size_t(f) * size_t(n_total) + size_t(done + k);
                    pc.push_back(cams[v]);
                    if (!opts.empty()) po.push_back(opts[v]);
                    pcells.push_back(cells[v]);
                }
            kifs_ctx* c = ctxs[p % ctxs.size()];
            hipStream_t stream = streams[p % streams.size()];
            if (p > 0 && streams.size() > 1)  // the caller orders passes on different streams
                CHECK(kifs_order_after(c, stream, streams[(p - 1) % streams.size()]) == KIFS_OK);
            const bool with_picture = picture == EVERY || (picture == LAST && p + 1 == splits.size());
            const long carries = family_stub_carries(), launches = family_stub_launches(), calls = stub_calls();
            const int st = kifs_render_accumulate_resume_async(c, stream, count, n, pc.data(), po.empty() ? nullptr : po.data(), grid,
                                                               pcells.data(), reinterpret_cast<float*>(plane), plane_pitch(), stride, in_plane,
                                                               with_picture ? outs.data() : nullptr, with_picture ? pitch() : 1, y0, y1, encode);
            if (st != KIFS_OK) return st;
            if (rows == 0) {
                CHECK(family_stub_launches() == launches && stub_calls() == calls);  // an empty band: nothing enqueued
            } else {
                CHECK(family_stub_carries() == carries + 1 && family_stub_launches() == launches + 1);
                CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ACCUMULATE && kifs_debug_last_round_steps(c) == 0);
                CHECK(kifs_debug_last_group_tiles(c) == -1 && kifs_debug_last_bunny_form(c) == -1);
                const kifs::accum::CarryParams& K = family_stub_last_carry();
                const std::vector<kifs::anim::SceneView>& scenes = family_stub_last_scenes();
                CHECK(K.sums == reinterpret_cast<float*>(plane) && K.sums_pitch_texels == plane_pitch() / 16 && K.sums_stride_texels == stride / 16);
                CHECK(K.prior == in_plane && K.picture == (with_picture ? 1u : 0u));
                CHECK(K.A.frames == count && K.A.samples == n && K.A.B.count == count * n && int(scenes.size()) == count * n);
                CHECK(K.A.B.frame.ssaa == grid && K.A.B.frame.ssaa_inv_height == 1.0f / (float(grid) * float(s.h)));
                CHECK(K.A.B.frame.y0 == y0 && K.A.B.frame.y1 == y1 && K.A.B.frame.encode == encode);
                CHECK(with_picture ? K.A.B.frame.pitch_words == pitch() / 4 && K.A.B.frame.out == reinterpret_cast<uint32_t*>(outs[0])
                                   : K.A.B.frame.pitch_words == 0 && K.A.B.frame.out == nullptr);
                for (int v = 0; v < count * n; ++v) {
                    const KifsSubpixel at = pcells[size_t(v)];
                    if (scenes[size_t(v)].pad[0] != (grid > 1 ? uint32_t(at.i) | uint32_t(at.j) << 8 : 0u)) CHECK(false);
                }
                ++g_checks;
            }
            if (between && rows > 0) {
                existing_call(c, pc, po, pcells, n, done, true);
                existing_call(c, pc, po, pcells, n, done, false);
            }
            done += n;
            in_plane += uint32_t(n);
            if (with_picture) last_picture = done;
        }
        // the plane: the fold of everything, float(total) in w; the pictures: of the last pass that had one
        for (int f = 0; f < count; ++f)
            for (int y = y0; y < y1; ++y) {
                const uint8_t* trow = plane + stride * size_t(f) + plane_pitch() * size_t(y - y0);
                const uint8_t* row = outs[size_t(f)] + pitch() * size_t(y - y0);
                for (int x = 0; x < s.w; ++x) {
                    const uint32_t seed = seed_of(f, x, y);
                    uint32_t t[4], px;
                    std::memcpy(t, trow + 16 * size_t(x), 16);
                    const uint32_t acc = folded(f, x, y, 0, n_total, prior ? &seed : nullptr);
                    const float w = float(prior + uint32_t(n_total));
                    if (t[0] != acc || t[1] != ~acc || t[2] != acc * 3u || t[3] != accumulate_model::bits(w)) CHECK(false);
                    std::memcpy(&px, row + 4 * size_t(x), 4);
                    if (last_picture < 0) {
                        if (px != 0xEEEEEEEEu) CHECK(false);
                    } else {
                        const uint32_t shown = folded(f, x, y, 0, last_picture, prior ? &seed : nullptr);
                        if (px != accumulate_model::pixel(shown, int(prior) + last_picture)) CHECK(false);
                    }
                }
                for (size_t b = size_t(s.w) * 16; b < plane_pitch(); ++b)
                    if (trow[b] != 0xEE) CHECK(false);
                for (size_t b = size_t(s.w) * 4; b < pitch(); ++b)
                    if (row[b] != 0xEE) CHECK(false);
            }
        ++g_checks;
        for (int f = 0; f < count; ++f)  // behind every frame's rows, and behind the last frame
            for (size_t b = stride * size_t(f) + plane_pitch() * size_t(rows); b < (f + 1 < count ? stride * size_t(f + 1) : plane_bytes()); ++b)
                if (plane[b] != 0xEE) CHECK(false);
        for (size_t b = band * size_t(count); b < bytes(); ++b)
            if (dev[b] != 0xEE) CHECK(false);
        return KIFS_OK;
    }
};

// {frames, sub-frames per pass}: the passes of a frame are three of these (the last one a lone sub-frame short where it can be)
const int SHAPES[4][2] = {{1, 1}, {6, 8}, {8, 64}, {13, 5}};

void shapes(int w, int h) {
    const Scene s = scene(w, h, 40);
    const std::vector<KifsOptionsUniform> none;
    hipStream_t extra[2] = {nullptr, nullptr};
    for (hipStream_t& e : extra) CHECK(hipStreamCreateWithFlags(&e, hipStreamNonBlocking) == hipSuccess);
    for (const auto& shape : SHAPES) {
        const int count = shape[0], n = shape[1];
        const std::vector<int> splits = {n, n, n > 1 ? n - 1 : 1};
        const int total = splits[0] + splits[1] + splits[2], views = count * total;
        const auto cams = cameras(views, 3);
        const auto opts = morph(s.options, views);
        for (int given = 0; given < 2; ++given) {
            kifs_ctx* a = context_for(s, !given);  // options given: contexts that never had kifs_set_options
            kifs_ctx* b = context_for(s, !given);
            const std::vector<kifs_ctx*> one = {a}, two = {a, b};
            const std::vector<hipStream_t> own = {nullptr}, both = {extra[0], extra[1]};
            for (const int g : {1, 3, 8}) {
                Frame F{s, count, splits, cams, given ? opts : none, g, g == 1 ? std::vector<KifsSubpixel>(size_t(views), KifsSubpixel{0, 0}) : cells_for(views, g)};
                F.alloc();
                const uint32_t priors[3] = {0u, 1u, LIMIT - uint32_t(total)};
                for (int k = 0; k < 3; ++k) {
                    CHECK(F.run(one, own, 0, h, priors[k], Picture(k % 3), k == 1 ? 0 : 1, g == 3) == KIFS_OK);
                }
                CHECK(F.run(two, own, 0, h, 0, LAST, 1, false) == KIFS_OK);    // two contexts on one plane
                CHECK(F.run(one, both, 0, h, 1, EVERY, 1, false) == KIFS_OK);  // two streams
                CHECK(F.run(two, both, 0, h, 0, NEVER, 1, g == 8 && n == 5) == KIFS_OK);
                F.release();
                Frame B{s, count, splits, cams, given ? opts : none, g, F.cells, 48, 32};
                B.alloc();
                CHECK(B.run(one, own, h / 3, h - 3, 0, LAST, 1, false) == KIFS_OK);  // a band, padded pitches on both destinations
                CHECK(B.run(two, both, h / 3, h - 3, 7, EVERY, 0, false) == KIFS_OK);
                CHECK(B.run(one, own, h / 2, h / 2, 0, EVERY) == KIFS_OK);           // an empty band: nothing enqueued
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
    const size_t pitch = size_t(s.w) * 4, fb = pitch * s.h, pp = size_t(s.w) * 16, pb = pp * s.h;
    uint8_t* dev = dev_alloc(fb * 3);
    uint8_t* plane = dev_alloc(pb * 3 + 64);
    std::memset(dev, 0xEE, fb * 3);
    std::memset(plane, 0xEE, pb * 3 + 64);
    std::vector<uint8_t*> outs(513, dev);
    outs[1] = dev + fb;
    outs[2] = dev + 2 * fb;
    kifs_ctx* c = context_for(s, true);
    const KifsCameraUniform* cm = cams.data();
    const KifsOptionsUniform* op = opts.data();
    uint8_t* const* out = outs.data();
    float* sums = reinterpret_cast<float*>(plane);
    std::vector<KifsSubpixel> zero(513, KifsSubpixel{0, 0}), in3 = cells_for(6, 3);
    auto call = [&](kifs_ctx* ctx, int count, int samples, const KifsCameraUniform* cam, const KifsOptionsUniform* o, int grid,
                    const KifsSubpixel* cells, float* plane_at, size_t plane_pitch, size_t plane_stride, uint32_t prior, uint8_t* const* to,
                    size_t p, int y0, int y1, int encode) {
        const long calls = stub_calls(), launches = stub_launches() + family_stub_launches();  // a refused call makes no HIP call
        const int st = kifs_render_accumulate_resume_async(ctx, nullptr, count, samples, cam, o, grid, cells, plane_at, plane_pitch, plane_stride,
                                                           prior, to, p, y0, y1, encode);
        CHECK(st != KIFS_OK && stub_calls() == calls && stub_launches() + family_stub_launches() == launches);
        return st;
    };
    // the jittered call's, with their statuses
    for (const int grid : {0, -1, KIFS_MAX_JITTER_GRID + 1, 0x7fffffff})
        CHECK(call(c, 3, 2, cm, op, grid, zero.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    for (int v = 0; v < 6; ++v) {
        auto bad = in3;
        bad[size_t(v)].i = 3;
        CHECK(call(c, 3, 2, cm, op, 3, bad.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        bad = in3;
        bad[size_t(v)].j = 255;
        CHECK(call(c, 3, 2, cm, op, 3, bad.data(), sums, pp, pb, 4, nullptr, 0, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    CHECK(call(c, 3, 2, cm, op, 3, nullptr, sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // NULL: samples != 9
    CHECK(call(c, 3, 2, cm, op, 1, nullptr, sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // NULL: samples != 1
    CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    CHECK(call(nullptr, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, nullptr, op, 3, in3.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    uint8_t* null_out[3] = {dev, nullptr, dev}, *odd_out[3] = {dev, dev, dev + 1};
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, null_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // an ENTRY of a given array
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, odd_out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 0, cm, op, 1, zero.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, KIFS_MAX_ACCUMULATE + 1, cm, op, 1, zero.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // per pass
    CHECK(call(c, 0, 2, cm, op, 1, zero.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 513, 1, cm, op, 1, zero.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 0x7fffffff, 64, cm, op, 8, nullptr, sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 2) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, out, pitch, -1, s.h, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, nullptr, 0, 0, s.h + 1, 1) == KIFS_ERR_BAD_ARG);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, out, pitch - 4, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 4, out, pitch + 2, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);
    CHECK(call(c, 3, 2, cm, op, 3, in3.data(), nullptr, pp, pb, 4, out, pitch - 4, 0, s.h, 1) == KIFS_ERR_BAD_SIZE);  // the shared checks come first
    {
        std::vector<KifsOptionsUniform> o(opts.begin(), opts.begin() + 6);
        o[4].max_iterations += 1;
        CHECK(call(c, 3, 2, cm, o.data(), 3, in3.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
    }
    {
        kifs_ctx* bare = context_for(s, false);
        CHECK(call(bare, 3, 2, cm, nullptr, 3, in3.data(), sums, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        CHECK(call(bare, 3, 2, cm, nullptr, 3, in3.data(), nullptr, pp, pb, 4, out, pitch, 0, s.h, 1) == KIFS_ERR_UNCONFIGURED);
        kifs_destroy(bare);
    }
    {
        const Scene wide = scene(8200, 1, 40);
        kifs_ctx* b = context_for(wide, true);
        std::vector<KifsSubpixel> c8(2, KifsSubpixel{7, 7});
        CHECK(call(b, 1, 2, cm, nullptr, 8, c8.data(), sums, size_t(wide.w) * 16, 0, 0, out, size_t(wide.w) * 4, 0, 1, 1) == KIFS_ERR_BAD_SIZE);
        kifs_destroy(b);
    }
    // the call's own: the plane and the number of sub-frames, with a picture and without
    for (int with = 0; with < 2; ++with) {
        uint8_t* const* to = with ? out : nullptr;
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), nullptr, pp, pb, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        for (const size_t off : {size_t(4), size_t(8), size_t(12), size_t(1)})
            CHECK(call(c, 3, 2, cm, op, 3, in3.data(), reinterpret_cast<float*>(plane + off), pp, pb, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp - 16, pb, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp + 8, pb + 8 * s.h, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, 0, pb, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb + 8, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb - 16, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // frames would overlap
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, 0, 4, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, LIMIT - 1, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, LIMIT, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);
        CHECK(call(c, 3, 2, cm, op, 3, in3.data(), sums, pp, pb, 0xffffffffu, to, pitch, 0, s.h, 1) == KIFS_ERR_BAD_ARG);  // (no overflow on the way)
    }
    for (size_t i = 0; i < fb * 3; ++i)
        if (dev[i] != 0xEE) CHECK(false);
    for (size_t i = 0; i < pb * 3 + 64; ++i)
        if (plane[i] != 0xEE) CHECK(false);
    CHECK(hipFree(dev) == hipSuccess && hipFree(plane) == hipSuccess);
    // and the same arguments unrefused, the total at the limit itself
    Frame A{s, 3, {2}, cams, opts, 3, in3};
    A.alloc();
    CHECK(A.run({c}, {nullptr}, 0, s.h, LIMIT - 2, LAST) == KIFS_OK);
    A.release();
    kifs_destroy(c);
}

// Every HIP call of an 8 x 64 pass over a plane that holds a sub-frame already fails once, in turn, and then its launch, on a
// fresh context and on a warm one: the call reports KIFS_ERR_RUNTIME or absorbs the failure; KIFS_ANIMATION_RING + 1 more
// runs each return a status and from the first that succeeds on every frame and texel is exact; the destroy leaves
// nothing behind.
void injected_failures() {
    const Scene s = scene(40, 13, 10);
    const auto cams = cameras(512, 13);
    const auto opts = morph(s.options, 512);
    Frame T{s, 8, {64}, cams, opts, 8, cells_for(512, 8)};
    T.alloc();
    const size_t own_allocations = stub_live_device_allocations(), own_handles = stub_live_streams_and_events();
    for (int warm = 0; warm < 2; ++warm) {
        int failed = 0;
        for (long n = 0; n < 400; ++n) {  // n == 0: the launch itself
            kifs_ctx* c = context_for(s, true);
            if (warm)
                for (int k = 0; k < KIFS_ANIMATION_RING; ++k) CHECK(T.run({c}, {nullptr}, 0, s.h, 1, LAST, 1, false) == KIFS_OK);
            const long before = stub_calls();
            if (n == 0) family_stub_fail_next();
            else stub_fail_in(n);
            const int st = T.run({c}, {nullptr}, 0, s.h, 1, LAST, 1, false);  // (KIFS_OK: frames and plane have been compared)
            const bool reached = n == 0 || stub_calls() - before >= n;
            stub_fail_in(-1);
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
            if (n == 0) CHECK(st == KIFS_ERR_RUNTIME);
            if (st != KIFS_OK) ++failed;
            bool ok_seen = false;
            for (int k = 0; k < KIFS_ANIMATION_RING + 1; ++k) {
                const int again = T.run({c}, {nullptr}, 0, s.h, 1, LAST, 1, false);
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
    std::printf("progressive_driver: %ld checks ok\n", g_checks);
    return 0;
}
