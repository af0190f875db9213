// fold_trap_driver.cpp -- TEST INFRASTRUCTURE: drives the host side of kifs_render_folded_trapped_async and
// kifs_eval_fold_trap (kifs_fold_trap.cpp, with the seven other host units) against tests/hip_stub/hip_stub.cpp and
// fold_trap_stub.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (`make asan-fold-trap`;
// tests/test_fold_trap_host_sanitizers.py).  A stand-alone CPU program: every refusal, with nothing launched and nothing
// written; 1, 3 and 64 frames; bands; supersampling factors 1..4; the plane with and without a term; what a launch
// carries -- the record AS THE COPY LEFT IT AT LAUNCH TIME with the scaling step's constants as the contract computes them
// and the trap field for field, ALL THREE CULLS ZERO in the frame constants, the light, the term and its flag, the plane,
// the band's tile table, the fixed launch shape, the views; more calls than the ring is deep, each with a record of its
// own; a failure injected at every HIP call and at the launch; animated batches interleaved on the same ring; a caller's
// stream; kifs_eval_fold_trap; the plain render calls before, between and after the call on one context, with the same
// bytes and the same launch state; and a final census of what is still alive.  Prints "fold_trap_driver: N checks ok".
#include <hip/hip_runtime_api.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/kifs_hip.h"
#include "fold_trap_model.hpp"

struct StubRenderLaunch {  // as tests/hip_stub/hip_stub.cpp declares it
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
long stub_calls();
long stub_launches();
size_t stub_live_device_allocations();
size_t stub_live_streams_and_events();
void fold_trap_stub_fail_next();
long fold_trap_stub_launches();
long fold_trap_stub_evals();
}
const FoldTrapStubLaunch& fold_trap_stub_last();
const FoldTrapStubEval& fold_trap_stub_last_eval();

static long g_checks = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        ++g_checks;                                                                                       \
        if (!(cond)) {                                                                                    \
            std::fprintf(stderr, "fold_trap_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                                 \
        }                                                                                                 \
    } while (0)

namespace {

constexpr uint8_t SENT = 0xA5;
constexpr int W = 102, H = 45;
const KifsAmbientOcclusion TERM{5, 0.02f, 0.75f, 4.0f};
const KifsLight REFERENCE{{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 5};
const KifsLight LIGHT_A{{-0.55f, 0.75f, 0.36f}, 0.15f, 0.85f, {0.6f, 0.6f, 0.5f}, 3};
const KifsFoldSystem MENGER{KIFS_FOLD_ABS | KIFS_FOLD_SORT | KIFS_FOLD_MIRROR_Z, 3, 3.0f, {1.0f, 1.0f, 1.0f}, {1, 0, 0, 0, 1, 0, 0, 0, 1}};
const KifsFoldSystem ALL{31u, 8, 1.8f, {1.0f, 0.8f, 0.6f}, {0.9f, -0.3f, 0.1f, 0.3f, 0.9f, -0.2f, -0.1f, 0.2f, 0.95f}};
const KifsOrbitTrap TRAP{{0.25f, -0.5f, 1.0f, 0.0f}, 7u, 6, 0.5f, -0.125f, {1.0f, 0.26f, 0.0f}, {0.007f, 0.045f, 0.58f}};

template <class T>
T* dev_alloc(size_t count) {
    void* p = nullptr;
    CHECK(hipMalloc(&p, count * sizeof(T)) == hipSuccess);
    return static_cast<T*>(p);
}

KifsOptionsUniform options_of(uint32_t group, uint32_t shape) {
    KifsGuiData gui;
    kifs_host_gui_default(&gui);
    gui.fractal_group = group;
    gui.primitive_shape = shape;
    gui.max_iterations = 77;
    KifsOptionsUniform o;
    CHECK(kifs_host_options(&gui, &o) == KIFS_OK);
    return o;
}

KifsCameraUniform camera_of(float phi) {
    KifsCameraData cd;
    kifs_host_camera_default(&cd);
    cd.phi = phi;
    KifsCameraUniform cam;
    CHECK(kifs_host_camera(&cd, &cam) == KIFS_OK);
    return cam;
}

kifs_ctx* context(int w, int h, uint32_t group, uint32_t shape) {
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    KifsScreenUniform screen;
    CHECK(kifs_host_screen(uint32_t(w), uint32_t(h), &screen) == KIFS_OK);
    const KifsOptionsUniform o = options_of(group, shape);
    const KifsCameraUniform cam = camera_of(0.3f);
    CHECK(kifs_set_screen(c, &screen) == KIFS_OK && kifs_set_options(c, &o) == KIFS_OK && kifs_set_camera(c, &cam) == KIFS_OK);
    return c;
}

// `count` colour destinations and planes for bands of up to `rows` rows of `w` pixels, padded and sentinel-filled.
struct Buffers {
    int count, rows, w;
    size_t cpitch, cbytes, ppitch, pbytes;
    uint8_t* colour;
    uint8_t* plane;
    std::vector<uint8_t*> outs;
    Buffers(int count_, int rows_, int w_, size_t cpad = 12, size_t ppad = 8)
        : count(count_), rows(rows_), w(w_), cpitch(size_t(w_) * 4 + cpad), cbytes(size_t(rows_) * cpitch + 64), ppitch(size_t(w_) * 4 + ppad),
          pbytes(size_t(rows_) * ppitch + 64), colour(dev_alloc<uint8_t>(size_t(count_) * cbytes)), plane(dev_alloc<uint8_t>(size_t(count_) * pbytes)) {
        for (int i = 0; i < count; ++i) outs.push_back(colour + size_t(i) * cbytes);
        fill();
    }
    void fill() {
        std::memset(colour, SENT, size_t(count) * cbytes);
        std::memset(plane, SENT, size_t(count) * pbytes);
    }
    float* u() const { return reinterpret_cast<float*>(plane); }
    bool untouched() const {
        for (size_t i = 0; i < size_t(count) * cbytes; ++i)
            if (colour[i] != SENT) return false;
        for (size_t i = 0; i < size_t(count) * pbytes; ++i)
            if (plane[i] != SENT) return false;
        return true;
    }
    // The first n views hold the model's words for rows [y0, y1) -- the plane too, when `planed` -- and every other byte the sentinel.
    bool holds_model(int n, int y0, int y1, int encode, int k, bool term, int e, int N, int K, bool planed) const {
        std::vector<uint8_t> wc(size_t(count) * cbytes, SENT), wp(size_t(count) * pbytes, SENT);
        for (int v = 0; v < n; ++v)
            for (int r = 0; r < y1 - y0; ++r)
                for (int x = 0; x < w; ++x) {
                    const uint32_t px = fold_trap_model::pixel(v, y0 + r, x, encode, k, term, e, N, K);
                    std::memcpy(&wc[size_t(v) * cbytes + size_t(r) * cpitch + size_t(x) * 4], &px, 4);
                    if (planed) {
                        const float uu = fold_trap_model::u_of(v, y0 + r, x, N, K);
                        std::memcpy(&wp[size_t(v) * pbytes + size_t(r) * ppitch + size_t(x) * 4], &uu, 4);
                    }
                }
        return std::memcmp(wc.data(), colour, wc.size()) == 0 && std::memcmp(wp.data(), plane, wp.size()) == 0;
    }
    ~Buffers() { CHECK(hipFree(colour) == hipSuccess && hipFree(plane) == hipSuccess); }
};

const KifsFoldSystem* g_fold = &MENGER;  // the records of call()
const KifsOrbitTrap* g_trap = &TRAP;

int call(kifs_ctx* c, const Buffers& b, int count, const KifsCameraUniform* cams, const KifsLight* light, const KifsAmbientOcclusion* ao,
         int y0, int y1, int encode, bool planed = false, void* stream = nullptr) {
    return kifs_render_folded_trapped_async(c, stream, count, cams, b.outs.data(), b.cpitch, g_fold, g_trap, light, ao, planed ? b.u() : nullptr,
                                            b.ppitch, b.pbytes, y0, y1, encode);
}

// The contract's Lh, restated: dot3 as an fma chain, one square root, three divides.
void unit_of(const float d[3], float out[3]) {
    const float len = std::sqrt(std::fmaf(d[2], d[2], std::fmaf(d[1], d[1], d[0] * d[0])));
    for (int i = 0; i < 3; ++i) out[i] = d[i] / len;
}

// The record as the contract's host side makes it of a system and a trap.
bool record_is(const kifs::foldorbit::Record& R, const KifsFoldSystem& fs, const KifsOrbitTrap& t) {
    const kifs::fold::Fold& F = R.fold;
    bool ok = F.stages == fs.stages && F.iterations == fs.iterations && F.scale == fs.scale;
    const float kk = fs.scale - 1.0f;
    for (int i = 0; i < 3; ++i) {
        const float ti = -(kk * fs.offset[i]);
        ok = ok && std::memcmp(&F.t[i], &ti, 4) == 0;
    }
    const float hh = 0.5f * F.t[2];
    ok = ok && std::memcmp(&F.h, &hh, 4) == 0;
    if (fs.stages & KIFS_FOLD_ROTATE) ok = ok && std::memcmp(F.R, fs.rotation, sizeof fs.rotation) == 0;
    else
        for (float v : F.R) ok = ok && v == 0.0f;
    static_assert(sizeof(KifsOrbitTrap) == sizeof(kifs::trap::Trap), "the trap travels field for field");
    return ok && std::memcmp(&R.trap, &t, sizeof t) == 0 && R.pad[0] == 0u && R.pad[1] == 0u;
}

// The systems and the traps the API refuses.
std::vector<KifsFoldSystem> bad_systems() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<KifsFoldSystem> bad;
    for (uint32_t stages : {32u, 33u, 63u, 0x80000000u, 0xffffffffu}) {
        KifsFoldSystem f = ALL;
        f.stages = stages;
        bad.push_back(f);
    }
    for (int n : {-1, KIFS_MAX_FOLD_ITERATIONS + 1, 1 << 20, INT_MIN, INT_MAX}) {
        KifsFoldSystem f = ALL;
        f.iterations = n;
        bad.push_back(f);
    }
    for (float s : {0.5f, 0.99999994f, 16.000002f, 17.0f, 0.0f, -2.0f, nan, inf, -inf}) {
        KifsFoldSystem f = ALL;
        f.scale = s;
        bad.push_back(f);
    }
    for (int i = 0; i < 3; ++i)
        for (float v : {nan, inf, -inf}) {
            KifsFoldSystem f = ALL;
            f.offset[i] = v;
            bad.push_back(f);
        }
    for (int i = 0; i < 9; ++i)
        for (float v : {nan, inf, -inf}) {
            KifsFoldSystem f = ALL;  // (ROTATE is set: the matrix is read)
            f.rotation[i] = v;
            bad.push_back(f);
        }
    return bad;
}
// `orbit`: only what kifs_eval_fold_trap validates -- centre, axes, iterations.
std::vector<KifsOrbitTrap> bad_traps(bool orbit) {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<KifsOrbitTrap> bad;
    for (uint32_t axes : {0u, 16u, 31u, 0x80000000u, 0xffffffffu}) {
        KifsOrbitTrap t = TRAP;
        t.axes = axes;
        bad.push_back(t);
    }
    for (int n : {-1, KIFS_MAX_TRAP_ITERATIONS + 1, 1 << 20, INT_MIN, INT_MAX}) {
        KifsOrbitTrap t = TRAP;
        t.iterations = n;
        bad.push_back(t);
    }
    for (int i = 0; i < 4; ++i)
        for (float v : {nan, inf, -inf}) {
            KifsOrbitTrap t = TRAP;
            t.centre[i] = v;
            bad.push_back(t);
        }
    if (orbit) return bad;
    for (float v : {nan, inf, -inf}) {
        KifsOrbitTrap t = TRAP;
        t.scale = v;
        bad.push_back(t);
        t = TRAP;
        t.bias = v;
        bad.push_back(t);
    }
    for (int i = 0; i < 3; ++i)
        for (float v : {-1.0e-30f, -1.0f, nan, inf, -inf}) {
            KifsOrbitTrap t = TRAP;
            t.mid[i] = v;
            bad.push_back(t);
            t = TRAP;
            t.far[i] = v;
            bad.push_back(t);
        }
    return bad;
}

void refusals() {
    kifs_ctx* c = context(W, H, 0, 3);
    Buffers b(2, H, W);
    const KifsCameraUniform cams[2] = {camera_of(0.1f), camera_of(0.2f)};
    std::vector<KifsCameraUniform> many(65, cams[0]);
    std::vector<uint8_t*> many_outs(65, b.outs[0]);
    const long launches = fold_trap_stub_launches(), renders = stub_launches();
    const size_t live = stub_live_device_allocations();  // (a refused call does not even take a slot of the ring)
    auto refused = [&](int got, int status) {
        CHECK(got == status);
        CHECK(fold_trap_stub_launches() == launches && stub_launches() == renders);
        CHECK(b.untouched());
    };
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // null pointers
    refused(call(nullptr, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    refused(kifs_render_folded_trapped_async(c, nullptr, 1, nullptr, nullptr, b.cpitch, &MENGER, &TRAP, &LIGHT_A, &TERM, b.u(), b.ppitch, b.pbytes, 0, H, 1),
            KIFS_ERR_BAD_ARG);
    g_fold = nullptr;
    refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    g_fold = &MENGER;
    g_trap = nullptr;
    refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    refused(call(c, b, 1, nullptr, nullptr, nullptr, 0, H, 1), KIFS_ERR_BAD_ARG);
    g_trap = &TRAP;
    // the system and the trap
    for (const KifsFoldSystem& f : bad_systems()) {
        g_fold = &f;
        refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
        refused(call(c, b, 1, nullptr, nullptr, nullptr, 0, H, 1), KIFS_ERR_BAD_ARG);
    }
    g_fold = &MENGER;
    for (const KifsOrbitTrap& t : bad_traps(false)) {
        g_trap = &t;
        refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
        refused(call(c, b, 1, nullptr, nullptr, nullptr, 0, H, 1), KIFS_ERR_BAD_ARG);
    }
    g_trap = &TRAP;
    // the light: direction components, its length, the weights, the shininess
    std::vector<KifsLight> bad;
    for (int i = 0; i < 3; ++i) {
        for (float v : {nan, inf, -inf}) {
            KifsLight l = LIGHT_A;
            l.direction[i] = v;
            bad.push_back(l);
        }
        for (float v : {-1.0e-30f, -1.0f, nan, inf, -inf}) {
            KifsLight l = LIGHT_A;
            l.specular[i] = v;
            bad.push_back(l);
        }
    }
    const float lengths[][3] = {{0.0f, 0.0f, 0.0f}, {-0.0f, 0.0f, -0.0f}, {1.0e-20f, 1.0e-20f, 0.0f}, {0.0f, 1.0e-30f, 1.0e-30f},
                                {1.0e-45f, 0.0f, 0.0f}, {2.0e19f, 2.0e19f, 2.0e19f}, {3.0e38f, 0.0f, 0.0f}};
    for (const auto& d : lengths) {
        KifsLight l = LIGHT_A;
        std::memcpy(l.direction, d, sizeof l.direction);
        bad.push_back(l);
    }
    for (float v : {-1.0e-30f, -0.5f, nan, inf, -inf}) {
        KifsLight l = LIGHT_A;
        l.ambient = v;
        bad.push_back(l);
        l = LIGHT_A;
        l.diffuse = v;
        bad.push_back(l);
    }
    for (int e : {-1, KIFS_MAX_SHININESS_LOG2 + 1, 32, INT_MIN, INT_MAX}) {
        KifsLight l = LIGHT_A;
        l.shininess_log2 = e;
        bad.push_back(l);
    }
    for (const KifsLight& l : bad) {
        refused(call(c, b, 1, nullptr, &l, nullptr, 0, H, 1), KIFS_ERR_BAD_ARG);
        refused(call(c, b, 1, nullptr, &l, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    }
    // the term, when there is one: what kifs_render_occlusion_async refuses
    const KifsAmbientOcclusion bad_terms[] = {
        {0, 0.02f, 0.75f, 4.0f}, {17, 0.02f, 0.75f, 4.0f}, {-3, 0.02f, 0.75f, 4.0f}, {INT_MIN, 0.02f, 0.75f, 4.0f}, {INT_MAX, 0.02f, 0.75f, 4.0f},
        {5, 0.0f, 0.75f, 4.0f}, {5, -0.0f, 0.75f, 4.0f}, {5, -0.02f, 0.75f, 4.0f}, {5, nan, 0.75f, 4.0f}, {5, inf, 0.75f, 4.0f}, {5, -inf, 0.75f, 4.0f},
        {5, 0.02f, 0.0f, 4.0f}, {5, 0.02f, -0.75f, 4.0f}, {5, 0.02f, 1.0000001f, 4.0f}, {5, 0.02f, nan, 4.0f}, {5, 0.02f, inf, 4.0f},
        {5, 0.02f, 0.75f, -1.0e-30f}, {5, 0.02f, 0.75f, nan}, {5, 0.02f, 0.75f, inf}, {5, 0.02f, 0.75f, -inf}};
    for (const KifsAmbientOcclusion& t : bad_terms) refused(call(c, b, 1, nullptr, &LIGHT_A, &t, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    // the count, and NULL cameras with more than one frame
    for (int count : {0, -1, INT_MIN, 65, KIFS_MAX_BATCH, INT_MAX})
        refused(kifs_render_folded_trapped_async(c, nullptr, count, many.data(), many_outs.data(), b.cpitch, &MENGER, &TRAP, &LIGHT_A, nullptr, nullptr, 0, 0,
                                                 0, H, 1),
                KIFS_ERR_BAD_ARG);
    refused(call(c, b, 2, nullptr, &LIGHT_A, nullptr, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    // destinations
    {
        uint8_t* outs[2] = {b.outs[0], nullptr};
        refused(kifs_render_folded_trapped_async(c, nullptr, 2, cams, outs, b.cpitch, &MENGER, &TRAP, &LIGHT_A, nullptr, b.u(), b.ppitch, b.pbytes, 0, H, 1),
                KIFS_ERR_BAD_ARG);
        for (size_t off : {1u, 2u, 3u}) {
            outs[1] = b.outs[1] + off;
            refused(kifs_render_folded_trapped_async(c, nullptr, 2, cams, outs, b.cpitch, &MENGER, &TRAP, &LIGHT_A, nullptr, b.u(), b.ppitch, b.pbytes, 0, H, 1),
                    KIFS_ERR_BAD_ARG);
        }
    }
    // encode and band
    for (int encode : {-1, 2, 256, INT_MAX}) refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, encode, true), KIFS_ERR_BAD_ARG);
    refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, -1, H, 1, true), KIFS_ERR_BAD_ARG);
    refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H + 1, 1, true), KIFS_ERR_BAD_ARG);
    refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 10, 9, 1, true), KIFS_ERR_BAD_ARG);
    // the colour pitch: as the batch call refuses it
    for (size_t pitch : {size_t(W) * 4 - 4, size_t(W) * 4 + 2, size_t(0)})
        refused(kifs_render_folded_trapped_async(c, nullptr, 1, nullptr, b.outs.data(), pitch, &MENGER, &TRAP, &LIGHT_A, nullptr, b.u(), b.ppitch, b.pbytes, 0,
                                                 H, 1),
                KIFS_ERR_BAD_SIZE);
    // the plane: as the occlusion call refuses it -- misaligned, a pitch below the width or no multiple of four (or beyond 32
    // bits of words), a stride no multiple of four, below a band with more than one frame, or beyond 32 bits of words
    auto planed = [&](int count, float* plane, size_t pitch, size_t stride) {
        return kifs_render_folded_trapped_async(c, nullptr, count, count > 1 ? cams : nullptr, b.outs.data(), b.cpitch, &MENGER, &TRAP, &LIGHT_A, &TERM, plane,
                                                pitch, stride, 0, H, 1);
    };
    for (size_t off : {1u, 2u, 3u}) refused(planed(1, reinterpret_cast<float*>(b.plane + off), b.ppitch, b.pbytes), KIFS_ERR_BAD_ARG);
    for (size_t pitch : {size_t(W) * 4 - 4, size_t(W) * 4 + 2, size_t(0), size_t(1) << 34}) refused(planed(1, b.u(), pitch, b.pbytes), KIFS_ERR_BAD_ARG);
    for (size_t stride : {b.pbytes + 2, size_t(1) << 34}) refused(planed(1, b.u(), b.ppitch, stride), KIFS_ERR_BAD_ARG);
    refused(planed(2, b.u(), b.ppitch, size_t(H) * b.ppitch - 4), KIFS_ERR_BAD_ARG);
    refused(planed(2, b.u(), b.ppitch, 0), KIFS_ERR_BAD_ARG);
    // ... and with more than one sample per pixel there is no plane
    for (int k = 2; k <= KIFS_MAX_SUPERSAMPLING; ++k) {
        CHECK(kifs_set_supersampling(c, k) == KIFS_OK);
        refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
    }
    CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
    // an empty band with good arguments: OK, nothing enqueued
    refused(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 7, 7, 1, true), KIFS_OK);
    CHECK(stub_live_device_allocations() == live);
    // the two Julia pipelines have no folded form
    for (uint32_t group : {1u, 2u}) {
        kifs_ctx* j = context(W, H, group, 0);
        refused(call(j, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_BAD_ARG);
        refused(call(j, b, 1, nullptr, nullptr, nullptr, 7, 7, 1), KIFS_ERR_BAD_ARG);
        kifs_destroy(j);
    }
    // a context that is not configured
    int st = 0;
    kifs_ctx* bare = kifs_create(0, &st);
    CHECK(bare && st == KIFS_OK);
    refused(call(bare, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_UNCONFIGURED);
    KifsScreenUniform screen;
    CHECK(kifs_host_screen(W, H, &screen) == KIFS_OK && kifs_set_screen(bare, &screen) == KIFS_OK);
    const KifsOptionsUniform o = options_of(0, 3);
    CHECK(kifs_set_options(bare, &o) == KIFS_OK);
    refused(call(bare, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true), KIFS_ERR_UNCONFIGURED);  // no camera, none given
    CHECK(call(bare, b, 1, cams, &LIGHT_A, &TERM, 0, H, 1, true) == KIFS_OK);                  // ... and one given
    CHECK(fold_trap_stub_launches() == launches + 1 && b.holds_model(1, 0, H, 1, 1, true, 3, 3, 6, true));
    kifs_destroy(bare);
    // the ranges' edges are served, and so is a matrix of NaNs that the stages do not name: it does not travel
    KifsFoldSystem edges[4] = {ALL, ALL, ALL, ALL};
    edges[0].iterations = 0;
    edges[0].stages = 0u;
    edges[1].iterations = KIFS_MAX_FOLD_ITERATIONS;
    edges[1].scale = 16.0f;
    edges[2].scale = 1.0f;
    edges[2].offset[0] = 3.0e38f;
    edges[3].stages = 31u & ~uint32_t(KIFS_FOLD_ROTATE);
    for (float& v : edges[3].rotation) v = nan;
    KifsOrbitTrap tedges[4] = {TRAP, TRAP, TRAP, TRAP};
    tedges[0].iterations = 0;
    tedges[0].axes = 1u;
    tedges[1].iterations = KIFS_MAX_TRAP_ITERATIONS;
    tedges[1].axes = 15u;
    tedges[2].scale = -3.0e38f;
    tedges[2].mid[1] = 0.0f;
    tedges[3].bias = 3.0e38f;
    tedges[3].far[2] = 3.0e38f;
    for (int i = 0; i < 4; ++i) {
        g_fold = &edges[i];
        g_trap = &tedges[i];
        b.fill();
        CHECK(call(c, b, 1, nullptr, nullptr, nullptr, 0, H, 1, i & 1) == KIFS_OK);
        CHECK(b.holds_model(1, 0, H, 1, 1, false, 0, edges[i].iterations, tedges[i].iterations, i & 1));
        CHECK(record_is(fold_trap_stub_last().record, edges[i], tedges[i]));
    }
    g_fold = &MENGER;
    g_trap = &TRAP;
    kifs_destroy(c);
}

void what_a_launch_carries() {
    std::vector<KifsCameraUniform> cams;
    for (int i = 0; i < 64; ++i) cams.push_back(camera_of(0.05f * float(i + 1)));
    for (const uint32_t shape : {0u, 4u, 5u, 17u}) {
        kifs_ctx* c = context(W, H, 0, shape);
        hipStream_t own = nullptr;
        CHECK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking) == hipSuccess);
        // the plain render of this context has its culls on: the launch below is what turns them off
        {
            Buffers p(1, H, W, 0);
            CHECK(kifs_render_async(c, nullptr, p.outs[0], size_t(W) * 4, 0, H, KIFS_ENCODE_SRGB) == KIFS_OK);
            StubRenderLaunch plain{};
            stub_last_render(&plain);
            CHECK((plain.cull != 0) == (shape != 17u));  // (an unknown id has no bounding radius: nothing to cull by)
        }
        const void* records_seen[KIFS_ANIMATION_RING + 1] = {};
        long served = 0;
        for (int count : {1, 3, 64}) {
            Buffers b(count, H, W);
            for (int k = 1; k <= KIFS_MAX_SUPERSAMPLING; ++k) {
                CHECK(kifs_set_supersampling(c, k) == KIFS_OK);
                for (int band = 0; band < 3; ++band) {
                    const int y0 = band == 0 ? 0 : band == 1 ? 5 : 41, y1 = band == 0 ? H : band == 1 ? 30 : H;
                    for (int form = 0; form < 3; ++form) {  // a term and a light; a light alone; neither
                        const bool term = form == 1, lit = form != 2;
                        const bool planed = k == 1 && ((count + band + form) & 1) == 0;  // (with and without a term, over the forms)
                        const int encode = (band + form) & 1;
                        const KifsAmbientOcclusion t{1 + (count + k + band) % 16, 0.01f * float(k), 1.0f / float(band + 1), 0.5f * float(count)};
                        const bool shiny = ((count + k + band) & 1) != 0;
                        const KifsLight l{{0.3f * float(k) - 1.0f, 0.25f * float(band) + 0.1f, -0.2f * float(count)}, 0.05f * float(k), 1.0f / float(count),
                                          {shiny ? 0.5f : 0.0f, 0.0f, shiny ? 0.25f * float(band) : 0.0f}, (count + 3 * k + band) % 11};
                        // a record of its own for every call: more of them than the ring is deep, one after another
                        const KifsFoldSystem fs{uint32_t((count + 2 * k + 5 * band + 11 * form) % 32), (5 * count + 7 * k + band + form) % 25,
                                                1.0f + 0.37f * float(k) + 0.11f * float(band), {0.1f * float(k), -0.7f * float(band), 0.3f * float(count)},
                                                {0.9f, -0.1f * float(k), 0.2f, 0.1f, 0.8f, -0.3f, 0.05f * float(form), 0.25f, 1.1f}};
                        const KifsOrbitTrap tr{{0.1f * float(count), -0.2f * float(k), 0.3f * float(band), 0.05f * float(form)}, 1u + uint32_t((count + k + band + form) % 15),
                                               (3 * count + 5 * k + band + 2 * form) % 33, 0.25f * float(k), -0.1f * float(band),
                                               {0.1f * float(form), 0.2f, 0.3f * float(k)}, {1.0f / float(count), 0.0f, 0.5f}};
                        g_fold = &fs;
                        g_trap = &tr;
                        const int e_of = lit ? l.shininess_log2 : 0;
                        void* stream = (band == 1) ? own : nullptr;
                        b.fill();
                        const long launches = fold_trap_stub_launches(), renders = stub_launches();
                        CHECK(call(c, b, count, count == 1 && band == 0 ? nullptr : cams.data(), lit ? &l : nullptr, term ? &t : nullptr, y0, y1, encode, planed,
                                   stream) == KIFS_OK);
                        g_fold = &MENGER;
                        g_trap = &TRAP;
                        CHECK(fold_trap_stub_launches() == launches + 1 && stub_launches() == renders);  // one launch, no sort
                        CHECK(b.holds_model(count, y0, y1, encode, k, term, e_of, fs.iterations, tr.iterations, planed));
                        const FoldTrapStubLaunch& L = fold_trap_stub_last();
                        const kifs::foldorbit::Params& O = L.params;
                        const kifs::FrameParams& P = O.B.frame;
                        CHECK(L.group == 0u && L.primitive == shape);
                        CHECK(stream ? L.stream == own : (L.stream != nullptr && L.stream != own));
                        // the record as the copy left it when the launch read it: this call's, not a neighbour's in the ring
                        CHECK(record_is(L.record, fs, tr));
                        // ... in a slot of the ring, which comes round after KIFS_ANIMATION_RING calls
                        const void* slot = O.record;
                        if (served >= KIFS_ANIMATION_RING) CHECK(slot == records_seen[served % KIFS_ANIMATION_RING]);
                        for (long j = 1; j < KIFS_ANIMATION_RING && j <= served; ++j) CHECK(slot != records_seen[(served - j) % KIFS_ANIMATION_RING]);
                        records_seen[served % KIFS_ANIMATION_RING] = slot;
                        ++served;
                        // every cull is off: the per-ray cull, the wave-level quick exit and the tile-level one
                        CHECK(P.cull_n2 == 0.0f && P.quick_cull_n2 == 0.0f && P.tile_cull_beta == 0.0f && P.tile_cull_sqrtk == 0.0f);
                        // the plane
                        CHECK(O.plane == (planed ? b.u() : nullptr));
                        CHECK(!planed || (O.pitch_words == b.ppitch / 4 && O.stride_words == b.pbytes / 4));
                        const KifsLight& given = lit ? l : REFERENCE;
                        float unit[3];
                        unit_of(given.direction, unit);
                        CHECK(std::memcmp(&O.light.direction, given.direction, 12) == 0 && std::memcmp(&O.light.unit, unit, 12) == 0);
                        CHECK(O.light.ambient == given.ambient && O.light.diffuse == given.diffuse && std::memcmp(&O.light.specular, given.specular, 12) == 0);
                        CHECK(O.light.shininess_log2 == e_of && O.light.highlight == ((lit && shiny) ? 1u : 0u));
                        CHECK(O.has_ao == (term ? 1u : 0u));
                        CHECK(!term || (O.ao.samples == t.samples && O.ao.step == t.step && O.ao.decay == t.decay && O.ao.strength == t.strength));
                        CHECK(O.B.count == count && !O.B.table);
                        CHECK(P.ssaa == k && P.ssaa_inv_height == 1.0f / (float(k) * float(H)) && P.height == float(H) && P.width == W);
                        CHECK(P.y0 == y0 && P.y1 == y1 && P.encode == encode && P.pitch_words == b.cpitch / 4);
                        CHECK(P.tile_count == 4u * unsigned((y1 - y0 + 7) / 8) && P.tile_order);
                        CHECK(!P.tile_cost && !P.counters && P.round_steps == 0 && P.workgroups_per_cu == 0 && !P.geom && !P.stripe_rows);
                        CHECK(P.out == reinterpret_cast<uint32_t*>(b.outs[0]));
                        const KifsCameraUniform& first = (count == 1 && band == 0) ? camera_of(0.3f) : cams[0];
                        CHECK(std::memcmp(&P.origin, first.origin, 12) == 0 && std::memcmp(&P.m1, first.matrix[1], 12) == 0);
                        for (int v = 0; v < count; ++v) {
                            const kifs::BatchView& view = O.B.view[v];
                            const KifsCameraUniform& cam = (count == 1 && band == 0) ? first : cams[size_t(v)];
                            CHECK(view.out == reinterpret_cast<uint32_t*>(b.outs[size_t(v)]));
                            CHECK(std::memcmp(&view.origin, cam.origin, 12) == 0 && std::memcmp(&view.m0, cam.matrix[0], 12) == 0);
                            CHECK(std::memcmp(&view.m2, cam.matrix[2], 12) == 0);
                        }
                    }
                }
            }
            CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
        }
        Buffers b(1, H, W);
        // kifs_order_after applies to a caller's stream as to any other
        CHECK(kifs_order_after(c, own, nullptr) == KIFS_OK);
        CHECK(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true, own) == KIFS_OK && fold_trap_stub_last().stream == own);
        // a failed launch is a runtime error that wrote nothing, and the next call is served
        b.fill();
        fold_trap_stub_fail_next();
        CHECK(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true) == KIFS_ERR_RUNTIME);
        CHECK(b.untouched());
        CHECK(call(c, b, 1, nullptr, &LIGHT_A, &TERM, 0, H, 1, true) == KIFS_OK && b.holds_model(1, 0, H, 1, 1, true, 3, 3, 6, true));
        CHECK(hipStreamDestroy(own) == hipSuccess);
        kifs_destroy(c);
    }
    // a frame tall enough for the tile-level cull (64 rows and more): off as well
    {
        kifs_ctx* c = context(256, 128, 0, 2);
        Buffers b(1, 128, 256);
        CHECK(call(c, b, 1, nullptr, &LIGHT_A, nullptr, 0, 128, 1) == KIFS_OK);
        const kifs::FrameParams& P = fold_trap_stub_last().params.B.frame;
        CHECK(P.cull_n2 == 0.0f && P.quick_cull_n2 == 0.0f && P.tile_cull_beta == 0.0f && P.tile_cull_sqrtk == 0.0f);
        Buffers p(1, 128, 256, 0);
        CHECK(kifs_render_async(c, nullptr, p.outs[0], size_t(256) * 4, 0, 128, KIFS_ENCODE_SRGB) == KIFS_OK);
        StubRenderLaunch plain{};
        stub_last_render(&plain);
        CHECK(plain.cull != 0 && plain.quick_cull != 0 && plain.tile_cull != 0);  // (where the plain render keeps all three)
        kifs_destroy(c);
    }
    // a virtual screen beyond the frame limit is a bad size, as for the batch call
    kifs_ctx* big = context(20000, 64, 0, 2);
    CHECK(kifs_set_supersampling(big, 4) == KIFS_OK);
    uint8_t* out = dev_alloc<uint8_t>(64);
    std::memset(out, SENT, 64);
    const long launches = fold_trap_stub_launches();
    CHECK(kifs_render_folded_trapped_async(big, nullptr, 1, nullptr, &out, size_t(20000) * 4, &MENGER, &TRAP, &LIGHT_A, nullptr, nullptr, 0, 0, 0, 64, 1) ==
          KIFS_ERR_BAD_SIZE);
    CHECK(fold_trap_stub_launches() == launches && out[0] == SENT && out[63] == SENT);
    CHECK(hipFree(out) == hipSuccess);
    kifs_destroy(big);
}

// A failure injected at every HIP call of a call (n-th call from its start) and at its launch (n == 0), on a fresh context
// and on one that has served a call: the call returns KIFS_OK or KIFS_ERR_RUNTIME, a failed call has written nothing
// unless the launch itself went out, nothing leaks, and the calls after it are served with their own records.
void failures() {
    Buffers b(3, H, W);
    std::vector<KifsCameraUniform> cams;
    for (int i = 0; i < 3; ++i) cams.push_back(camera_of(0.2f * float(i + 1)));
    for (int warm = 0; warm < 2; ++warm) {
        int failed = 0;
        bool past_the_end = false;
        for (long n = 0; n < 200 && !past_the_end; ++n) {
            kifs_ctx* c = context(W, H, 0, 4);
            if (warm) CHECK(call(c, b, 3, cams.data(), &LIGHT_A, &TERM, 0, H, 1, true) == KIFS_OK);
            b.fill();
            const long before = stub_calls(), launches = fold_trap_stub_launches();
            if (n == 0) fold_trap_stub_fail_next();
            else stub_fail_in(n);
            g_fold = &ALL;
            const int st = call(c, b, 3, cams.data(), &LIGHT_A, &TERM, 0, H, 1, true);
            g_fold = &MENGER;
            const bool reached = n == 0 || stub_calls() - before >= n;
            stub_fail_in(-1);
            past_the_end = !reached;
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
            if (n == 0) CHECK(st == KIFS_ERR_RUNTIME);
            if (!reached) CHECK(st == KIFS_OK);
            if (st != KIFS_OK) ++failed;
            const bool launched = fold_trap_stub_launches() == launches + 1 && n != 0;
            if (launched) {  // the launch went out (the failure struck behind it, or was survivable): with this call's record
                CHECK(b.holds_model(3, 0, H, 1, 1, true, 3, 8, 6, true));
                CHECK(record_is(fold_trap_stub_last().record, ALL, TRAP));
            } else {
                CHECK(st == KIFS_ERR_RUNTIME && b.untouched());
            }
            // the calls after it, once round the ring and one more: served, each with its record
            bool ok_seen = false;
            for (int k = 0; k < KIFS_ANIMATION_RING + 1; ++k) {
                KifsOrbitTrap t = TRAP;
                t.iterations = k;
                g_trap = &t;
                b.fill();
                const int again = call(c, b, 3, cams.data(), &LIGHT_A, &TERM, 0, H, 1, true);
                g_trap = &TRAP;
                CHECK(again == KIFS_OK || (again == KIFS_ERR_RUNTIME && !ok_seen));
                ok_seen = ok_seen || again == KIFS_OK;
                if (again == KIFS_OK) {
                    CHECK(b.holds_model(3, 0, H, 1, 1, true, 3, 3, k, true));
                    CHECK(record_is(fold_trap_stub_last().record, MENGER, t));
                }
            }
            CHECK(ok_seen);
            kifs_destroy(c);
            CHECK(stub_live_device_allocations() == 2);  // the driver's two buffers
        }
        CHECK(past_the_end && failed >= 3);  // the copy, the launch and the event among them
    }
}

// Animated batches between the calls, on the same ring: each launch reads its own slot.
void interleaved_with_animation() {
    kifs_ctx* c = context(W, H, 0, 4);
    Buffers b(1, H, W);
    const int frames = 5;
    std::vector<KifsOptionsUniform> options;
    std::vector<KifsCameraUniform> cams;
    for (int i = 0; i < frames; ++i) {
        KifsOptionsUniform o = options_of(0, 4);
        o.fractal_color[0] = 0.1f * float(i + 1);
        options.push_back(o);
        cams.push_back(camera_of(0.3f * float(i + 1)));
    }
    const size_t frame_bytes = size_t(W) * size_t(H) * 4;
    uint8_t* dev = dev_alloc<uint8_t>(frame_bytes * size_t(frames));
    std::vector<uint8_t*> outs;
    for (int i = 0; i < frames; ++i) outs.push_back(dev + frame_bytes * size_t(i));
    std::vector<uint8_t> first;
    for (int round = 0; round < 3 * KIFS_ANIMATION_RING; ++round) {
        std::memset(dev, SENT, frame_bytes * size_t(frames));
        CHECK(kifs_render_animation_async(c, nullptr, frames, cams.data(), options.data(), outs.data(), size_t(W) * 4, 0, H, 1) == KIFS_OK);
        if (round == 0) first.assign(dev, dev + frame_bytes * size_t(frames));
        CHECK(std::memcmp(first.data(), dev, first.size()) == 0);  // the animated batch reads its own table, whatever lay in the slot before
        CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ANIMATION);
        for (int rep = 0; rep <= round % 3; ++rep) {  // one to three calls between two batches: every phase of the ring
            KifsFoldSystem f = ALL;
            f.iterations = (round + 3 * rep) % 25;
            KifsOrbitTrap t = TRAP;
            t.iterations = (2 * round + rep) % 33;
            t.centre[1] = float(round);
            g_fold = &f;
            g_trap = &t;
            b.fill();
            CHECK(call(c, b, 1, nullptr, &LIGHT_A, nullptr, 0, H, 1, true) == KIFS_OK);
            g_fold = &MENGER;
            g_trap = &TRAP;
            CHECK(b.holds_model(1, 0, H, 1, 1, false, 3, f.iterations, t.iterations, true));
            CHECK(record_is(fold_trap_stub_last().record, f, t));
            CHECK(kifs_debug_last_kernel(c) == KIFS_KERNEL_ANIMATION);  // left alone
        }
    }
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess);
}

void interleaved_with_renders() {
    // 1024 x 512: 2048 tiles, where the plain launches record costs and sort them
    const int w = 1024, h = 512, frames = 3;
    kifs_ctx* c = context(w, h, 0, 4);
    std::vector<KifsCameraUniform> cams;
    for (int i = 0; i < frames; ++i) cams.push_back(camera_of(0.4f * float(i + 1)));
    const size_t frame_bytes = size_t(w) * size_t(h) * 4;
    uint8_t* dev = dev_alloc<uint8_t>(frame_bytes * size_t(frames));
    std::vector<uint8_t*> outs;
    for (int i = 0; i < frames; ++i) outs.push_back(dev + frame_bytes * size_t(i));
    Buffers b(frames, h, w);
    hipStream_t own = nullptr;
    CHECK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking) == hipSuccess);
    std::vector<uint32_t> order(2048), order_after(2048);
    auto render_all = [&](std::vector<uint8_t>& lone, std::vector<uint8_t>& batch) {
        std::memset(dev, SENT, frame_bytes * size_t(frames));
        CHECK(kifs_render_async(c, nullptr, dev, size_t(w) * 4, 0, h, KIFS_ENCODE_SRGB) == KIFS_OK);
        lone.assign(dev, dev + frame_bytes);
        CHECK(kifs_render_batch_async(c, nullptr, frames, cams.data(), outs.data(), size_t(w) * 4, 0, h, KIFS_ENCODE_SRGB) == KIFS_OK);
        batch.assign(dev, dev + frame_bytes * size_t(frames));
    };
    std::vector<uint8_t> lone[4], batch[4];
    render_all(lone[0], batch[0]);
    for (int round = 1; round < 4; ++round) {
        const int kernel = kifs_debug_last_kernel(c), steps = kifs_debug_last_round_steps(c), tiles = kifs_debug_last_group_tiles(c);
        StubRenderLaunch before{}, after{};
        stub_last_render(&before);
        size_t n = 0;
        CHECK(kifs_debug_get_tile_order(c, order.data(), order.size(), &n) == KIFS_OK && n == 2048);
        const long renders = stub_launches();
        if (round == 2) CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);
        for (int rep = 0; rep < 3; ++rep) {
            const bool term = round != 2, planed = round != 2;
            const int count = rep == 2 ? frames : 1;
            void* stream = (round == 3 && rep == 1) ? own : nullptr;  // (another stream than the plain launches')
            b.fill();
            CHECK(call(c, b, count, count > 1 ? cams.data() : nullptr, &LIGHT_A, term ? &TERM : nullptr, 0, h, 1, planed, stream) == KIFS_OK);
            CHECK(b.holds_model(count, 0, h, 1, round == 2 ? 2 : 1, term, 3, 3, 6, planed));
        }
        stub_last_render(&after);
        CHECK(stub_launches() == renders);  // no render launch, no sort, no support kernel
        CHECK(std::memcmp(&before, &after, sizeof before) == 0);
        CHECK(kifs_debug_last_kernel(c) == kernel && kifs_debug_last_round_steps(c) == steps && kifs_debug_last_group_tiles(c) == tiles);
        CHECK(kifs_debug_get_tile_order(c, order_after.data(), order_after.size(), &n) == KIFS_OK && n == 2048 && order == order_after);
        if (round == 2) CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
        render_all(lone[round], batch[round]);
        CHECK(lone[round] == lone[0] && batch[round] == batch[0]);
    }
    CHECK(hipStreamDestroy(own) == hipSuccess);
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess);
}

}  // namespace

// kifs_eval_fold_trap: host pointers in and out, one launch, nothing left behind.
void evaluation() {
    kifs_ctx* c = context(W, H, 0, 3);
    std::vector<float> pts(3 * 1000), u(1000, -7.0f);
    for (size_t i = 0; i < pts.size(); ++i) pts[i] = 0.001f * float(i);
    CHECK(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), 1, u.data()) == KIFS_OK);  // (a context's first launch: what it allocates once, it keeps)
    u[0] = -7.0f;
    const long evals = fold_trap_stub_evals(), launches = fold_trap_stub_launches(), renders = stub_launches();
    const size_t live = stub_live_device_allocations();
    auto refused = [&](int got, int status) {
        CHECK(got == status);
        CHECK(fold_trap_stub_evals() == evals && fold_trap_stub_launches() == launches && stub_launches() == renders);
        CHECK(stub_live_device_allocations() == live);
        for (float v : u) CHECK(v == -7.0f);
    };
    refused(kifs_eval_fold_trap(nullptr, &MENGER, &TRAP, pts.data(), 10, u.data()), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, nullptr, &TRAP, pts.data(), 10, u.data()), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, &MENGER, nullptr, pts.data(), 10, u.data()), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, &MENGER, &TRAP, nullptr, 10, u.data()), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), 10, nullptr), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), -1, u.data()), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), INT_MIN, u.data()), KIFS_ERR_BAD_ARG);
    for (const KifsFoldSystem& f : bad_systems()) refused(kifs_eval_fold_trap(c, &f, &TRAP, pts.data(), 10, u.data()), KIFS_ERR_BAD_ARG);
    for (const KifsOrbitTrap& t : bad_traps(true)) refused(kifs_eval_fold_trap(c, &MENGER, &t, pts.data(), 10, u.data()), KIFS_ERR_BAD_ARG);
    refused(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), 0, u.data()), KIFS_OK);  // nothing to do
    for (uint32_t group : {1u, 2u}) {
        kifs_ctx* j = context(W, H, group, 0);
        const size_t with_j = stub_live_device_allocations();
        CHECK(kifs_eval_fold_trap(j, &MENGER, &TRAP, pts.data(), 10, u.data()) == KIFS_ERR_BAD_ARG);
        CHECK(fold_trap_stub_evals() == evals && stub_live_device_allocations() == with_j);
        kifs_destroy(j);
    }
    int st = 0;
    kifs_ctx* bare = kifs_create(0, &st);
    CHECK(bare && st == KIFS_OK);
    const size_t with_bare = stub_live_device_allocations();  // (a context's own allocations)
    CHECK(kifs_eval_fold_trap(bare, &MENGER, &TRAP, pts.data(), 10, u.data()) == KIFS_ERR_UNCONFIGURED);
    CHECK(fold_trap_stub_evals() == evals && stub_live_device_allocations() == with_bare);
    kifs_destroy(bare);
    refused(KIFS_OK, KIFS_OK);  // ... all gone with it, and nothing was written
    // the gradient's fields are neither read nor validated
    KifsOrbitTrap wild = TRAP;
    wild.scale = std::numeric_limits<float>::quiet_NaN();
    wild.mid[0] = -1.0f;
    wild.far[2] = std::numeric_limits<float>::infinity();
    for (int n : {1, 255, 256, 257, 1000}) {
        std::fill(u.begin(), u.end(), -7.0f);
        const long before = fold_trap_stub_evals();
        CHECK(kifs_eval_fold_trap(c, &ALL, n == 256 ? &wild : &TRAP, pts.data(), n, u.data()) == KIFS_OK);
        CHECK(fold_trap_stub_evals() == before + 1 && fold_trap_stub_launches() == launches && stub_launches() == renders);
        CHECK(stub_live_device_allocations() == live);
        const FoldTrapStubEval& E = fold_trap_stub_last_eval();
        CHECK(E.group == 0u && E.primitive == 3u && E.params.n == n && E.params.fold.iterations == 8 && E.params.fold.stages == 31u);
        const float kk = ALL.scale - 1.0f, t2 = -(kk * ALL.offset[2]), hh = 0.5f * t2;
        CHECK(E.params.fold.t[2] == t2 && E.params.fold.h == hh && std::memcmp(E.params.fold.R, ALL.rotation, 36) == 0);
        CHECK(std::memcmp(&E.params.trap.centre, TRAP.centre, 16) == 0 && E.params.trap.axes == 7u && E.params.trap.iterations == 6);
        CHECK(E.params.frame.max_iterations == 77);
        for (int i = 0; i < 1000; ++i) CHECK(u[size_t(i)] == (i < n ? fold_trap_model::eval_of(i, 8, 6) + pts[size_t(3 * i)] : -7.0f));
    }
    // the screen the evaluation borrows is given back: a frame after it is the frame before it
    Buffers b(1, H, W);
    CHECK(call(c, b, 1, nullptr, nullptr, nullptr, 0, H, 1, true) == KIFS_OK && b.holds_model(1, 0, H, 1, 1, false, 0, 3, 6, true));
    // a failed launch is a runtime error that leaves nothing allocated, and the next call is served
    std::fill(u.begin(), u.end(), -7.0f);
    const size_t with_frame = stub_live_device_allocations();  // (the frame's destination, the band's tile table, the ring's slot)
    fold_trap_stub_fail_next();
    CHECK(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), 10, u.data()) == KIFS_ERR_RUNTIME);
    CHECK(stub_live_device_allocations() == with_frame);
    for (float v : u) CHECK(v == -7.0f);
    CHECK(kifs_eval_fold_trap(c, &MENGER, &TRAP, pts.data(), 10, u.data()) == KIFS_OK && u[9] == fold_trap_model::eval_of(9, 3, 6) + pts[27]);
    kifs_destroy(c);
}

int main() {
    refusals();
    what_a_launch_carries();
    failures();
    interleaved_with_animation();
    evaluation();
    interleaved_with_renders();
    CHECK(stub_live_device_allocations() == 0);
    CHECK(stub_live_streams_and_events() == 0);
    std::printf("fold_trap_driver: %ld checks ok\n", g_checks);
    return 0;
}
