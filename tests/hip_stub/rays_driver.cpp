// rays_driver.cpp -- TEST INFRASTRUCTURE: drives the host side of kifs_trace_rays_async (kifs_rays.cpp, with the seven
// other host units) against tests/hip_stub/hip_stub.cpp and rays_stub.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make asan-rays`; tests/test_rays_host_sanitizers.py).  A stand-alone CPU program: every
// refusal, with nothing launched, no HIP call made and the outputs untouched; both outputs, either alone; n at 0, 1, 255,
// 256, 257, 1000 and KIFS_MAX_RAYS with the grid the launch gets and the byte extents an int could not hold; the frame
// constants a launch carries -- the options', the iteration counts', the extensions', nothing of a screen, a camera or a
// supersampling factor -- on a context that has none of them and on one that has all three; the stream; a failed launch;
// the existing render calls before, between and after traces on one context, with the same bytes and the same launch
// state; and a final census of what is still alive.  Prints "rays_driver: N checks ok".
#include <hip/hip_runtime_api.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/kifs_hip.h"
#include "rays_model.hpp"

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
long stub_calls();
long stub_launches();
size_t stub_live_device_allocations();
size_t stub_live_streams_and_events();
void rays_stub_fail_next();
long rays_stub_launches();
}
const RaysStubLaunch& rays_stub_last();

static long g_checks = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        ++g_checks;                                                                              \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "rays_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

namespace {

constexpr uint8_t SENT = 0xA5;
constexpr size_t SLACK = 64;  // slots beyond the call's n that must keep the sentinel

template <class T>
T* dev_alloc(size_t count) {
    void* p = nullptr;
    CHECK(hipMalloc(&p, count * sizeof(T)) == hipSuccess);
    return static_cast<T*>(p);
}

KifsOptionsUniform options_of(uint32_t group, uint32_t shape, bool heatmap) {
    KifsGuiData gui;
    kifs_host_gui_default(&gui);
    gui.fractal_group = group;
    gui.primitive_shape = shape;
    gui.max_iterations = 77;
    gui.is_heatmap = heatmap ? 1 : 0;
    KifsOptionsUniform o;
    CHECK(kifs_host_options(&gui, &o) == KIFS_OK);
    return o;
}

// n rays with distinct components, in "device memory", the reserved words poisoned with NaNs: nobody may read them.
KifsRay* make_rays(size_t n) {
    KifsRay* r = dev_alloc<KifsRay>(n + 1);
    uint32_t nan = 0x7fc00000u;
    for (size_t k = 0; k <= n; ++k) {
        for (int i = 0; i < 3; ++i) {
            r[k].origin[i] = 0.25f * float(k % 17) - float(i);
            r[k].direction[i] = float(i + 1) * (k % 2 ? -0.5f : 0.75f) + 0.001f * float(k % 101);
        }
        std::memcpy(&r[k].reserved0, &nan, 4);
        std::memcpy(&r[k].reserved1, &nan, 4);
    }
    return r;
}

struct Outputs {
    float* geom;
    uint8_t* rgba;
    size_t slots;
    explicit Outputs(size_t n) : geom(dev_alloc<float>(4 * (n + SLACK))), rgba(dev_alloc<uint8_t>(4 * (n + SLACK))), slots(n + SLACK) { fill(); }
    void fill() {
        std::memset(geom, SENT, slots * 16);
        std::memset(rgba, SENT, slots * 4);
    }
    bool untouched_from(size_t first, bool g, bool c) const {
        const uint8_t* gb = reinterpret_cast<const uint8_t*>(geom);
        if (g)
            for (size_t i = first * 16; i < slots * 16; ++i)
                if (gb[i] != SENT) return false;
        if (c)
            for (size_t i = first * 4; i < slots * 4; ++i)
                if (rgba[i] != SENT) return false;
        return true;
    }
    ~Outputs() {
        CHECK(hipFree(geom) == hipSuccess);
        CHECK(hipFree(rgba) == hipSuccess);
    }
};

// The first n slots hold the model's words for these rays.
bool holds_model(const Outputs& out, const KifsRay* rays, size_t n, bool g, bool c, int encode) {
    for (size_t k = 0; k < n; ++k) {
        const float* ray = reinterpret_cast<const float*>(rays + k);
        if (g) {
            uint32_t want[4];
            rays_model::texel(ray, k, want);
            if (std::memcmp(out.geom + 4 * k, want, 16) != 0) return false;
        }
        if (c) {
            const uint32_t want = rays_model::pixel(ray, k, encode);
            if (std::memcmp(out.rgba + 4 * k, &want, 4) != 0) return false;
        }
    }
    return true;
}

// A call that must be refused with `status`: nothing launched, no HIP call made, nothing written.
void refused(int got, int status, long launches, long calls, const Outputs& out) {
    CHECK(got == status);
    CHECK(rays_stub_launches() == launches);
    CHECK(stub_calls() == calls);
    CHECK(out.untouched_from(0, true, true));
}

void refusals() {
    const size_t n = 300;
    KifsRay* rays = make_rays(n);
    Outputs out(n);
    const KifsOptionsUniform sphere = options_of(0, 0, false);
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    const long launches = rays_stub_launches();
    long calls = stub_calls();
    // options never set (with otherwise good arguments, n == 0 included); a null context
    refused(kifs_trace_rays_async(c, nullptr, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB), KIFS_ERR_UNCONFIGURED, launches, calls, out);
    refused(kifs_trace_rays_async(c, nullptr, rays, 0, out.geom, out.rgba, KIFS_ENCODE_SRGB), KIFS_ERR_UNCONFIGURED, launches, calls, out);
    refused(kifs_trace_rays_async(nullptr, nullptr, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB), KIFS_ERR_BAD_ARG, launches, calls, out);
    CHECK(kifs_set_options(c, &sphere) == KIFS_OK);
    calls = stub_calls();
    auto bad = [&](const KifsRay* r, int count, float* g, uint8_t* p, int encode) {
        refused(kifs_trace_rays_async(c, nullptr, r, count, g, p, encode), KIFS_ERR_BAD_ARG, launches, calls, out);
    };
    for (int count : {-1, INT_MIN, KIFS_MAX_RAYS + 1, INT_MAX}) bad(rays, count, out.geom, out.rgba, KIFS_ENCODE_SRGB);
    bad(nullptr, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB);
    bad(nullptr, 0, out.geom, out.rgba, KIFS_ENCODE_SRGB);
    for (size_t off : {4u, 8u, 12u, 1u}) {
        bad(reinterpret_cast<const KifsRay*>(reinterpret_cast<const uint8_t*>(rays) + off), int(n) - 1, out.geom, out.rgba, KIFS_ENCODE_SRGB);
        bad(rays, int(n) - 1, reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out.geom) + off), out.rgba, KIFS_ENCODE_SRGB);
        bad(rays, int(n) - 1, reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out.geom) + off), nullptr, KIFS_ENCODE_SRGB);
    }
    for (size_t off : {1u, 2u, 3u}) {
        bad(rays, int(n) - 1, out.geom, out.rgba + off, KIFS_ENCODE_SRGB);
        bad(rays, int(n) - 1, nullptr, out.rgba + off, KIFS_ENCODE_SRGB);
    }
    bad(rays, int(n), nullptr, nullptr, KIFS_ENCODE_SRGB);
    bad(rays, 0, nullptr, nullptr, KIFS_ENCODE_SRGB);
    for (int encode : {-1, 2, 256, INT_MAX}) bad(rays, int(n), out.geom, out.rgba, encode);
    // n == 0 with good arguments: OK, nothing enqueued
    refused(kifs_trace_rays_async(c, nullptr, rays, 0, out.geom, out.rgba, KIFS_ENCODE_UNORM), KIFS_OK, launches, calls, out);
    refused(kifs_trace_rays_async(c, nullptr, rays, 0, out.geom, nullptr, KIFS_ENCODE_SRGB), KIFS_OK, launches, calls, out);
    // and the same arguments with a count are served
    CHECK(kifs_trace_rays_async(c, nullptr, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_OK);
    CHECK(rays_stub_launches() == launches + 1);
    CHECK(holds_model(out, rays, n, true, true, 1) && out.untouched_from(n, true, true));
    kifs_destroy(c);
    CHECK(hipFree(rays) == hipSuccess);
}

void sizes_and_outputs() {
    static_assert(KIFS_MAX_RAYS == 1 << 28, "the header's limit");
    // the grid, restated: one workgroup per 256 rays, and the byte extents of the largest call need 64 bits
    CHECK(kifs::rays::workgroups(0) == 0u && kifs::rays::workgroups(1) == 1u && kifs::rays::workgroups(255) == 1u);
    CHECK(kifs::rays::workgroups(256) == 1u && kifs::rays::workgroups(257) == 2u && kifs::rays::workgroups(1000) == 4u);
    CHECK(kifs::rays::workgroups(KIFS_MAX_RAYS) == (1u << 20) && kifs::rays::workgroups(INT_MAX) == (1u << 23));
    CHECK(uint64_t(KIFS_MAX_RAYS) * 32u == (1ull << 33) && uint64_t(KIFS_MAX_RAYS) * 32u > uint64_t(INT_MAX));
    const size_t most = 1000;
    KifsRay* rays = make_rays(most);
    const KifsOptionsUniform julia = options_of(1, 0, false);
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);  // no screen, no camera
    CHECK(c && st == KIFS_OK);
    CHECK(kifs_set_options(c, &julia) == KIFS_OK);
    for (size_t n : {size_t(1), size_t(255), size_t(256), size_t(257), size_t(1000)}) {
        for (int form = 0; form < 3; ++form) {  // both outputs, geometry only, colour only
            const bool g = form != 2, p = form != 1;
            const int encode = form == 1 ? KIFS_ENCODE_UNORM : KIFS_ENCODE_SRGB;
            Outputs out(n);
            const long launches = rays_stub_launches(), calls = stub_calls();
            CHECK(kifs_trace_rays_async(c, nullptr, rays, int(n), g ? out.geom : nullptr, p ? out.rgba : nullptr, encode) == KIFS_OK);
            CHECK(rays_stub_launches() == launches + 1 && stub_calls() == calls);  // one launch, no other HIP call
            const RaysStubLaunch& L = rays_stub_last();
            CHECK(L.params.n == int(n) && L.workgroups == uint32_t((n + 255) / 256));
            CHECK(L.params.rays == reinterpret_cast<const float*>(rays));
            CHECK(L.params.geom == (g ? out.geom : nullptr) && L.params.rgba == (p ? reinterpret_cast<uint32_t*>(out.rgba) : nullptr));
            CHECK(L.params.frame.encode == encode && L.group == 1u);
            CHECK(holds_model(out, rays, n, g, p, encode));
            CHECK(out.untouched_from(n, g, p) && out.untouched_from(0, !g, !p));  // the slack, and the output not given
        }
    }
    {   // the largest call: recorded, not modelled (the stand-in touches no memory for it)
        Outputs out(8);
        const long launches = rays_stub_launches();
        CHECK(kifs_trace_rays_async(c, nullptr, rays, KIFS_MAX_RAYS, out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_OK);
        CHECK(rays_stub_launches() == launches + 1);
        const RaysStubLaunch& L = rays_stub_last();
        CHECK(L.params.n == KIFS_MAX_RAYS && L.workgroups == (1u << 20));
        CHECK(uint64_t(L.workgroups) * 256u == uint64_t(KIFS_MAX_RAYS));
        CHECK(out.untouched_from(0, true, true));
    }
    kifs_destroy(c);
    CHECK(hipFree(rays) == hipSuccess);
}

bool zero3(const kifs::V3& v) { return v.x == 0.0f && v.y == 0.0f && v.z == 0.0f; }

// What a launch's frame constants must say whatever the context's screen, camera and supersampling factor are.
void check_frame(const kifs::FrameParams& P, const KifsOptionsUniform& o, int sdf, int nrm, int fold, const KifsExtensions& e) {
    CHECK(P.max_iterations == o.max_iterations && P.max_distance == o.max_distance && P.epsilon == o.epsilon);
    CHECK(P.is_heatmap == o.is_heatmap && P.power == o.power);
    CHECK(std::memcmp(&P.c, o.constant, 16) == 0 && std::memcmp(&P.fractal_color, o.fractal_color, 12) == 0);
    CHECK(std::memcmp(&P.background_color, o.background_color, 12) == 0);
    CHECK(P.sdf_iters == sdf && P.normal_iters == nrm && P.fold_iters == fold);
    CHECK(P.orbit_blocks == sdf / 6 && P.orbit_rem == sdf % 6);
    CHECK(P.soft_shadow == e.soft_shadow && P.shadow_steps == e.shadow_steps && P.shadow_k == e.shadow_k);
    CHECK(P.shadow_t0 == e.shadow_t0 && P.shadow_max_t == e.shadow_max_t);
    // nothing of a camera, a screen or a supersampling factor
    CHECK(zero3(P.origin) && P.m0.x == 1.0f && P.m1.y == 1.0f && P.m2.z == 1.0f && P.m0.y == 0.0f && P.m1.x == 0.0f);
    CHECK(P.height == 1.0f && P.aspect == 1.0f && P.width == 1 && P.ssaa == 1);
    CHECK(P.quick_cull_n2 == 0.0f && P.tile_cull_beta == 0.0f && P.round_steps == 0);
    CHECK(!P.tile_order && !P.tile_cost && !P.counters && !P.geom && !P.out && !P.stripe_rows && P.srgb_table);
    // the scene's bounding radius and cull constant, from the options alone
    CHECK(P.bound_n2 > 4.0f && P.bound_n2 < 4.01f && P.fold_n2_stop > 0.0f);
    if (o.is_heatmap) CHECK(P.shape_n2 > 0.0f);  // (the kernel makes no cull test in heatmap mode, whatever cull_n2 says)
    else CHECK(P.cull_n2 > 0.0f && P.cull_n2 <= P.shape_n2);
}

void frame_constants() {
    const size_t n = 64;
    KifsRay* rays = make_rays(n);
    Outputs out(n);
    const KifsExtensions none{};
    const KifsExtensions shadows{1u, 24, 8.0f, 0.02f, 6.0f};
    int st = 0;
    // a context that never had a screen or a camera set
    kifs_ctx* bare = kifs_create(0, &st);
    CHECK(bare && st == KIFS_OK);
    // and one that has all three, with values a leak would show
    kifs_ctx* full = kifs_create(1, &st);
    CHECK(full && st == KIFS_OK);
    KifsScreenUniform screen;
    CHECK(kifs_host_screen(330, 149, &screen) == KIFS_OK);
    KifsCameraData cd;
    kifs_host_camera_default(&cd);
    cd.phi = 0.7f;
    cd.theta = 0.3f;
    KifsCameraUniform cam;
    CHECK(kifs_host_camera(&cd, &cam) == KIFS_OK);
    CHECK(kifs_set_screen(full, &screen) == KIFS_OK && kifs_set_camera(full, &cam) == KIFS_OK);
    CHECK(kifs_set_supersampling(full, 3) == KIFS_OK);
    struct Case { uint32_t group, shape; bool heatmap; int sdf, nrm, fold; const KifsExtensions* ext; float shape_n2; };
    const Case cases[] = {
        {0, 0, false, 100, 10, 10, &none, 1.1f * (1.0f + 1e-4f) * (1.0f + 1e-4f)},   // sphere: B = 1
        {0, 4, false, 100, 10, 7, &shadows, 1.1f * (2.0f + 1e-4f) * (2.0f + 1e-4f)},  // Sierpinski: B = 2
        {1, 0, false, 24, 6, 10, &none, 1.1f * (2.0f + 1e-4f) * (2.0f + 1e-4f)},      // Julia: a certified radius inside
        {1, 0, true, 25, 6, 10, &shadows, 1.1f * (2.0f + 1e-4f) * (2.0f + 1e-4f)},
        {2, 0, false, 8, 4, 10, &none, 1.1f * (2.0f + 1e-4f) * (2.0f + 1e-4f)},
    };
    for (const Case& k : cases) {
        const KifsOptionsUniform o = options_of(k.group, k.shape, k.heatmap);
        for (kifs_ctx* c : {bare, full}) {
            CHECK(kifs_set_options(c, &o) == KIFS_OK && kifs_set_iters(c, k.sdf, k.nrm, k.fold) == KIFS_OK);
            CHECK(kifs_set_extensions(c, k.ext) == KIFS_OK);
            for (int encode : {KIFS_ENCODE_SRGB, KIFS_ENCODE_UNORM}) {
                CHECK(kifs_trace_rays_async(c, nullptr, rays, int(n), out.geom, out.rgba, encode) == KIFS_OK);
                const RaysStubLaunch& L = rays_stub_last();
                check_frame(L.params.frame, o, k.sdf, k.nrm, k.fold, *k.ext);
                CHECK(L.params.frame.encode == encode && L.group == k.group);
                CHECK(k.group != 0u || L.primitive == k.shape);
                const float rel = L.params.frame.shape_n2 / k.shape_n2;
                CHECK(rel > 0.9999f && rel < 1.0001f);
                CHECK(L.stream != nullptr);  // the context's own stream
            }
        }
    }
    // the two launches of one scene carry the same constants bit for bit, screen or none
    const KifsOptionsUniform o = options_of(1, 0, false);
    kifs::FrameParams seen[2];
    int i = 0;
    for (kifs_ctx* c : {bare, full}) {
        CHECK(kifs_set_options(c, &o) == KIFS_OK && kifs_set_iters(c, 12, 10, 10) == KIFS_OK && kifs_set_extensions(c, &none) == KIFS_OK);
        CHECK(kifs_trace_rays_async(c, nullptr, rays, int(n), out.geom, nullptr, KIFS_ENCODE_SRGB) == KIFS_OK);
        seen[i] = rays_stub_last().params.frame;
        seen[i].srgb_table = nullptr;  // (each context owns its table)
        ++i;
    }
    CHECK(std::memcmp(&seen[0], &seen[1], sizeof seen[0]) == 0);
    // a caller's stream is the launch's
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(kifs_trace_rays_async(bare, s, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_OK);
    CHECK(rays_stub_last().stream == s);
    CHECK(kifs_order_after(bare, s, nullptr) == KIFS_OK);  // kifs_order_after applies to that stream as to any other
    CHECK(kifs_trace_rays_async(bare, s, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_OK);
    CHECK(hipStreamDestroy(s) == hipSuccess);
    // a failed launch is a runtime error, and the next call is served
    out.fill();
    rays_stub_fail_next();
    CHECK(kifs_trace_rays_async(bare, nullptr, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_ERR_RUNTIME);
    CHECK(out.untouched_from(0, true, true));
    CHECK(kifs_trace_rays_async(bare, nullptr, rays, int(n), out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_OK);
    CHECK(holds_model(out, rays, n, true, true, 1));
    // the bare context still has no screen: a render is refused as before
    CHECK(kifs_render_async(bare, nullptr, out.rgba, 4, 0, 1, KIFS_ENCODE_SRGB) == KIFS_ERR_UNCONFIGURED);
    kifs_destroy(bare);
    kifs_destroy(full);
    CHECK(hipFree(rays) == hipSuccess);
}

void interleaved_with_renders() {
    const int w = 330, h = 149, frames = 3;
    const size_t n = 500;
    KifsRay* rays = make_rays(n);
    Outputs out(n);
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    KifsScreenUniform screen;
    CHECK(kifs_host_screen(uint32_t(w), uint32_t(h), &screen) == KIFS_OK);
    const KifsOptionsUniform o = options_of(1, 0, false);
    CHECK(kifs_set_screen(c, &screen) == KIFS_OK && kifs_set_options(c, &o) == KIFS_OK);
    std::vector<KifsCameraUniform> cams(size_t(frames), KifsCameraUniform{});
    for (int i = 0; i < frames; ++i) {
        KifsCameraData cd;
        kifs_host_camera_default(&cd);
        cd.phi = 0.4f * float(i + 1);
        CHECK(kifs_host_camera(&cd, &cams[size_t(i)]) == KIFS_OK);
    }
    CHECK(kifs_set_camera(c, &cams[0]) == KIFS_OK);
    const size_t frame_bytes = size_t(w) * size_t(h) * 4;
    uint8_t* dev = dev_alloc<uint8_t>(frame_bytes * size_t(frames));
    float* plane = dev_alloc<float>(size_t(w) * size_t(h) * 4);
    std::vector<uint8_t*> outs;
    for (int i = 0; i < frames; ++i) outs.push_back(dev + frame_bytes * size_t(i));
    auto render_all = [&](std::vector<uint8_t>& lone, std::vector<uint8_t>& batch, std::vector<uint8_t>& geom) {
        std::memset(dev, SENT, frame_bytes * size_t(frames));
        CHECK(kifs_render_async(c, nullptr, dev, size_t(w) * 4, 0, h, KIFS_ENCODE_SRGB) == KIFS_OK);
        lone.assign(dev, dev + frame_bytes);
        CHECK(kifs_render_batch_async(c, nullptr, frames, cams.data(), outs.data(), size_t(w) * 4, 0, h, KIFS_ENCODE_SRGB) == KIFS_OK);
        batch.assign(dev, dev + frame_bytes * size_t(frames));
        CHECK(kifs_render_geometry_async(c, nullptr, 1, nullptr, outs.data(), size_t(w) * 4, plane, size_t(w) * 16, 0, 0, h, KIFS_ENCODE_UNORM) == KIFS_OK);
        geom.assign(reinterpret_cast<uint8_t*>(plane), reinterpret_cast<uint8_t*>(plane) + size_t(w) * size_t(h) * 16);
    };
    std::vector<uint8_t> lone[3], batch[3], geom[3];
    render_all(lone[0], batch[0], geom[0]);
    for (int round = 1; round < 3; ++round) {
        // the launch state a trace must leave alone
        const int kernel = kifs_debug_last_kernel(c), steps = kifs_debug_last_round_steps(c), tiles = kifs_debug_last_group_tiles(c);
        StubRenderLaunch before{}, after{};
        stub_last_render(&before);
        const long renders = stub_launches();
        if (round == 2) CHECK(kifs_set_supersampling(c, 2) == KIFS_OK);  // the factor is not read, and stays
        for (int rep = 0; rep < 3; ++rep) {
            out.fill();
            CHECK(kifs_trace_rays_async(c, nullptr, rays, int(n) - rep, out.geom, out.rgba, KIFS_ENCODE_SRGB) == KIFS_OK);
            CHECK(holds_model(out, rays, n - size_t(rep), true, true, 1) && out.untouched_from(n - size_t(rep), true, true));
            CHECK(rays_stub_last().params.frame.ssaa == 1);
        }
        stub_last_render(&after);
        CHECK(stub_launches() == renders);  // no render launch, no sort, no support kernel
        CHECK(std::memcmp(&before, &after, sizeof before) == 0);
        CHECK(kifs_debug_last_kernel(c) == kernel && kifs_debug_last_round_steps(c) == steps && kifs_debug_last_group_tiles(c) == tiles);
        if (round == 2) {  // the factor the trace did not read is still the context's: a render supersamples
            CHECK(kifs_render_async(c, nullptr, dev, size_t(w) * 4, 0, h, KIFS_ENCODE_SRGB) == KIFS_OK);
            stub_last_render(&after);
            CHECK(after.ssaa == 2);
            CHECK(kifs_set_supersampling(c, 1) == KIFS_OK);
        }
        render_all(lone[round], batch[round], geom[round]);
        CHECK(lone[round] == lone[0] && batch[round] == batch[0] && geom[round] == geom[0]);
    }
    kifs_destroy(c);
    CHECK(hipFree(dev) == hipSuccess && hipFree(plane) == hipSuccess);
    CHECK(hipFree(rays) == hipSuccess);
}

}  // namespace

int main() {
    refusals();
    sizes_and_outputs();
    frame_constants();
    interleaved_with_renders();
    CHECK(stub_live_device_allocations() == 0);
    CHECK(stub_live_streams_and_events() == 0);
    std::printf("rays_driver: %ld checks ok\n", g_checks);
    return 0;
}
