// tile_memory_driver.cpp -- TEST INFRASTRUCTURE: the tile order's feedback (kifs_schedule.cpp: feedback_before,
// feedback_after, tile_table) against hip_stub.cpp and tile_memory_stub.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer (make -C kifs_raymarching_amd/csrc asan-tile-memory; tests/
// test_tile_memory_host_sanitizers.py).  Batches of three views of a 2048 x 256 Julia frame (64 x 32 tiles: the smallest
// frame with feedback) are walked through record, sort and adopt over many periods.  The stand-in's render writes the same
// costs every time, so the driver plants others in the cost table behind every recording launch and keeps a model of the sort's memory
// (the rule of tile_order_kernel, restated): after every sort the table handed to it must be the planted one, left
// zeroed; the memory must equal the model word for word -- a cost held for `window` sorts, then given up --; the order
// must be the model's; and the launch behind the sort must read the buffer the sort wrote, the two launches after it
// the same one, the launch before it the other.  Lone frames afterwards sort without the memory and leave it alone, and a change of
// options makes the next sort start the memory afresh.  The memory's rule itself is the stand-in's here; the kernel's is held
// on the GPU (tests/test_gpu_tile_cost.py).  Then
// a failure is injected at every HIP call of such a walk in turn, and at the sort's own launch: the call that meets it
// reports it, and the context renders exact frames afterwards.  Prints "tile_memory_driver: N checks ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <utility>
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
struct StubMemorySort {  // tile_memory_stub.cpp: the latest sort with a memory
    uint32_t *cost, *seen, *order;
    uint32_t tile_count, tiles_x, shift, window;
    hipStream_t stream;
    long calls;
};

extern "C" {
void stub_last_render(StubRenderLaunch* out);
void stub_fail_in(long n);
long stub_calls();
size_t stub_live_device_allocations();
size_t stub_live_streams_and_events();
void stub_memory_sort(StubMemorySort* out);
void stub_memory_fail_in(long n);
}

static long g_checks = 0;
#define CHECK(cond)                                                                                \
    do {                                                                                           \
        ++g_checks;                                                                                \
        if (!(cond)) {                                                                             \
            std::fprintf(stderr, "tile_memory_driver: %s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                          \
        }                                                                                          \
    } while (0)

namespace {

constexpr int W = 2048, H = 256, VIEWS = 3, TILES_X = 64, TILES = 64 * 32, PERIOD = 3;
constexpr uint32_t WINDOW = 16;  // rules::ORDER_WINDOW_BATCH
constexpr size_t FRAME = size_t(W) * H * 4;

KifsScreenUniform g_screen;
KifsOptionsUniform g_options;

std::vector<KifsCameraUniform> cameras(int first) {
    std::vector<KifsCameraUniform> out(VIEWS, KifsCameraUniform{});
    for (int i = 0; i < VIEWS; ++i) {
        KifsCameraData c;
        kifs_host_camera_default(&c);
        c.origin_distance = 3.0f + 0.25f * float((first + i) % 7);
        c.phi = 0.37f * float(first + i);
        CHECK(kifs_host_camera(&c, &out[size_t(i)]) == KIFS_OK);
    }
    return out;
}

kifs_ctx* context() {
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    CHECK(kifs_set_screen(c, &g_screen) == KIFS_OK && kifs_set_options(c, &g_options) == KIFS_OK);
    return c;
}

struct Frames {
    uint8_t* dev[VIEWS];
    Frames() {
        for (auto& d : dev) {
            void* p = nullptr;
            CHECK(hipMalloc(&p, FRAME) == hipSuccess);
            d = static_cast<uint8_t*>(p);
        }
    }
    ~Frames() {
        for (auto& d : dev) (void)hipFree(d);
    }
};

// The frames a fresh context renders one by one: what every batch must deliver, whatever its tile order.
std::vector<uint8_t> lone_frames(const std::vector<KifsCameraUniform>& cams) {
    kifs_ctx* c = context();
    std::vector<uint8_t> out(FRAME * cams.size());
    for (size_t i = 0; i < cams.size(); ++i) {
        CHECK(kifs_set_camera(c, &cams[i]) == KIFS_OK);
        CHECK(kifs_render(c, out.data() + i * FRAME, size_t(W) * 4, 0, H, 1) == KIFS_OK);
    }
    kifs_destroy(c);
    return out;
}

int batch(kifs_ctx* c, hipStream_t s, const Frames& f, const std::vector<KifsCameraUniform>& cams) {
    return kifs_render_batch_async(c, s, VIEWS, cams.data(), f.dev, size_t(W) * 4, 0, H, 1);
}

bool frames_equal(const Frames& f, const std::vector<uint8_t>& want) {
    for (int i = 0; i < VIEWS; ++i)
        if (std::memcmp(f.dev[i], want.data() + size_t(i) * FRAME, FRAME) != 0) return false;
    return true;
}

// ---- the model of the sort's memory
struct Model {
    std::vector<uint32_t> seen = std::vector<uint32_t>(TILES, 0u);
    std::vector<uint32_t> sort(const std::vector<uint32_t>& cost, uint32_t shift) {
        std::vector<std::pair<uint32_t, uint32_t>> keyed(TILES);
        for (uint32_t i = 0; i < uint32_t(TILES); ++i) {
            const uint32_t old = seen[i], age = (old & 0xffu) + 1u;
            seen[i] = (cost[i] >= (old >> 8) || age >= WINDOW) ? cost[i] << 8 : ((old & ~0xffu) | age);
            keyed[i] = {1023u - std::min((seen[i] >> 8) >> shift, 1023u), i};
        }
        std::sort(keyed.begin(), keyed.end());
        std::vector<uint32_t> order(TILES);
        for (uint32_t i = 0; i < uint32_t(TILES); ++i) order[i] = (keyed[i].second % TILES_X) | ((keyed[i].second / TILES_X) << 16);
        return order;
    }
};

// Costs for the recording launch `period`: a few hundred tiles with work, one tile with a cost nothing reaches again
// (planted once, in period 2), everything else empty.
std::vector<uint32_t> planted(int period) {
    std::vector<uint32_t> cost(TILES, 0u);
    uint32_t x = 12345u + 977u * uint32_t(period);
    for (int k = 0; k < 300; ++k) {
        x = x * 1664525u + 1013904223u;
        cost[(x >> 8) % TILES] = 1u + (x >> 20) % 1000u;
    }
    cost[777] = period == 2 ? 1040u : 3u;
    return cost;
}

void walk_record_sort_adopt() {
    kifs_ctx* c = context();
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    Frames f;
    Model model;
    StubRenderLaunch r{};
    StubMemorySort m{};
    stub_memory_sort(&m);
    const long sorts0 = m.calls;
    uint32_t* cost_table = nullptr;  // known from the first sort on
    std::vector<uint32_t> cost_now(TILES, 0u);
    int order_before = 0, held_for = -1;
    const int launches = PERIOD * (int(WINDOW) + 6);
    for (int j = 0; j < launches; ++j) {
        const auto cams = cameras(5 * j);
        const int k = j % PERIOD, period = j / PERIOD;
        CHECK(batch(c, s, f, cams) == KIFS_OK);
        stub_last_render(&r);
        CHECK(r.count == VIEWS && r.tile_count == unsigned(TILES) && r.round_steps > 0);
        CHECK((r.tile_cost != 0) == (k == 0));  // the first launch of a period records, no other
        stub_memory_sort(&m);
        CHECK(m.calls - sorts0 == period + (k >= 1 ? 1 : 0));  // one sort per period, in front of its second launch
        if (k == 1) {
            CHECK(m.tile_count == uint32_t(TILES) && m.tiles_x == uint32_t(TILES_X) && m.window == (period == 0 ? 1u : WINDOW) && m.stream == s);  // (the first sort starts the memory)
            CHECK(m.shift <= 31u);
            CHECK(!cost_table || m.cost == cost_table);  // one cost table: the recording launch's
            cost_table = m.cost;
            const std::vector<uint32_t> want = model.sort(cost_now, m.shift);
            for (int i = 0; i < TILES; ++i) CHECK(m.cost[i] == 0u);  // left ready for the next recording launch
            CHECK(std::memcmp(m.seen, model.seen.data(), TILES * 4) == 0);
            CHECK(std::memcmp(m.order, want.data(), TILES * 4) == 0);
            CHECK(r.order != order_before);  // the launch behind the sort reads the buffer the sort wrote
            if (period >= 2 && (model.seen[777] >> 8) == 1040u) held_for = period - 2;
        } else if (j > 0) {
            CHECK(r.order == order_before);  // nothing else moves the order
        }
        order_before = r.order;
        if (j % 7 == 0) CHECK(frames_equal(f, lone_frames(cams)));
        if (k == 0 && cost_table) {  // the recording launch is over (the stand-in is synchronous): its costs
            cost_now = planted(period);
            std::memcpy(cost_table, cost_now.data(), TILES * 4);
        } else if (k == 0) {  // (the table is not known yet: what the stand-in's render wrote stays)
            for (uint32_t i = 0; i < uint32_t(TILES); ++i) cost_now[i] = (i * 2654435761u) >> 20;
        }
    }
    // the cost nothing reached again stayed on top for WINDOW - 1 sorts after its own, then gave way
    CHECK(held_for == int(WINDOW) - 1);
    // lone frames on the same table: their sorts take no memory and leave it alone; the batches go on afterwards
    stub_memory_sort(&m);
    const long before = m.calls;
    const auto cams = cameras(1);
    for (int j = 0; j < 2 * 4; ++j) {
        CHECK(kifs_set_camera(c, &cams[0]) == KIFS_OK);
        CHECK(kifs_render_async(c, s, f.dev[0], size_t(W) * 4, 0, H, 1) == KIFS_OK);
    }
    stub_memory_sort(&m);
    CHECK(m.calls == before && std::memcmp(m.seen, model.seen.data(), TILES * 4) == 0);
    for (int j = 0; j < 2 * PERIOD; ++j) CHECK(batch(c, s, f, cams) == KIFS_OK);
    stub_memory_sort(&m);
    CHECK(m.calls >= before + 1 && m.calls <= before + 3);
    CHECK(frames_equal(f, lone_frames(cams)));
    // another scene: the first sort of its costs starts the memory afresh (a window of one), the later ones remember again
    KifsGuiData gui;
    kifs_host_gui_default(&gui);
    gui.fractal_group = 1;
    gui.max_iterations = 96;
    KifsOptionsUniform other;
    CHECK(kifs_host_options(&gui, &other) == KIFS_OK && kifs_set_options(c, &other) == KIFS_OK);
    stub_memory_sort(&m);
    long seen_sorts = m.calls;
    std::vector<uint32_t> windows;
    for (int j = 0; j < 4 * PERIOD; ++j) {
        CHECK(batch(c, s, f, cams) == KIFS_OK);
        stub_memory_sort(&m);
        if (m.calls != seen_sorts) windows.push_back(m.window);
        seen_sorts = m.calls;
    }
    CHECK(windows.size() >= 3);
    // (a sort of costs recorded before the change may come first)
    const size_t fresh = windows[0] == 1u ? 0 : 1;
    CHECK(windows[fresh] == 1u);
    for (size_t i = 0; i < windows.size(); ++i) CHECK(i == fresh || windows[i] == WINDOW);
    CHECK(kifs_set_options(c, &g_options) == KIFS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    kifs_destroy(c);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

// A failure at the n-th HIP call of a walk of two periods, for every n; then at the sort's launch.
void injected_failures() {
    const auto cams = cameras(3);
    const std::vector<uint8_t> want = lone_frames(cams);
    bool met = true;
    for (long n = 1; met && n < 400; ++n) {
        kifs_ctx* c = context();
        hipStream_t s = nullptr;
        CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
        Frames f;
        const long calls0 = stub_calls();
        stub_fail_in(n);
        int failed = 0;
        for (int j = 0; j < 2 * PERIOD; ++j) {
            const int st = batch(c, s, f, cams);
            if (st != KIFS_OK) ++failed;
            CHECK(st == KIFS_OK || st == KIFS_ERR_RUNTIME);
        }
        met = stub_calls() - calls0 >= n;
        stub_fail_in(-1);
        CHECK(failed <= 1 || !met);
        for (int j = 0; j < PERIOD + 1; ++j) CHECK(batch(c, s, f, cams) == KIFS_OK);  // usable afterwards, frames exact
        CHECK(frames_equal(f, want));
        kifs_destroy(c);
        CHECK(hipStreamDestroy(s) == hipSuccess);
    }
    CHECK(!met);  // the walk has fewer than 400 HIP calls: every one of them was tried
    for (long n = 1; n <= 2; ++n) {
        kifs_ctx* c = context();
        Frames f;
        stub_memory_fail_in(n);
        int failed = 0;
        for (int j = 0; j < 3 * PERIOD; ++j) failed += batch(c, nullptr, f, cams) != KIFS_OK;
        CHECK(failed == 1);
        for (int j = 0; j < PERIOD + 1; ++j) CHECK(batch(c, nullptr, f, cams) == KIFS_OK);
        CHECK(frames_equal(f, want));
        kifs_destroy(c);
    }
}

}  // namespace

int main() {
    CHECK(kifs_host_screen(uint32_t(W), uint32_t(H), &g_screen) == KIFS_OK);
    KifsGuiData gui;
    kifs_host_gui_default(&gui);
    gui.fractal_group = 1;  // Julia: feedback from 2048 tiles
    CHECK(kifs_host_options(&gui, &g_options) == KIFS_OK);
    walk_record_sort_adopt();
    injected_failures();
    CHECK(stub_live_device_allocations() == 0 && stub_live_streams_and_events() == 0);
    std::printf("tile_memory_driver: %ld checks ok\n", g_checks);
    return 0;
}
