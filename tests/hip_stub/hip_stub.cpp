// hip_stub.cpp -- TEST INFRASTRUCTURE, never shipped: a synchronous in-memory stand-in for the HIP runtime calls and
// the kernel launchers that the HOST side of the library uses (kifs_api.cpp, kifs_schedule.cpp, kifs_shards.cpp,
// kifs_multi.cpp, kifs_host.cpp, kifs_adaptive.cpp, kifs_animation.cpp), so that those 2 700 lines of slot / stream /
// event / buffer bookkeeping can run under
// AddressSanitizer and UndefinedBehaviorSanitizer on a box without a GPU (the GPU pool does not
// offer sanitizers).  `make -C kifs_raymarching_amd/csrc asan` links it with the sanitised host objects into
// build/kifs_host_asan; tests/test_host_sanitizers.py runs that.
//
// What it models: "device memory" is malloc'ed host memory, registered so that hipPointerGetAttributes can tell it from
// host pointers (and a hipFree of something never allocated, or twice, is an error); every asynchronous call executes at
// once -- host call order is one valid serialisation of stream order, because a stream can only wait for an event that
// has already been recorded.  The render "kernel" writes a pattern that depends on the view's camera and the pixel's
// FRAME coordinates only, through the launch's own tile table, stripe table, pitch and in-place flag -- so a gathered
// multi-device frame must equal the frame one context renders, exactly as on the GPU -- and checks that the tile table
// is a permutation.  With diagnostics on it writes the kernel's per-wave records, and a geometry launch its plane of
// texels, each at the kernel's own address and through need_device.  A hipStreamWaitEvent on an event that was never
// recorded aborts: HIP takes it for a wait that is over, so an ordering somebody relied on is missing.  The sparse
// pack / unpack / fill / stripe kernels are restated on the CPU from their documented formats
// (kifs_support_kernels.hip:115-125,184-187,211).  stub_fail_in(n): the n-th HIP call or launch from now on fails once
// (hipErrorOutOfMemory / hipErrorLaunchFailure), for the error paths.  A hipFree under another device than the one that
// was current at the hipMalloc aborts.  KIFS_STUB_TRACE=FILE writes one line per call (see trace() below): two builds of
// the host code are compared call for call by running the driver on both and diffing the files.  A render launch's line
// also says what the launch was told (its shape, which optional tables it got, which culls are on, which of the two order
// buffers it read); stub_last_render() hands the same fields of the latest render launch to the driver.
// The adaptive passes: the geometry texel is (x, y, origin.x, t) with t = +inf where the pixel pattern holds the
// background, so a frame has hits and misses; the classify stand-in applies the header's pair rule to those texels and
// fills the queues and counts; the adaptive render overwrites every queued pixel with a pattern of camera, frame
// coordinates and k.  The animation render is the render pattern with every non-background pixel also a function of the
// view's scene record.  A frame of more than SAMPLE_ABOVE pixels (no scenario but the 4096 x 4096 adaptive one has
// such a frame) gets only a bounded sample of its tiles written and classified: see stub_sampled_tile.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"

struct ihipStream_t { int device; int ordinal; };
struct ihipEvent_t { int device; bool recorded; int ordinal; };

namespace {

int g_devices = [] { const char* e = std::getenv("KIFS_STUB_DEVICES"); return e ? std::atoi(e) : 4; }();
int g_current = 0;
hipError_t g_last = hipSuccess;
long g_fail_in = -1;  // countdown to an injected failure
std::map<uintptr_t, size_t> g_device_mem, g_host_mem;
std::map<uintptr_t, int> g_device_of;  // the device that was current at the hipMalloc
std::map<uintptr_t, int> g_order_ordinal;  // allocations read as a tile order, in order of their first such launch
int g_order_ordinals = 0;
std::set<ihipStream_t*> g_streams;
std::set<ihipEvent_t*> g_events;
long g_calls = 0, g_launches = 0, g_device_syncs = 0, g_stream_waits = 0, g_event_syncs = 0;
long g_device_frees = 0;
std::map<int, long> g_waits_on, g_syncs_on;  // per event ordinal
std::vector<int> g_adaptive_rounds;  // the view count of every adaptive render launch since the driver last asked

hipError_t fail(hipError_t e) { g_last = e; return e; }

// KIFS_STUB_TRACE=FILE: one line per call -- name, current device, stream and event as ordinals in order of creation
// (0: the null stream / no event), bytes of a copy, memset or allocation -- so that two builds of the host code can be
// compared call for call (what the synchronous stub itself cannot see: a wrong stream, a missing wait).
std::FILE* g_trace = [] {
    const char* e = std::getenv("KIFS_STUB_TRACE");
    std::FILE* f = e ? std::fopen(e, "w") : nullptr;
    if (f) std::setvbuf(f, nullptr, _IOLBF, 0);  // line by line: an abort must not lose the tail
    return f;
}();
int g_stream_ordinals = 0, g_event_ordinals = 0;

void trace(const char* call, hipStream_t s = nullptr, hipEvent_t e = nullptr, size_t bytes = 0) {
    if (g_trace) std::fprintf(g_trace, "%s dev=%d stream=%d event=%d bytes=%zu\n", call, g_current, s ? s->ordinal : 0, e ? e->ordinal : 0, bytes);
}

bool injected() {
    ++g_calls;
    if (g_fail_in > 0 && --g_fail_in == 0) { g_fail_in = -1; return true; }
    return false;
}

bool inside(const std::map<uintptr_t, size_t>& m, const void* p, size_t bytes = 1) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto it = m.upper_bound(a);
    if (it == m.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

// Which allocation a launch reads its tile order from: an ordinal given at the allocation's first such launch (0: none).
// Counted apart from the other allocations, so that d_order / d_order_alt keep their names when something else is
// allocated or no longer is.
int order_allocation_of(const void* p) {
    auto it = g_device_mem.upper_bound(reinterpret_cast<uintptr_t>(p));
    if (!p || it == g_device_mem.begin()) return 0;
    --it;
    if (reinterpret_cast<uintptr_t>(p) >= it->first + it->second) return 0;
    int& ordinal = g_order_ordinal[it->first];
    if (!ordinal) ordinal = ++g_order_ordinals;
    return ordinal;
}

void need_device(const void* p, size_t bytes, const char* what) {
    if (bytes && !inside(g_device_mem, p, bytes)) {
        std::fprintf(stderr, "hip_stub: %s touches %zu bytes at %p outside every device allocation\n", what, bytes, p);
        std::abort();
    }
}

}  // namespace

// What the latest render launch was told (host_driver.cpp declares the same struct).
struct StubRenderLaunch {
    int count;
    unsigned tile_count;
    int round_steps, group_tiles, bunny_coop, workgroups_per_cu;
    int tile_cost, counters, geom, stripe_rows, table;  // set or not
    int ssaa, encode, y0, y1;
    int cull, quick_cull, tile_cull;  // on or off
    int order;                        // the allocation the tile order was read from (order_allocation_of)
    int orbit_x2;                     // FrameParams::orbit_x2: the doubled orbit trip is allowed
};
static StubRenderLaunch g_last_render{};

extern "C" {

// ---- test hooks
void stub_last_render(StubRenderLaunch* out) { *out = g_last_render; }
void stub_fail_in(long n) { g_fail_in = n; }
void stub_trace_mark(const char* what) { if (g_trace) std::fprintf(g_trace, "# %s\n", what); }
long stub_calls() { return g_calls; }
long stub_launches() { return g_launches; }
long stub_device_synchronizes() { return g_device_syncs; }
long stub_stream_waits() { return g_stream_waits; }
long stub_event_synchronizes() { return g_event_syncs; }
long stub_device_frees() { return g_device_frees; }
int stub_events_created() { return g_event_ordinals; }  // the ordinal of the newest event
long stub_stream_waits_on(int event_ordinal) { return g_waits_on[event_ordinal]; }
long stub_event_synchronizes_on(int event_ordinal) { return g_syncs_on[event_ordinal]; }
int stub_has_device_allocation_of(size_t bytes) {
    for (const auto& a : g_device_mem)
        if (a.second == bytes) return 1;
    return 0;
}
// The view counts of the adaptive render launches since the last call, oldest first; returns how many there were.
int stub_adaptive_rounds(int* out, int max) {
    const int n = int(g_adaptive_rounds.size());
    for (int i = 0; i < n && i < max; ++i) out[i] = g_adaptive_rounds[size_t(i)];
    g_adaptive_rounds.clear();
    return n;
}
size_t stub_live_device_allocations() { return g_device_mem.size(); }
size_t stub_live_streams_and_events() { return g_streams.size() + g_events.size() + g_host_mem.size(); }

// ---- devices
hipError_t hipGetDeviceCount(int* n) { *n = g_devices; return g_devices > 0 ? hipSuccess : fail(hipErrorNoDevice); }
hipError_t hipGetDevice(int* d) { *d = g_current; return hipSuccess; }
hipError_t hipSetDevice(int d) {
    if (d < 0 || d >= g_devices) return fail(hipErrorInvalidDevice);
    g_current = d;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { trace("hipDeviceSynchronize"); ++g_device_syncs; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t attr, int device) {
    trace("hipDeviceGetAttribute");
    if (injected()) return fail(hipErrorInvalidDevice);
    if (attr != hipDeviceAttributeMultiprocessorCount || device < 0 || device >= g_devices) return fail(hipErrorInvalidValue);
    *value = 256;
    return hipSuccess;
}
hipError_t hipDeviceCanAccessPeer(int* can, int a, int b) { *can = a != b; return hipSuccess; }
hipError_t hipDeviceEnablePeerAccess(int, unsigned) { return hipSuccess; }
hipError_t hipGetLastError(void) { hipError_t e = g_last; g_last = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }

// ---- memory
hipError_t hipMalloc(void** p, size_t bytes) {
    trace("hipMalloc", nullptr, nullptr, bytes);
    if (injected()) return fail(hipErrorOutOfMemory);
    *p = std::malloc(bytes ? bytes : 1);
    if (!*p) return fail(hipErrorOutOfMemory);
    std::memset(*p, 0xCD, bytes);  // fresh device memory holds garbage: nobody may rely on zeros
    g_device_mem[reinterpret_cast<uintptr_t>(*p)] = bytes ? bytes : 1;
    g_device_of[reinterpret_cast<uintptr_t>(*p)] = g_current;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    trace("hipFree");
    auto it = g_device_mem.find(reinterpret_cast<uintptr_t>(p));
    if (it == g_device_mem.end()) {
        std::fprintf(stderr, "hip_stub: hipFree(%p): not a live device allocation\n", p);
        std::abort();
    }
    if (g_device_of[it->first] != g_current) {  // HIP would find the owner; the library frees under the device it allocated under
        std::fprintf(stderr, "hip_stub: hipFree(%p) under device %d: allocated under device %d\n", p, g_current, g_device_of[it->first]);
        std::abort();
    }
    g_device_of.erase(it->first);
    g_order_ordinal.erase(it->first);
    g_device_mem.erase(it);
    ++g_device_frees;
    std::free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    trace("hipHostMalloc", nullptr, nullptr, bytes);
    if (injected()) return fail(hipErrorOutOfMemory);
    *p = std::malloc(bytes ? bytes : 1);
    g_host_mem[reinterpret_cast<uintptr_t>(*p)] = bytes ? bytes : 1;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    if (!p) return hipSuccess;
    trace("hipHostFree");
    if (!g_host_mem.erase(reinterpret_cast<uintptr_t>(p))) std::abort();
    std::free(p);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p) {
    std::memset(a, 0, sizeof *a);
    if (inside(g_device_mem, p)) { a->type = hipMemoryTypeDevice; return hipSuccess; }
    if (inside(g_host_mem, p)) { a->type = hipMemoryTypeHost; return hipSuccess; }
    return fail(hipErrorInvalidValue);  // plain host memory: what the real runtime says too
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { trace("hipMemcpy", nullptr, nullptr, n); if (n) std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
    trace("hipMemcpyAsync", st, nullptr, n);
    if (injected()) return fail(hipErrorLaunchFailure);
    if (n) std::memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyPeerAsync(void* d, int, const void* s, int, size_t n, hipStream_t st) {
    trace("hipMemcpyPeerAsync", st, nullptr, n);
    if (injected()) return fail(hipErrorLaunchFailure);
    need_device(d, n, "hipMemcpyPeerAsync(dst)");
    need_device(s, n, "hipMemcpyPeerAsync(src)");
    if (n) std::memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t st) {
    trace("hipMemcpy2DAsync", st, nullptr, w * h);
    for (size_t y = 0; y < h; ++y) std::memmove(static_cast<char*>(d) + y * dp, static_cast<const char*>(s) + y * sp, w);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) { trace("hipMemset", nullptr, nullptr, n); need_device(d, n, "hipMemset"); std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
    trace("hipMemsetAsync", st, nullptr, n);
    need_device(d, n, "hipMemsetAsync");
    std::memset(d, v, n);
    return hipSuccess;
}

// ---- streams and events (everything has already happened by the time anybody asks)
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    if (injected()) return fail(hipErrorOutOfMemory);
    *s = new ihipStream_t{g_current, ++g_stream_ordinals};
    g_streams.insert(*s);
    trace("hipStreamCreateWithFlags", *s);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    if (!g_streams.erase(s)) std::abort();
    trace("hipStreamDestroy", s);
    delete s;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { if (s && !g_streams.count(s)) std::abort(); trace("hipStreamSynchronize", s); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    if ((s && !g_streams.count(s)) || !g_events.count(e)) std::abort();  // a destroyed stream or event
    trace("hipStreamWaitEvent", s, e);
    ++g_stream_waits;
    ++g_waits_on[e->ordinal];
    if (!e->recorded) {  // HIP takes this for a wait that is already over: whoever meant to order two streams has not
        std::fprintf(stderr, "hip_stub: hipStreamWaitEvent on an event that was never recorded\n");
        std::abort();
    }
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    if (injected()) return fail(hipErrorOutOfMemory);
    *e = new ihipEvent_t{g_current, false, ++g_event_ordinals};
    g_events.insert(*e);
    trace("hipEventCreate", nullptr, *e);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) {
    if (!g_events.erase(e)) std::abort();
    trace("hipEventDestroy", nullptr, e);
    delete e;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (injected()) return fail(hipErrorLaunchFailure);
    if (!g_events.count(e) || (s && !g_streams.count(s))) std::abort();
    trace("hipEventRecord", s, e);
    e->recorded = true;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) { if (!g_events.count(e)) std::abort(); trace("hipEventSynchronize", nullptr, e); ++g_event_syncs; ++g_syncs_on[e->ordinal]; return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t e) { if (!g_events.count(e)) std::abort(); trace("hipEventQuery", nullptr, e); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    if (!g_events.count(a) || !g_events.count(b)) std::abort();
    trace("hipEventElapsedTime", nullptr, b);
    if (!a->recorded || !b->recorded) return fail(hipErrorInvalidHandle);
    *ms = 0.125f;
    return hipSuccess;
}

}  // extern "C"

// ---- the launchers of kifs_internal.hpp, on the CPU ------------------------------------------------------------------
namespace kifs {

namespace {
constexpr int TW = 32, TH = 8;

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// The stand-in for a pixel's colour: a function of the camera and the pixel's frame coordinates.  A quarter of the
// 32 x 8 tiles hold something, the rest is background (so the sparse gather has both kinds).
uint32_t stub_key(const BatchView& v) {
    return bits(v.origin.x) * 2654435761u ^ bits(v.origin.y) * 40503u ^ bits(v.origin.z) * 69069u ^ bits(v.m1.x);
}
bool stub_hit(uint32_t key, int x, int y) { return (((unsigned(x) >> 5) + 3u * (unsigned(y) >> 3) + (key >> 7)) & 3u) == 0u; }
uint32_t stub_pixel(const BatchView& v, int x, int y, uint32_t background) {
    const uint32_t key = stub_key(v);
    if (!stub_hit(key, x, y)) return background;
    uint32_t c = (unsigned(x) * 73856093u ^ unsigned(y) * 19349663u ^ key) | 0xff000000u;
    return c == background ? c ^ 1u : c;
}
// The geometry texel's t: a hit where the pixel pattern holds something, a miss (+inf) where it holds the background.
float stub_depth(const BatchView& v, int x, int y) {
    return stub_hit(stub_key(v), x, y) ? v.origin.z + 0.25f * float((x + 2 * y) & 3) : INFINITY;
}
// What the adaptive render writes over an edge pixel: the camera, the frame coordinates and k.
uint32_t stub_adaptive_pixel(const BatchView& v, int x, int y, int k) {
    return (unsigned(x) * 2246822519u ^ unsigned(y) * 3266489917u ^ stub_key(v) * 668265263u ^ unsigned(k) * 374761393u) | 0xff000000u;
}
// What an animated frame's scene adds to every pixel that is not background: all of the record but its padding.
uint32_t stub_scene_key(const anim::SceneView& s) {
    const float f[11] = {s.c.x, s.c.y, s.c.z, s.c.w, s.power, s.fractal_color.x, s.fractal_color.y, s.fractal_color.z,
                         s.background_color.x, s.background_color.y, s.background_color.z};
    uint32_t k = 2166136261u;
    for (float v : f) k = (k ^ bits(v)) * 16777619u;
    return k & 0x00ffffffu;
}
// A frame of more than SAMPLE_ABOVE pixels is too much per-pixel work under the sanitizers: the render and classify
// stand-ins then check the extents of everything they would touch through need_device as always, but write and
// classify only the tiles of this sample (every 32nd tile column and the one beside it, every 64th tile row, and the
// last of each: every camera's pattern then has hits, misses and a border between them in it), and a
// neighbour outside the sample does not exist for the pair rule.  The driver's model does the same.
constexpr size_t SAMPLE_ABOVE = size_t(1) << 23;
bool stub_sampled_tile(int tiles_x, int tiles_y, int tx, int tj) {
    return (tx % 32 <= 1 || tx == tiles_x - 1) && (tj % 64 == 0 || tj == tiles_y - 1);
}
}  // namespace

namespace {
void stub_render(const BatchParams& B, const anim::SceneView* scenes);
}

hipError_t launch_render(const BatchParams& B, uint32_t, uint32_t, hipStream_t st) {
    ++g_launches;
    const FrameParams& P = B.frame;
    const StubRenderLaunch L = {B.count, P.tile_count, P.round_steps, P.group_tiles, P.bunny_coop, P.workgroups_per_cu,
                                P.tile_cost != nullptr, P.counters != nullptr, P.geom != nullptr, P.stripe_rows != nullptr, B.table != nullptr,
                                P.ssaa, P.encode, P.y0, P.y1, P.cull_n2 != 0.0f, P.quick_cull_n2 != 0.0f, P.tile_cull_beta != 0.0f,
                                order_allocation_of(P.tile_order), P.orbit_x2 != 0};
    g_last_render = L;
    if (g_trace)
        std::fprintf(g_trace, "launch_render dev=%d stream=%d count=%d tiles=%u rounds=%d group_tiles=%d bunny=%d per_cu=%d cost=%d counters=%d "
                              "geom=%d stripes=%d table=%d ssaa=%d encode=%d y=%d..%d culls=%d%d%d order=%d\n", g_current, st ? st->ordinal : 0,
                     L.count, L.tile_count, L.round_steps, L.group_tiles, L.bunny_coop, L.workgroups_per_cu, L.tile_cost, L.counters, L.geom,
                     L.stripe_rows, L.table, L.ssaa, L.encode, L.y0, L.y1, L.cull, L.quick_cull, L.tile_cull, L.order);
    if (injected()) return fail(hipErrorLaunchFailure);
    stub_render(B, nullptr);
    return hipSuccess;
}

namespace {
// The pixels, texels, wave records and tile costs of a render launch; `scenes` non-null: an animated one.
void stub_render(const BatchParams& B, const anim::SceneView* scenes) {
    const FrameParams& P = B.frame;
    const int tiles_x = (P.width + TW - 1) / TW, tiles_y = (P.y1 - P.y0 + TH - 1) / TH;
    const bool sample = !P.stripe_rows && size_t(P.width) * size_t(P.y1 - P.y0) > SAMPLE_ABOVE;
    // the tile table must name every tile of the launch exactly once
    std::vector<char> seen;
    for (int f = 0; f < B.count; ++f) {
        if (B.table) need_device(B.table + f, sizeof(BatchView), "render: a view of the table");
        const BatchView& v = B.table ? B.table[f] : B.view[f];
        uint32_t* out = v.out;
        uint32_t background = P.background_rgba, scene_key = 0;
        if (scenes) {
            need_device(scenes + f, sizeof(anim::SceneView), "render: a scene record");
            background = scenes[f].background_rgba;
            scene_key = stub_scene_key(scenes[f]);
        }
        if (sample) {  // (what the tiles left out would have touched)
            const size_t rows = size_t(P.y1 - P.y0);
            need_device(out + (P.out_frame_rows ? size_t(P.y0) * P.pitch_words : 0), ((rows - 1) * P.pitch_words + size_t(P.width)) * 4, "render: a view's rows");
            if (P.geom)
                need_device(P.geom + 4 * size_t(f) * P.geom_stride_texels, ((rows - 1) * P.geom_pitch_texels + size_t(P.width)) * 16, "render: a view's plane");
        }
        seen.assign(size_t(P.tile_count), 0);
        need_device(P.tile_order, size_t(P.tile_count) * 4, "render: tile order");
        for (uint32_t i = 0; i < P.tile_count; ++i) {
            const uint32_t tx = P.tile_order[i] & 0xffffu, tj = P.tile_order[i] >> 16;
            if (int(tx) >= tiles_x) { std::fprintf(stderr, "hip_stub: tile column %u outside the frame\n", tx); std::abort(); }
            const size_t flat = size_t(tj) * size_t(tiles_x) + tx;
            if (flat >= seen.size() || seen[flat]) { std::fprintf(stderr, "hip_stub: the tile table is not a permutation\n"); std::abort(); }
            seen[flat] = 1;
            if (sample && !stub_sampled_tile(tiles_x, tiles_y, int(tx), int(tj))) continue;
            int base;
            if (P.stripe_rows) {
                need_device(P.stripe_rows + tj, 4, "render: stripe table");
                base = int(P.stripe_rows[tj]);
            } else {
                base = P.y0 + TH * int(tj);
            }
            for (int r = 0; r < TH; ++r) {
                const int y = base + r;
                if (y >= P.y1) break;
                const size_t row = P.out_frame_rows ? size_t(y) : (P.stripe_rows ? size_t(TH) * tj + size_t(r) : size_t(y - P.y0));
                const int x0 = int(tx) * TW, x1 = std::min(x0 + TW, P.width);
                need_device(out + row * P.pitch_words + x0, size_t(x1 - x0) * 4, "render: a tile row's pixels");
                for (int x = x0; x < x1; ++x) {
                    uint32_t* dst = out + row * P.pitch_words + x;
                    *dst = stub_pixel(v, x, y, background);
                    if (scenes && *dst != background) *dst ^= scene_key;
                    if (P.geom) {  // the geometry plane: rows of a band packed, one plane per view (kifs_geometry_kernels.hip:62-66)
                        float* texel = P.geom + 4 * (size_t(f) * P.geom_stride_texels + (size_t(TH) * tj + size_t(r)) * P.geom_pitch_texels + size_t(x));
                        need_device(texel, 16, "render: a geometry texel");
                        const float value[4] = {float(x), float(y), v.origin.x, stub_depth(v, x, y)};
                        std::memcpy(texel, value, sizeof value);
                    }
                }
            }
        }
    }
    if (P.counters) {  // the diagnostics: one 4-word record per wave, four waves per workgroup, tile_count * count workgroups
        const size_t workgroups = size_t(P.tile_count) * size_t(B.count);  // (kifs_scene.hpp: counters + 8 + 4 * (blockIdx.x * 4 + wave))
        for (size_t g = 0; g < workgroups; ++g)
            for (size_t wave = 0; wave < 4; ++wave) {
                unsigned long long* rec = P.counters + 8 + 4 * (g * 4 + wave);
                need_device(rec, 4 * sizeof(unsigned long long), "render: a wave record");
                rec[0] = 1000 + g;
                rec[1] = wave;
                rec[2] = rec[3] = 1;
            }
    }
    if (P.tile_cost) {  // the feedback's per-tile costs: something the sort can chew on
        need_device(P.tile_cost, size_t(P.tile_count) * 4, "render: tile costs");
        for (uint32_t i = 0; i < P.tile_count; ++i) P.tile_cost[i] = (i * 2654435761u) >> 20;
    }
}

// The pair rule of include/kifs_hip.h ("pair") on two texels (n.x, n.y, n.z, t), f32.
bool stub_pair(const float* p, const float* q, float normal_cos, float depth_rel) {
    const bool hp = bits(p[3]) != 0x7f800000u, hq = bits(q[3]) != 0x7f800000u;
    if (hp != hq) return true;
    if (!hp) return false;
    const float d = (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2];
    return !(d >= normal_cos) || std::fabs(p[3] - q[3]) > depth_rel * std::fmin(p[3], q[3]);
}
}  // namespace

hipError_t launch_animation_render(const anim::Params& A, uint32_t, uint32_t, hipStream_t st) {
    ++g_launches;
    const FrameParams& P = A.B.frame;
    if (g_trace)
        std::fprintf(g_trace, "launch_animation_render dev=%d stream=%d count=%d tiles=%u table=%d encode=%d y=%d..%d order=%d\n", g_current,
                     st ? st->ordinal : 0, A.B.count, P.tile_count, A.B.table != nullptr, P.encode, P.y0, P.y1, order_allocation_of(P.tile_order));
    if (injected()) return fail(hipErrorLaunchFailure);
    if (P.tile_cost || P.counters || P.geom || P.stripe_rows || P.round_steps != 0) {
        std::fprintf(stderr, "hip_stub: an animated launch with costs, diagnostics, a plane, stripes or rounds\n");
        std::abort();
    }
    stub_render(A.B, A.scenes);
    return hipSuccess;
}

hipError_t launch_adaptive_classify(const float* planes, uint32_t stride_texels, int width, int height, int count, float normal_cos,
                                    float depth_rel, uint32_t* queues, uint32_t* counts, hipStream_t st) {
    ++g_launches;
    if (g_trace)
        std::fprintf(g_trace, "launch_adaptive_classify dev=%d stream=%d count=%d width=%d height=%d stride=%u\n", g_current, st ? st->ordinal : 0,
                     count, width, height, stride_texels);
    if (injected()) return fail(hipErrorLaunchFailure);
    const uint32_t capacity = stride_texels;  // (as the real launcher hands it to the kernel)
    const int tiles_x = (width + TW - 1) / TW, tiles_y = (height + TH - 1) / TH;
    const bool sample = size_t(width) * size_t(height) > SAMPLE_ABOVE;
    for (int view = 0; view < count; ++view) {
        const float* plane = planes + 4 * size_t(view) * stride_texels;
        uint32_t* queue = queues + size_t(view) * capacity;
        need_device(plane, size_t(width) * size_t(height) * 16, "classify: a view's plane");
        need_device(queue, size_t(capacity) * 4, "classify: a view's queue");
        need_device(counts + view, 4, "classify: a view's count");
        if (counts[view] != 0) { std::fprintf(stderr, "hip_stub: classify: the edge count was not cleared\n"); std::abort(); }
        // the block's layout as kifs_adaptive.cpp states it: planes | queues | counters of THIS launch's views, nothing between
        if (static_cast<const void*>(queues) != planes + 4 * size_t(count) * stride_texels || counts != queues + size_t(count) * capacity) {
            std::fprintf(stderr, "hip_stub: classify: the scratch block is not planes | queues | counters of %d views\n", count);
            std::abort();
        }
        const auto exists = [&](int x, int y) {
            return x >= 0 && y >= 0 && x < width && y < height && (!sample || stub_sampled_tile(tiles_x, tiles_y, x / TW, y / TH));
        };
        const auto texel = [&](int x, int y) { return plane + 4 * (size_t(y) * size_t(width) + size_t(x)); };
        uint32_t n = 0;
        for (int tj = 0; tj < tiles_y; ++tj)
            for (int tx = 0; tx < tiles_x; ++tx) {
                if (sample && !stub_sampled_tile(tiles_x, tiles_y, tx, tj)) continue;
                for (int y = tj * TH; y < std::min(height, tj * TH + TH); ++y)
                    for (int x = tx * TW; x < std::min(width, tx * TW + TW); ++x) {
                        const float* p = texel(x, y);
                        const int nb[4][2] = {{x - 1, y}, {x + 1, y}, {x, y - 1}, {x, y + 1}};
                        bool edge = false;
                        for (const auto& q : nb) edge = edge || (exists(q[0], q[1]) && stub_pair(p, texel(q[0], q[1]), normal_cos, depth_rel));
                        if (!edge) continue;
                        if (n >= capacity) { std::fprintf(stderr, "hip_stub: classify: view %d's queue is full\n", view); std::abort(); }
                        queue[n++] = uint32_t(x) | (uint32_t(y) << 16);
                    }
            }
        counts[view] = n;
    }
    return hipSuccess;
}

hipError_t launch_adaptive_render(const adaptive::Params& A, uint32_t, uint32_t, uint32_t groups_per_view, hipStream_t st) {
    ++g_launches;
    const FrameParams& P = A.B.frame;
    if (g_trace)
        std::fprintf(g_trace, "launch_adaptive_render dev=%d stream=%d count=%d ssaa=%d groups=%u capacity=%u encode=%d\n", g_current,
                     st ? st->ordinal : 0, A.B.count, P.ssaa, groups_per_view, A.capacity, P.encode);
    g_adaptive_rounds.push_back(A.B.count);
    if (injected()) return fail(hipErrorLaunchFailure);
    if (A.B.table || A.B.count < 1 || A.B.count > MAX_BATCH_INLINE || groups_per_view < 1) {
        std::fprintf(stderr, "hip_stub: an adaptive render launch of %d views, table %p, %u groups per view\n", A.B.count, (const void*)A.B.table, groups_per_view);
        std::abort();
    }
    for (int f = 0; f < A.B.count; ++f) {
        const BatchView& v = A.B.view[f];
        need_device(A.counts + f, 4, "adaptive render: a view's count");
        const uint32_t n = std::min(A.counts[f], A.capacity);
        const uint32_t* queue = A.queues + size_t(f) * A.capacity;
        need_device(queue, size_t(n) * 4, "adaptive render: a view's queue");
        for (uint32_t e = 0; e < n; ++e) {
            const int x = int(queue[e] & 0xffffu), y = int(queue[e] >> 16);
            if (x >= P.width || y >= P.y1) { std::fprintf(stderr, "hip_stub: adaptive render: entry (%d, %d) outside the frame\n", x, y); std::abort(); }
            uint32_t* dst = v.out + size_t(y) * P.pitch_words + size_t(x);
            need_device(dst, 4, "adaptive render: a pixel");
            *dst = stub_adaptive_pixel(v, x, y, P.ssaa);
        }
    }
    return hipSuccess;
}

hipError_t launch_tile_order(uint32_t* cost, uint32_t* order, uint32_t tile_count, uint32_t tiles_x, uint32_t shift, hipStream_t st) {
    ++g_launches;
    if (g_trace) std::fprintf(g_trace, "launch_tile_order dev=%d stream=%d tiles=%u tiles_x=%u shift=%u\n", g_current, st ? st->ordinal : 0, tile_count, tiles_x, shift);
    need_device(cost, size_t(tile_count) * 4, "tile_order: costs");
    need_device(order, size_t(tile_count) * 4, "tile_order: order");
    std::vector<std::pair<uint32_t, uint32_t>> keyed(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) keyed[i] = {~(cost[i] >> shift), i};  // descending cost, stable
    std::sort(keyed.begin(), keyed.end());
    for (uint32_t i = 0; i < tile_count; ++i) {
        const uint32_t t = keyed[i].second;
        order[i] = (t % tiles_x) | ((t / tiles_x) << 16);
        cost[t] = 0;
    }
    return hipSuccess;
}

hipError_t launch_unpack_stripes(uint8_t* dst, size_t dst_pitch, size_t dst_frame_stride, const uint8_t* src, size_t src_pitch,
                                 size_t src_shard_stride, const uint32_t* stripe_rows, int n_stripes, int count, int width,
                                 int height, hipStream_t st) {
    ++g_launches;
    trace("launch_unpack_stripes", st);
    if (injected()) return fail(hipErrorLaunchFailure);
    for (int f = 0; f < count; ++f)
        for (int s = 0; s < n_stripes; ++s)
            for (int r = 0; r < TH && int(stripe_rows[s]) + r < height; ++r) {
                uint8_t* d = dst + size_t(f) * dst_frame_stride + (size_t(stripe_rows[s]) + r) * dst_pitch;
                const uint8_t* q = src + size_t(f) * src_shard_stride + (size_t(TH) * s + r) * src_pitch;
                need_device(d, size_t(width) * 4, "unpack_stripes: frame row");
                need_device(q, size_t(width) * 4, "unpack_stripes: shard row");
                std::memcpy(d, q, size_t(width) * 4);
            }
    return hipSuccess;
}

hipError_t launch_pack_sparse(const uint8_t* src, size_t src_pitch, size_t src_shard_stride, const uint32_t* stripe_rows, int n_stripes,
                              int count, int width, int height, uint32_t background, uint32_t* records, uint32_t* n_records, hipStream_t st) {
    ++g_launches;
    trace("launch_pack_sparse", st);
    if (injected()) return fail(hipErrorLaunchFailure);
    const int tiles_x = (width + TW - 1) / TW;
    need_device(n_records, 4, "pack_sparse: count");
    if (*n_records != 0) { std::fprintf(stderr, "hip_stub: pack_sparse: the record count was not cleared\n"); std::abort(); }
    uint32_t n = 0;
    for (int f = 0; f < count; ++f)
        for (int s = 0; s < n_stripes; ++s)
            for (int c = 0; c < tiles_x; ++c) {
                uint32_t px[TH * TW];
                bool any = false;
                for (int r = 0; r < TH; ++r)
                    for (int x = 0; x < TW; ++x) {
                        uint32_t v = background;
                        if (int(stripe_rows[s]) + r < height && c * TW + x < width) {
                            const uint8_t* q = src + size_t(f) * src_shard_stride + (size_t(TH) * s + r) * src_pitch + size_t(c * TW + x) * 4;
                            need_device(q, 4, "pack_sparse: shard pixel");
                            std::memcpy(&v, q, 4);
                        }
                        px[r * TW + x] = v;
                        any = any || v != background;
                    }
                if (!any) continue;
                uint32_t* rec = records + size_t(n) * SPARSE_RECORD_WORDS_HOST;
                need_device(rec, size_t(SPARSE_RECORD_WORDS_HOST) * 4, "pack_sparse: record");
                rec[0] = uint32_t((f * n_stripes + s) * tiles_x + c);
                rec[1] = rec[2] = rec[3] = 0;
                std::memcpy(rec + 4, px, sizeof px);
                ++n;
            }
    *n_records = n;
    return hipSuccess;
}

hipError_t launch_unpack_sparse(uint8_t* dst, size_t dst_pitch, size_t dst_frame_stride, const uint32_t* records, uint32_t n_records,
                                const uint32_t* stripe_rows, int n_stripes, int count, int width, int height, int erase,
                                uint32_t background, hipStream_t st) {
    ++g_launches;
    trace("launch_unpack_sparse", st);
    if (injected()) return fail(hipErrorLaunchFailure);
    const int tiles_x = (width + TW - 1) / TW;
    for (uint32_t i = 0; i < n_records; ++i) {
        const uint32_t* rec = records + size_t(i) * SPARSE_RECORD_WORDS_HOST;
        need_device(rec, size_t(SPARSE_RECORD_WORDS_HOST) * 4, "unpack_sparse: record");
        const uint32_t id = rec[0];
        if (id >= uint32_t(count) * uint32_t(n_stripes) * uint32_t(tiles_x)) continue;
        const int f = int(id / uint32_t(n_stripes * tiles_x)), rest = int(id % uint32_t(n_stripes * tiles_x));
        const int s = rest / tiles_x, c = rest % tiles_x;
        for (int r = 0; r < TH && int(stripe_rows[s]) + r < height; ++r)
            for (int x = 0; x < TW && c * TW + x < width; ++x) {
                uint8_t* d = dst + size_t(f) * dst_frame_stride + (size_t(stripe_rows[s]) + r) * dst_pitch + size_t(c * TW + x) * 4;
                need_device(d, 4, "unpack_sparse: frame pixel");
                const uint32_t v = erase ? background : rec[4 + r * TW + x];
                std::memcpy(d, &v, 4);
            }
    }
    return hipSuccess;
}

hipError_t launch_fill_stripes(uint8_t* dst, size_t dst_pitch, size_t dst_frame_stride, const uint32_t* stripe_rows, int n_stripes,
                               int count, int width, int height, uint32_t background, hipStream_t st) {
    ++g_launches;
    trace("launch_fill_stripes", st);
    if (injected()) return fail(hipErrorLaunchFailure);
    for (int f = 0; f < count; ++f)
        for (int s = 0; s < n_stripes; ++s)
            for (int r = 0; r < TH && int(stripe_rows[s]) + r < height; ++r) {
                uint8_t* d = dst + size_t(f) * dst_frame_stride + (size_t(stripe_rows[s]) + r) * dst_pitch;
                need_device(d, size_t(width) * 4, "fill_stripes: frame row");
                for (int x = 0; x < width; ++x) std::memcpy(d + size_t(x) * 4, &background, 4);
            }
    return hipSuccess;
}

hipError_t launch_eval_points(const FrameParams&, uint32_t, uint32_t, const float*, int n, float* sdf, float* nrm, hipStream_t st) {
    ++g_launches;
    trace("launch_eval_points", st);
    if (sdf) std::memset(sdf, 0, size_t(n) * 4);
    if (nrm) std::memset(nrm, 0, size_t(n) * 12);
    return hipSuccess;
}

hipError_t launch_eval_math(int, const float* in, float, const float*, float* out, int n, hipStream_t st) {
    ++g_launches;
    trace("launch_eval_math", st);
    std::memcpy(out, in, size_t(n) * 4);
    return hipSuccess;
}

}  // namespace kifs
