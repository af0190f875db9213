// accumulate_stub.cpp -- TEST INFRASTRUCTURE, never shipped: the stand-in for launch_accumulate_render
// (kifs_accumulate_kernels.hip) beside hip_stub.cpp's stand-ins for the HIP runtime and the other launchers, so that the
// host side of kifs_render_accumulate_async (kifs_accumulate.cpp) runs under AddressSanitizer and
// UndefinedBehaviorSanitizer on a box without a GPU (`make asan-accumulate`).  Like the render stand-in it goes through
// the launch's own tile table, band, pitch, view table (or inline views) and scene table, checks that everything it
// reads and writes lies in "device memory" (hipPointerGetAttributes of the first and last byte), that the tile table is a
// permutation and that the launch carries what the host promises; the pixel it writes is accumulate_model.hpp's fold of
// the frame's sub-frames in order.  accumulate_stub_fail_next(): the next launch fails once (hipErrorLaunchFailure).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "accumulate_model.hpp"

namespace {

bool g_fail_next = false;
long g_launches = 0;
int g_last_views = 0, g_last_table = 0;

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "accumulate_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "accumulate_stub: %s\n", what);
    std::abort();
}

}  // namespace

extern "C" {
void accumulate_stub_fail_next() { g_fail_next = true; }
long accumulate_stub_launches() { return g_launches; }
int accumulate_stub_last_views() { return g_last_views; }
int accumulate_stub_last_table() { return g_last_table; }
}

namespace kifs {

hipError_t launch_accumulate_render(const accum::Params& A, uint32_t group, uint32_t, hipStream_t) {
    ++g_launches;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    const FrameParams& P = A.B.frame;
    const int views = A.B.count;
    g_last_views = views;
    g_last_table = A.B.table != nullptr;
    if (A.frames < 1 || A.samples < 1 || A.samples > 64 || views != A.frames * A.samples || views > MAX_BATCH) refuse("frames x samples is not the launch's views");
    if ((A.B.table != nullptr) != (views > MAX_BATCH_INLINE)) refuse("a view table for an inline launch, or none beyond the inline views");
    if (P.tile_cost || P.counters || P.geom || P.stripe_rows || P.round_steps != 0 || P.ssaa != 1 || P.out_frame_rows) refuse("costs, diagnostics, a plane, stripes, rounds or supersampling");
    if (group > 2u || !A.scenes) refuse("no pipeline or no scene table");
    need_device(A.scenes, sizeof(anim::SceneView) * size_t(views), "the scene table");
    if (A.B.table) need_device(A.B.table, sizeof(BatchView) * size_t(views), "the view table");
    need_device(P.tile_order, size_t(P.tile_count) * 4, "the tile order");
    const int tiles_x = (P.width + TILE_W - 1) / TILE_W;
    std::vector<char> seen(size_t(P.tile_count), 0);
    for (uint32_t i = 0; i < P.tile_count; ++i) {
        const uint32_t tx = P.tile_order[i] & 0xffffu, tj = P.tile_order[i] >> 16;
        const size_t flat = size_t(tj) * size_t(tiles_x) + tx;
        if (int(tx) >= tiles_x || flat >= seen.size() || seen[flat]) refuse("the tile table is not a permutation");
        seen[flat] = 1;
    }
    for (int f = 0; f < A.frames; ++f) {
        const BatchView* v = (A.B.table ? A.B.table : A.B.view) + size_t(f) * size_t(A.samples);
        for (int s = 1; s < A.samples; ++s)
            if (v[s].out != v[0].out) refuse("the sub-frames of a frame carry different destinations");
        for (uint32_t i = 0; i < P.tile_count; ++i) {
            const int x0 = int(P.tile_order[i] & 0xffffu) * TILE_W, x1 = x0 + TILE_W < P.width ? x0 + TILE_W : P.width;
            const int tj = int(P.tile_order[i] >> 16);
            for (int r = 0; r < TILE_H; ++r) {
                const int y = P.y0 + TILE_H * tj + r;
                if (y >= P.y1) break;
                uint32_t* row = v[0].out + size_t(y - P.y0) * P.pitch_words;
                need_device(row + x0, size_t(x1 - x0) * 4, "a tile row's pixels");
                for (int x = x0; x < x1; ++x) {
                    uint32_t acc = accumulate_model::sample(v[0], A.scenes[size_t(f) * size_t(A.samples)], x, y);
                    for (int s = 1; s < A.samples; ++s)
                        acc = accumulate_model::fold(acc, accumulate_model::sample(v[s], A.scenes[size_t(f) * size_t(A.samples) + size_t(s)], x, y));
                    row[x] = accumulate_model::pixel(acc, A.samples);
                }
            }
        }
    }
    return hipSuccess;
}

}  // namespace kifs
