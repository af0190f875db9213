// accumulate_jitter_stub.cpp -- TEST INFRASTRUCTURE, never shipped: a stand-in for launch_accumulate_render
// (kifs_accumulate_kernels.hip) that RECORDS what a launch carries -- its Params and the scene table the host uploaded --
// so that accumulate_jitter_driver.cpp can check every view's cell (pad[0] = i | j << 8), the grid (FrameParams::ssaa)
// and the virtual screen's 1 / height (`make asan-jitter`).  Beside hip_stub.cpp's stand-ins for the HIP runtime and the
// other launchers; accumulate_stub.cpp, which refuses any grid but 1, stays the unjittered driver's.  Like it, this one
// goes through the launch's tile table, band, pitch, views and scenes, checks that everything it reads and writes lies
// in "device memory", that a cell lies inside its grid and that an unjittered launch carries zero pad words; the pixel it
// writes is accumulate_model.hpp's fold of the frame's sub-frames, each sampled at ITS pixel of the virtual screen.
// jitter_stub_fail_next(): the next launch fails once (hipErrorLaunchFailure).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "accumulate_model.hpp"

namespace {

bool g_fail_next = false;
long g_launches = 0;
kifs::accum::Params g_params{};
std::vector<kifs::anim::SceneView> g_scenes;

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "accumulate_jitter_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "accumulate_jitter_stub: %s\n", what);
    std::abort();
}

}  // namespace

extern "C" {
void jitter_stub_fail_next() { g_fail_next = true; }
long jitter_stub_launches() { return g_launches; }
}
// what the last launch that was not made to fail carried
const kifs::accum::Params& jitter_stub_last_params() { return g_params; }
const std::vector<kifs::anim::SceneView>& jitter_stub_last_scenes() { return g_scenes; }

namespace kifs {

hipError_t launch_accumulate_render(const accum::Params& A, uint32_t group, uint32_t, hipStream_t) {
    ++g_launches;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    const FrameParams& P = A.B.frame;
    const int views = A.B.count, g = P.ssaa;
    if (A.frames < 1 || A.samples < 1 || A.samples > 64 || views != A.frames * A.samples || views > MAX_BATCH) refuse("frames x samples is not the launch's views");
    if ((A.B.table != nullptr) != (views > MAX_BATCH_INLINE)) refuse("a view table for an inline launch, or none beyond the inline views");
    if (P.tile_cost || P.counters || P.geom || P.stripe_rows || P.round_steps != 0 || P.out_frame_rows) refuse("costs, diagnostics, a plane, stripes or rounds");
    if (g < 1 || g > 8) refuse("a grid outside 1..8");
    if (group > 2u || !A.scenes) refuse("no pipeline or no scene table");
    need_device(A.scenes, sizeof(anim::SceneView) * size_t(views), "the scene table");
    if (A.B.table) need_device(A.B.table, sizeof(BatchView) * size_t(views), "the view table");
    g_params = A;
    g_scenes.assign(A.scenes, A.scenes + views);
    for (int v = 0; v < views; ++v) {
        const uint32_t* pad = A.scenes[v].pad;
        if (pad[1] || pad[2] || pad[3] || (pad[0] >> 16)) refuse("pad words beyond the cell");
        if (int(pad[0] & 0xffu) >= g || int(pad[0] >> 8) >= g) refuse("a cell outside its grid (an unjittered launch: a pad word that is not zero)");
    }
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
        const size_t first = size_t(f) * size_t(A.samples);
        const BatchView* v = (A.B.table ? A.B.table : A.B.view) + first;
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
                    uint32_t acc = 0;
                    for (int s = 0; s < A.samples; ++s) {
                        const anim::SceneView& sc = A.scenes[first + size_t(s)];
                        const uint32_t one = accumulate_model::sample(v[s], sc, g * x + int(sc.pad[0] & 0xffu), g * y + int(sc.pad[0] >> 8));
                        acc = s == 0 ? one : accumulate_model::fold(acc, one);
                    }
                    row[x] = accumulate_model::pixel(acc, A.samples);
                }
            }
        }
    }
    return hipSuccess;
}

}  // namespace kifs
