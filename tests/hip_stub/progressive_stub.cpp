// progressive_stub.cpp -- TEST INFRASTRUCTURE, never shipped: stand-ins for BOTH accumulate launchers
// (kifs_accumulate_kernels.hip) for progressive_driver.cpp (`make asan-progressive`): launch_accumulate_render as
// accumulate_jitter_stub.cpp has it, and launch_accumulate_carry, which RECORDS the CarryParams a pass carries -- the
// plane, its pitch and stride in texels, the sub-frames already in it, whether the pass has destinations -- and models
// the pass on a plane of 16-byte texels: word 0 is accumulate_model.hpp's fold of the frame's sub-frames (started from
// the texel when prior > 0, from the first sub-frame otherwise: with prior == 0 the texel is NOT read), words 1 and 2
// are derived from it, word 3 holds float(total); the pixel, when the pass has destinations, is the model's pixel of
// (fold, total).  The fold is a left fold, so passes that concatenate to one call's views leave that call's pixel.  Both
// launchers go through the launch's tile table, band, pitches, views and scenes and check that everything they read
// and write lies in "device memory".  progressive_stub_fail_next(): the next launch of either kind fails once.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "accumulate_model.hpp"

namespace {

bool g_fail_next = false;
long g_launches = 0, g_carries = 0;
kifs::accum::CarryParams g_carry{};
std::vector<kifs::anim::SceneView> g_scenes;

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "progressive_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "progressive_stub: %s\n", what);
    std::abort();
}

// One launch of either kind; K null: launch_accumulate_render.
hipError_t run(const kifs::accum::Params& A, uint32_t group, const kifs::accum::CarryParams* K) {
    using namespace kifs;
    ++g_launches;
    if (K) ++g_carries;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    const FrameParams& P = A.B.frame;
    const int views = A.B.count, g = P.ssaa;
    if (A.frames < 1 || A.samples < 1 || A.samples > 64 || views != A.frames * A.samples || views > MAX_BATCH) refuse("frames x samples is not the launch's views");
    if ((A.B.table != nullptr) != (views > MAX_BATCH_INLINE)) refuse("a view table for an inline launch, or none beyond the inline views");
    if (P.tile_cost || P.counters || P.geom || P.stripe_rows || P.round_steps != 0 || P.out_frame_rows) refuse("costs, diagnostics, a geometry plane, stripes or rounds");
    if (g < 1 || g > 8) refuse("a grid outside 1..8");
    if (group > 2u || !A.scenes) refuse("no pipeline or no scene table");
    need_device(A.scenes, sizeof(anim::SceneView) * size_t(views), "the scene table");
    if (A.B.table) need_device(A.B.table, sizeof(BatchView) * size_t(views), "the view table");
    for (int v = 0; v < views; ++v) {
        const uint32_t* pad = A.scenes[v].pad;
        if (pad[1] || pad[2] || pad[3] || (pad[0] >> 16)) refuse("pad words beyond the cell");
        if (int(pad[0] & 0xffu) >= g || int(pad[0] >> 8) >= g) refuse("a cell outside its grid");
    }
    const bool picture = !K || K->picture != 0;
    if (K) {
        if (K->picture > 1u) refuse("the picture flag is 0 or 1");
        if (!K->sums || (reinterpret_cast<uintptr_t>(K->sums) & 15u) != 0) refuse("no plane, or a misaligned one");
        if (K->sums_pitch_texels < uint32_t(P.width)) refuse("a plane row shorter than the frame's");
        if (A.frames > 1 && uint64_t(K->sums_stride_texels) < uint64_t(P.y1 - P.y0) * K->sums_pitch_texels) refuse("planes that overlap");
        if (uint64_t(K->prior) + uint64_t(A.samples) > (1ull << 24)) refuse("more sub-frames than float(total) holds");
        g_carry = *K;
        g_scenes.assign(A.scenes, A.scenes + views);
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
        for (int s = 0; s < A.samples; ++s) {
            if (v[s].out != v[0].out) refuse("the sub-frames of a frame carry different destinations");
            if (!picture && v[s].out) refuse("a destination in a pass without a picture");
            if (picture && !v[s].out) refuse("no destination in a pass with a picture");
        }
        for (uint32_t i = 0; i < P.tile_count; ++i) {
            const int x0 = int(P.tile_order[i] & 0xffffu) * TILE_W, x1 = x0 + TILE_W < P.width ? x0 + TILE_W : P.width;
            const int tj = int(P.tile_order[i] >> 16);
            for (int r = 0; r < TILE_H; ++r) {
                const int y = P.y0 + TILE_H * tj + r;
                if (y >= P.y1) break;
                uint32_t* row = picture ? v[0].out + size_t(y - P.y0) * P.pitch_words : nullptr;
                if (picture) need_device(row + x0, size_t(x1 - x0) * 4, "a tile row's pixels");
                uint32_t* texels = nullptr;
                if (K) {
                    texels = reinterpret_cast<uint32_t*>(K->sums) + 4 * (size_t(f) * K->sums_stride_texels + size_t(y - P.y0) * K->sums_pitch_texels);
                    need_device(texels + 4 * x0, size_t(x1 - x0) * 16, "a tile row's texels");
                }
                for (int x = x0; x < x1; ++x) {
                    uint32_t acc = (K && K->prior) ? texels[4 * x] : 0u;
                    for (int s = 0; s < A.samples; ++s) {
                        const anim::SceneView& sc = A.scenes[first + size_t(s)];
                        const uint32_t one = accumulate_model::sample(v[s], sc, g * x + int(sc.pad[0] & 0xffu), g * y + int(sc.pad[0] >> 8));
                        acc = (s == 0 && !(K && K->prior)) ? one : accumulate_model::fold(acc, one);
                    }
                    const uint32_t total = (K ? K->prior : 0u) + uint32_t(A.samples);
                    if (K) {
                        const float w = float(total);
                        texels[4 * x] = acc;
                        texels[4 * x + 1] = ~acc;
                        texels[4 * x + 2] = acc * 3u;
                        std::memcpy(&texels[4 * x + 3], &w, 4);
                    }
                    if (picture) row[x] = accumulate_model::pixel(acc, int(total));
                }
            }
        }
    }
    return hipSuccess;
}

}  // namespace

extern "C" {
void progressive_stub_fail_next() { g_fail_next = true; }
long progressive_stub_launches() { return g_launches; }  // of either kind
long progressive_stub_carries() { return g_carries; }
}
// what the last pass that was not made to fail carried
const kifs::accum::CarryParams& progressive_stub_last_carry() { return g_carry; }
const std::vector<kifs::anim::SceneView>& progressive_stub_last_scenes() { return g_scenes; }

namespace kifs {

hipError_t launch_accumulate_render(const accum::Params& A, uint32_t group, uint32_t, hipStream_t) { return run(A, group, nullptr); }

hipError_t launch_accumulate_carry(const accum::CarryParams& K, uint32_t group, uint32_t, hipStream_t) { return run(K.A, group, &K); }

}  // namespace kifs
