// accumulate_family_stub.cpp -- TEST INFRASTRUCTURE, never shipped: the stand-in for the three accumulate launchers
// (kifs_accumulate_kernels.hip) beside hip_stub.cpp's stand-ins for the HIP runtime and the other launchers, so that the
// host side of the accumulated calls runs under AddressSanitizer and UndefinedBehaviorSanitizer on a box without a GPU
// (`make asan-accumulate`, `asan-jitter`, `asan-progressive`, `asan-converge`: one stand-in for the four drivers).
//
// Every launcher goes through the launch's own tile table, band, pitches, view table (or inline views) and scene table
// and checks that everything it reads and writes lies in "device memory" (hipPointerGetAttributes of the first and last
// byte), that the tile table is a permutation and that the launch carries what the host promises: the views are
// frames x samples, a view table exactly beyond the inline views, no costs, diagnostics, geometry plane, stripes or
// rounds, a grid of 1..8, every view's cell inside the grid and no pad word set beyond the cell (an unjittered launch:
// all zero), the sub-frames of a frame with one destination, a destination exactly when the pass has a picture, and
// of a pass every plane-layout rule the API refuses by.  family_stub_expect_grid(g) adds the unjittered driver's rule:
// a launch with any other grid aborts.
//
// The model: launch_accumulate_render writes accumulate_model.hpp's fold of the frame's sub-frames in order, each
// sampled at ITS pixel of the virtual screen.  launch_accumulate_carry models the pass on a plane of 16-byte texels: word
// 0 is the fold (started from the texel when prior > 0, from the first sub-frame otherwise: with prior == 0 the texel is
// NOT read), words 1 and 2 are derived from it, word 3 holds float(total); the fold is a left fold, so passes that
// concatenate to one call's views leave that call's pixel.  launch_accumulate_converge models the pass on the two
// planes with converge_model.hpp: a pixel is active on restart, or when the model's rule says so of the texel and the
// moment it READS; an active pixel's word 0 is the fold (started from the texel unless the pass restarts), its w grows
// by the pass's sub-frames and its moment folds the same samples; an inactive pixel's two texels are not written; every
// pixel of a pass with destinations gets the model's pixel of its state; the pixels active afterwards are ADDED to the
// frame's count, which must have been zeroed before the launch (the stand-in refuses a word that is not).
//
// What the last launch of each kind that was not made to fail carried is recorded: the Params and the uploaded scene
// table of any launch, a carried pass's CarryParams, a converging pass's ConvergeParams.  family_stub_fail_next(): the
// next launch of any kind fails once (hipErrorLaunchFailure).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "converge_model.hpp"

namespace {

bool g_fail_next = false;
int g_expect_grid = 0;  // 0: any
long g_launches = 0, g_carries = 0, g_converges = 0;
kifs::accum::Params g_params{};
std::vector<kifs::anim::SceneView> g_scenes;
kifs::accum::CarryParams g_carry{};
kifs::accum::ConvergeParams g_converge{};

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "accumulate_family_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "accumulate_family_stub: %s\n", what);
    std::abort();
}

// One launch of any kind; C: a carried pass, V: a converging pass, neither: launch_accumulate_render.
hipError_t run(const kifs::accum::Params& A, uint32_t group, const kifs::accum::CarryParams* C, const kifs::accum::ConvergeParams* V) {
    using namespace kifs;
    ++g_launches;
    if (C) ++g_carries;
    if (V) ++g_converges;
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
    if (g_expect_grid && g != g_expect_grid) refuse("a grid other than the one the driver expects");
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
    const bool picture = V ? V->picture != 0 : !C || C->picture != 0;
    float* const sums = V ? V->sums : C ? C->sums : nullptr;
    const uint32_t sums_pitch = V ? V->sums_pitch_texels : C ? C->sums_pitch_texels : 0u;
    const uint32_t sums_stride = V ? V->sums_stride_texels : C ? C->sums_stride_texels : 0u;
    const size_t rows = size_t(P.y1 - P.y0);
    if (C || V) {
        if (!sums || (reinterpret_cast<uintptr_t>(sums) & 15u) != 0) refuse("no plane, or a misaligned one");
        if (sums_pitch < uint32_t(P.width)) refuse("a plane row shorter than the frame's");
        if (A.frames > 1 && uint64_t(sums_stride) < rows * sums_pitch) refuse("planes that overlap");
    }
    if (C) {
        if (C->picture > 1u) refuse("the picture flag is 0 or 1");
        if (uint64_t(C->prior) + uint64_t(A.samples) > (1ull << 24)) refuse("more sub-frames than float(total) holds");
        g_carry = *C;
    }
    if (V) {
        if (V->picture > 1u || V->restart > 1u) refuse("the picture and restart flags are 0 or 1");
        if (!V->moments || (reinterpret_cast<uintptr_t>(V->moments) & 3u) != 0) refuse("no moments plane, or a misaligned one");
        if (V->moments_pitch_words < uint32_t(P.width)) refuse("a moments row shorter than the frame's");
        if (A.frames > 1 && uint64_t(V->moments_stride_words) < rows * V->moments_pitch_words) refuse("moments planes that overlap");
        if (V->min_samples < 2u || V->min_samples > (1u << 24) || !(V->tol2 >= 0.0f)) refuse("a rule the API refuses");
        if (V->counts) {
            need_device(V->counts, size_t(A.frames) * 4, "the counts");
            for (int f = 0; f < A.frames; ++f)
                if (V->counts[f] != 0u) refuse("a count that was not zeroed before the launch");
        }
        g_converge = *V;
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
                uint32_t* words = nullptr;
                if (sums) {
                    texels = reinterpret_cast<uint32_t*>(sums) + 4 * (size_t(f) * sums_stride + size_t(y - P.y0) * sums_pitch);
                    need_device(texels + 4 * x0, size_t(x1 - x0) * 16, "a tile row's texels");
                }
                if (V) {
                    words = reinterpret_cast<uint32_t*>(V->moments) + size_t(f) * V->moments_stride_words + size_t(y - P.y0) * V->moments_pitch_words;
                    need_device(words + x0, size_t(x1 - x0) * 4, "a tile row's moments");
                }
                for (int x = x0; x < x1; ++x) {
                    // the state the pass starts from: read only where the contract reads it
                    const bool from_plane = V ? V->restart == 0u : C && C->prior != 0u;
                    converge_model::Pixel px{};
                    if (from_plane) {
                        px.acc = texels[4 * x];
                        if (V) {
                            std::memcpy(&px.n, &texels[4 * x + 3], 4);
                            px.q = words[x];
                        }
                    }
                    const bool active = !V || V->restart != 0u || converge_model::active(px, V->min_samples, V->tol2, A.samples);
                    if (active) {
                        for (int s = 0; s < A.samples; ++s) {
                            const anim::SceneView& sc = A.scenes[first + size_t(s)];
                            const uint32_t one = accumulate_model::sample(v[s], sc, g * x + int(sc.pad[0] & 0xffu), g * y + int(sc.pad[0] >> 8));
                            converge_model::add(px, one, s == 0 && !from_plane);
                        }
                        if (V) px.n += float(A.samples);
                        if (sums) {
                            const float w = V ? px.n : float(C->prior + uint32_t(A.samples));
                            texels[4 * x] = px.acc;
                            texels[4 * x + 1] = ~px.acc;
                            texels[4 * x + 2] = px.acc * 3u;
                            std::memcpy(&texels[4 * x + 3], &w, 4);
                        }
                        if (V) words[x] = px.q;
                    }
                    const int total = V ? int(px.n) : int((C ? C->prior : 0u) + uint32_t(A.samples));
                    if (picture) row[x] = accumulate_model::pixel(px.acc, total);
                    if (V && V->counts && converge_model::active(px, V->min_samples, V->tol2, A.samples)) ++V->counts[f];
                }
            }
        }
    }
    return hipSuccess;
}

}  // namespace

extern "C" {
void family_stub_fail_next() { g_fail_next = true; }
void family_stub_expect_grid(int grid) { g_expect_grid = grid; }  // 0: any
long family_stub_launches() { return g_launches; }  // of any kind
long family_stub_carries() { return g_carries; }
long family_stub_converges() { return g_converges; }
}
const kifs::accum::Params& family_stub_last_params() { return g_params; }
const std::vector<kifs::anim::SceneView>& family_stub_last_scenes() { return g_scenes; }
const kifs::accum::CarryParams& family_stub_last_carry() { return g_carry; }
const kifs::accum::ConvergeParams& family_stub_last_converge() { return g_converge; }

namespace kifs {

hipError_t launch_accumulate_render(const accum::Params& A, uint32_t group, uint32_t, hipStream_t) { return run(A, group, nullptr, nullptr); }

hipError_t launch_accumulate_carry(const accum::CarryParams& K, uint32_t group, uint32_t, hipStream_t) { return run(K.A, group, &K, nullptr); }

hipError_t launch_accumulate_converge(const accum::ConvergeParams& K, uint32_t group, uint32_t, hipStream_t) {
    return run(K.A, group, nullptr, &K);
}

}  // namespace kifs
