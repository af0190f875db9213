// kifs_schedule.cpp -- one launch of the render path: kernel parameters from the uniform images, tile
// tables and their temporal feedback, and the launch shape (which kernel form, how many tiles per
// workgroup, residency).  Host code only; kernels live in the three *_kernels.hip files.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <vector>

#include "kifs_context.hpp"

namespace kifs {
namespace host {

// ---- launch-shape rules: every tuned constant of this file, in one place ---------------------------------------
// Each was read off a sweep on MI355X (gfx950, 256 CUs, 1024 SIMDs); the record it came from is named beside it.
// To re-derive them on other silicon: tools/sweep_kernels.sh forces every shape in turn over 5 frame sizes x 4
// camera distances x 2 scenes x batches of 1 / 8 / 32 (-> sweep_shapes.jsonl), tools/cliff_sweep.py then checks
// the rule in place (-> sweep.jsonl: ns per disc pixel must fall smoothly with the load).  `load` = the launch's
// tiles that can hold rays with real work: disc_tiles() x views.
namespace rules {
// residency_for(): lone Julia frames whose heavy tiles fit the device once or twice cap their own residency
// (1080p at distance 5: 207 -> 172 us at one workgroup per CU; 4096^2 needs every slot: 0.70 vs 1.95 ms capped)
constexpr double RESIDENCY_ONE_PER_CU = 1024.0;   // heavy tiles <= this: one workgroup per CU   (profiles/r01/README.md: 182.9 -> 172.8 us)
constexpr double RESIDENCY_TWO_PER_CU = 2048.0;   // <= this: two; above: uncapped               (same table)
// tile-order feedback (cost per tile -> counting sort -> next order) pays from this many tiles per launch geometry
constexpr uint32_t FEEDBACK_MIN_TILES = 2048u;        // Julia pipelines: 720p and up (round 1; no sweep record kept --
                                                      //   re-derive: KIFS_TILE_FEEDBACK=0 / 2 under tools/cliff_sweep.py)
constexpr uint32_t FEEDBACK_MIN_TILES_KIFS = 16384u;  // KIFS: 8K 2.58 -> 2.23 ms, 1080p nothing (round 1, same way)
constexpr int FEEDBACK_PERIOD_LONE = 4;               // refresh every n-th lone launch           (tools/sweep_period.sh, r02)
constexpr int FEEDBACK_PERIOD_BATCH = 3;              // every n-th batched launch                (tools/sweep_period.sh, r02)
// a batch's order is made from every tile's largest cost of its last n sorts (n x the period launches), not of the last one:
// 1080p Julia x48 on the orbit, five sets of poses in turn, n = 1/3/5/8/16/32/64: 0.788/0.781/0.721/0.719/0.722/0.718/0.723 ms
// (KIFS_ORDER_WINDOW; profiles/r16/README.md) -- flat once the window holds every set; 16 sorts are 48 launches
constexpr uint32_t ORDER_WINDOW_BATCH = 16u;
// ray re-queuing: march steps per round
constexpr int ROUND_STEPS_JULIA = 16;     // Julia and generalised Julia (4/8/12/16/24/32 -> 62.8/72.2/75.0/76.8/76.8/77.6
                                          // Gpixel/s at 32 frames per launch)                    (tools/sweep_rounds.sh)
constexpr int ROUND_STEPS_OTHER = 8;      // KIFS scenes; gen-Julia marches under 32 steps        (tools/sweep_rounds.sh)
constexpr int ROUND_STEPS_KIFS_WAVE = 4;  // KIFS scenes, one wave per tile (2/3/4/5/6/8/12/16 steps: 1080p Sierpinski x48 82.2/83.2/82.7/82.4/81.9/81.8/80.0/78.9
                                          // Gpixel/s, 8K x8 32.9/33.0/33.2/33.0/32.9/32.8/32.2/31.9; the 256-thread kernel keeps 8: x8 43.2 against 42.8)   (r03)
constexpr int ROUND_STEPS_LONE_JULIA = 32;  // an uncapped lone Julia frame (4096^2: 0.430 vs 0.445 ms at 16)
constexpr uint64_t REQUEUE_MIN_WORKGROUPS = 4096u;  // below: no rounds at all (256^2 x 8: 0.038 vs 0.062 ms)
// shape of the re-queuing path, from profiles/r02/sweep_shapes.jsonl (every shape forced in turn):
constexpr double WAVE_FROM_LONE = 30000.0;    // one wave per tile (render_wave_kernel) from this load: lone frames,
constexpr double WAVE_FROM_JULIA = 12500.0;   //   batched Julia (1080p x32: 1.13 -> 0.88 ms; 4096^2 x8 +27 %; re-swept r03 after the wave
                                              //   kernel's +15 %: 1080p x16 63.9 against 65.8 with pairs, x20 70.5 against 66.6, x24 76.2 / 67.8),
constexpr double WAVE_FROM_OTHER = 32000.0;   //   everything else (8K Sierpinski x4 +16 %)
constexpr double PAIR_FROM_BATCH = 3500.0;    // two tiles per 256-thread workgroup: batches (1080p Julia 0.319 -> 0.281 ms;
                                              //   below it pairing halves the workgroups side by side: 720p x8 0.222 -> 0.188 with one)
constexpr double PAIR_FROM_GENJULIA = 5000.0;   // generalised Julia (r04, chunks drawn by ticket: x4 8.9 -> 8.0 Gpixel/s, x8 13.4 / 13.5, x12 15.8 -> 16.4,
                                                //   x16 17.7 -> 19.4, x24 19.4 -> 22.4; 12 000 until then)          (tools/sweep_group_shapes.sh)
constexpr double PAIR_FROM_BATCH_KIFS = 7000.0; // KIFS scenes (r04: 1080p Sierpinski x8 43.4 with one tile against 42.2 with two, x16 54.6 / 61.7)
constexpr double PAIR_FROM_LONE_KIFS = 12000.0; // a big lone KIFS frame (1440p Sierpinski at distance 2: -11 %)
// the bunny (tools/sweep_bunny_coop.sh -> profiles/r03/sweep_bunny_coop.txt; 1080p at distance 5 is 149 heavy tiles a frame):
constexpr double BUNNY_ROUNDS_FROM = 450.0;   // below: whole rays, four lanes per pixel (x2: 0.421 against 0.528 ms; x4: 0.592 against 0.536)
constexpr double BUNNY_PAIR_FROM = 1600.0;    // two tiles per workgroup (r04, chunks drawn by ticket: x8 28.3 -> 25.4 Gpixel/s; x12 30.4 -> 33.0; x16 30.0 -> 39.1)
constexpr int ROUND_STEPS_BUNNY_COOP = 4;     // its rounds (x48: 1/2/3/4/6/8 steps -> 52.2/53.6/53.8/53.5/53.3/52.8 Gpixel/s; the lanes-per-ray form: 4-8 alike)
constexpr double BUNNY_W2LDS_FROM = 2600.0;   // pairs with layer 2 of the network in LDS, three waves per SIMD (r04, profiles/r04/sweep_bunny_w2lds.txt:
                                              //   x16 39.1 -> 37.1 Gpixel/s, x20 40.1 -> 44.4, x24 40.6 -> 49.0, x28 40.4 -> 49.0, x32 39.9 -> 49.1)
constexpr double BUNNY_COOP_FROM = 5000.0;    // four waves per 64 rays (same file: x28 43.9 against 49.0 for the form above, x32 48.4 / 49.1, x40 55.0 / 50.0, x48 58.0 / 50.0)
}  // namespace rules

// Tuning overrides (KIFS_ROUND_STEPS, KIFS_GROUP_TILES, KIFS_BUNNY_COOP, KIFS_TILE_FEEDBACK, KIFS_JULIA_CERT_CULL,
// KIFS_FEEDBACK_PERIOD, KIFS_BATCH_PERIOD, KIFS_ORDER_WINDOW; KIFS_LDS_PAD in kifs_kernels.hip) are honoured only when KIFS_TUNING=1 is set as well: they exist
// for tools/sweep_kernels.sh and friends, not for production hosts.  Read once per process, clamped here.
struct Knobs {
    int round_steps, group_tiles;        // -1: not set
    int bunny_coop;                      // -1, or a form 0 / 1 / 2 (FrameParams::bunny_coop)
    int tile_feedback;                   // 0 = never, 1 (default) = per pipeline thresholds, 2 = every frame of 2048+ tiles
    int julia_cert_cull;                 // 0: the Julia culls stay on the patch sphere (julia_culls); -1 / other: certified radius
    uint64_t period_lone, period_batch;  // launches between two refreshes of the tile order
    uint32_t order_window;               // sorts a batch's order remembers (1: the latest costs alone)
};
static const Knobs& knobs() {
    static const Knobs k = [] {
        const char* on = std::getenv("KIFS_TUNING");
        const auto knob = [on](const char* name) {
            const char* e = (on && on[0] == '1') ? std::getenv(name) : nullptr;
            return e ? int(std::strtol(e, nullptr, 10)) : -1;
        };
        const int coop = knob("KIFS_BUNNY_COOP"), mode = knob("KIFS_TILE_FEEDBACK");
        const int lone = knob("KIFS_FEEDBACK_PERIOD"), batch = knob("KIFS_BATCH_PERIOD"), window = knob("KIFS_ORDER_WINDOW");
        return Knobs{knob("KIFS_ROUND_STEPS"), knob("KIFS_GROUP_TILES"), std::min(coop, 2), mode >= 0 ? mode : 1, knob("KIFS_JULIA_CERT_CULL"),
                     uint64_t(lone < 0 ? rules::FEEDBACK_PERIOD_LONE : lone < 3 ? 3 : lone),
                     uint64_t(batch < 0 ? rules::FEEDBACK_PERIOD_BATCH : batch < 2 ? 2 : batch),
                     window < 1 ? rules::ORDER_WINDOW_BATCH : uint32_t(std::min(window, 255))};
    }();
    return k;
}

bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    static const bool verbose = std::getenv("KIFS_DEBUG") != nullptr;
    if (verbose) std::fprintf(stderr, "kifs: %s failed: %s\n", what, hipGetErrorString(e));
    return false;
}

int frame_dims(const kifs_ctx* c, int* w, int* h) {
    // width/height arrive as f32 (data.rs:71-73 casts u32 -> f32); demand exact integers
    float fw = c->screen.width, fh = c->screen.height;
    if (!(fw >= 1.0f) || !(fh >= 1.0f) || fw > 65536.0f || fh > 65536.0f) return KIFS_ERR_BAD_SIZE;
    if (fw != std::floor(fw) || fh != std::floor(fh)) return KIFS_ERR_BAD_SIZE;
    *w = int(fw);
    *h = int(fh);
    return KIFS_OK;
}

int render_dims(const kifs_ctx* c, int* w, int* h) {
    const int st = frame_dims(c, w, h);
    if (st != KIFS_OK) return st;
    const int64_t k = c->supersampling;  // the virtual k W x k H screen stays within frame_dims' limit
    return (int64_t(*w) * k > 65536 || int64_t(*h) * k > 65536) ? KIFS_ERR_BAD_SIZE : KIFS_OK;
}

// Exact squared form of `norm > T` for norm = sqrtf(n2) (correctly rounded, monotone):
// returns the largest binary32 v with sqrtf(v) <= T, so that norm > T  <=>  n2 > v.
float squared_threshold(float T) {
    if (T != T) return INFINITY;          // norm > NaN is never true
    if (T < 0.0f) return -1.0f;           // every non-NaN norm (>= 0) exceeds a negative T
    if (T == INFINITY) return INFINITY;
    double sq = double(T) * double(T);
    float v = sq >= double(FLT_MAX) ? FLT_MAX : float(sq);
    while (v > 0.0f && std::sqrt(v) > T) v = std::nextafterf(v, -INFINITY);
    for (;;) {
        float up = std::nextafterf(v, INFINITY);
        if (up != INFINITY && std::sqrt(up) <= T) v = up; else break;
    }
    return v;
}

// Exact squared form of `norm < T`: returns the smallest binary32 v with sqrtf(v) >= T, so
// that norm < T  <=>  n2 < v  (n2 >= +0 or NaN).
float squared_lower_threshold(float T) {
    if (T != T || T <= 0.0f) return 0.0f;  // norm < T is never true
    if (T == INFINITY) return INFINITY;    // true for every finite norm
    double sq = double(T) * double(T);
    float v = sq >= double(FLT_MAX) ? FLT_MAX : float(sq);
    while (std::sqrt(v) < T) {
        if (v == FLT_MAX) return INFINITY;
        v = std::nextafterf(v, INFINITY);
    }
    for (;;) {
        float down = std::nextafterf(v, -INFINITY);
        if (down >= 0.0f && std::sqrt(down) >= T) v = down; else break;
    }
    return v;
}

// The doubled orbit trip (FrameParams::orbit_x2) equals the contract's trip bit for bit when no unscaled intermediate
// lands in the denormal range and no scaled one overflows.  Sufficient (DESIGN section 4 has the argument): every
// |c_i| in [2^-14, 2^10] -- a nonzero fma(2x, y, c.y) or x^2 - d + c.x is then at least 2^-62 -- and max_distance and
// bound_n2 in (0, 2^60], which keep 4|q|^2 below 2^124 on every trip a lane is still inside.  Nothing depends on the
// ray: the start point's squares are absorbed by w_0^2 = 0.01.
static bool orbit_x2_eligible(const kifs::FrameParams& P) {
    const float lo = 0x1p-14f, hi = 0x1p10f, far = 0x1p60f;
    for (float ci : {P.c.x, P.c.y, P.c.z, P.c.w})
        if (!(std::fabs(ci) >= lo && std::fabs(ci) <= hi)) return false;
    return P.max_distance > 0.0f && P.max_distance <= far && P.bound_n2 > 0.0f && P.bound_n2 <= far;
}

// ---- a certified radius of the power-2 Julia set --------------------------------------------------------------
// The patch sphere of julia.wgsl:8-9 has radius 2; the set is much smaller.  For the estimate
//   q_0 = (p, 0.1), q_{k+1} = q_k^2 + c, dqs = prod_{k<n} 4 |q_k|^2, d = 0.25 ln|q_n|^2 sqrt(|q_n|^2 / dqs)
// (n: the trip at which |q|^2 > max_distance, or sdf_iters) the quaternion norm is multiplicative, so
// |q_{k+1}| >= |q_k|^2 - |c|.  With a = sqrt(rho^2 + 0.01) and a^2 - |c| > a (rho beyond the escape radius), L_0 = a,
// L_{k+1} = L_k^2 - |c|, every point with |p| >= rho has |q_k| >= L_k, growing;
//   g_k = |q_k| / prod_{j<k} 2 |q_j|  obeys  g_{k+1} >= g_k (1 - |c| / |q_k|^2) / 2,  and
//   ln|q_n| >= 2^n G,  G = ln(a^2 - |c|) - ln a,
// hence for every n:  d = ln|q_n| g_n / 2  >=  D(rho) = a G P / 2,  P = prod_{k<sdf_iters} (1 - |c| / L_k^2),
// increasing in rho.  A ray whose closest approach to the origin is >= rho samples only points with |p| >= rho: outside
// the patch sphere d = |p| - 2 > epsilon as ever, in the shell d >= D(rho) > epsilon.  It never hits.  DESIGN section 4
// has the float-error argument behind the margins: D(rho) >= 16 epsilon + 2^-14, nothing overflows in f32.
struct JuliaBound {
    double D;   // the lower bound of the estimate over |p| >= rho; <= 0: rho is not beyond the escape radius
    int trips;  // n_max: trips until L_k^2 > max_distance, at most sdf_iters
};
static JuliaBound julia_bound(double rho, double cn, double max_distance, int sdf_iters) {
    const double a = std::sqrt(rho * rho + 0.01);
    if (!(a * a - cn > a)) return {0.0, 0};
    const double G = std::log(a * a - cn) - std::log(a);
    double L = a, P = 1.0;
    int trips = sdf_iters;
    for (int k = 0; k < sdf_iters; ++k) {
        if (k >= 1 && trips == sdf_iters && L * L > max_distance) trips = k;
        if (L > 1.0e150) break;  // every further factor is 1 in double
        P *= 1.0 - cn / (L * L);
        L = L * L - cn;
    }
    return {0.5 * a * G * P, trips};
}

static double julia_cull_radius_uncached(const float c[4], float epsilon, float max_distance, int sdf_iters, double* bound);
// The smallest radius the certificate holds for, by bisection on [escape radius, 2 + epsilon] in double; 0: none
// (|c| too large for the shell, a NaN, a huge epsilon or max_distance).  `bound`, when given, receives D(rho).
double julia_cull_radius(const float c[4], float epsilon, float max_distance, int sdf_iters, double* bound) {
    // (asked again with every launch: the latest answer is kept, per thread)
    struct Asked { float c[4], epsilon, max_distance; int sdf_iters; };
    thread_local Asked last{};
    thread_local double last_rho = -1.0, last_bound = 0.0;
    const Asked now{{c[0], c[1], c[2], c[3]}, epsilon, max_distance, sdf_iters};
    if (last_rho >= 0.0 && std::memcmp(&last, &now, sizeof now) == 0) {
        if (bound) *bound = last_bound;
        return last_rho;
    }
    double D = 0.0;
    const double rho = julia_cull_radius_uncached(c, epsilon, max_distance, sdf_iters, &D);
    last = now;
    last_rho = rho;
    last_bound = D;
    if (bound) *bound = D;
    return rho;
}
static double julia_cull_radius_uncached(const float c[4], float epsilon, float max_distance, int sdf_iters, double* bound) {
    *bound = 0.0;
    double cc = 0.0;
    for (int i = 0; i < 4; ++i) {
        if (!(std::fabs(c[i]) <= 0x1p10f)) return 0.0;  // (also NaN)
        cc += double(c[i]) * double(c[i]);
    }
    // fill_params' `sane` for the Julia patch (B = 2)
    const float R = 2.0f + epsilon;
    if (!(R > 0.5f && R < 1.0e6f && epsilon >= 0.0f && max_distance < 1.0e15f) || sdf_iters < 0) return 0.0;
    const double cn = std::sqrt(cc), eps = double(epsilon), md = double(max_distance), top = 2.0 + eps;
    const double need = 16.0 * eps + 0x1p-14, room = 0x1p100;
    const auto holds = [&](double rho) {
        const JuliaBound b = julia_bound(rho, cn, md, sdf_iters);
        if (!(b.D >= need)) return false;
        // f32 range: dqs <= max(4 max_distance, 4 |q_0|^2)^n_max and the last |q|^2 <= (max_distance + |c|)^2
        const double factor = std::max(4.0 * md, 4.0 * (top * top + 0.01));
        return b.trips * std::log2(factor) <= 100.0 && (md + cn) * (md + cn) <= room;
    };
    if (!holds(top)) return 0.0;
    const double a_esc = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * cn));
    double lo = std::sqrt(std::max(a_esc * a_esc - 0.01, 0.0)), hi = top;  // holds(lo) is false: D(lo) = 0
    if (!(lo < hi)) return 0.0;
    for (int i = 0; i < 36; ++i) {  // to 2^-36 of the shell: a launch with a constant per frame asks once per frame
        const double mid = 0.5 * (lo + hi);
        (holds(mid) ? hi : lo) = mid;
    }
    *bound = julia_bound(hi, cn, md, sdf_iters).D;
    return hi;
}

// The cull thresholds: cull_n2 for the per-ray culls, the wave-level quick exit's sphere (0: off), and its tile-level
// form (render_wave_kernel): for an orthonormal camera matrix |d| >= 1 and two pixel
// centres of a 32 x 8 tile are at most (31, 7) pixels = (31, 7) * 2 / height apart in uv, so a
// ray of the tile and the ray through the tile's centre differ by at most
// asin(|(31, 7)| / height) <= 1.05 * 31.8 / height radians (the ratio is below 0.5 from 64 rows);
// 34 / height leaves 2 % for the matrix check's tolerance.  fill_views() switches it off when
// a view's matrix is not orthonormal (`tile` false: it has).
static void set_culls(kifs::FrameParams& P, float cull_n2, float quick_n2, bool tile) {
    P.cull_n2 = cull_n2;
    P.quick_cull_n2 = quick_n2;
    P.tile_cull_sqrtk = std::sqrt(quick_n2);
    P.tile_cull_beta = (tile && quick_n2 > 0.0f && P.height >= 64.0f) ? 34.0f / P.height : 0.0f;
}

// The thresholds of a launch of the power-2 Julia pipeline whose culls are on (not its heatmap), from the certified
// radius `rho` its frames share (any rho' >= a frame's own is valid for it; 0: none): (1 + 2^-6) rho^2 for the culls, and
// the quick exits keep their ratio to it, 1.2 / 1.1 -- wave_is_culled and tile_is_culled argue with that room, not
// with the radius.  Without a radius, or with KIFS_JULIA_CERT_CULL=0 under KIFS_TUNING=1: the patch sphere's,
// 1.1 and 1.2 (2 + epsilon)^2.  `tile`: the tile-level exit is allowed.
void julia_culls(kifs::FrameParams& P, double rho, bool tile) {
    const float R = 2.0f + P.epsilon;
    float cull = 1.1f * R * R, quick = 1.2f * R * R;
    if (rho > 0.0 && knobs().julia_cert_cull != 0) {
        const float r = float(rho);
        cull = (1.0f + 0x1p-6f) * r * r;
        quick = cull * (1.2f / 1.1f);
    }
    set_culls(P, cull, P.max_iterations > 0 ? quick : 0.0f, tile);
}
// Whether julia_culls() applies to the launch P describes: the Julia pipeline with its culls on.
bool takes_julia_culls(const kifs::FrameParams& P, uint32_t group) {
    return group == uint32_t(kifs::GROUP_JULIA) && !P.is_heatmap && P.shape_n2 > 0.0f;
}

// A launch whose frames bring their own options (one pipeline, one epsilon and march budget: anim::same_pipeline): the
// largest of the frames' radii serves them all; the patch sphere if one of them has none.  After fill_params, before
// fill_views.
void julia_culls_of_frames(const kifs_ctx* c, kifs::FrameParams& P, const KifsOptionsUniform* options, int count) {
    if (!takes_julia_culls(P, options[0].fractal_group_id)) return;
    double rho = 0.0;
    for (int i = 0; i < count; ++i) {
        const double r = julia_cull_radius(options[i].constant, P.epsilon, P.max_distance, c->sdf_iters, nullptr);
        if (!(r > 0.0)) {
            rho = 0.0;
            break;
        }
        rho = std::max(rho, r);
    }
    julia_culls(P, rho, true);
}

int fill_params(const kifs_ctx* c, kifs::FrameParams* P) {
    int w, h;
    int st = frame_dims(c, &w, &h);
    if (st != KIFS_OK) return st;
    const KifsCameraUniform& cam = c->camera;
    const KifsOptionsUniform& o = c->options;
    if (o.fractal_group_id > 2u) return KIFS_ERR_BAD_ARG;  // FractalGroup::from_id -> None
    P->height = c->screen.height;
    P->aspect = c->screen.aspect_ratio;
    P->origin = {cam.origin[0], cam.origin[1], cam.origin[2]};
    P->m0 = {cam.matrix[0][0], cam.matrix[0][1], cam.matrix[0][2]};
    P->m1 = {cam.matrix[1][0], cam.matrix[1][1], cam.matrix[1][2]};
    P->m2 = {cam.matrix[2][0], cam.matrix[2][1], cam.matrix[2][2]};
    P->max_iterations = o.max_iterations;
    P->max_distance = o.max_distance;
    P->epsilon = o.epsilon;
    P->fractal_color = {o.fractal_color[0], o.fractal_color[1], o.fractal_color[2]};
    P->background_color = {o.background_color[0], o.background_color[1], o.background_color[2]};
    P->is_heatmap = o.is_heatmap;
    P->power = o.power;
    P->c = {o.constant[0], o.constant[1], o.constant[2], o.constant[3]};
    P->sdf_iters = c->sdf_iters;
    P->normal_iters = c->normal_iters;
    P->fold_iters = c->fold_iters;
    P->soft_shadow = c->ext.soft_shadow;
    P->shadow_steps = c->ext.shadow_steps;
    P->shadow_k = c->ext.shadow_k;
    P->shadow_t0 = c->ext.shadow_t0;
    P->shadow_max_t = c->ext.shadow_max_t;
    P->bound_n2 = squared_threshold(2.0f + o.epsilon);
    {   // Bounding-sphere culls: every scene's estimate obeys d(p) >= |p| - B, so outside radius
        // R = B + epsilon (plus margin) `d < epsilon` cannot happen.  B per scene:
        //   Julia / gen-Julia: 2 (the patch of julia.wgsl:8-9)      sphere r=1: 1
        //   cylinder (r=1, half-height 2): sqrt(5)                   box (1,1,1): sqrt(3)
        //   torus (1, 0.3): 1.3        bunny: 1 (patch |p| - 0.8 outside the unit ball)
        //   Sierpinski: 2 -- folds are isometries and pos <- 2 pos - 1 gives r_k >= 2^k r_0 -
        //   sqrt(3)(2^k - 1), hence (r_k - 2)/2^k >= r_0 - 2 for every number of folds.
        float B = 2.0f;
        if (o.fractal_group_id == uint32_t(kifs::GROUP_KIFS)) {
            switch (o.primitive_id) {
            case kifs::PRIM_SPHERE: B = 1.0f; break;
            case kifs::PRIM_CYLINDER: B = 2.2360680f; break;
            case kifs::PRIM_BOX: B = 1.7320508f; break;
            case kifs::PRIM_TORUS: B = 1.3f; break;
            case kifs::PRIM_SIERPINSKI: B = 2.0f; break;
            case kifs::PRIM_BUNNY: B = 1.0f; break;
            default: B = -1.0f; break;  // unknown id: the SDF is the constant 1, no bound
            }
        }
        const float R = B + o.epsilon;
        // (max_distance below 1e15 -- the GUI's range ends at 1e4 -- and, per view, an origin within 1e15 of the
        // scene: fill_views; the long-ray loop's square root of |p|^2 relies on |p|^2 being finite then)
        const bool sane = B > 0.0f && R > 0.5f && R < 1.0e6f && o.epsilon >= 0.0f && o.max_distance < 1.0e15f;
        P->shape_n2 = sane ? 1.1f * R * R : 0.0f;
        // the wave-level quick exit uses a sphere 9 % larger again; like the culls, not in heatmap mode
        set_culls(*P, P->shape_n2, (sane && !o.is_heatmap && o.max_iterations > 0) ? 1.2f * R * R : 0.0f, true);
        P->inv_height = 1.0f / c->screen.height;
        // the power-2 Julia set: a certified radius inside the patch sphere, when there is one
        if (takes_julia_culls(*P, o.fractal_group_id))
            julia_culls(*P, julia_cull_radius(o.constant, o.epsilon, o.max_distance, c->sdf_iters, nullptr), true);
    }
    {   // Ray re-queuing (render_group_kernel): rounds of this many march steps -- 16 for the Julia
        // pipelines (generalised Julia: 1080p lone 0.882 -> 0.869 ms, x8 +2.7 %, x48 +1 % over rounds of 8),
        // 8 for the others (measured; KIFS_ROUND_STEPS overrides, 0 switches it off).
        // Not for heatmap frames (their per-ray step count is kept by the one-wave-per-block
        // march), not with a non-positive epsilon (the queue rebuilds p from t and relies on
        // t > 0 after a step), not for marches too short to repay the rounds' barriers.
        const int forced = knobs().round_steps;
        int rounds = forced >= 0 ? forced : (o.fractal_group_id != uint32_t(kifs::GROUP_KIFS) ? rules::ROUND_STEPS_JULIA : rules::ROUND_STEPS_OTHER);
        if (forced < 0 && rounds == rules::ROUND_STEPS_JULIA && o.max_iterations < 32 && o.fractal_group_id == uint32_t(kifs::GROUP_GENJULIA))
            rounds = rules::ROUND_STEPS_OTHER;  // (a short march of heavy steps still repays shorter rounds)
        if (o.is_heatmap || !(o.epsilon > 0.0f) || o.max_iterations < 2 * rounds) rounds = 0;
        P->round_steps = rounds;
    }
    P->ssaa = c->supersampling;
    P->ssaa_inv_height = 1.0f / (float(c->supersampling) * c->screen.height);
    P->orbit_blocks = c->sdf_iters / 6;
    P->orbit_rem = c->sdf_iters % 6;
    P->orbit_x2 = orbit_x2_eligible(*P) ? 1 : 0;
    P->c2 = {2.0f * P->c.x, 2.0f * P->c.y, 2.0f * P->c.z, 2.0f * P->c.w};
    P->max_distance4 = 4.0f * P->max_distance;
    P->fold_n2_stop = squared_lower_threshold(o.max_distance);
    P->width = w;
    P->y0 = 0;
    P->y1 = h;
    P->stripe_rows = nullptr;
    P->out_frame_rows = 0;
    P->encode = KIFS_ENCODE_SRGB;
    P->pitch_words = uint32_t(w);
    P->out = nullptr;
    P->srgb_table = c->d_srgb;
    P->tile_order = nullptr;
    P->tile_count = 0;
    P->tile_cost = nullptr;
    P->counters = c->d_counters;
    P->workgroups_per_cu = 0;
    P->group_tiles = 1;
    P->bunny_coop = 0;
    P->geom = nullptr;
    P->geom_pitch_texels = 0;
    P->geom_stride_texels = 0;
    return KIFS_OK;
}

bool is_device_pointer(const void* p) {
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // unregistered host memory reports an error; clear it
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

void free_table(TileTable& t) {
    if (t.d_order) (void)hipFree(t.d_order);
    if (t.d_order_alt) (void)hipFree(t.d_order_alt);
    if (t.d_cost) (void)hipFree(t.d_cost);
    if (t.d_seen) (void)hipFree(t.d_seen);
    if (t.costs_written) (void)hipEventDestroy(t.costs_written);
    if (t.stream_left) (void)hipEventDestroy(t.stream_left);
    if (t.sorted) (void)hipEventDestroy(t.sorted);
    t = TileTable();
}

// Device image of a stripe list, cached by content.  Stripes must be ascending and inside the frame: the
// list is validated against THIS frame height before the cache is consulted (the cache is keyed by the
// list alone, and a list cached for a taller frame must not be accepted after kifs_set_screen shrank it).
const RowTable* row_table(kifs_ctx* c, const int* stripes, int n, int height) {
    for (int i = 0; i < n; ++i)
        if (stripes[i] < 0 || int64_t(stripes[i]) * kifs::TILE_H >= height || (i > 0 && stripes[i] <= stripes[i - 1]))
            return nullptr;
    for (const RowTable* r : c->row_tables)
        if (int(r->stripes.size()) == n && std::equal(stripes, stripes + n, r->stripes.begin())) return r;
    std::vector<uint32_t> rows(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) rows[size_t(i)] = uint32_t(stripes[i]) * uint32_t(kifs::TILE_H);
    if (c->row_tables.size() >= 4096) return nullptr;  // a caller inventing a new partition every frame
    RowTable* r = new (std::nothrow) RowTable();
    if (!r) return nullptr;
    r->stripes.assign(stripes, stripes + n);
    if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&r->d_rows), std::max<size_t>(rows.size(), 1) * sizeof(uint32_t)),
                "hipMalloc(stripe rows)") ||
        (n > 0 && !hip_ok(hipMemcpy(r->d_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice),
                          "hipMemcpy(stripe rows)"))) {
        if (r->d_rows) (void)hipFree(r->d_rows);
        delete r;
        return nullptr;
    }
    c->row_tables.push_back(r);
    return r;
}

// Order in which workgroups take tiles: nearest to the frame centre first (squared
// distance of the tile centre, ties by row then column), so the long rays start first.
// Tiles are TILE_W x TILE_H pixels; rows are counted from the top of the band.
TileTable* tile_table(kifs_ctx* c, int width, int height, int y0, int y1, const RowTable* rows) {
    TileTable* slot = nullptr;
    for (auto& t : c->tables) {
        if (t.d_order && t.width == width && t.height == height && t.y0 == y0 && t.y1 == y1 && t.rows == rows) {
            t.last_use = ++c->use_clock;
            return &t;
        }
        if (!slot || t.last_use < slot->last_use) slot = &t;
    }
    const int tx = (width + kifs::TILE_W - 1) / kifs::TILE_W;
    const int ty = rows ? int(rows->stripes.size()) : (y1 - y0 + kifs::TILE_H - 1) / kifs::TILE_H;
    if (tx > 0xffff || ty > 0xffff) return nullptr;
    struct Key { int64_t d2; uint32_t id; };
    std::vector<Key> keys;
    keys.reserve(size_t(tx) * ty);
    for (int j = 0; j < ty; ++j)
        for (int i = 0; i < tx; ++i) {
            // doubled coordinates keep everything in integers
            int64_t cx = int64_t(2 * i + 1) * kifs::TILE_W - width;
            const int64_t first = rows ? int64_t(rows->stripes[size_t(j)]) * kifs::TILE_H
                                       : int64_t(y0) + int64_t(j) * kifs::TILE_H;  // the tile's first frame row
            int64_t cy = 2 * first + kifs::TILE_H - height;
            keys.push_back({cx * cx + cy * cy, (uint32_t(j) << 16) | uint32_t(i)});
        }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        return a.d2 != b.d2 ? a.d2 < b.d2 : a.id < b.id;
    });
    std::vector<uint32_t> order(keys.size());
    for (size_t k = 0; k < keys.size(); ++k) order[k] = keys[k].id;
    // the slot being replaced may still be read by an enqueued launch: drain first
    if (slot->d_order) {
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize(before tile table eviction)");
        free_table(*slot);
    }
    const size_t bytes = order.size() * sizeof(uint32_t);
    if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&slot->d_order), bytes), "hipMalloc(tile order)") ||
        !hip_ok(hipMalloc(reinterpret_cast<void**>(&slot->d_order_alt), bytes), "hipMalloc(tile order 2)") ||
        !hip_ok(hipMalloc(reinterpret_cast<void**>(&slot->d_cost), bytes), "hipMalloc(tile cost)") ||
        !hip_ok(hipMalloc(reinterpret_cast<void**>(&slot->d_seen), bytes), "hipMalloc(tile cost memory)") ||
        !hip_ok(hipEventCreateWithFlags(&slot->costs_written, hipEventDisableTiming), "hipEventCreate") ||
        !hip_ok(hipEventCreateWithFlags(&slot->stream_left, hipEventDisableTiming), "hipEventCreate") ||
        !hip_ok(hipEventCreateWithFlags(&slot->sorted, hipEventDisableTiming), "hipEventCreate") ||
        !hip_ok(hipMemcpy(slot->d_order, order.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy(tile order)") ||
        !hip_ok(hipMemset(slot->d_cost, 0, bytes), "hipMemset(tile cost)") ||
        !hip_ok(hipMemset(slot->d_seen, 0, bytes), "hipMemset(tile cost memory)")) {
        free_table(*slot);
        return nullptr;
    }
    slot->width = width; slot->height = height; slot->y0 = y0; slot->y1 = y1;
    slot->rows = rows;
    slot->count = uint32_t(order.size());
    slot->last_use = ++c->use_clock;
    return slot;
}

// How many of a launch's tiles (per view) can contain rays with real work: those the projected
// bounding sphere of the scene covers (fill_params: every estimate obeys d(p) >= |p| - B, so a ray that
// passes the origin at more than R = B + epsilon never hits).  pi r_px^2 / 256 with
// r_px = H/2 * R / sqrt(d^2 - R^2) (focal length 1, uv.y in [-1, 1]), scaled by the launch's share of the
// frame's rows; every tile when the camera is inside the sphere or the culls are off.  This is the
// quantity the launch-shape rules below are written in: it follows the camera distance and the frame
// size together, where tile counts and pixel counts do not.
double disc_tiles(const kifs::FrameParams& P, int frame_height, uint32_t tile_count) {
    if (P.cull_n2 <= 0.0f || P.is_heatmap) return double(tile_count);
    const double R2 = double(P.shape_n2) / 1.1;  // (B + epsilon)^2: the bounding sphere, whatever radius the culls stand on
    const double d2 = double(P.origin.x) * P.origin.x + double(P.origin.y) * P.origin.y +
                      double(P.origin.z) * P.origin.z;
    const double frame_px = double(P.width) * double(frame_height);
    double disk_px = frame_px;  // camera inside the sphere: everything is a candidate
    if (d2 > R2 * 1.0001) {
        const double r_uv = std::sqrt(R2 / (d2 - R2));          // tangent of the sphere's angular radius
        const double r_px = r_uv * 0.5 * double(frame_height);
        disk_px = std::min(frame_px, 3.14159265358979 * r_px * r_px);
    }
    // a band or shard of a frame gets its share of the disk
    const double share = frame_px > 0 ? double(tile_count) * (kifs::TILE_W * kifs::TILE_H) / frame_px : 1.0;
    return std::min(double(tile_count), disk_px * std::min(1.0, share) / (kifs::TILE_W * kifs::TILE_H));
}

// Residency rule for the Julia pipelines.  The long rays of a frame slow each other down as soon
// as they share a SIMD (~1490 cycles per march step alone, ~1570 with one neighbour, ~1900 with
// seven), and after the bounding-sphere culls nothing else needs the slots: the only tiles
// with real work are those the projected bounding sphere covers.  If those are few enough to be
// spread over the 256 CUs in a couple of rounds, capping residency lets every long wave run
// near its lone-wave speed (1080p, camera at distance 5: 207 -> 172 us at one workgroup per
// CU); if they are many (4096^2, or a camera close to the fractal) the frame needs every slot for
// its long-marching waves and full residency wins (4096^2: 0.70 ms vs 1.95 ms capped).
int residency_for(const kifs::FrameParams& P, uint32_t group, double heavy_tiles) {
    if (group != kifs::GROUP_JULIA || P.cull_n2 <= 0.0f || P.is_heatmap) return 0;
    if (heavy_tiles <= rules::RESIDENCY_ONE_PER_CU) return 1;
    if (heavy_tiles <= rules::RESIDENCY_TWO_PER_CU) return 2;
    return 0;
}

// The background pixel, encoded exactly as the kernels would (unorm8 / srgb8 of kifs_device_math.hpp).
uint32_t background_pixel(const kifs_ctx* c, kifs::V3 colour, int encode) {
    uint32_t ch[3];
    const float bg[3] = {colour.x, colour.y, colour.z};
    for (int i = 0; i < 3; ++i) {
        const float x = bg[i];
        if (encode == KIFS_ENCODE_SRGB) {
            uint32_t k = 0;
            for (uint32_t step = 128; step >= 1; step >>= 1) k += (x >= c->h_srgb[k + step]) ? step : 0u;
            ch[i] = k;
        } else {
            float v = (x >= 0.0f) ? x : 0.0f;
            v = (v > 1.0f) ? 1.0f : v;
            ch[i] = uint32_t(int(v * 255.0f + 0.5f));
        }
    }
    return ch[0] | (ch[1] << 8) | (ch[2] << 16) | 0xff000000u;
}

// ---- one launch, step by step: enqueue_batch() below calls these in order ----------------------------------------
static bool is_bunny(const kifs_ctx* c) {
    return c->options.fractal_group_id == uint32_t(kifs::GROUP_KIFS) && c->options.primitive_id == uint32_t(kifs::PRIM_BUNNY);
}

// What a caller can get wrong before anything is looked up: state, count, destinations, encoding, frame size.
static int check_arguments(const kifs_ctx* c, int count, const KifsCameraUniform* cameras, uint8_t* const* outs, int encode) {
    if (!c->have_screen || !c->have_options || (!c->have_camera && !cameras)) return KIFS_ERR_UNCONFIGURED;
    if (count < 1 || count > kifs::MAX_BATCH || !outs) return KIFS_ERR_BAD_ARG;
    for (int i = 0; i < count; ++i)
        if (!outs[i] || (reinterpret_cast<uintptr_t>(outs[i]) & 3u) != 0) return KIFS_ERR_BAD_ARG;
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    return KIFS_OK;
}

// A batch beyond the kernel argument's room: the views go through a device table, the next slot of the ring.
int take_view_slot(kifs_ctx* c, int* slot) {
    const int vs = *slot = c->view_slot;
    c->view_slot = (vs + 1) % kifs_ctx::VIEW_RING;
    // (each part on its own: a slot that a failed allocation left half made is completed when the ring comes round to it)
    const size_t bytes = sizeof(kifs::BatchView) * size_t(kifs::MAX_BATCH);
    if ((!c->d_views[vs] && !hip_ok(hipMalloc(reinterpret_cast<void**>(&c->d_views[vs]), bytes), "hipMalloc(view table)")) ||
        (!c->h_views[vs] && !hip_ok(hipHostMalloc(reinterpret_cast<void**>(&c->h_views[vs]), bytes, hipHostMallocDefault), "hipHostMalloc(view table)")) ||
        (!c->views_used[vs] && !hip_ok(hipEventCreateWithFlags(&c->views_used[vs], hipEventDisableTiming), "hipEventCreate(view table)")))
        return KIFS_ERR_RUNTIME;
    // the launch that last read this slot (four big launches ago) must be over before its images change
    if (c->views_busy[vs] && !hip_ok(hipEventSynchronize(c->views_used[vs]), "wait(view table)")) return KIFS_ERR_RUNTIME;
    c->views_busy[vs] = false;
    return KIFS_OK;
}

// The views, and what they decide for the whole launch: P's camera is view 0's, and the culls go when a view does not
// meet what they assume.
void fill_views(const kifs_ctx* c, kifs::FrameParams& P, kifs::BatchView* views, int count, const KifsCameraUniform* cameras,
                uint8_t* const* outs) {
    bool far_origin = false;  // a view whose origin is not within 1e15 of the scene: no culls for this launch
    // a view beyond 32 from the scene: oo - b^2 of ray_never_inside cancels too much for the certified radius's margin of
    // 2^-6; the patch sphere's 10 % serves the launch
    bool distant_origin = false;
    for (int i = 0; i < count; ++i) {
        const KifsCameraUniform& cam = cameras ? cameras[i] : c->camera;
        kifs::BatchView& v = views[i];
        v.origin = {cam.origin[0], cam.origin[1], cam.origin[2]};
        v.m0 = {cam.matrix[0][0], cam.matrix[0][1], cam.matrix[0][2]};
        v.m1 = {cam.matrix[1][0], cam.matrix[1][1], cam.matrix[1][2]};
        v.m2 = {cam.matrix[2][0], cam.matrix[2][1], cam.matrix[2][2]};
        v.out = reinterpret_cast<uint32_t*>(outs[i]);
        if (!(double(v.origin.x) * v.origin.x + double(v.origin.y) * v.origin.y + double(v.origin.z) * v.origin.z < 1.0e30))
            far_origin = true;  // (also NaN)
        if (double(v.origin.x) * v.origin.x + double(v.origin.y) * v.origin.y + double(v.origin.z) * v.origin.z > 1024.0)
            distant_origin = true;
        if (P.tile_cull_beta > 0.0f) {  // the tile-level cull's angle bound assumes an orthonormal matrix
            const kifs::V3* m[3] = {&v.m0, &v.m1, &v.m2};
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) {
                    const double dot = double(m[a]->x) * m[b]->x + double(m[a]->y) * m[b]->y + double(m[a]->z) * m[b]->z;
                    if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1.0e-3)) P.tile_cull_beta = 0.0f;
                }
        }
    }
    if (distant_origin && P.cull_n2 > 0.0f && P.cull_n2 != P.shape_n2)  // (only julia_culls makes the two differ)
        julia_culls(P, 0.0, P.tile_cull_beta > 0.0f);
    if (far_origin) P.cull_n2 = P.quick_cull_n2 = P.tile_cull_beta = P.shape_n2 = 0.0f;
    P.origin = views[0].origin;
    P.m0 = views[0].m0;
    P.m1 = views[0].m1;
    P.m2 = views[0].m2;
}

// Band, pitch and geometry plane: checked against the frame (P.y1 is still its height), then written into P.
int set_destination(const kifs_ctx* c, kifs::FrameParams& P, int count, uint8_t* out, size_t pitch, int y0, int y1, int encode,
                           bool striped, float* geom, size_t geom_pitch, size_t geom_stride) {
    if (y0 < 0 || y1 > P.y1 || y0 > y1) return KIFS_ERR_BAD_ARG;
    if (pitch < size_t(P.width) * 4 || (pitch & 3u) != 0 || (pitch >> 2) > 0xffffffffull) return KIFS_ERR_BAD_SIZE;
    if (geom) {  // the geometry plane: 16-byte texels, rows of a band packed, one plane per view `geom_stride` apart
        if (striped || P.ssaa > 1) return KIFS_ERR_BAD_ARG;
        if ((reinterpret_cast<uintptr_t>(geom) & 15u) != 0 || geom_pitch < size_t(P.width) * 16 || (geom_pitch & 15u) != 0 ||
            (geom_stride & 15u) != 0 || (count > 1 && geom_stride < size_t(y1 - y0) * geom_pitch) ||
            (geom_pitch >> 4) > 0xffffffffull || (geom_stride >> 4) > 0xffffffffull)
            return KIFS_ERR_BAD_ARG;
        P.geom = geom;
        P.geom_pitch_texels = uint32_t(geom_pitch >> 4);
        P.geom_stride_texels = uint32_t(geom_stride >> 4);
    }
    P.y0 = y0;
    P.y1 = y1;
    P.encode = encode;
    P.background_rgba = background_pixel(c, P.background_color, encode);
    P.pitch_words = uint32_t(pitch >> 2);
    P.out = reinterpret_cast<uint32_t*>(out);
    return KIFS_OK;
}

// Temporal feedback on the tile order.  A launch can leave a cost per tile (render_kernel: the run time of the tile's
// slowest wave; the throughput kernels: the work of its wave or workgroup, cost_from_work); a one-workgroup counting sort
// on the context's side stream turns those costs into a new order while the following launch is running, so the sort is
// off the critical path.  The longest rays sit at the fractal's silhouette, which no static
// order knows; with them first the frame ends when they do.  Tables:
//   d_order      read by the launches      d_order_alt   written by the sort, then swapped in
//   d_cost       written by the first launch of a period, read by the sort
//   d_seen       a batch's sorts only: every tile's largest cost of the last ORDER_WINDOW_BATCH sorts, which the order is
//                made from -- a batch's views move on between launches (an orbit), and the order of the latest views alone
//                served the next ones worse than no feedback at all (profiles/r16/launch_spread.md)
// Events order everything whichever streams the caller uses.  Off for small frames, where it does not pay for itself;
// KIFS frames gain from it only when they are large (8K: 2.58 -> 2.23 ms; 1080p: nothing).
// The order is refreshed every `period` launches (views change slowly; the events the refresh needs cost a few
// microseconds each): every fourth lone launch, every third batched one (its launches are long and its views move: an
// orbit; measured best for fixed and moving cameras).  Within a period of launches k = 0..period-1:
//   k == 0: record costs, event;   k == 1: sort the costs of launch 0;   k == 2: the new order is in use.
// With several frames in flight (several contexts and streams on one device) or a batch the sort runs in the launch stream
// itself: streams share a handful of hardware queues, and an event wait parked in a queue also holds up whatever other
// context's launches sit behind it (measured: two contexts fell back to running one after the other).  The 10 us then
// hide behind the other frames' kernels.  A lone frame keeps the side stream: there nothing else can.
struct Feedback {  // what the step before a launch hands to the step after it
    bool use = false, inline_sort = false, record_costs = false; uint64_t k = 0;  // k: the launch's place in its period
};

// The side stream's sort is done with d_order_alt: wait for it, swap it in.
static int adopt_sorted_order(TileTable* tt, hipStream_t stream) {
    if (!hip_ok(hipStreamWaitEvent(stream, tt->sorted, 0), "wait(sorted)")) return KIFS_ERR_RUNTIME;
    std::swap(tt->d_order, tt->d_order_alt);
    tt->sort_pending = false;
    return KIFS_OK;
}

// Before the launch.  `plain` false: a geometry or supersampled launch, which follows a stream change like any other but
// neither records costs nor moves the sort (its tiles cost something else), so that a later plain launch of the same
// geometry finds the order where the plain launches left it.
static int feedback_before(kifs_ctx* c, TileTable* tt, hipStream_t stream, int count, uint32_t tiles_x, bool plain, Feedback* f) {
    const bool is_kifs = c->options.fractal_group_id == uint32_t(kifs::GROUP_KIFS);
    f->use = tt->feedback && knobs().tile_feedback != 0 && !is_bunny(c) &&  // (the bunny's quad kernel records no costs)
             tt->count >= ((is_kifs && knobs().tile_feedback < 2) ? rules::FEEDBACK_MIN_TILES_KIFS : rules::FEEDBACK_MIN_TILES);
    if (!f->use) return KIFS_OK;
    if (tt->last_stream && tt->last_stream != stream) {
        // The caller moved to another stream: order this stream after the launches of the old one, so that the buffer
        // rotation below keeps its "nobody still reads it" guarantee.
        if (!hip_ok(hipEventRecord(tt->stream_left, tt->last_stream), "record(stream change)") ||
            !hip_ok(hipStreamWaitEvent(stream, tt->stream_left, 0), "wait(stream change)"))
            return KIFS_ERR_RUNTIME;
    }
    tt->last_stream = stream;
    if (!plain) return KIFS_OK;
    f->k = tt->launches % (count > 1 ? knobs().period_batch : knobs().period_lone);
    f->inline_sort = c->frames_in_flight > 1 || count > 1;
    f->record_costs = f->k == 0;
    // A side-stream sort from earlier launches owns d_cost and d_order_alt -- the one behind launch 1 of this lone period,
    // lone launches before a batch, or a period cut short when feedback was switched off in between (options changed to a
    // pipeline without it and back).  Take its result before anything here records costs or sorts again: the sort reads
    // cost[] twice and must not see it change.
    if (tt->sort_pending && adopt_sorted_order(tt, stream) != KIFS_OK) return KIFS_ERR_RUNTIME;
    if (f->inline_sort && f->k == 1) {
        // A batch's sort remembers (tile_order_kernel): its views move, and where the long tiles were for the last few sets
        // of views says more about the next set than the latest set alone.  d_seen belongs to these sorts, which are in
        // stream order; a lone launch's sort (rules fitted to the latest costs) neither reads nor writes it.
        // Costs of another scene or on another scale (options, iteration counts or the launch's shape changed since the
        // memory's were recorded: record_scene) say nothing about this one: a window of one sort replaces every entry.
        const uint32_t window = tt->seen_stale ? 1u : knobs().order_window;
        if (count > 1) tt->seen_stale = false;  // (only the remembering sort takes the memory's fresh start)
        const hipError_t e = count > 1 ? kifs::launch_tile_order_remembering(tt->d_cost, tt->d_seen, tt->d_order_alt, tt->count, tiles_x,
                                                                             tt->cost_shift, window, stream)
                                       : kifs::launch_tile_order(tt->d_cost, tt->d_order_alt, tt->count, tiles_x, tt->cost_shift, stream);
        if (!hip_ok(e, "tile_order_kernel launch")) return KIFS_ERR_RUNTIME;
        std::swap(tt->d_order, tt->d_order_alt);  // stream order: the sort precedes this launch
    }
    return KIFS_OK;
}

// After a plain launch: the event behind the recorded costs, or the side stream's sort of them.
static int feedback_after(kifs_ctx* c, TileTable* tt, hipStream_t stream, uint32_t tiles_x, const Feedback& f) {
    if (!f.use) {  // no bookkeeping, no events: nothing depends on this launch
        tt->launches = 0;  // (a pending side-stream sort stays pending: the next feedback launch waits for it)
        return KIFS_OK;
    }
    tt->launches += 1;
    if (f.record_costs) tt->costs_marked = false;
    if (f.inline_sort) return KIFS_OK;
    if (f.record_costs) {
        // Launch k = 0 of the period wrote d_cost.  The previous sort (period before) read it and finished before that
        // period's launch 2 started, i.e. long ago on this timeline.
        if (!hip_ok(hipEventRecord(tt->costs_written, stream), "record(render)")) return KIFS_ERR_RUNTIME;
        tt->costs_marked = true;
    } else if (f.k == 1) {
        // The costs may come from a launch that sorts inline and records no event -- a batch, or frames_in_flight > 1,
        // before this lone launch.  costs_written is then unrecorded or a period old, and a wait for it would let the sort
        // read costs that launch is still writing: mark this point of the stream instead (it follows that launch).
        if (!tt->costs_marked) {
            if (!hip_ok(hipEventRecord(tt->costs_written, stream), "record(render, late)")) return KIFS_ERR_RUNTIME;
            tt->costs_marked = true;
        }
        // sort those costs into d_order_alt: the buffer last read by launches of the period before the previous adoption,
        // all of which precede launch 0 of this period
        if (!c->side_stream && !hip_ok(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking), "side stream")) return KIFS_ERR_RUNTIME;
        if (!hip_ok(hipStreamWaitEvent(c->side_stream, tt->costs_written, 0), "wait(render 0)") ||
            !hip_ok(kifs::launch_tile_order(tt->d_cost, tt->d_order_alt, tt->count, tiles_x, tt->cost_shift, c->side_stream), "tile_order_kernel launch") ||
            !hip_ok(hipEventRecord(tt->sorted, c->side_stream), "record(sorted)"))
            return KIFS_ERR_RUNTIME;
        tt->sort_pending = true;
    }
    return KIFS_OK;
}

// The sort's shift for the costs the launch P describes records.  The throughput kernels record work (cost_from_work: at
// most 4 chunks per tile x (max_iterations march steps + one shaded chunk)), which the sort's 1024 bins must resolve up
// to the top; render_kernel records run times in units of 1024 cycles, sorted as they are.
static uint32_t work_cost_shift(const kifs::FrameParams& P) {
    if (P.round_steps <= 0) return 0u;
    const uint64_t top = 4ull * uint64_t(std::max(P.group_tiles, 1)) * (uint64_t(std::max(P.max_iterations, 0)) + 8ull);
    uint32_t shift = 0;
    while (shift < 31u && (top >> shift) > 1023ull) ++shift;
    return shift;
}

// What a batch's recorded costs depend on besides the views: the scene (options, iteration counts, extensions) and the
// scale they are counted on (the shape's shift).  A recording launch whose key differs from the memory's marks it stale.
static void record_scene(const kifs_ctx* c, TileTable* tt) {
    uint64_t h = 1469598103934665603ull;  // FNV-1a
    const auto mix = [&h](const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    };
    const int iters[3] = {c->sdf_iters, c->normal_iters, c->fold_iters};
    mix(&c->options, sizeof c->options);
    mix(iters, sizeof iters);
    mix(&c->ext, sizeof c->ext);
    mix(&tt->cost_shift, sizeof tt->cost_shift);
    if (h != tt->seen_scene) tt->seen_stale = true;
    tt->seen_scene = h;
}

// A residency-capped lone Julia frame keeps the patch sphere's culls.  With one workgroup per CU the certified radius made
// the 1080p frame at distance 5 LONGER, 0.152 -> 0.172 ms (fixed view 0.142 -> 0.173), although it marches half the rays
// and no wave can take more steps: the same library, KIFS_JULIA_CERT_CULL on / off, with or without the tile-order
// feedback; at two workgroups per CU and uncapped the smaller sphere is 1 - 2 % ahead (profiles/r11/README.md).  The cap
// exists so that the frame's long waves run undisturbed; what the smaller sphere changes is what their neighbours do
// meanwhile -- half as many tiles march, so the other CUs turn to the launch's 7 800 empty tiles early.  Not explained
// further; the residency rule was fitted to the patch sphere's load and is re-fitted with the other shape rules.
static void capped_frame_culls(kifs::FrameParams& P) {
    if (P.workgroups_per_cu >= 1 && P.cull_n2 > 0.0f && P.cull_n2 != P.shape_n2) julia_culls(P, 0.0, P.tile_cull_beta > 0.0f);
}

// The shape of a geometry or supersampled launch: one kernel form for every scene, whole rays, no costs, no diagnostics.
// A lone geometry frame keeps the block kernel's residency cap.
static void fixed_shape(const kifs_ctx* c, kifs::FrameParams& P, int count, int frame_height) {
    P.tile_cost = nullptr;
    P.counters = nullptr;
    P.round_steps = 0;
    const bool lone = count == 1 && c->frames_in_flight <= 1;
    P.workgroups_per_cu = (P.geom && lone) ? residency_for(P, c->options.fractal_group_id, disc_tiles(P, frame_height, P.tile_count)) : 0;
    capped_frame_culls(P);
}

// The shape of a plain launch.  Everything is decided from `load`: the launch's tiles that can hold rays with real work
// (the projected bounding sphere's tiles, all views), tools/cliff_sweep.py's x axis.
static void choose_shape(const kifs_ctx* c, kifs::FrameParams& P, int count, int frame_height) {
    // The diagnostics buffer holds one record per wave of the screen kifs_debug_counters saw (counter_words).  A launch
    // with more waves -- a larger screen set since, a batch -- runs as if diagnostics were off: nothing is reallocated
    // here, an earlier enqueued launch may still be writing the buffer.
    if (P.counters && 8ull + 16ull * uint64_t(P.tile_count) * uint64_t(count) > uint64_t(c->counter_words)) P.counters = nullptr;
    if (P.counters) P.round_steps = 0;  // the per-wave diagnostics belong to the one-wave-per-block march
    const uint32_t group_id = c->options.fractal_group_id;
    const bool free_rounds = knobs().round_steps < 0;  // (a forced KIFS_ROUND_STEPS replaces every round length below)
    const bool lone = count == 1 && c->frames_in_flight <= 1;
    const bool bunny_scene = is_bunny(c);
    const double heavy_tiles = disc_tiles(P, frame_height, P.tile_count);
    const double load = heavy_tiles * double(count);
    // the residency cap serves a lone frame's latency; concurrent frames want every slot
    P.workgroups_per_cu = lone ? residency_for(P, group_id, heavy_tiles) : 0;
    capped_frame_culls(P);
    // a residency-capped launch is a lone frame bound by its longest rays: re-queuing helps throughput, not that (1080p
    // Julia: 0.143 ms without, 0.146 ms with)
    if (P.workgroups_per_cu >= 1) P.round_steps = 0;
    // (an uncapped lone Julia frame -- 4096^2 -- prefers longer rounds: 0.430 ms at 32 steps, 0.445 at 16)
    if (P.round_steps == rules::ROUND_STEPS_JULIA && count == 1 && group_id == uint32_t(kifs::GROUP_JULIA) && P.max_iterations >= 64 && free_rounds)
        P.round_steps = rules::ROUND_STEPS_LONE_JULIA;
    // (nor does the lone bunny frame: 0.461 ms with the quad kernel, 0.670 ms in rounds; nor two of them)
    if (bunny_scene && (count == 1 || (load < rules::BUNNY_ROUNDS_FROM && free_rounds))) P.round_steps = 0;
    // nor does a launch too small to fill the device twice over (256x256 x 8 views = 2048 workgroups: 0.038 ms without, 0.062 with)
    if (uint64_t(P.tile_count) * uint64_t(count) < rules::REQUEUE_MIN_WORKGROUPS) P.round_steps = 0;
    // Shape of the re-queuing path (profiles/r02/sweep_shapes.jsonl: 5 frame sizes x 4 camera distances x 2 scenes x
    // batches of 1 / 8 / 32, every shape forced in turn):
    //   one WAVE per tile (render_wave_kernel) once the launch has several times more heavy tiles than the device has
    //     workgroup slots -- then slots, not critical paths, set its duration, and single-wave workgroups give four times
    //     as many (1080p Julia x32: 1.13 -> 0.88 ms; 4096^2 x8 +27 %; 8K Sierpinski x4 +16 %) -- from a load of 12 500
    //     tiles for the Julia pipeline, 32 000 for the others, 30 000 for a lone frame (all its heavy tiles are one view's);
    //   otherwise 256-thread workgroups (render_group_kernel), whose four waves take a tile's first, crowded rounds side
    //     by side (a lone wave needs +30 % for the same tile): TWO tiles of the cost order per workgroup when the launch is
    //     a batch with enough heavy tiles to pair (one tile's queue is short for most of its life, neighbours of the cost
    //     order fill each other's waves: batched 1080p Julia 0.319 -> 0.281 ms; below 3 500 heavy tiles pairing only
    //     halves the workgroups that can run side by side: 720p x8 at distance 5, 0.222 -> 0.188 ms with one) or a big
    //     lone KIFS frame (1440p Sierpinski at distance 2: -11 %), else ONE.
    // Not the bunny (four lanes per ray, 216 VGPRs: pairs just run longer); the generalised Julia pairs tiles only from
    // 12 000 heavy tiles (1080p x32: 0.140 -> 0.125 ms per frame; x8: nothing, and its few, very long workgroups lost 7 %
    // when paired on smaller launches) and keeps 256-thread workgroups throughout (one wave per tile: x32 0.150 ms, x8
    // 0.31 against 0.22).
    const int forced = knobs().group_tiles;
    const bool julia = group_id == uint32_t(kifs::GROUP_JULIA);
    const bool genjulia = group_id == uint32_t(kifs::GROUP_GENJULIA);
    const bool kifs_scene = group_id == uint32_t(kifs::GROUP_KIFS);
    const double wave_from = lone ? rules::WAVE_FROM_LONE : (julia ? rules::WAVE_FROM_JULIA : rules::WAVE_FROM_OTHER);
    int shape = 1;
    // (one wave per tile needs views to interleave: TWO frames of 4096^2 -- 19 600 heavy tiles, past WAVE_FROM_JULIA -- run
    // 31.5 Gpixel/s that way against 42.8 with pairs, four 52.0 against 44.0: r04, profiles/r04/sweep_group_shapes.txt)
    if (load >= wave_from && !genjulia && (count >= 3 || load >= rules::WAVE_FROM_LONE)) shape = 0;
    else if (!lone && load >= (genjulia ? rules::PAIR_FROM_GENJULIA : kifs_scene ? rules::PAIR_FROM_BATCH_KIFS : rules::PAIR_FROM_BATCH))
        shape = 2;
    else if (lone && kifs_scene && load >= rules::PAIR_FROM_LONE_KIFS) shape = 2;
    if (forced >= 0) shape = forced;
    P.bunny_coop = 0;
    if (bunny_scene) {  // its own rules: four lanes per ray (216 VGPRs) or four waves per 64 rays
        const int coop = knobs().bunny_coop;  // (KIFS_BUNNY_COOP under KIFS_TUNING forces a form)
        P.bunny_coop = coop >= 0 ? coop : (load >= rules::BUNNY_COOP_FROM ? 1 : load >= rules::BUNNY_W2LDS_FROM ? 2 : 0);
        shape = P.bunny_coop ? 2 : forced >= 1 ? forced : (load >= rules::BUNNY_PAIR_FROM ? 2 : 1);
        if (P.bunny_coop == 1 && P.round_steps == rules::ROUND_STEPS_OTHER && free_rounds) P.round_steps = rules::ROUND_STEPS_BUNNY_COOP;
    }
    P.group_tiles = shape;
    if (shape == 0 && kifs_scene && !bunny_scene && P.round_steps == rules::ROUND_STEPS_OTHER && free_rounds)
        P.round_steps = rules::ROUND_STEPS_KIFS_WAVE;
}

// What kifs_debug_last_* report of the launch P describes, whichever kind it is.
static void report_shape(kifs_ctx* c, const kifs::FrameParams& P) {
    const bool bunny = is_bunny(c), rounds = P.round_steps > 0;
    c->last_round_steps = P.round_steps;
    c->last_group_tiles = rounds ? P.group_tiles : -1;
    c->last_bunny_form = bunny && rounds ? P.bunny_coop : -1;
    c->last_kernel = P.geom ? KIFS_KERNEL_GEOMETRY : P.ssaa > 1 ? KIFS_KERNEL_SSAA
                   : rounds ? (bunny ? (P.bunny_coop == 1 ? KIFS_KERNEL_BUNNY_COOP : KIFS_KERNEL_GROUP)
                                     : (P.group_tiles == 0 ? KIFS_KERNEL_WAVE : KIFS_KERNEL_GROUP))
                            : (bunny ? KIFS_KERNEL_BUNNY_QUAD : KIFS_KERNEL_BLOCK);
}

// The launch itself and what goes with every one: the profiling event pair around it, and the view table of a batch
// beyond the kernel argument (ring slot `vs`) uploaded before it and marked in use after it.
static int launch(kifs_ctx* c, hipStream_t stream, kifs::BatchParams& B, bool big, int vs) {
    const bool timed = c->profiling && !c->prof_a.empty() && (c->prof_seen++ % uint64_t(c->prof_every)) == 0;
    const size_t pslot = c->prof_count % (c->prof_a.empty() ? 1 : c->prof_a.size());
    if (timed && !hip_ok(hipEventRecord(c->prof_a[pslot], stream), "record(profile start)")) return KIFS_ERR_RUNTIME;
    if (big) {
        if (!hip_ok(hipMemcpyAsync(c->d_views[vs], c->h_views[vs], sizeof(kifs::BatchView) * size_t(B.count), hipMemcpyHostToDevice, stream),
                    "copy(view table)"))
            return KIFS_ERR_RUNTIME;
        B.table = c->d_views[vs];
    }
    if (!hip_ok(kifs::launch_render(B, c->options.fractal_group_id, c->options.primitive_id, stream), "render_kernel launch")) return KIFS_ERR_RUNTIME;
    if (big) {
        if (!hip_ok(hipEventRecord(c->views_used[vs], stream), "record(view table)")) return KIFS_ERR_RUNTIME;
        c->views_busy[vs] = true;
    }
    if (timed) {
        if (!hip_ok(hipEventRecord(c->prof_b[pslot], stream), "record(profile stop)")) return KIFS_ERR_RUNTIME;
        ++c->prof_count;
    }
    return KIFS_OK;
}

int enqueue_batch(kifs_ctx* c, hipStream_t stream, int count, const KifsCameraUniform* cameras,
                  uint8_t* const* outs, size_t pitch, int y0, int y1, int encode,
                  const int* stripes, int n_stripes, int in_place, float* geom, size_t geom_pitch, size_t geom_stride) {
    hip_ok(hipGetLastError(), "stale error before enqueue");
    int st = check_arguments(c, count, cameras, outs, encode);
    if (st != KIFS_OK) return st;
    kifs::BatchParams B;
    kifs::FrameParams& P = B.frame;
    int rw, rh;
    if ((st = fill_params(c, &P)) != KIFS_OK) return st;
    if ((st = render_dims(c, &rw, &rh)) != KIFS_OK) return st;  // (the virtual screen of a supersampled launch)
    B.count = count;
    B.table = nullptr;
    const int h = P.y1;  // the frame's height
    st = set_destination(c, P, count, outs[0], pitch, y0, y1, encode, stripes != nullptr, geom, geom_pitch, geom_stride);
    if (st != KIFS_OK) return st;  // (before a slot of the view ring is taken: a rejected call leaves no trace)
    const bool big = count > kifs::MAX_BATCH_INLINE;
    int vs = -1;
    if (big && (st = take_view_slot(c, &vs)) != KIFS_OK) return st;
    fill_views(c, P, big ? c->h_views[vs] : B.view, count, cameras, outs);
    if (y1 == y0) return KIFS_OK;
    const RowTable* rows = nullptr;
    if (stripes) {
        if (n_stripes == 0) return KIFS_OK;
        rows = row_table(c, stripes, n_stripes, h);
        if (!rows) return KIFS_ERR_BAD_ARG;
        P.stripe_rows = rows->d_rows;
        P.out_frame_rows = in_place ? 1 : 0;
    }
    TileTable* tt = tile_table(c, P.width, h, y0, y1, rows);
    if (!tt) return KIFS_ERR_RUNTIME;
    const uint32_t tiles_x = uint32_t((P.width + kifs::TILE_W - 1) / kifs::TILE_W);
    const bool plain = !P.geom && P.ssaa <= 1;
    Feedback feedback;
    st = feedback_before(c, tt, stream, count, tiles_x, plain, &feedback);
    if (st != KIFS_OK) return st;
    P.tile_order = tt->d_order;
    P.tile_count = tt->count;
    if (plain) {
        P.tile_cost = feedback.record_costs ? tt->d_cost : nullptr;
        choose_shape(c, P, count, h);
        if (feedback.record_costs) {
            tt->cost_shift = work_cost_shift(P);
            if (count > 1) {
                record_scene(c, tt);
            } else {  // a lone launch's costs, should a batch's sort meet them: not the memory's scene either
                tt->seen_scene = 0;
                tt->seen_stale = true;
            }
        }
    } else {
        fixed_shape(c, P, count, h);
    }
    report_shape(c, P);
    st = launch(c, stream, B, big, vs);
    if (st != KIFS_OK || !plain) return st;
    return feedback_after(c, tt, stream, tiles_x, feedback);
}

int enqueue(kifs_ctx* c, hipStream_t stream, uint8_t* dev_out, size_t pitch, int y0, int y1, int encode) {
    if (!c->have_camera) return KIFS_ERR_UNCONFIGURED;
    if (!dev_out) return KIFS_ERR_BAD_ARG;
    return enqueue_batch(c, stream, 1, nullptr, &dev_out, pitch, y0, y1, encode);
}

bool order_around(TileTable* tt, hipStream_t stream, bool before) {
    if (!tt->last_stream || tt->last_stream == stream) return true;
    hipStream_t from = before ? tt->last_stream : stream, to = before ? stream : tt->last_stream;
    return hip_ok(hipEventRecord(tt->stream_left, from), "record(order around feedback launches)") &&
           hip_ok(hipStreamWaitEvent(to, tt->stream_left, 0), "wait(order around feedback launches)");
}

bool grow(uint8_t*& buf, size_t& have, size_t need, const char* what) {
    if (need <= have) return true;
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    have = 0;
    if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&buf), need), what)) return false;
    have = need;
    return true;
}

}  // namespace host
}  // namespace kifs

// ---- C ABI: the host model of the culls, GPU-free (include/kifs_hip.h) -------------------------------------------
extern "C" double kifs_host_julia_cull_radius(const float constant[4], float epsilon, float max_distance, int sdf_iters,
                                              double* bound) {
    if (bound) *bound = 0.0;
    if (!constant) return 0.0;
    return kifs::host::julia_cull_radius(constant, epsilon, max_distance, sdf_iters, bound);
}

extern "C" int kifs_host_cull_thresholds(const KifsScreenUniform* screen, const KifsOptionsUniform* options, int sdf_iters,
                                         const KifsCameraUniform* cameras, int count, float out[5]) {
    if (!screen || !options || !cameras || !out || sdf_iters < 0 || count < 1 || count > kifs::MAX_BATCH) return KIFS_ERR_BAD_ARG;
    kifs_ctx c;  // (plain data until something is rendered: no device behind it)
    c.screen = *screen;
    c.options = *options;
    c.camera = cameras[0];
    c.sdf_iters = sdf_iters;
    kifs::FrameParams P;
    if (const int st = kifs::host::fill_params(&c, &P); st != KIFS_OK) return st;
    std::vector<kifs::BatchView> views(static_cast<size_t>(count));
    std::vector<uint8_t*> outs(static_cast<size_t>(count), nullptr);
    kifs::host::fill_views(&c, P, views.data(), count, cameras, outs.data());
    out[0] = P.cull_n2;
    out[1] = P.quick_cull_n2;
    out[2] = P.tile_cull_sqrtk;
    out[3] = P.tile_cull_beta;
    out[4] = P.shape_n2;
    return KIFS_OK;
}
