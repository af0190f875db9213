// kifs_scene.hpp -- device-side scene: the signed-distance functions, normals and
// the sphere-tracing loop of the reference fragment shader, written for wave64.
//
// What each function computes is fixed by the reference (paths under
// src/shaders/ of LesbianLemon/kifs-raymarching):
//   julia_sdf / julia_normal        julia.wgsl:5-27 / :29-56
//   genjulia_sdf / genjulia_normal  gen_julia.wgsl:5-27 / :30-55, quaternions.wgsl:57-63
//   primitive SDFs, fold, Sierpinski, bunny, central-difference normal   kifs.wgsl:16-167
//   ray set-up and march            dependencies/entry.wgsl:49-59 / :6-29
// How it is computed is this library's own: the variant (fractal group x
// primitive) is a template parameter so the uniform `switch` of kifs.wgsl:139-155
// and the pipeline choice of graphics.rs:310-321 vanish at compile time; all
// frame constants sit in SGPRs (kernarg); per-pixel state is registers only.
#pragma once

#include "kifs_bunny_weights.h"
#include "kifs_device_math.hpp"

namespace kifs {

// ---- quaternion helpers (quaternions.wgsl) ----------------------------------------------
// Evaluation order of the quaternion step (a legal reading of quaternions.wgsl:22-28,42-50,
// chosen because it is exactly what the packed-f32 loop below computes):
//     s = y*y + z*z;  d = fma(w,w,s) = |ijk|^2;  |q|^2 = fma(x,x,d)
//     q^2 + c: real = fma(x,x,-d) + c.x;  ijk = fma(2x, ijk, c.ijk)
KIFS_DEV float quat_ijk2(V4 q) { return fmaf_(q.w, q.w, q.y * q.y + q.z * q.z); }
KIFS_DEV float quat_norm2(V4 q) { return fmaf_(q.x, q.x, quat_ijk2(q)); }
KIFS_DEV V4 quat_sq_add(V4 q, V4 c) {
    float tr = 2.0f * q.x;
    return V4{fmaf_(q.x, q.x, -quat_ijk2(q)) + c.x, fmaf_(tr, q.y, c.y), fmaf_(tr, q.z, c.z),
              fmaf_(tr, q.w, c.w)};
}

// quat_pow (quaternions.wgsl:57-63) with the work it shares with its callers made explicit (the
// arithmetic contract): d = |ijk|^2 and qs = |q|^2 come from the caller;
// length(q) = sqrt(qs); the two divisions are products with correctly rounded reciprocals;
// L = log2(qs) is taken once: pow(norm, x) = exp2(x L / 2), and `dq_factor` receives
// gen_julia.wgsl:16's pow(qs, x - 1) = exp2((x - 1) L).
// This is the inner loop of the slowest pipeline and a lone wave pays ~35 cycles for every taken
// branch, so the step runs on the straight-line cores of kifs_device_math.hpp and checks ONCE, at
// its end, that every lane's arguments were ordinary; a wave with a NaN, an infinity, a zero or a
// denormal anywhere repeats the step with the general functions (same operations, same bits for
// ordinary lanes).
template <bool GENERAL>
KIFS_DEV V4 quat_pow_step(V4 q, float d, float qs, float x, float& dq_factor, bool& ordinary) {
    const float L = GENERAL ? log2_(qs) : log2_core(qs);
    const float e1 = (x - 1.0f) * L;
    dq_factor = GENERAL ? exp2_(e1) : exp2_core(e1);
    const float inv = GENERAL ? 1.0f / sqrt_(qs) : rcp_mid(sqrt_mid(qs));
    const float ca = q.x * inv;
    const float phi = GENERAL ? acos_(ca) : acos_core(ca);
    const float ninv = GENERAL ? 1.0f / sqrt_(d) : rcp_mid(sqrt_mid(d));
    const V3 n{q.y * ninv, q.z * ninv, q.w * ninv};
    const float e2 = x * (0.5f * L);
    const float pw = GENERAL ? exp2_(e2) : exp2_core(e2);
    const float a = x * phi;
    float cs, sn;
    if constexpr (GENERAL) sincos_(a, sn, cs);
    else sincos_core(a, sn, cs);
    // every argument a core saw was in its range: |q|^2 and |ijk|^2 mid-range (then their square roots
    // are too, and L is finite), both exponents inside (-128, 128) (a NaN exponent means a NaN L: caught
    // by the first test; v_max skips NaNs), |cos phi| <= 1 (false for NaN); the sin/cos argument x phi is
    // then at most 10 pi for the powers the caller lets through
    ordinary = (max(bits(qs) - 0x21800000u, bits(d) - 0x21800000u) < (0x5d800000u - 0x21800000u)) &&
               (__builtin_fmaxf(abs_(e1), abs_(e2)) < 127.99999f) && (abs_(ca) <= 1.0f);
    return V4{pw * cs, pw * (n.x * sn), pw * (n.y * sn), pw * (n.z * sn)};
}

// `lanes`: the lanes whose result is used (the others may hold anything and do not force the general path).
#ifdef KIFS_EVAL_COUNT
static __device__ unsigned long long g_pow_counts[8];  // [0] wave-level steps, [1] of which repeated with the general functions, [2] lanes at [0]
#endif
KIFS_DEV V4 quat_pow_shared(V4 q, float d, float qs, float x, float& dq_factor, bool lanes = true) {
    bool ordinary = false;
    V4 t{};
    const bool power_ok = abs_(x) <= 1.0e5f;  // uniform: |x phi| <= pi |x| stays inside the sin/cos cores' range
    if (__builtin_expect(power_ok, 1)) t = quat_pow_step<false>(q, d, qs, x, dq_factor, ordinary);
#ifdef KIFS_EVAL_COUNT
    {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(true);
        if (__lane_id() == uint32_t(__builtin_ctzll(m))) {
            atomicAdd(&g_pow_counts[0], 1ull);
            atomicAdd(&g_pow_counts[2], (unsigned long long)__builtin_popcountll(m));
            if (__builtin_amdgcn_ballot_w64(lanes && !ordinary) != 0ull) atomicAdd(&g_pow_counts[1], 1ull);
        }
    }
#endif
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(lanes && !ordinary) != 0ull, 0))
        t = quat_pow_step<true>(q, d, qs, x, dq_factor, ordinary);
    return t;
}

KIFS_DEV V4 quat_pow(V4 q, float x) {
    const float d = quat_ijk2(q);
    const float qs = fmaf_(q.x, q.x, d);
    float unused;
    return quat_pow_shared(q, d, qs, x, unused);
}

// ---- Julia ---------------------------------------------------------------------
// The orbit loop of julia.wgsl:15-23,
//     dqs *= 4*qs;  q = q^2 + c;  qs = |q|^2;  if (qs > max_distance) break;
// hand-written for gfx950.  A frame's run time is the latency of its longest rays, and a
// lone wave pays ~5 cycles per instruction of any kind, so the loop is written to the
// minimum instruction count: 8 packed-f32 ops + 1 compare + 1 exec update per trip.
//
// Register pairs (fixed, so that 32-bit halves can be named):
//   v[40:41] YZ = [y, z]          v[42:43] WD = [w, dq]        v[44:45] Q = [|q|^2, x_next]
//   v[46:47] T  = [2x, 4|q_prev|^2]                            v[48:51] temporaries
// Per trip (HEAD then TAIL):
//   YZ = fma(T.lo, YZ, [cy,cz])              y,z of q_{k+1}
//   WD = fma(T, WD, [cw, 0])                 w of q_{k+1};  dq *= 4|q_{k-1}|^2  (one trip late)
//   T  = [Q.hi, Q.lo] * [2, 4]               2 x_{k+1}, 4|q_k|^2
//   A  = YZ*YZ; B = A.lo + A.hi (both lanes); A = fma(WD.lo, WD.lo, B) = d (both lanes)
//   Q  = fma(Q.hi, Q.hi, [d, -d]) + [0, cx]  = [|q_{k+1}|^2, x_{k+2}]
//   vcc = |q_{k+1}|^2 > max_distance;  exec &= ~vcc     (an escaped lane's registers freeze)
// x_{k+2} is computed one trip early from the squares that |q_{k+1}|^2 needs anyway.  The
// factor 4|q_k|^2 still missing from dq when a lane stops sits frozen in T.hi and is applied
// after the loop, so dq goes through exactly the products of the textbook loop, in order.
// The trip count is wave-uniform (SGPR); the loop is unrolled twice with one peeled trip
// for odd counts and leaves as soon as every lane has escaped.
#define KIFS_ORBIT_HEAD                                                                    \
    "v_pk_fma_f32 v[40:41], v[46:47], v[40:41], %[cyz] op_sel_hi:[0,1,1]\n"                  \
    "v_pk_fma_f32 v[42:43], v[46:47], v[42:43], %[cw0]\n"                                    \
    "v_pk_mul_f32 v[46:47], v[44:45], %[k24] op_sel:[1,0] op_sel_hi:[0,1]\n"
#define KIFS_ORBIT_TAIL                                                                    \
    "v_pk_mul_f32 v[48:49], v[40:41], v[40:41]\n"                                            \
    "v_pk_add_f32 v[50:51], v[48:49], v[48:49] op_sel:[0,1] op_sel_hi:[0,1]\n"               \
    "v_pk_fma_f32 v[48:49], v[42:43], v[42:43], v[50:51] op_sel_hi:[0,0,1]\n"                \
    "v_pk_fma_f32 v[44:45], v[44:45], v[44:45], v[48:49] op_sel:[1,1,0] op_sel_hi:[1,1,1] neg_hi:[0,0,1]\n" \
    "v_pk_add_f32 v[44:45], v[44:45], %[c0x]\n"
#define KIFS_ORBIT_TRIP                                                                    \
    KIFS_ORBIT_HEAD KIFS_ORBIT_TAIL                                                          \
    "v_cmp_lt_f32 vcc, %[maxd], v44\n"                                                       \
    "s_andn2_b64 exec, exec, vcc\n"

// Orbit + distance estimate for points inside the bounding sphere.  `lanes` is the exec mask
// of the lanes whose result is wanted (wave-uniform SGPR pair); the others keep garbage.
// The trip count is wave-uniform: the loop is unrolled six times (a taken branch costs a lone
// wave ~35 cycles, as much as half a trip) with a one-trip remainder loop in front, and leaves
// as soon as every lane has escaped.
KIFS_DEV float julia_interior(const FrameParams& P, V3 p, unsigned long long lanes) {
    F2 yz{p.y, p.z};
    F2 wd{0.1f, 1.0f};          // w = 0.1 (julia.wgsl:1), dq = 1 (:14)
    F2 q{1.0f, p.x};            // .hi = real part of q_0 (.lo is overwritten by the first TAIL)
    F2 t{p.x + p.x, 1.0f};      // 2 x_0, neutral first dq factor
    F2 ta, tb;
    const F2 cyz{P.c.y, P.c.z}, cw0{P.c.w, 0.0f}, c0x{0.0f, P.c.x}, k24{2.0f, 4.0f};
    int n = P.sdf_iters, rem;
    unsigned long long saved_exec;
    asm volatile(
        "s_mov_b64 %[save], exec\n"
        "s_and_b64 exec, exec, %[lanes]\n"
        KIFS_ORBIT_TAIL  // squares of q_0: Q = [|q_0|^2, x_1]
        // rem = n % 6 single trips, then n / 6 blocks of six
        "s_mul_hi_u32 %[rem], %[n], 0x2aaaaaab\n"   // n / 6 for 0 <= n < 2^31
        "s_mul_i32 %[rem], %[rem], 6\n"
        "s_sub_u32 %[rem], %[n], %[rem]\n"
        "s_sub_u32 %[n], %[n], %[rem]\n"
        "s_cmp_eq_u32 %[rem], 0\n"
        "s_cbranch_scc1 1f\n"
        "0:\n"
        KIFS_ORBIT_TRIP
        "s_sub_u32 %[rem], %[rem], 1\n"
        "s_cmp_lg_u32 %[rem], 0\n"
        "s_cbranch_scc1 0b\n"
        "1:\n"
        "s_cmp_eq_u32 %[n], 0\n"
        "s_cbranch_scc1 3f\n"
        "2:\n"
        KIFS_ORBIT_TRIP KIFS_ORBIT_TRIP KIFS_ORBIT_TRIP
        "s_cbranch_execz 3f\n"
        KIFS_ORBIT_TRIP KIFS_ORBIT_TRIP KIFS_ORBIT_TRIP
        "s_cbranch_execz 3f\n"
        "s_sub_u32 %[n], %[n], 6\n"
        "s_cmp_lg_u32 %[n], 0\n"
        "s_cbranch_scc1 2b\n"
        "3:\n"
        "s_mov_b64 exec, %[save]\n"
        : "+{v[40:41]}"(yz), "+{v[42:43]}"(wd), "+{v[44:45]}"(q), "+{v[46:47]}"(t),
          "=&{v[48:49]}"(ta), "=&{v[50:51]}"(tb), [save] "=&s"(saved_exec), [n] "+s"(n),
          [rem] "=&s"(rem)
        : [cyz] "s"(cyz), [cw0] "s"(cw0), [c0x] "s"(c0x), [k24] "s"(k24),
          [maxd] "s"(P.max_distance), [lanes] "s"(lanes)
        : "vcc", "scc");
    const float qs = q.x;
    const float dqs = wd.y * t.y;  // the factor the loop had not applied yet
    // zero / denormal / inf / NaN |q|^2 is rare: only then does the wave run the general log
    const bool ordinary = (qs >= 1.17549435e-38f) && (qs <= 3.40282347e38f);
    float lg;
    if (__builtin_expect((__builtin_amdgcn_ballot_w64(!ordinary) & lanes) == 0ull, 1))
        lg = log_normal(qs);
    else
        lg = log_general(qs);
    return (0.25f * lg) * sqrt_(qs / dqs);
}

// scene_SDF of julia.wgsl:5-27 for one point (point evaluation, normals of other variants).
KIFS_DEV float julia_sdf(const FrameParams& P, V3 p) {
    const float n2 = dot(p, p);
    const bool outside = n2 > P.bound_n2;  // == length(p) > 2 + epsilon (:7-10)
    const unsigned long long in_lanes = __builtin_amdgcn_ballot_w64(!outside);
    float d = sqrt_(n2) - 2.0f;
    if (in_lanes != 0ull) {
        float di = julia_interior(P, p, in_lanes);
        d = outside ? d : di;
    }
    return d;
}

KIFS_DEV V3 julia_normal(const FrameParams& P, V3 p) {
    V4 q{p.x, p.y, p.z, 0.1f};
    // Jacobian columns; A(q) = [x -y -z -w; y x 0 0; z 0 x 0; w 0 0 x]^T-as-columns
    // (julia.wgsl:40-45 uses the column-major constructor), J <- A*J column by column.
    V4 j0{1, 0, 0, 0}, j1{0, 1, 0, 0}, j2{0, 0, 1, 0}, j3{0, 0, 0, 1};
    auto apply = [&](V4 v) {
        V4 r;
        r.x = fmaf_(q.w, v.w, fmaf_(q.z, v.z, fmaf_(q.y, v.y, q.x * v.x)));
        r.y = fmaf_(q.x, v.y, (-q.y) * v.x);
        r.z = fmaf_(q.x, v.z, (-q.z) * v.x);
        r.w = fmaf_(q.x, v.w, (-q.w) * v.x);
        return r;
    };
    for (int i = 0; i < P.normal_iters; ++i) {
        j0 = apply(j0); j1 = apply(j1); j2 = apply(j2); j3 = apply(j3);
        q = quat_sq_add(q, P.c);
        if (quat_norm2(q) > P.max_distance) break;
    }
    V3 g;
    g.x = fmaf_(j3.x, q.w, fmaf_(j2.x, q.z, fmaf_(j1.x, q.y, j0.x * q.x)));
    g.y = fmaf_(j3.y, q.w, fmaf_(j2.y, q.z, fmaf_(j1.y, q.y, j0.y * q.x)));
    g.z = fmaf_(j3.z, q.w, fmaf_(j2.z, q.z, fmaf_(j1.z, q.y, j0.z * q.x)));
    return normalize(g);
}

// ---- generalised Julia -----------------------------------------------------------
// `lanes`: the lanes whose estimate the caller will use.  The others leave at once (their value is unspecified): a ray
// that has hit sits near the set, where orbits are longest, and stays in its wave until the round ends -- unmasked it
// made the wave run full-length orbits for a result nobody reads (the Julia loop and the Sierpinski folds mask theirs
// the same way).
KIFS_DEV float genjulia_sdf(const FrameParams& P, V3 p, unsigned long long lanes = ~0ull) {
    const float n2 = dot(p, p);
    if (n2 > P.bound_n2) return sqrt_(n2) - 2.0f;  // == length(p) > 2 + epsilon
    if ((lanes & (1ull << __lane_id())) == 0ull) return 0.0f;
    V4 q{p.x, p.y, p.z, 0.1f};
    float d = quat_ijk2(q);
    float qs = fmaf_(q.x, q.x, d);  // = quat_norm2(q)
    float dqs = 1.0f;
    const float pp = P.power * P.power;
    for (int i = 0; i < P.sdf_iters; ++i) {
        float pw1;  // pow(qs, power - 1)
        V4 t = quat_pow_shared(q, d, qs, P.power, pw1);
        dqs = dqs * (pp * pw1);
        q = V4{t.x + P.c.x, t.y + P.c.y, t.z + P.c.z, t.w + P.c.w};
        d = quat_ijk2(q);
        qs = fmaf_(q.x, q.x, d);
        if (qs > P.max_distance) break;
    }
    return (0.25f * log_(qs)) * sqrt_(qs / dqs);
}

KIFS_DEV V3 genjulia_normal(const FrameParams& P, V3 p) {
    const float h = P.epsilon;
    // six offset orbits (gen_julia.wgsl:35-40); `position +- h_axis` adds +-0 elsewhere
    V4 o[6] = {
        {p.x + h, p.y + 0.0f, p.z + 0.0f, 0.1f}, {p.x - h, p.y - 0.0f, p.z - 0.0f, 0.1f},
        {p.x + 0.0f, p.y + h, p.z + 0.0f, 0.1f}, {p.x - 0.0f, p.y - h, p.z - 0.0f, 0.1f},
        {p.x + 0.0f, p.y + 0.0f, p.z + h, 0.1f}, {p.x - 0.0f, p.y - 0.0f, p.z - h, 0.1f},
    };
    for (int i = 0; i < P.normal_iters; ++i) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            V4 t = quat_pow(o[k], P.power);
            o[k] = V4{t.x + P.c.x, t.y + P.c.y, t.z + P.c.z, t.w + P.c.w};
        }
    }
    float l[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) l[k] = log2_(length(o[k]));
    return normalize(V3{l[0] - l[1], l[2] - l[3], l[4] - l[5]});
}

// ---- KIFS ------------------------------------------------------------------------
// Mirror in a plane through the origin with normal e_a + e_b (kifs.wgsl:6-14 with the
// normals of :58-62): signed distance (pa+pb)/|n|, reflect only from the negative side.  The
// division by the constant |n| = sqrt(2) is a multiplication by fl(1/sqrt(2)): the arithmetic
// contract's choice, one ulp from the quotient, inside WGSL's bound for `/`.
KIFS_DEV void mirror2(float& pa, float& pb) {
    const float nn = 1.0f / sqrt_(2.0f);
    const float sd = (pa + pb) * nn;
    const float k = 2.0f * min_(sd, 0.0f);
    pa = fmaf_(-k, nn, pa);
    pb = fmaf_(-k, nn, pb);
}

KIFS_DEV V3 tetrahedral_fold(V3 p) {  // kifs.wgsl:56-66
    mirror2(p.x, p.y);
    mirror2(p.y, p.z);
    mirror2(p.x, p.z);
    return p;
}

// One mirror of the fold in the loop below: sd = (a + b) * fl(1/sqrt(2)); m = min(sd, 0) -- the
// hardware minimum, see below -- left in v46 for the caller's two updates  p -= m * (2/sqrt(2)).
#define KIFS_MIRROR_SD(a, b)                                                               \
    "v_add_f32_e32 v46, " a ", " b "\n"                                                    \
    "v_mul_f32_e32 v46, 0x3f3504f3, v46\n"                                                 \
    "v_min_f32_e32 v46, 0, v46\n"

// One fold + scale step of kifs.wgsl:72-78 for the lanes in EXEC, then EXEC &= n2 < stop.
//   v[40:41] = [x, y]   v42 = z   v43 = n2   v44 = scale   v[46:47] = [m, -]   s[76:77] = [-2/sqrt(2), -]
#define KIFS_FOLD_STEP                                                                     \
    KIFS_MIRROR_SD("v40", "v41")                                                           \
    "v_pk_fma_f32 v[40:41], v[46:47], s[76:77], v[40:41] op_sel_hi:[0,0,1]\n"              \
    KIFS_MIRROR_SD("v41", "v42")                                                           \
    "v_fmac_f32_e32 v41, 0xbfb504f3, v46\n"                                                \
    "v_fmac_f32_e32 v42, 0xbfb504f3, v46\n"                                                \
    KIFS_MIRROR_SD("v40", "v42")                                                           \
    "v_fmac_f32_e32 v40, 0xbfb504f3, v46\n"                                                \
    "v_fmac_f32_e32 v42, 0xbfb504f3, v46\n"                                                \
    "v_pk_fma_f32 v[40:41], v[40:41], 2.0, -1.0 op_sel_hi:[1,0,0]\n"   /* p = 2 p - 1 */    \
    "v_fma_f32 v42, v42, 2.0, -1.0\n"                                                      \
    "v_add_f32_e32 v44, v44, v44\n"                                    /* scale *= 2 */     \
    "v_mul_f32_e32 v43, v40, v40\n"                                    /* n2 = dot(p, p) */ \
    "v_fmac_f32_e32 v43, v41, v41\n"                                                       \
    "v_fmac_f32_e32 v43, v42, v42\n"                                                       \
    "v_cmpx_gt_f32_e32 vcc, %[stop], v43\n"

// The fold loop of the Sierpinski estimate, hand-scheduled: 20 instructions per fold (the
// compiler's version of the same arithmetic: 27, and a taken branch every fold; here every second).
//  * min_(sd, 0) is the hardware minimum: they differ only for sd = -0 (the mirror then adds a
//    zero of the other sign to both coordinates, and p = 2 p - 1, fma(2, +-0, -1) = -1, forgets the
//    sign of a zero before anything but another signed-zero sum can see it) and for NaN (a NaN
//    sum means a coordinate is NaN already and stays NaN on both paths: the estimate is NaN);
//  * 2 * m is exact, so fma(-(2 m), 1/sqrt(2), p) = fma(m, -(2/sqrt(2)), p) bit for bit.
// `lanes`: lanes that take part (the others keep their values).
KIFS_DEV void sierpinski_folds(const FrameParams& P, V3& p, float& n2, float& scale,
                               unsigned long long lanes) {
    F2 xy{p.x, p.y}, q;
    float z = p.z;
    const F2 knn{-2.0f * (1.0f / sqrt_(2.0f)), 0.0f};
    int n = P.fold_iters;
    unsigned long long saved_exec;
    asm volatile(
        "s_mov_b64 %[save], exec\n"
        "s_cmp_lt_i32 %[n], 1\n"
        "s_cbranch_scc1 1f\n"
        "s_and_b64 exec, exec, %[lanes]\n"   // lanes whose result nobody reads do not fold
        "v_cmpx_gt_f32_e32 vcc, %[stop], v43\n"
        "s_cbranch_execz 1f\n"
        ".p2align 6\n"   // the back edge's target on a 64-byte line (a lone wave refetches after a taken branch)
        "0:\n"
        KIFS_FOLD_STEP
        "s_sub_u32 %[n], %[n], 1\n"
        "s_cmp_eq_u32 %[n], 0\n"
        "s_cbranch_scc1 1f\n"
        "s_cbranch_execz 1f\n"
        KIFS_FOLD_STEP
        "s_sub_u32 %[n], %[n], 1\n"
        "s_cmp_eq_u32 %[n], 0\n"
        "s_cbranch_scc1 1f\n"
        "s_cbranch_execnz 0b\n"
        "1:\n"
        "s_mov_b64 exec, %[save]\n"
        : "+{v[40:41]}"(xy), "+{v42}"(z), "+{v43}"(n2), "+{v44}"(scale), "=&{v[46:47]}"(q),
          [save] "=&s"(saved_exec), [n] "+s"(n)
        : [stop] "s"(P.fold_n2_stop), "{s[76:77]}"(knn), [lanes] "s"(lanes)
        : "vcc", "scc");
    p = V3{xy.x, xy.y, z};
}

// `lanes`: the lanes whose estimate the caller will use (the others get an unspecified value).
KIFS_DEV float sierpinski_sdf(const FrameParams& P, V3 p, unsigned long long lanes) {  // kifs.wgsl:68-81
    // The loop condition `r < max_distance` is evaluated on the squared norm (exact: see
    // FrameParams::fold_n2_stop), so the square root is taken once, after the loop.
    float scale = 1.0f;
    float n2 = dot(p, p);
    sierpinski_folds(P, p, n2, scale, lanes);
    // scale is 2^k exactly (k folds made), so dividing by it is multiplying by 2^-k, itself exact: the
    // same single rounding (if any: only in the denormal range).  2^-k by an exponent flip while it is a
    // normal number (k <= 126: decided per launch); the division otherwise.
    if (__builtin_expect(P.fold_iters <= 126, 1)) return (sqrt_(n2) - 2.0f) * from_bits(0x7f000000u - bits(scale));
    return (sqrt_(n2) - 2.0f) / scale;
}

KIFS_DEV V4 mat4_vec(const float* m, V4 v) {  // column-major 4x4 times vector
    V4 r;
    r.x = fmaf_(m[12], v.w, fmaf_(m[8], v.z, fmaf_(m[4], v.y, m[0] * v.x)));
    r.y = fmaf_(m[13], v.w, fmaf_(m[9], v.z, fmaf_(m[5], v.y, m[1] * v.x)));
    r.z = fmaf_(m[14], v.w, fmaf_(m[10], v.z, fmaf_(m[6], v.y, m[2] * v.x)));
    r.w = fmaf_(m[15], v.w, fmaf_(m[11], v.z, fmaf_(m[7], v.y, m[3] * v.x)));
    return r;
}
KIFS_DEV V4 add4(V4 a, V4 b) { return V4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
KIFS_DEV V4 sin4(V4 a) { return V4{sin_(a.x), sin_(a.y), sin_(a.z), sin_(a.w)}; }
// the same values without branches (kifs_device_math.hpp), for the form whose dependent chain sets the frame time
KIFS_DEV V4 sin4_flat(V4 a) { return V4{sin_flat(a.x), sin_flat(a.y), sin_flat(a.z), sin_flat(a.w)}; }
KIFS_DEV V4 ld4(const float* v) { return V4{v[0], v[1], v[2], v[3]}; }

KIFS_DEV float bunny_sdf(V3 p) {  // kifs.wgsl:84-137; weights in constant memory
    if (dot(p, p) > 1.0f) return length(p) - 0.8f;
    V4 q{p.x * -1.0f, p.z * 1.0f, p.y * -1.0f, 1.0f};
    V4 f0[4], f1[4], f2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f0[k] = sin4(mat4_vec(KIFS_BUNNY_L0[k], q));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        V4 a = mat4_vec(KIFS_BUNNY_L1[k][0], f0[0]);
        a = add4(a, mat4_vec(KIFS_BUNNY_L1[k][1], f0[1]));
        a = add4(a, mat4_vec(KIFS_BUNNY_L1[k][2], f0[2]));
        a = add4(a, mat4_vec(KIFS_BUNNY_L1[k][3], f0[3]));
        a = add4(a, ld4(KIFS_BUNNY_B1[k]));
        f1[k] = add4(sin4(a), f0[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        V4 a = mat4_vec(KIFS_BUNNY_L2[k][0], f1[0]);
        a = add4(a, mat4_vec(KIFS_BUNNY_L2[k][1], f1[1]));
        a = add4(a, mat4_vec(KIFS_BUNNY_L2[k][2], f1[2]));
        a = add4(a, mat4_vec(KIFS_BUNNY_L2[k][3], f1[3]));
        a = add4(a, ld4(KIFS_BUNNY_B2[k]));
        V4 sn = sin4(a);
        f2[k] = V4{sn.x / 1.4f + f1[k].x, sn.y / 1.4f + f1[k].y, sn.z / 1.4f + f1[k].z,
                   sn.w / 1.4f + f1[k].w};
    }
    float r = dot(f2[0], ld4(KIFS_BUNNY_OUT[0]));
#pragma unroll
    for (int k = 1; k < 4; ++k) r = r + dot(f2[k], ld4(KIFS_BUNNY_OUT[k]));
    return r - 0.16f;
}

template <int PRIM>
KIFS_DEV float kifs_sdf(const FrameParams& P, V3 p, unsigned long long lanes = ~0ull) {  // kifs.wgsl:139-155
    if constexpr (PRIM == PRIM_SPHERE) {
        return length(p) - 1.0f;
    } else if constexpr (PRIM == PRIM_CYLINDER) {
        V2 d{abs_(length(V2{p.x, p.y})) - 1.0f, abs_(p.z) - 2.0f};
        V2 dm{max_(d.x, 0.0f), max_(d.y, 0.0f)};
        return min_(max_(d.x, d.y), 0.0f) + length(dm);
    } else if constexpr (PRIM == PRIM_BOX) {
        V3 q{abs_(p.x) - 1.0f, abs_(p.y) - 1.0f, abs_(p.z) - 1.0f};
        V3 qm{max_(q.x, 0.0f), max_(q.y, 0.0f), max_(q.z, 0.0f)};
        return length(qm) + min_(max_(q.x, max_(q.y, q.z)), 0.0f);
    } else if constexpr (PRIM == PRIM_TORUS) {
        V2 q{length(V2{p.x, p.y}) - 1.0f, p.z};
        return length(q) - 0.3f;
    } else if constexpr (PRIM == PRIM_SIERPINSKI) {
        return sierpinski_sdf(P, p, lanes);
    } else if constexpr (PRIM == PRIM_BUNNY) {
        return bunny_sdf(p);
    } else {
        return 1.0f;
    }
}

// Central differences with h = epsilon, no division by 2h (kifs.wgsl:157-167), for any estimate.
template <class Sdf>
KIFS_DEV V3 normal_fd(float h, V3 p, Sdf sdf) {
    float dx = sdf(V3{p.x + h, p.y + 0.0f, p.z + 0.0f}) - sdf(V3{p.x - h, p.y - 0.0f, p.z - 0.0f});
    float dy = sdf(V3{p.x + 0.0f, p.y + h, p.z + 0.0f}) - sdf(V3{p.x - 0.0f, p.y - h, p.z - 0.0f});
    float dz = sdf(V3{p.x + 0.0f, p.y + 0.0f, p.z + h}) - sdf(V3{p.x - 0.0f, p.y - 0.0f, p.z - h});
    return normalize(V3{dx, dy, dz});
}

template <int PRIM>
KIFS_DEV V3 kifs_normal(const FrameParams& P, V3 p) {
    return normal_fd(P.epsilon, p, [&](V3 q) { return kifs_sdf<PRIM>(P, q); });
}

// `lanes`: mask of the lanes whose estimate is used; a scene may skip the others' work.
template <int GROUP, int PRIM>
KIFS_DEV float scene_sdf(const FrameParams& P, V3 p, unsigned long long lanes = ~0ull) {
    if constexpr (GROUP == GROUP_JULIA) return julia_sdf(P, p);
    else if constexpr (GROUP == GROUP_GENJULIA) return genjulia_sdf(P, p, lanes);
    else return kifs_sdf<PRIM>(P, p, lanes);
}

template <int GROUP, int PRIM>
KIFS_DEV V3 scene_normal(const FrameParams& P, V3 p) {
    if constexpr (GROUP == GROUP_JULIA) return julia_normal(P, p);
    else if constexpr (GROUP == GROUP_GENJULIA) return genjulia_normal(P, p);
    else return kifs_normal<PRIM>(P, p);
}

// ---- fs_main: pixel -> ray (entry.wgsl:49-59) ---------------------------------------
KIFS_DEV V3 ray_direction(const FrameParams& P, int x, int y) {
    float px = float(x) + 0.5f, py = float(y) + 0.5f;  // fragment centre, y = 0 at the top
    float uvx = (2.0f * px) / P.height - P.aspect;
    float uvy = (2.0f * py) / P.height - 1.0f;
    V3 d{(uvx * P.m1.x - uvy * P.m2.x) - P.m0.x, (uvx * P.m1.y - uvy * P.m2.y) - P.m0.y,
         (uvx * P.m1.z - uvy * P.m2.z) - P.m0.z};
    return normalize(d);
}

// ---- the lighting model: entry.wgsl:14-19 and the soft-shadow extension, stated once --------------
// Every shading site of the library -- the whole-ray drivers below, the pooled shaders of kifs_kernels.hip -- is made
// of these pieces, so the operations and their order exist in one place.
// The direct term: dot(n, (1,1,1)) clamped; the light is not normalised (:17).
KIFS_DEV float direct_term(V3 n) { return clamp_((n.x + n.y) + n.z, 0.0f, 1.0f); }
// The colour of a hit whose (attenuated) direct term is `lit` (:18-19).
KIFS_DEV V3 lit_colour(const FrameParams& P, float lit) {
    const float diffuse = fmaf_(0.9f, lit, 0.1f);
    return V3{diffuse * P.fractal_color.x, diffuse * P.fractal_color.y, diffuse * P.fractal_color.z};
}
// Heatmap mode: the loop counter at which the ray stopped, as a fraction of max_iterations (:27-29).
KIFS_DEV V3 heatmap_colour(const FrameParams& P, int i_final) {
    const float f = float(i_final) / float(P.max_iterations);
    return V3{f * P.fractal_color.x, f * P.fractal_color.y, f * P.fractal_color.z};
}

// Extension: soft shadows (not in the reference; see KifsExtensions).  A secondary march from the hit point towards
// the light, operation for operation as specified in include/kifs_hip.h.
struct ShadowRay {
    V3 start;    // the hit point lifted off the surface
    float t;     // distance marched along the light direction
    float res;   // the attenuation so far
    int j;       // estimates taken
};
KIFS_DEV V3 shadow_start(const FrameParams& P, V3 p, V3 n) {
    const float off = 2.0f * P.epsilon;
    return V3{fmaf_(off, n.x, p.x), fmaf_(off, n.y, p.y), fmaf_(off, n.z, p.z)};
}
KIFS_DEV ShadowRay shadow_ray_from(const FrameParams& P, V3 start) { return ShadowRay{start, P.shadow_t0, 1.0f, 0}; }
KIFS_DEV ShadowRay shadow_ray(const FrameParams& P, V3 p, V3 n) { return shadow_ray_from(P, shadow_start(P, p, n)); }
// The position whose estimate the ray takes next.
KIFS_DEV V3 shadow_point(const ShadowRay& s) {
    const V3 L = normalize(V3{1.0f, 1.0f, 1.0f});
    return V3{fmaf_(s.t, L.x, s.start.x), fmaf_(s.t, L.y, s.start.y), fmaf_(s.t, L.z, s.start.z)};
}
// One step with the estimate h at shadow_point(s); true when the ray is over (s.res is then its factor).  The caller
// counts it (++s.j) where that suits its loop: a wave whose rays step together keeps the count in a scalar register.
KIFS_DEV bool shadow_step(const FrameParams& P, float h, ShadowRay& s) {
    if (h < P.epsilon) {
        s.res = 0.0f;
        return true;
    }
    s.res = min_(s.res, (P.shadow_k * h) / s.t);
    s.t = s.t + h;
    return (s.t > P.shadow_max_t) || !(s.j + 1 < P.shadow_steps);
}
// Whole secondary rays, one per lane.  `lanes_hit` selects the lanes that take part; the loop leaves when none of
// them is still marching.
template <class Sdf>
KIFS_DEV float soft_shadow(const FrameParams& P, V3 p, V3 n, bool lanes_hit, Sdf sdf) {
    ShadowRay s = shadow_ray(P, p, n);
    bool marching = lanes_hit && (0 < P.shadow_steps);
    for (; __builtin_amdgcn_ballot_w64(marching) != 0ull; ++s.j) {
        if (marching) marching = !shadow_step(P, sdf(shadow_point(s), ~0ull), s);
    }
    return s.res;
}

// Colour of a hit at p, soft shadows if enabled.  `sdf(p, lanes)`: the scene's estimate (lanes = whose value is used);
// `normal(p)`: its normal.  n_out, when given, receives the normal the shading used (the geometry output's).
template <class Sdf, class Normal>
KIFS_DEV V3 generic_shade(const FrameParams& P, V3 p, Sdf sdf, Normal normal, V3* n_out = nullptr) {
    const V3 n = normal(p);
    if (n_out) *n_out = n;
    float lit = direct_term(n);
    // (a lane whose direct term is not positive marches no secondary ray: its factor is 1 and 0 * 1 = 0)
    if (__builtin_expect(P.soft_shadow != 0u, 0)) lit = lit * soft_shadow(P, p, n, lit > 0.0f, sdf);
    return lit_colour(P, lit);
}
// The same for pipeline <GROUP, PRIM> (Julia: julia.wgsl:29-56 for the normal; its PRIM slot is not a primitive).
template <int GROUP, int PRIM>
KIFS_DEV V3 shade_hit(const FrameParams& P, V3 p, V3* n_out = nullptr) {
    constexpr int NPRIM = GROUP == GROUP_JULIA ? 0 : PRIM;
    return generic_shade(
        P, p, [&](V3 q, unsigned long long lanes) { return scene_sdf<GROUP, NPRIM>(P, q, lanes); },
        [&](V3 q) { return scene_normal<GROUP, NPRIM>(P, q); }, n_out);
}

// ---- the long-ray loop: every live lane inside the bounding sphere -------------------------
// The rays that decide a frame's run time skim the fractal for hundreds of steps, deep inside
// the bounding sphere, alone on their SIMD.  For that state -- no live lane outside the sphere,
// |q|^2 an ordinary positive number, not heatmap mode -- this routine runs whole march steps
// (entry.wgsl:12-25 with julia.wgsl:5-27 inlined) as one hand-scheduled instruction stream
// with two taken branches per step; anything else returns to the general loop, which redoes
// the step it was handed.  Arithmetic is operation-for-operation the C++ above: dot(p,p) as
// an fma chain, the packed orbit, log_normal, the correctly rounded divide and square root
// (the same v_div_scale/v_rcp/v_div_fmas/v_div_fixup and v_sqrt + one-ulp-fixup sequences
// hipcc emits, with their wait states), `d < epsilon`, t += d, p = fma(t, dir, origin).
//
// Registers: v[30:31] p.yz  v[32:33] [p.x, 1]  v[34:35] [t, dir.x]  v[36:37] dir.yz
//            v[38:39] [0.1, 1]  v[40:51] orbit (see julia_interior)  v52-v63 scratch, v59 = c1
//            s[84:85] caller exec  s[86:87] live lanes of the step  s[88:91] [2,4],[2,1]
//            s92 mantissa mask  s93/s94 class masks  s96/s97 trip counters  s[80:83] compare masks
// One orbit trip, two forms of the same operations (results bit for bit the same):
//  * PACKED: 8 v_pk_*_f32 + v_cmpx -- the fewest instructions, for a wave alone on its SIMD (a lone wave
//    issues one instruction per ~5 cycles whatever it is): the latency path.
//  * SCALAR: 13 plain f32 operations + v_cmpx -- the fewest VALU CYCLES, for SIMDs with several busy
//    waves, where the vector pipe is the limit: a wave64 v_fma_f32 occupies it for 2.25 cycles, a packed
//    one for 4.3 (tools/microbench/valu_rate.hip), so the packed trip costs 38 cycles and this one 33.
//    Same registers, the pairs of the packed form taken apart: v40 y  v41 z  v42 w  v43 dq  v44 |q|^2
//    v45 x_next  v46 2x  v47 4|q_prev|^2  v48-v50 scratch.
#define KIFS_FAST_TRIP_PACKED                                                               \
    "v_pk_fma_f32 v[40:41], v[46:47], v[40:41], %[cyz] op_sel_hi:[0,1,1]\n"                   \
    "v_pk_fma_f32 v[42:43], v[46:47], v[42:43], %[cw0]\n"                                     \
    "v_pk_mul_f32 v[46:47], v[44:45], s[88:89] op_sel:[1,0] op_sel_hi:[0,1]\n"                \
    "v_pk_mul_f32 v[48:49], v[40:41], v[40:41]\n"                                             \
    "v_pk_add_f32 v[50:51], v[48:49], v[48:49] op_sel:[0,1] op_sel_hi:[0,1]\n"                \
    "v_pk_fma_f32 v[48:49], v[42:43], v[42:43], v[50:51] op_sel_hi:[0,0,1]\n"                 \
    "v_pk_fma_f32 v[44:45], v[44:45], v[44:45], v[48:49] op_sel:[1,1,0] op_sel_hi:[1,1,1] neg_hi:[0,0,1]\n" \
    "v_pk_add_f32 v[44:45], v[44:45], %[c0x]\n"                                               \
    "v_cmpx_nlt_f32 vcc, %[maxd], v44\n" /* exec &= !(|q|^2 > max_distance): escaped lanes freeze */
#define KIFS_FAST_TRIP_SCALAR                                                               \
    "v_fma_f32 v40, v46, v40, %[cy]\n"        /* y' = fma(2x, y, c.y) */                      \
    "v_fma_f32 v41, v46, v41, %[cz]\n"                                                        \
    "v_fma_f32 v42, v46, v42, %[cw]\n"                                                        \
    "v_fma_f32 v43, v47, v43, 0\n"            /* dq = fma(4|q_prev|^2, dq, 0) (one trip late) */ \
    "v_mul_f32_e32 v46, 2.0, v45\n"           /* 2 x_next */                                  \
    "v_mul_f32_e32 v47, 4.0, v44\n"           /* 4 |q|^2 */                                   \
    "v_mul_f32_e32 v48, v40, v40\n"                                                           \
    "v_mul_f32_e32 v49, v41, v41\n"                                                           \
    "v_add_f32_e32 v50, v48, v49\n"           /* s = y*y + z*z */                             \
    "v_fma_f32 v48, v42, v42, v50\n"          /* d = fma(w, w, s) */                          \
    "v_fma_f32 v44, v45, v45, v48\n"          /* |q|^2 = fma(x, x, d) */                      \
    "v_fma_f32 v45, v45, v45, -v48\n"         /* fma(x, x, -d) */                             \
    "v_add_f32_e32 v45, %[cx], v45\n"         /* + c.x: the x after next */                   \
    "v_cmpx_nlt_f32 vcc, %[maxd], v44\n"
// the squares of q_0 in front of the first trip, same two forms
#define KIFS_JULIA_PROLOGUE_PACKED                                                          \
    "v_pk_mul_f32 v[46:47], v[32:33], s[90:91]\n"         /* T = [2 x_0, 1] */               \
    "v_mov_b64 v[40:41], v[30:31]\n"                      /* YZ = [y_0, z_0] */              \
    "v_mov_b64 v[42:43], v[38:39]\n"                      /* WD = [0.1, 1] */                \
    "v_pk_mul_f32 v[48:49], v[40:41], v[40:41]\n"         /* squares of q_0 -> Q = [|q_0|^2, x_1] */ \
    "v_pk_add_f32 v[50:51], v[48:49], v[48:49] op_sel:[0,1] op_sel_hi:[0,1]\n"               \
    "v_pk_fma_f32 v[48:49], v[42:43], v[42:43], v[50:51] op_sel_hi:[0,0,1]\n"                \
    "v_pk_fma_f32 v[44:45], v[32:33], v[32:33], v[48:49] op_sel_hi:[0,0,1] neg_hi:[0,0,1]\n" \
    "v_pk_add_f32 v[44:45], v[44:45], %[c0x]\n"
#define KIFS_JULIA_PROLOGUE_SCALAR                                                          \
    "v_mul_f32_e32 v46, 2.0, v32\n"                                                          \
    "v_mov_b32_e32 v47, 1.0\n"                                                               \
    "v_mov_b64 v[40:41], v[30:31]\n"                                                         \
    "v_mov_b64 v[42:43], v[38:39]\n"                                                         \
    "v_mul_f32_e32 v48, v40, v40\n"                                                          \
    "v_mul_f32_e32 v49, v41, v41\n"                                                          \
    "v_add_f32_e32 v50, v48, v49\n"                                                          \
    "v_fma_f32 v48, v42, v42, v50\n"                                                         \
    "v_fma_f32 v44, v32, v32, v48\n"                                                         \
    "v_fma_f32 v45, v32, v32, -v48\n"                                                        \
    "v_add_f32_e32 v45, %[cx], v45\n"
// SCALAR, DOUBLED: the scalar trip with the orbit carried as Q = 2q (X = 2x, Y = 2y, Z = 2z, W = 2w): 11 plain f32
// operations + v_cmpx instead of 13 -- the `2x` of ijk' and the `4|q|^2` of dq come for free.  Every result is the
// contract's value times an exact power of two ("exactness-preserving rewrites", for the proof and
// its condition, FrameParams::orbit_x2, checked on the host):
//   Y' = fma(X, Y, 2c.y) = 2 y'   S = Y*Y + Z*Z = 4 s   D = fma(W, W, S) = 4 d   N4 = fma(X, X, D) = 4 |q|^2
//   R = fma(X, X, -D) = 4 fma(x, x, -d)   X' = fma(R, 0.5, 2c.x) = 2 x' (R * 0.5 is exact inside the fma)
// dq is NOT scaled: DQ = fma(N4, DQ, 0) is the contract's dq *= 4|q|^2 on the same operands, applied at the start of
// the next trip, so after the last trip DQ is already dqs.  Registers: v40 Y  v41 z  v52 W  v53 DQ  v44 N4
// v45 / v46 X (X_k and X_{k+1} alternate: trip A reads X_k from v46 and writes X_{k+2} there, trip B the other way
// round, so a block of six trips ends where it began)  v48-v50 scratch.
#define KIFS_FAST_TRIP_X2_(xk, xk1)                                                         \
    "v_fma_f32 v40, " xk ", v40, %[cy]\n"     /* Y' = fma(X, Y, 2c.y) */                      \
    "v_fma_f32 v41, " xk ", v41, %[cz]\n"                                                     \
    "v_fma_f32 v52, " xk ", v52, %[cw]\n"                                                     \
    "v_fma_f32 v53, v44, v53, 0\n"            /* dq = fma(4|q_prev|^2, dq, 0) */              \
    "v_mul_f32_e32 v48, v40, v40\n"                                                           \
    "v_mul_f32_e32 v49, v41, v41\n"                                                           \
    "v_add_f32_e32 v50, v48, v49\n"           /* S = Y*Y + Z*Z */                             \
    "v_fma_f32 v48, v52, v52, v50\n"          /* D = fma(W, W, S) */                          \
    "v_fma_f32 v44, " xk1 ", " xk1 ", v48\n"  /* N4 = fma(X, X, D) */                         \
    "v_fma_f32 v49, " xk1 ", " xk1 ", -v48\n" /* R = fma(X, X, -D) */                         \
    "v_fma_f32 " xk ", v49, 0.5, %[cx]\n"     /* X after next = fma(R, 0.5, 2c.x) */          \
    "v_cmpx_nlt_f32 vcc, %[maxd4], v44\n"     /* !(4|q|^2 > 4 max_distance) */
#define KIFS_FAST_TRIP_X2_A KIFS_FAST_TRIP_X2_("v46", "v45")
#define KIFS_FAST_TRIP_X2_B KIFS_FAST_TRIP_X2_("v45", "v46")
// The squares of Q_0 = 2 q_0 (w_0 = 0.1: v38 holds 0.2).  No test on the start point is needed: a y_0^2 or z_0^2 that
// rounds differently at 4x scale is below 2^-124, and d_0 = fma(w_0, w_0, s_0) >= 0.01 absorbs it.
#define KIFS_JULIA_PROLOGUE_X2                                                              \
    "v_add_f32_e32 v46, v32, v32\n"                       /* X_0 = 2 x_0 */                  \
    "v_pk_add_f32 v[40:41], v[30:31], v[30:31]\n"         /* [Y_0, Z_0] */                   \
    "v_mov_b64 v[52:53], v[38:39]\n"                      /* [W_0, DQ] = [0.2, 1] */         \
    "v_mul_f32_e32 v48, v40, v40\n"                                                          \
    "v_mul_f32_e32 v49, v41, v41\n"                                                          \
    "v_add_f32_e32 v50, v48, v49\n"                                                          \
    "v_fma_f32 v48, v52, v52, v50\n"                                                         \
    "v_fma_f32 v44, v46, v46, v48\n"                                                         \
    "v_fma_f32 v49, v46, v46, -v48\n"                                                        \
    "v_fma_f32 v45, v49, 0.5, %[cx]\n"                    /* X_1 */

// The loop over blocks of six trips (s96 = blocks left; label 12 in, label 14 out), two forms:
//  * SINGLE: one block per pass -- the throughput kernel's (its SIMDs hold several busy waves: a taken branch is
//    hidden, the code it fetches is not: two blocks per pass cost the headline 0.4 %).
//  * PAIRED: two blocks per pass, an odd block left over out of line (labels 16 / 17) -- the latency kernels': a lone
//    wave pays for every taken branch, and with one block per pass the reference's 100 iterations took the back edge
//    sixteen times per march step (lone 1080p frame at the reference's constants 0.218 -> 0.210 ms, the headline
//    workload's 12 iterations 0.1557 -> 0.1546; profiles/r04/ab_paired_blocks.txt).
#define KIFS_ORBIT_BLOCK_(exit)                                                             \
    KIFS_FAST_TRIP exit KIFS_FAST_TRIP exit KIFS_FAST_TRIP
#define KIFS_ORBIT_LOOP_SINGLE                                                              \
    "12:\n"                                                                                 \
    "s_cmp_eq_u32 s96, 0\n"                                                                 \
    "s_cbranch_scc1 14f\n"                                                                  \
    "13:\n"                                                                                 \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT) "s_cbranch_execz 14f\n"                               \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT) "s_cbranch_execz 14f\n"                               \
    "s_sub_u32 s96, s96, 1\n"                                                               \
    "s_cmp_lg_u32 s96, 0\n"                                                                 \
    "s_cbranch_scc1 13b\n"
// SINGLE for the doubled trip: the six trips of a pass alternate A, B (see KIFS_FAST_TRIP_X2_)
#define KIFS_ORBIT_LOOP_SINGLE_X2                                                           \
    "12:\n"                                                                                 \
    "s_cmp_eq_u32 s96, 0\n"                                                                 \
    "s_cbranch_scc1 14f\n"                                                                  \
    "13:\n"                                                                                 \
    KIFS_FAST_TRIP_X2_A KIFS_TRIP_EXIT KIFS_FAST_TRIP_X2_B KIFS_TRIP_EXIT                   \
    KIFS_FAST_TRIP_X2_A "s_cbranch_execz 14f\n"                                             \
    KIFS_FAST_TRIP_X2_B KIFS_TRIP_EXIT KIFS_FAST_TRIP_X2_A KIFS_TRIP_EXIT                   \
    KIFS_FAST_TRIP_X2_B "s_cbranch_execz 14f\n"                                             \
    "s_sub_u32 s96, s96, 1\n"                                                               \
    "s_cmp_lg_u32 s96, 0\n"                                                                 \
    "s_cbranch_scc1 13b\n"
// The remainder trips (sdf_iters % 6) of the doubled trip, out of line: in pairs A, B; an odd last one is an A trip
// followed by a swap of v45 / v46, so that the blocks start from the A state again.
#define KIFS_ORBIT_REMAINDER_X2                                                             \
    "30:\n"                                                                                 \
    "s_mov_b32 s97, %[rem]\n"                                                               \
    "s_cmp_lt_u32 s97, 2\n"                                                                 \
    "s_cbranch_scc1 32f\n"                                                                  \
    "31:\n"                                                                                 \
    KIFS_FAST_TRIP_X2_A KIFS_TRIP_EXIT_BACK KIFS_FAST_TRIP_X2_B KIFS_TRIP_EXIT_BACK         \
    "s_sub_u32 s97, s97, 2\n"                                                               \
    "s_cmp_gt_u32 s97, 1\n"                                                                 \
    "s_cbranch_scc1 31b\n"                                                                  \
    "32:\n"                                                                                 \
    "s_cmp_eq_u32 s97, 0\n"                                                                 \
    "s_cbranch_scc1 12b\n"                                                                  \
    KIFS_FAST_TRIP_X2_A KIFS_TRIP_EXIT_BACK                                                 \
    "v_swap_b32 v45, v46\n"                                                                 \
    "s_branch 12b\n"
// the remainder trips of the other forms: one trip at a time
#define KIFS_ORBIT_REMAINDER_ONE                                                             \
    "30:\n"                                                                                 \
    "s_mov_b32 s97, %[rem]\n"                                                               \
    "31:\n"                                                                                 \
    KIFS_FAST_TRIP KIFS_TRIP_EXIT_BACK                                                      \
    "s_sub_u32 s97, s97, 1\n"                                                               \
    "s_cmp_lg_u32 s97, 0\n"                                                                 \
    "s_cbranch_scc1 31b\n"                                                                  \
    "s_branch 12b\n"
#define KIFS_ORBIT_LOOP_PAIRED                                                            \
    "12:\n"                                                                                 \
    "s_cmp_lt_u32 s96, 2\n"                                                                 \
    "s_cbranch_scc1 16f\n"                                                                  \
    "13:\n"                                                                                 \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT) "s_cbranch_execz 14f\n"                               \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT) "s_cbranch_execz 14f\n"                               \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT) "s_cbranch_execz 14f\n"                               \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT) "s_cbranch_execz 14f\n"                               \
    "s_sub_u32 s96, s96, 2\n"                                                               \
    "s_cmp_gt_u32 s96, 1\n"                                                                 \
    "s_cbranch_scc1 13b\n"                                                                  \
    "s_cmp_lg_u32 s96, 0\n"                                                                 \
    "s_cbranch_scc1 17f\n" /* one block left (out of line) */
#define KIFS_ORBIT_LOOP_PAIRED_OUT_OF_LINE                                                  \
    "16:\n"                                                                                 \
    "s_cmp_eq_u32 s96, 0\n"                                                                 \
    "s_cbranch_scc1 14b\n"                                                                  \
    "17:\n"                                                                                 \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT_BACK) "s_cbranch_execz 14b\n"                          \
    KIFS_ORBIT_BLOCK_(KIFS_TRIP_EXIT_BACK) "s_branch 14b\n"

// quot = |q|^2 / dqs and root = sqrt(quot), both correctly rounded, any operands: the sequences
// hipcc emits (v_div_scale / v_rcp / Newton / v_div_fmas / v_div_fixup; v_sqrt + one-ulp fixup
// with the 2^32 pre-scaling for tiny arguments), with their wait states.  v44 = |q|^2, v53 = dqs,
// v55 = lg in; v54 = 0.25 lg and v60 = root out.
#define KIFS_DIVSQRT_FULL \
    /* ---- quot = |q|^2 / dqs, correctly rounded */ \
    "v_div_scale_f32 v60, s[82:83], v53, v53, v44\n" \
    "v_div_scale_f32 v61, vcc, v44, v53, v44\n" \
    "v_rcp_f32_e32 v62, v60\n" \
    "v_mul_f32_e32 v54, 0x3e800000, v55\n"  /* 0.25 * lg */ \
    "v_fma_f32 v63, -v60, v62, 1.0\n" \
    "v_fmac_f32_e32 v62, v63, v62\n" \
    "v_mul_f32_e32 v63, v61, v62\n" \
    "v_fma_f32 v55, -v60, v63, v61\n" \
    "v_fmac_f32_e32 v63, v55, v62\n" \
    "v_fma_f32 v60, -v60, v63, v61\n" \
    "v_div_fmas_f32 v60, v60, v62, v63\n" \
    "v_div_fixup_f32 v60, v60, v53, v44\n" \
    /* ---- root = sqrt(quot), correctly rounded */ \
    "v_mul_f32_e32 v61, 0x4f800000, v60\n" \
    "v_cmp_gt_f32_e32 vcc, 0x0f800000, v60\n"  /* below 2^-96: work on quot * 2^32 */ \
    "s_nop 1\n" \
    "v_cndmask_b32_e32 v60, v60, v61, vcc\n" \
    "v_sqrt_f32_e32 v61, v60\n" \
    "s_nop 0\n" \
    "v_add_u32_e32 v62, -1, v61\n"  /* candidates one ulp either side */ \
    "v_add_u32_e32 v63, 1, v61\n" \
    "v_fma_f32 v52, -v62, v61, v60\n" \
    "v_fma_f32 v56, -v63, v61, v60\n" \
    "v_cmp_ge_f32_e64 s[80:81], 0, v52\n" \
    "v_cmp_lt_f32_e64 s[82:83], 0, v56\n" \
    "s_nop 0\n" \
    "v_cndmask_b32_e64 v62, v61, v62, s[80:81]\n" \
    "v_cndmask_b32_e64 v61, v62, v63, s[82:83]\n" \
    "v_mul_f32_e32 v62, 0x37800000, v61\n" \
    "v_cndmask_b32_e32 v61, v61, v62, vcc\n"  /* undo the 2^32 scaling */ \
    "v_cmp_class_f32_e64 vcc, v60, s94\n"  /* sqrt(+-0) = +-0, sqrt(inf) = inf */ \
    "s_nop 1\n" \
    "v_cndmask_b32_e32 v60, v61, v60, vcc\n"

// The same two results when both operands are ordinary -- |q|^2 and dqs within [2^-10, 2^84): the
// exponents differ by at most 94, so v_div_scale would scale nothing (it does from 96), v_div_fmas
// is a plain fma, v_div_fixup passes the quotient through, and the quotient (> 2^-95) needs
// neither the 2^32 pre-scaling (below 2^-96) nor the zero / infinity patch of the square root: the same Newton and fixup arithmetic, nine instructions and four wait
// states shorter.  A wave with a lane outside the range runs KIFS_DIVSQRT_FULL out of line.
// Used when sdf_iters is small: after ~25 iterations dqs of a bounded orbit leaves the range.
#define KIFS_DIVSQRT_ORDINARY \
    "v_subrev_u32_e32 v60, 0x3a800000, v44\n"   /* bits - bits(2^-10) */ \
    "v_subrev_u32_e32 v61, 0x3a800000, v53\n" \
    "v_max_u32_e32 v60, v60, v61\n" \
    "v_cmp_gt_u32_e32 vcc, 0x2f000000, v60\n"   /* both below 2^84 (and not negative / NaN) */ \
    "s_xor_b64 vcc, vcc, exec\n" \
    "s_cbranch_scc1 46f\n" \
    "v_rcp_f32_e32 v62, v53\n" \
    "v_mul_f32_e32 v54, 0x3e800000, v55\n"      /* 0.25 * lg */ \
    "v_fma_f32 v63, -v53, v62, 1.0\n" \
    "v_fmac_f32_e32 v62, v63, v62\n" \
    "v_mul_f32_e32 v63, v44, v62\n" \
    "v_fma_f32 v55, -v53, v63, v44\n" \
    "v_fmac_f32_e32 v63, v55, v62\n" \
    "v_fma_f32 v60, -v53, v63, v44\n" \
    "v_fma_f32 v60, v60, v62, v63\n" \
    "v_sqrt_f32_e32 v61, v60\n" \
    "s_nop 0\n" \
    "v_add_u32_e32 v62, -1, v61\n"               /* candidates one ulp either side */ \
    "v_add_u32_e32 v63, 1, v61\n" \
    "v_fma_f32 v52, -v62, v61, v60\n" \
    "v_fma_f32 v56, -v63, v61, v60\n" \
    "v_cmp_ge_f32_e64 s[80:81], 0, v52\n" \
    "v_cmp_lt_f32_e64 s[82:83], 0, v56\n" \
    "s_nop 0\n" \
    "v_cndmask_b32_e64 v62, v61, v62, s[80:81]\n" \
    "v_cndmask_b32_e64 v60, v62, v63, s[82:83]\n" \
    "47:\n"

// SHORT_DIVSQRT: the launcher's choice for frames with few SDF iterations (KIFS_DIVSQRT_ORDINARY);
// THROUGHPUT: the scalar form of the orbit trip (launches whose SIMDs hold several busy waves);
// X2 (with THROUGHPUT): that trip in doubled coordinates, for scenes with FrameParams::orbit_x2 (a separate kernel: two
// of these asm statements in one kernel are more than the register allocator can take).
template <bool SHORT_DIVSQRT, bool THROUGHPUT, bool X2>
KIFS_DEV void julia_fast_march(const FrameParams& P, V3 dir, float& t, V3& p, bool& hit,
                               bool& marching, int& trips, int& outside_steps, int limit) {
    static_assert(THROUGHPUT || !X2, "the doubled trip is a form of the scalar one");
    F2 pyz{p.y, p.z}, px1{p.x, 1.0f}, tdx{t, dir.x};
    const F2 dyz{dir.y, dir.z};
    const F2 oyz{P.origin.y, P.origin.z};
    const float c1 = -1.1514610310E-1f;  // second log coefficient, needed in a VGPR
    const unsigned long long lanes = __builtin_amdgcn_ballot_w64(marching);
    unsigned long long hit_mask = 0, live_out;
    if constexpr (THROUGHPUT) {
#define KIFS_TRIP_EXIT "s_cbranch_execz 14f\n"  /* scalar slots are free where the vector pipe is the limit: test every trip */
#define KIFS_TRIP_EXIT_BACK "s_cbranch_execz 14b\n"  /* the same from the remainder trips, which sit BEHIND label 14 */
#define KIFS_ORBIT_LOOP_OUT_OF_LINE
        if constexpr (X2) {  // the doubled trip
            const F2 w0{2.0f * 0.1f, 1.0f};
#define KIFS_FAST_TRIP KIFS_FAST_TRIP_X2_A
#define KIFS_JULIA_PROLOGUE KIFS_JULIA_PROLOGUE_X2
#define KIFS_ORBIT_LOOP KIFS_ORBIT_LOOP_SINGLE_X2
#define KIFS_ORBIT_REMAINDER KIFS_ORBIT_REMAINDER_X2
#define KIFS_JULIA_LOG_BIAS "0xffffff80"  /* v44 = 4|q|^2: biased - 128 */
#define KIFS_JULIA_ORBIT_OUT "v44, 0x3e800000, v44"  /* |q|^2 = 0.25 (4|q|^2), exact; DQ (v53) is dqs */
#define KIFS_JULIA_C_OPERANDS [cy] "s"(P.c2.y), [cz] "s"(P.c2.z), [cw] "s"(P.c2.w), [cx] "s"(P.c2.x), \
                              [maxd4] "s"(P.max_distance4)
        if constexpr (SHORT_DIVSQRT) {
#define KIFS_JULIA_DIVSQRT KIFS_DIVSQRT_ORDINARY
#define KIFS_JULIA_DIVSQRT_OUT_OF_LINE "46:\n" KIFS_DIVSQRT_FULL "s_branch 47b\n"
#include "kifs_julia_march_asm.hpp"
#undef KIFS_JULIA_DIVSQRT
#undef KIFS_JULIA_DIVSQRT_OUT_OF_LINE
        } else {
#define KIFS_JULIA_DIVSQRT KIFS_DIVSQRT_FULL
#define KIFS_JULIA_DIVSQRT_OUT_OF_LINE
#include "kifs_julia_march_asm.hpp"
#undef KIFS_JULIA_DIVSQRT
#undef KIFS_JULIA_DIVSQRT_OUT_OF_LINE
        }
#undef KIFS_FAST_TRIP
#undef KIFS_JULIA_PROLOGUE
#undef KIFS_ORBIT_LOOP
#undef KIFS_ORBIT_REMAINDER
#undef KIFS_JULIA_LOG_BIAS
#undef KIFS_JULIA_ORBIT_OUT
#undef KIFS_JULIA_C_OPERANDS
        } else {
            const F2 w0{0.1f, 1.0f};
#define KIFS_FAST_TRIP KIFS_FAST_TRIP_SCALAR
#define KIFS_JULIA_PROLOGUE KIFS_JULIA_PROLOGUE_SCALAR
#define KIFS_ORBIT_LOOP KIFS_ORBIT_LOOP_SINGLE
#define KIFS_ORBIT_REMAINDER KIFS_ORBIT_REMAINDER_ONE
#define KIFS_JULIA_LOG_BIAS "0xffffff82"
#define KIFS_JULIA_ORBIT_OUT "v53, v43, v47"  /* dqs = dq * (4|q_last|^2) */
#define KIFS_JULIA_C_OPERANDS [cy] "s"(P.c.y), [cz] "s"(P.c.z), [cw] "s"(P.c.w), [cx] "s"(P.c.x)
        if constexpr (SHORT_DIVSQRT) {
#define KIFS_JULIA_DIVSQRT KIFS_DIVSQRT_ORDINARY
#define KIFS_JULIA_DIVSQRT_OUT_OF_LINE "46:\n" KIFS_DIVSQRT_FULL "s_branch 47b\n"
#include "kifs_julia_march_asm.hpp"
#undef KIFS_JULIA_DIVSQRT
#undef KIFS_JULIA_DIVSQRT_OUT_OF_LINE
        } else {
#define KIFS_JULIA_DIVSQRT KIFS_DIVSQRT_FULL
#define KIFS_JULIA_DIVSQRT_OUT_OF_LINE
#include "kifs_julia_march_asm.hpp"
#undef KIFS_JULIA_DIVSQRT
#undef KIFS_JULIA_DIVSQRT_OUT_OF_LINE
        }
#undef KIFS_FAST_TRIP
#undef KIFS_JULIA_PROLOGUE
#undef KIFS_ORBIT_LOOP
#undef KIFS_ORBIT_REMAINDER
#undef KIFS_JULIA_LOG_BIAS
#undef KIFS_JULIA_ORBIT_OUT
#undef KIFS_JULIA_C_OPERANDS
        }
#undef KIFS_TRIP_EXIT
#undef KIFS_TRIP_EXIT_BACK
#undef KIFS_ORBIT_LOOP_OUT_OF_LINE
    } else {
        const F2 w0{0.1f, 1.0f};
        const F2 cyz{P.c.y, P.c.z}, cw0{P.c.w, 0.0f}, c0x{0.0f, P.c.x};
#define KIFS_FAST_TRIP KIFS_FAST_TRIP_PACKED
#define KIFS_TRIP_EXIT  /* a lone wave pays for every instruction: test every third trip only */
#define KIFS_TRIP_EXIT_BACK
#define KIFS_JULIA_PROLOGUE KIFS_JULIA_PROLOGUE_PACKED
#define KIFS_ORBIT_LOOP KIFS_ORBIT_LOOP_PAIRED
#define KIFS_ORBIT_LOOP_OUT_OF_LINE KIFS_ORBIT_LOOP_PAIRED_OUT_OF_LINE
#define KIFS_ORBIT_REMAINDER KIFS_ORBIT_REMAINDER_ONE
#define KIFS_JULIA_LOG_BIAS "0xffffff82"
#define KIFS_JULIA_ORBIT_OUT "v53, v43, v47"  /* dqs = dq * (4|q_last|^2) */
#define KIFS_JULIA_C_OPERANDS [cyz] "s"(cyz), [cw0] "s"(cw0), [c0x] "s"(c0x)
        if constexpr (SHORT_DIVSQRT) {
#define KIFS_JULIA_DIVSQRT KIFS_DIVSQRT_ORDINARY
#define KIFS_JULIA_DIVSQRT_OUT_OF_LINE "46:\n" KIFS_DIVSQRT_FULL "s_branch 47b\n"
#include "kifs_julia_march_asm.hpp"
#undef KIFS_JULIA_DIVSQRT
#undef KIFS_JULIA_DIVSQRT_OUT_OF_LINE
        } else {
#define KIFS_JULIA_DIVSQRT KIFS_DIVSQRT_FULL
#define KIFS_JULIA_DIVSQRT_OUT_OF_LINE
#include "kifs_julia_march_asm.hpp"
#undef KIFS_JULIA_DIVSQRT
#undef KIFS_JULIA_DIVSQRT_OUT_OF_LINE
        }
#undef KIFS_FAST_TRIP
#undef KIFS_TRIP_EXIT
#undef KIFS_TRIP_EXIT_BACK
#undef KIFS_JULIA_PROLOGUE
#undef KIFS_ORBIT_LOOP
#undef KIFS_ORBIT_LOOP_OUT_OF_LINE
#undef KIFS_ORBIT_REMAINDER
#undef KIFS_JULIA_LOG_BIAS
#undef KIFS_JULIA_ORBIT_OUT
#undef KIFS_JULIA_C_OPERANDS
    }
    const unsigned lane = __lane_id();
    p = V3{px1.x, pyz.x, pyz.y};
    t = tdx.x;
    hit = hit || (((hit_mask >> lane) & 1ull) != 0ull);
    marching = ((live_out >> lane) & 1ull) != 0ull;
}

// ---- raymarch for the Julia pipeline: control flow kept wave-uniform ----------------------
// Same results as the generic loop below.  Each trip classifies the wave with two ballots:
// every marching lane inside the bounding sphere (the state of all long rays: one straight
// run through julia_interior), every marching lane outside (background: a sqrt and a
// subtract), or mixed.  That keeps taken branches -- the expensive thing for a lone wave --
// to the loop's back edge.
// A ray that can never come within the cull radius of the origin (see fill_params): decided at
// ray set-up from the closest approach of the ray's line.
KIFS_DEV bool ray_never_inside(const FrameParams& P, V3 dir) {
    const float oo = dot(P.origin, P.origin);
    const float b = -dot(P.origin, dir);
    const float c2 = fmaf_(-b, b, oo);
    return (b <= 0.0f) ? (oo > P.cull_n2) : (c2 > P.cull_n2);
}

// Issue priority of a wave by the age of its rays (wave-uniform `trips`): see julia_loop.
KIFS_DEV void march_priority(int trips) {
    if (trips >= 96) __builtin_amdgcn_s_setprio(3);
    else if (trips >= 32) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(1);
}

// Whether a ray sets out at all: inside the frame, with a step to make and room to make it in, and -- `cull`,
// wave-uniform: the bounding-sphere cull is on -- not passing the sphere by.  Every scene's estimate obeys
// d(p) >= |p| - B, so outside the sphere of radius R = B + epsilon it exceeds epsilon (Julia: length(p) - 2,
// julia.wgsl:8-9) and a ray that never enters can never satisfy `d < epsilon`: its pixel is background whatever else
// the loop does (only the heatmap's step count would notice, so heatmap frames march every ray).  The test keeps a
// 10 % margin on R^2, orders of magnitude above the rounding of p = fma(t, dir, origin) for any t < max_distance.
KIFS_DEV bool ray_sets_out(const FrameParams& P, V3 dir, bool valid, bool cull) {
    bool live = valid && (0 < P.max_iterations) && (0.0f < P.max_distance);
    if (cull) live = live && !ray_never_inside(P, dir);
    return live;
}
KIFS_DEV bool whole_ray_sets_out(const FrameParams& P, V3 dir, bool valid) {
    return ray_sets_out(P, dir, valid, P.is_heatmap == 0u && P.cull_n2 > 0.0f);
}
// The colour of a finished whole ray (entry.wgsl:26-31): `shade()` is the colour of its hit.
template <class Shade>
KIFS_DEV V3 whole_ray_colour(const FrameParams& P, bool hit, int i_final, Shade shade) {
    V3 colour = P.background_color;
    if (hit) colour = shade();
    if (P.is_heatmap) colour = heatmap_colour(P, i_final);
    return colour;
}

struct JuliaDiag {  // diagnostics of one wave's march (SGPRs)
    int fast_steps = 0, fast_entries = 0, general_steps = 0;
    unsigned long long fast_ticks = 0;
};

// The march loop proper: steps the wave's marching lanes until none is left or `trips` reaches
// `limit` (max_iterations for a whole ray, the end of the current round when the workgroup
// re-queues its rays).  State in, state out; i_final is the heatmap's loop counter.
template <bool SHORT_DIVSQRT, bool THROUGHPUT, bool X2 = false>
KIFS_DEV void julia_loop(const FrameParams& P, V3 dir, float& t, V3& p, bool& hit, bool& marching,
                         int& trips, int& i_final, int limit, JuliaDiag& diag) {
    const bool fast_ok = (P.is_heatmap == 0u) && (P.sdf_iters >= 1);  // wave-uniform
    for (;;) {
        const unsigned long long live = __builtin_amdgcn_ballot_w64(marching);
        if (live == 0ull || trips >= limit) break;
        if (__builtin_expect(fast_ok, 1)) {
            // The hand-written loop takes whole steps for inside and outside lanes alike; it only
            // comes back when it meets a |q|^2 that needs the general log (or it is finished).
            const int before = trips;
            // (unconditional: two s_memtime per entry cost nothing, and the conditional form trips the
            // compiler's SGPR handling around the asm block)
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            int outside_steps = 0;  // (a fresh SGPR for the asm block: struct members confuse the allocator)
            // issue priority by the ray's age: after the culls only rays that reach the fractal get here, and the
            // longer a ray has marched the more likely it is the one its launch ends with
            // (levels 1 / 2 / 3 from 0 / 32 / 96 steps; same-box A/B against "3 for all", three runs each, r03: 48 frames per
            // launch 105.5 -> 106.4 Gpixel/s, 4096^2 x16 64.6 -> 65.3, nothing either way at 8 / 1 per launch; of the other
            // marks tried 64 / 16 and 48 / 16 were 0.7 % behind, and level 0 for the first round cost 5 % at 8 per launch)
            march_priority(trips);
            julia_fast_march<SHORT_DIVSQRT, THROUGHPUT, X2>(P, dir, t, p, hit, marching, trips, outside_steps,
                                                limit < P.max_iterations ? limit : P.max_iterations);
            diag.general_steps += outside_steps;
            diag.fast_ticks += __builtin_amdgcn_s_memtime() - t0;
            ++diag.fast_entries;
            diag.fast_steps += trips - before;
            if (__builtin_amdgcn_ballot_w64(marching) == 0ull || trips >= limit) break;
        }
        const bool more = (trips + 1) < P.max_iterations;
        const float n2 = dot(p, p);
        const bool outside = n2 > P.bound_n2;  // == length(p) > 2 + epsilon
        const unsigned long long out_lanes = __builtin_amdgcn_ballot_w64(outside) & live;
        float d;
        if (__builtin_expect(out_lanes == 0ull, 1)) {
            d = julia_interior(P, p, live);
        } else {
            d = sqrt_(n2) - 2.0f;
            const unsigned long long in_lanes = live & ~out_lanes;
            if (in_lanes != 0ull) {
                float di = julia_interior(P, p, in_lanes);
                d = outside ? d : di;
            }
        }
        const bool h = marching && (d < P.epsilon);
        const bool go = marching && !h;
        hit = hit || h;
        if (__builtin_expect(P.is_heatmap != 0u, 0))  // i is only observable in heatmap mode
            i_final = h ? trips : (go ? trips + 1 : i_final);
        const float tn = t + d;
        t = go ? tn : t;
        p = V3{go ? fmaf_(tn, dir.x, P.origin.x) : p.x, go ? fmaf_(tn, dir.y, P.origin.y) : p.y,
               go ? fmaf_(tn, dir.z, P.origin.z) : p.z};
        marching = go && more && (tn < P.max_distance);
        ++trips;
        ++diag.general_steps;
    }
}

// A whole ray per lane, start to finish (heatmap mode, diagnostics, and the building block the
// re-queuing kernel path is checked against).
template <bool SHORT_DIVSQRT>
KIFS_DEV V3 raymarch_julia(const FrameParams& P, V3 dir, bool valid, int& steps) {
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    int trips = 0;     // == the loop counter i of entry.wgsl:11 for every marching lane
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    JuliaDiag diag;
    const bool stamp = P.counters != nullptr;
    const unsigned long long wave_t0 = stamp ? __builtin_amdgcn_s_memtime() : 0ull;
    julia_loop<SHORT_DIVSQRT, false>(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, diag);
    __builtin_amdgcn_s_setprio(0);
    steps = trips;
    if (__builtin_expect(stamp, 0)) {
        // per-wave record (no atomics: they would serialise the waves being measured):
        // total ticks, ticks in the long-ray loop, long-ray steps | entries << 32, general steps
        const unsigned long long wave_t1 = __builtin_amdgcn_s_memtime();
        if (__lane_id() == 0) {
            unsigned long long* rec = P.counters + 8 + 4ull * (blockIdx.x * 4u + (threadIdx.x >> 6));
            rec[0] = wave_t1 - wave_t0;
            rec[1] = diag.fast_ticks;
            rec[2] = (unsigned long long)diag.fast_steps | ((unsigned long long)diag.fast_entries << 32);
            rec[3] = (unsigned long long)diag.general_steps;
        }
    }
    return whole_ray_colour(P, hit, i_final, [&] { return shade_hit<GROUP_JULIA, 0>(P, p); });
}

// `sdf(p, lanes)`: the scene's estimate (lanes = whose value is used); `normal(p)`: its normal.
// The march loop proper, as julia_loop: until no lane marches or `trips` reaches `limit`.
// AGE_PRIORITY: issue priority by the rays' age at entry and at the marks (march_priority), for the one-wave-per-tile
// throughput kernel, where a round starts here with its rays' step count (same-box A/B, r03: 1080p Sierpinski x48 80.2 ->
// 81.7 Gpixel/s, the lone 8K frame 1.181 -> 1.142 ms); elsewhere one step up after 32 steps, as before (the graded form
// cost the lone 1080p Sierpinski frame 3 % and 8 per launch 1 %).
template <bool AGE_PRIORITY = false, class Sdf>
KIFS_DEV void generic_loop(const FrameParams& P, V3 dir, float& t, V3& p, bool& hit, bool& marching,
                           int& trips, int& i_final, int limit, Sdf sdf) {
    // Bounding-sphere culls (see ray_sets_out and fill_params): every scene's estimate obeys
    // d(p) >= |p| - B, so a lane outside R = B + epsilon and moving away can never satisfy
    // `d < epsilon`.  Not in heatmap mode.
    const bool cull = (P.is_heatmap == 0u) && (P.cull_n2 > 0.0f);  // wave-uniform
    if constexpr (AGE_PRIORITY) march_priority(trips);
    while (__builtin_amdgcn_ballot_w64(marching) != 0ull && trips < limit) {
        if constexpr (AGE_PRIORITY) {
            if (trips == 32 || trips == 96) march_priority(trips);
        } else {
            // a ray still marching after 32 steps is on the frame's critical path: issue it first
            if (trips == 32) __builtin_amdgcn_s_setprio(3);
        }
        const bool more = (trips + 1) < P.max_iterations;  // scalar
        if (cull) {  // early ray termination for lanes that are leaving for good
            const bool leaving = (dot(p, p) > P.cull_n2) && (dot(p, dir) > 0.0f);
            marching = marching && !leaving;
            if (__builtin_amdgcn_ballot_w64(marching) == 0ull) break;
        }
        // The SDF is evaluated for every lane (stopped lanes hold a valid old position, their
        // result is discarded): no divergent region around the expensive part, the state update
        // is a handful of selects.
        const float d = sdf(p, __builtin_amdgcn_ballot_w64(marching));
        const bool h = marching && (d < P.epsilon);
        const bool go = marching && !h;
        hit = hit || h;  // break leaves i un-incremented (:20)
        if (__builtin_expect(P.is_heatmap != 0u, 0))
            i_final = h ? trips : (go ? trips + 1 : i_final);
        const float tn = t + d;
        t = go ? tn : t;
        p = V3{go ? fmaf_(tn, dir.x, P.origin.x) : p.x, go ? fmaf_(tn, dir.y, P.origin.y) : p.y,
               go ? fmaf_(tn, dir.z, P.origin.z) : p.z};
        marching = go && more && (tn < P.max_distance);
        ++trips;
    }
}

// A whole ray per lane, start to finish.
template <class Sdf, class Normal>
KIFS_DEV V3 raymarch_with(const FrameParams& P, V3 dir, bool valid, int& steps, Sdf sdf, Normal normal) {
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    // Every marching lane has made the same number of steps, so the loop counter `i` of
    // entry.wgsl:11 is the wave-uniform trip count (an SGPR); a lane records it when it stops.
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, sdf);
    __builtin_amdgcn_s_setprio(0);
    steps = trips;
    return whole_ray_colour(P, hit, i_final, [&] { return generic_shade(P, p, sdf, normal); });
}

template <int GROUP, int PRIM>
KIFS_DEV V3 raymarch(const FrameParams& P, V3 dir, bool valid, int& steps) {
    // for the Julia pipeline the PRIM slot carries the long-ray loop's variant (launch_render): bit 0 the short divide /
    // square root, bit 1 the doubled orbit trip (throughput kernel only)
    if constexpr (GROUP == GROUP_JULIA) return raymarch_julia<(PRIM & 1) != 0>(P, dir, valid, steps);
    return raymarch_with(
        P, dir, valid, steps,
        [&](V3 q, unsigned long long lanes) { return scene_sdf<GROUP, PRIM>(P, q, lanes); },
        [&](V3 q) { return scene_normal<GROUP, PRIM>(P, q); });
}

// One round of the workgroup's ray queue for pipeline <GROUP, PRIM>: step the wave's lanes until
// `trips` reaches `limit`; and the colour of a hit.  (For the Julia pipeline the PRIM slot is the
// variant of the long-ray loop, see raymarch.)
template <int GROUP, int PRIM, bool THROUGHPUT = false>
KIFS_DEV void march_round(const FrameParams& P, V3 dir, float& t, V3& p, bool& hit, bool& marching,
                          int& trips, int limit) {
    int i_final = 0;  // heatmap frames do not take this path
    if constexpr (GROUP == GROUP_JULIA) {
        JuliaDiag diag;
        julia_loop<(PRIM & 1) != 0, THROUGHPUT, (PRIM & 2) != 0>(P, dir, t, p, hit, marching, trips, i_final, limit, diag);
    } else {
        generic_loop<THROUGHPUT>(P, dir, t, p, hit, marching, trips, i_final, limit,
                                 [&](V3 q, unsigned long long lanes) { return scene_sdf<GROUP, PRIM>(P, q, lanes); });
    }
}

// raymarch<GROUP, PRIM> for the geometry output (kifs_geometry_kernels.hip): the same whole ray per lane, handing out
// what the march and the shading held -- whether the loop broke at d < epsilon, the ray parameter t at the break (the
// tested position is fma(t, dir, origin), or the origin itself with t = 0 on the first step) and the normal the
// shading dotted with (1,1,1).  A lane that did not hit leaves n and t as they were passed in.
template <int GROUP, int PRIM>
KIFS_DEV V3 raymarch_geometry(const FrameParams& P, V3 dir, bool valid, bool& hit, float& t_hit, V3& n) {
    float t = 0.0f;
    V3 p = P.origin;
    hit = false;
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    if constexpr (GROUP == GROUP_JULIA) {
        JuliaDiag diag;
        julia_loop<(PRIM & 1) != 0, false>(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, diag);
    } else {
        generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations,
                     [&](V3 q, unsigned long long lanes) { return scene_sdf<GROUP, PRIM>(P, q, lanes); });
    }
    __builtin_amdgcn_s_setprio(0);
    return whole_ray_colour(P, hit, i_final, [&] {
        t_hit = t;
        return shade_hit<GROUP, PRIM>(P, p, &n);
    });
}

// ---- extension: ambient occlusion (kifs_render_occlusion_async, include/kifs_hip.h) -------------------------------
// The factor of a hit at the tested position p with the shading's normal n, operation for operation as the header
// states it: ao.samples estimates along the normal, each held against how far it stands off the hit.  Every lane takes
// every estimate (a lane that did not hit holds a valid old position and reads nothing of its result); `lanes`: the
// lanes whose factor is used.
template <class Sdf>
KIFS_DEV float ambient_occlusion(const FrameParams& P, const occl::AO& ao, V3 p, V3 n, unsigned long long lanes, Sdf sdf) {
    float occ = 0.0f, w = 1.0f;
    for (int i = 1; i <= ao.samples; ++i) {  // uniform
        const float h = ao.step * float(i);
        const V3 q{fmaf_(h, n.x, p.x), fmaf_(h, n.y, p.y), fmaf_(h, n.z, p.z)};
        const float d = sdf(q, lanes);
        occ = occ + w * (h - d);
        w = w * ao.decay;
    }
    return clamp_(1.0f - ao.strength * occ, 0.0f, 1.0f);
}

// The occlusion kernel's phases read the kernel argument anew, each where it works (kifs_occlusion_kernels.hip): held in
// SGPRs from the kernel's start, the term and the shading's constants would stay live across the march, whose
// hand-written loops pin s74-s97 and leave the frame constants barely enough.  The empty asm ties the loads that follow
// to its place; they are scalar loads of a uniform address, like the kernel argument's own.
namespace occl {
typedef const Params __attribute__((address_space(4))) * ConstParams;
KIFS_DEV ConstParams anew(ConstParams K) {
    asm volatile("" : "+s"(K));
    return K;
}
}  // namespace occl

// generic_shade's colour of a hit at p times the hit's factor, from the same pieces in the same order.  A lane that did
// not hit gets `miss` and the factor 1.  The normal and the shadow ray belong to the hit lanes, as in whole_ray_colour;
// the probes run for the whole wave, outside any divergent region, as the march's estimates do (generic_loop).
struct Occluded {
    V3 colour;
    float a;  // the hit's factor; 1 on a miss
};
template <class Sdf, class Normal>
KIFS_DEV Occluded occluded_shade(const FrameParams& P, const occl::AO& ao, V3 p, bool hit, V3 miss, Sdf sdf, Normal normal) {
    V3 n{0.0f, 0.0f, 0.0f};
    V3 shade = miss;
    if (hit) {
        n = normal(p);
        float lit = direct_term(n);
        if (__builtin_expect(P.soft_shadow != 0u, 0)) lit = lit * soft_shadow(P, p, n, lit > 0.0f, sdf);
        shade = lit_colour(P, lit);
    }
    const float f = ambient_occlusion(P, ao, p, n, __builtin_amdgcn_ballot_w64(hit), sdf);
    if (!hit) return Occluded{miss, 1.0f};
    return Occluded{V3{f * shade.x, f * shade.y, f * shade.z}, f};
}

// raymarch<GROUP, PRIM> for the occlusion launch (kifs_occlusion_kernels.hip): the same whole ray per lane through the
// view P, a hit's colour attenuated by its factor.  The factor is the hit's in heatmap mode too (the colour is the
// counter's there).  The shading reads the scene's constants and the term from the kernel argument K: nothing of a view
// is among them.  The Julia pipeline probes through the plain scene_sdf<GROUP_JULIA, 0>, as its shadow rays do.
// (always_inline: the bunny's estimate is large enough for the inliner to leave its ninth copy a call, which costs the
// kernel a stack.)
template <int GROUP, int PRIM>
KIFS_DEV Occluded raymarch_occluded(const FrameParams& P, occl::ConstParams K, V3 dir, bool valid) {
    constexpr int NPRIM = GROUP == GROUP_JULIA ? 0 : PRIM;
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    if constexpr (GROUP == GROUP_JULIA) {
        JuliaDiag diag;
        julia_loop<(PRIM & 1) != 0, false>(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, diag);
    } else {
        generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations,
                     [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return scene_sdf<GROUP, PRIM>(P, q, lanes); });
    }
    __builtin_amdgcn_s_setprio(0);
    const occl::ConstParams L = occl::anew(K);
    const FrameParams S = *(const FrameParams*)&L->B.frame;  // the scene, as every view of the launch shares it
    Occluded r{S.background_color, 1.0f};
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {  // wave-uniform
        const occl::AO ao{L->ao.samples, L->ao.step, L->ao.decay, L->ao.strength};
        const auto sdf = [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return scene_sdf<GROUP, NPRIM>(S, q, lanes); };
        r = occluded_shade(S, ao, p, hit, S.background_color, sdf, [&](V3 q) __attribute__((always_inline)) {
            if constexpr (GROUP == GROUP_KIFS)  // kifs_normal<PRIM>, its estimate inlined
                return normal_fd(S.epsilon, q, [&](V3 e) __attribute__((always_inline)) { return kifs_sdf<PRIM>(S, e); });
            else
                return scene_normal<GROUP, NPRIM>(S, q);
        });
    }
    if (S.is_heatmap) r.colour = heatmap_colour(S, i_final);
    return r;
}

// ---- extension: a configurable light (kifs_render_lit_async, include/kifs_hip.h) ----------------------------------
// The lighting model above with the light's constants as arguments, operation for operation as the header states it.
// With the reference's light -- (1,1,1), 0.1, 0.9, no highlight -- every piece computes the bits of the one it stands
// beside: dot's fma chain with ones is (n.x + n.y) + n.z.
// The direct term towards the light vector l, used as given (direct_term).
KIFS_DEV float direct_term_towards(V3 n, V3 l) { return clamp_(dot(n, l), 0.0f, 1.0f); }
// The colour of a hit whose (attenuated) direct term is `lit` (lit_colour).
KIFS_DEV V3 lit_colour_with(const FrameParams& P, float ambient, float diffuse, float lit) {
    const float k = fmaf_(diffuse, lit, ambient);
    return V3{k * P.fractal_color.x, k * P.fractal_color.y, k * P.fractal_color.z};
}
// shadow_point for a ray towards the unit vector L, and soft_shadow with it: start, step and count are theirs.
KIFS_DEV V3 shadow_point_towards(const ShadowRay& s, V3 L) {
    return V3{fmaf_(s.t, L.x, s.start.x), fmaf_(s.t, L.y, s.start.y), fmaf_(s.t, L.z, s.start.z)};
}
// (`towards()`: the unit vector, asked for step by step, so that a caller short of scalar registers can read it anew.)
template <class Sdf, class Unit>
KIFS_DEV float soft_shadow_towards(const FrameParams& P, V3 p, V3 n, Unit towards, bool lanes_hit, Sdf sdf) {
    ShadowRay s = shadow_ray_from(P, shadow_start(P, p, n));
    bool marching = lanes_hit && (0 < P.shadow_steps);
    for (; __builtin_amdgcn_ballot_w64(marching) != 0ull; ++s.j) {
        if (marching) marching = !shadow_step(P, sdf(shadow_point_towards(s, towards()), ~0ull), s);
    }
    return s.res;
}
// The Blinn-Phong highlight before its attenuation: the normal against the half vector of the unit light vector L and
// the way back along the ray, raised to 2^e by e squarings (e: uniform).
KIFS_DEV float highlight(V3 n, V3 L, V3 dir, int e) {
    const V3 h = normalize(V3{L.x - dir.x, L.y - dir.y, L.z - dir.z});
    float s = clamp_(dot(n, h), 0.0f, 1.0f);
    for (int i = 0; i < e; ++i) s = s * s;
    return s;
}

// The lit kernel's phases read the kernel argument anew as the occlusion kernel's do (occl::anew).
namespace light {
typedef const Params __attribute__((address_space(4))) * ConstParams;
KIFS_DEV ConstParams anew(ConstParams K) {
    asm volatile("" : "+s"(K));
    return K;
}
}  // namespace light

// occluded_shade with the launch's light, and the factor only when the launch has a term.  A lane that did not hit gets
// `miss`.  The light and the term are read from the kernel argument K where each is used -- the direction for the direct
// term and the highlight, the unit vector again for the shadow ray, the weights after it, the term last -- so that only
// the shadow ray's unit vector crosses a march (the bunny's estimate leaves few scalar registers to park anything in).
// `dir()`: the ray direction of the lane's sample, asked for where the highlight needs it -- after the march and the
// normal, so that the caller can recompute it instead of carrying it.  The highlight is taken before the shadow ray sets
// out: one register crosses the secondary march, not the half vector's three.
KIFS_DEV V3 load3(const V3 __attribute__((address_space(4))) * v) { return V3{v->x, v->y, v->z}; }
template <class Sdf, class Normal, class Dir>
KIFS_DEV V3 lit_shade(const FrameParams& P, light::ConstParams K, V3 p, bool hit, V3 miss, Sdf sdf, Normal normal, Dir dir) {
    V3 n{0.0f, 0.0f, 0.0f};
    V3 shade = miss;
    if (hit) {
        n = normal(p);
        const light::ConstParams A = light::anew(K);
        const bool highlit = A->light.highlight != 0u;  // uniform
        const float lit0 = direct_term_towards(n, load3(&A->light.direction));
        float s = 0.0f;
        if (highlit) s = highlight(n, load3(&A->light.unit), dir(), A->light.shininess_log2);
        float sh = 1.0f, lit = lit0;
        if (__builtin_expect(P.soft_shadow != 0u, 0)) {
            sh = soft_shadow_towards(
                P, p, n, [&]() __attribute__((always_inline)) { return load3(&light::anew(K)->light.unit); }, lit0 > 0.0f, sdf);
            lit = lit0 * sh;
        }
        const light::ConstParams B = light::anew(K);
        shade = lit_colour_with(P, B->light.ambient, B->light.diffuse, lit);
        if (highlit) {
            const float spec = (lit0 > 0.0f) ? s * sh : 0.0f;
            const V3 w = load3(&B->light.specular);
            shade = V3{fmaf_(w.x, spec, shade.x), fmaf_(w.y, spec, shade.y), fmaf_(w.z, spec, shade.z)};
        }
    }
    const light::ConstParams C = light::anew(K);
    if (C->has_ao != 0u) {  // uniform; the probes run for the whole wave, as occluded_shade's
        const occl::AO ao{C->ao.samples, C->ao.step, C->ao.decay, C->ao.strength};
        const float f = ambient_occlusion(P, ao, p, n, __builtin_amdgcn_ballot_w64(hit), sdf);
        shade = V3{f * shade.x, f * shade.y, f * shade.z};
    }
    return hit ? shade : miss;
}

// raymarch_occluded for the lit launch (kifs_lighting_kernels.hip): the same whole ray per lane through the view P, a
// hit's colour from the launch's light and, when the launch has a term, attenuated by the hit's factor.  The shading
// reads the scene's constants, the light and the term from the kernel argument K.
template <int GROUP, int PRIM, class Dir>
KIFS_DEV V3 raymarch_lit(const FrameParams& P, light::ConstParams K, V3 dir, bool valid, Dir redo_dir) {
    constexpr int NPRIM = GROUP == GROUP_JULIA ? 0 : PRIM;
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    if constexpr (GROUP == GROUP_JULIA) {
        JuliaDiag diag;
        julia_loop<(PRIM & 1) != 0, false>(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, diag);
    } else {
        generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations,
                     [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return scene_sdf<GROUP, PRIM>(P, q, lanes); });
    }
    __builtin_amdgcn_s_setprio(0);
    const light::ConstParams L = light::anew(K);
    const FrameParams S = *(const FrameParams*)&L->B.frame;  // the scene, as every view of the launch shares it
    V3 colour = S.background_color;
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {  // wave-uniform
        const auto sdf = [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return scene_sdf<GROUP, NPRIM>(S, q, lanes); };
        colour = lit_shade(
            S, K, p, hit, S.background_color, sdf,
            [&](V3 q) __attribute__((always_inline)) {
                if constexpr (GROUP == GROUP_KIFS)  // kifs_normal<PRIM>, its estimate inlined
                    return normal_fd(S.epsilon, q, [&](V3 e) __attribute__((always_inline)) { return kifs_sdf<PRIM>(S, e); });
                else
                    return scene_normal<GROUP, NPRIM>(S, q);
            },
            redo_dir);
    }
    if (S.is_heatmap) colour = heatmap_colour(S, i_final);
    return colour;
}

// ---- extension: orbit-trap surface colouring (kifs_render_trapped_async, include/kifs_hip.h) -----------------------
// The colour of a hit from where its orbit goes, operation for operation as the header states it: the squared distance
// of an orbit point to the trap over the components the trap names, its minimum over z_0 .. z_K, and a gradient of three
// stops over the clamped, scaled square root of that minimum.
namespace trap {
typedef const Params __attribute__((address_space(4))) * ConstParams;
KIFS_DEV ConstParams anew(ConstParams K) {
    asm volatile("" : "+s"(K));
    return K;
}
typedef const Trap __attribute__((address_space(4))) * ConstTrap;
KIFS_DEV Trap load(ConstTrap t) {
    return Trap{V4{t->centre.x, t->centre.y, t->centre.z, t->centre.w}, t->axes, t->iterations, t->scale, t->bias,
                V3{t->mid.x, t->mid.y, t->mid.z}, V3{t->far.x, t->far.y, t->far.z}};
}
}  // namespace trap

// d(z): e = z - centre, d = 0, then d = fma(e_i, e_i, d) for the components of `axes` (uniform) in the order x, y, z, w.
KIFS_DEV float trap_distance(const trap::Trap& T, V4 z) {
    float d = 0.0f;
    if (T.axes & 1u) {
        const float e = z.x - T.centre.x;
        d = fmaf_(e, e, d);
    }
    if (T.axes & 2u) {
        const float e = z.y - T.centre.y;
        d = fmaf_(e, e, d);
    }
    if (T.axes & 4u) {
        const float e = z.z - T.centre.z;
        d = fmaf_(e, e, d);
    }
    if (T.axes & 8u) {
        const float e = z.w - T.centre.w;
        d = fmaf_(e, e, d);
    }
    return d;
}

// u of the position p: the square root of the least d over the orbit z_0 .. z_K of pipeline <GROUP, PRIM> (Julia: the
// PRIM slot is not a primitive and is not read).  `lanes`: the lanes whose u is used; the trip count is wave-uniform --
// the loop leaves when none of them still runs -- and a lane that has stopped takes no further minimum.  The generalised
// Julia step is genjulia_normal's quat_pow, with its wave-level repeat on the general functions asked for by running
// lanes only.
template <int GROUP, int PRIM>
KIFS_DEV float orbit_trap(const FrameParams& S, const trap::Trap& T, V3 p, bool lanes = true) {
    constexpr bool JULIA = GROUP == GROUP_JULIA || GROUP == GROUP_GENJULIA;
    V4 z{p.x, p.y, p.z, JULIA ? 0.1f : 0.0f};
    float m = trap_distance(T, z);
    if constexpr (JULIA) {
        bool run = lanes;
        for (int k = 0; k < T.iterations && __builtin_amdgcn_ballot_w64(run) != 0ull; ++k) {
            if constexpr (GROUP == GROUP_JULIA) {
                z = quat_sq_add(z, S.c);
            } else {
                const float d = quat_ijk2(z);
                const float qs = fmaf_(z.x, z.x, d);
                float unused;
                const V4 t = quat_pow_shared(z, d, qs, S.power, unused, run);
                z = V4{t.x + S.c.x, t.y + S.c.y, t.z + S.c.z, t.w + S.c.w};
            }
            const float d = trap_distance(T, z);
            m = (run && (d < m)) ? d : m;
            run = run && !(quat_norm2(z) > S.max_distance);
        }
    } else if constexpr (PRIM == PRIM_SIERPINSKI) {
        V3 q = p;
        for (int k = 0; k < T.iterations; ++k) {  // uniform
            q = tetrahedral_fold(q);
            q = V3{fmaf_(2.0f, q.x, -1.0f), fmaf_(2.0f, q.y, -1.0f), fmaf_(2.0f, q.z, -1.0f)};
            const float d = trap_distance(T, V4{q.x, q.y, q.z, 0.0f});
            m = (d < m) ? d : m;
        }
    }
    return sqrt_(m);
}

// The gradient at u: t = clamp(fma(scale, u, bias)) as two ternaries (a NaN gives 0), the stops fractal_color, mid and
// far at t = 0, 1/2 and 1.
KIFS_DEV V3 trap_colour(const FrameParams& S, const trap::Trap& T, float u) {
    const float v = fmaf_(T.scale, u, T.bias);
    float t = (v > 0.0f) ? v : 0.0f;
    t = (t < 1.0f) ? t : 1.0f;
    const float x = t * 2.0f;
    const bool upper = x >= 1.0f;
    const float f = x - (upper ? 1.0f : 0.0f);
    const V3 a{upper ? T.mid.x : S.fractal_color.x, upper ? T.mid.y : S.fractal_color.y, upper ? T.mid.z : S.fractal_color.z};
    const V3 b{upper ? T.far.x : T.mid.x, upper ? T.far.y : T.mid.y, upper ? T.far.z : T.mid.z};
    return V3{fmaf_(f, b.x - a.x, a.x), fmaf_(f, b.y - a.y, a.y), fmaf_(f, b.z - a.z, a.z)};
}

// lit_shade with the hit's own colour in the place of fractal_color: `colour(p)` is asked for after the shadow ray, where
// the weights are, so that no colour crosses the secondary march.  Everything else -- the direct term, the highlight, the
// shadow ray, the weights, the optional factor, and where each reads the kernel argument K anew -- is lit_shade's, in its
// order (trap::Params carries light::Params' fields at their offsets).
template <class Sdf, class Normal, class Dir, class Colour>
KIFS_DEV V3 trapped_shade(const FrameParams& P, trap::ConstParams K, V3 p, bool hit, V3 miss, Sdf sdf, Normal normal, Dir dir,
                          Colour colour) {
    V3 n{0.0f, 0.0f, 0.0f};
    V3 shade = miss;
    if (hit) {
        n = normal(p);
        const trap::ConstParams A = trap::anew(K);
        const bool highlit = A->light.highlight != 0u;  // uniform
        const float lit0 = direct_term_towards(n, load3(&A->light.direction));
        float s = 0.0f;
        if (highlit) s = highlight(n, load3(&A->light.unit), dir(), A->light.shininess_log2);
        float sh = 1.0f, lit = lit0;
        if (__builtin_expect(P.soft_shadow != 0u, 0)) {
            sh = soft_shadow_towards(
                P, p, n, [&]() __attribute__((always_inline)) { return load3(&trap::anew(K)->light.unit); }, lit0 > 0.0f, sdf);
            lit = lit0 * sh;
        }
        const V3 col = colour(p);
        const trap::ConstParams B = trap::anew(K);
        const float k = fmaf_(B->light.diffuse, lit, B->light.ambient);
        shade = V3{k * col.x, k * col.y, k * col.z};
        if (highlit) {
            const float spec = (lit0 > 0.0f) ? s * sh : 0.0f;
            const V3 w = load3(&B->light.specular);
            shade = V3{fmaf_(w.x, spec, shade.x), fmaf_(w.y, spec, shade.y), fmaf_(w.z, spec, shade.z)};
        }
    }
    const trap::ConstParams C = trap::anew(K);
    if (C->has_ao != 0u) {  // uniform; the probes run for the whole wave, as occluded_shade's
        const occl::AO ao{C->ao.samples, C->ao.step, C->ao.decay, C->ao.strength};
        const float f = ambient_occlusion(P, ao, p, n, __builtin_amdgcn_ballot_w64(hit), sdf);
        shade = V3{f * shade.x, f * shade.y, f * shade.z};
    }
    return hit ? shade : miss;
}

// raymarch_lit for the trapped launch (kifs_trap_kernels.hip): the same whole ray per lane through the view P, a hit's
// colour the gradient at its orbit's trap distance, shaded by the launch's light and, when the launch has a term,
// attenuated by the hit's factor.  The trap is read from the kernel argument K after the march and the shadow ray, where
// it is used.  A heatmap frame evaluates no trap: its colour is the counter's.
template <int GROUP, int PRIM, class Dir>
KIFS_DEV V3 raymarch_trapped(const FrameParams& P, trap::ConstParams K, V3 dir, bool valid, Dir redo_dir) {
    constexpr int NPRIM = GROUP == GROUP_JULIA ? 0 : PRIM;
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    if constexpr (GROUP == GROUP_JULIA) {
        JuliaDiag diag;
        julia_loop<(PRIM & 1) != 0, false>(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, diag);
    } else {
        generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations,
                     [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return scene_sdf<GROUP, PRIM>(P, q, lanes); });
    }
    __builtin_amdgcn_s_setprio(0);
    const trap::ConstParams L = trap::anew(K);
    const FrameParams S = *(const FrameParams*)&L->B.frame;  // the scene, as every view of the launch shares it
    V3 colour = S.background_color;
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {  // wave-uniform
        const auto sdf = [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return scene_sdf<GROUP, NPRIM>(S, q, lanes); };
        colour = trapped_shade(
            S, K, p, hit, S.background_color, sdf,
            [&](V3 q) __attribute__((always_inline)) {
                if constexpr (GROUP == GROUP_KIFS)  // kifs_normal<PRIM>, its estimate inlined
                    return normal_fd(S.epsilon, q, [&](V3 e) __attribute__((always_inline)) { return kifs_sdf<PRIM>(S, e); });
                else
                    return scene_normal<GROUP, NPRIM>(S, q);
            },
            redo_dir,
            [&](V3 q) __attribute__((always_inline)) {
                if (S.is_heatmap) return S.fractal_color;  // uniform
                const trap::Trap T = trap::load(&trap::anew(K)->trap);
                return trap_colour(S, T, orbit_trap<GROUP, NPRIM>(S, T, q));
            });
    }
    if (S.is_heatmap) colour = heatmap_colour(S, i_final);
    return colour;
}

// ---- extension: kaleidoscopic IFS scenes (kifs_render_folded_async, include/kifs_hip.h) ----------------------------
// The estimate of a base primitive seen through N rounds of fold, rotate and scale, operation for operation as the header
// states it.  The fold system is read from the kernel argument where the estimate runs (fold::anew), at the head of every
// estimate: its eighteen words held from the kernel's start would cross the bunny's estimate, which leaves few scalar
// registers.
namespace fold {
typedef const Params __attribute__((address_space(4))) * ConstParams;
typedef const Fold __attribute__((address_space(4))) * ConstFold;
KIFS_DEV ConstFold anew(ConstFold F) {
    asm volatile("" : "+s"(F));
    return F;
}
KIFS_DEV ConstParams anew(ConstParams K) {
    asm volatile("" : "+s"(K));
    return K;
}
}  // namespace fold

// base(p') / acc of the position p.  `lanes`: the lanes whose estimate is used (the others get an unspecified value).
// The stage mask, N and the exit -- once no lane of `lanes` still folds -- are wave-uniform: the stages are scalar
// branches.  A lane whose |p| has reached max_distance (on the squared norm: FrameParams::fold_n2_stop; a NaN compares
// false) stops for good and keeps its p and acc.  SORT is the contract's ternaries: the hardware maximum and minimum
// would move a NaN and may order a pair of zeros of either sign differently.  With N = 0 the loop is never entered and
// base(p) / 1.0f is base(p).
template <int PRIM>
KIFS_DEV float folded_sdf(const FrameParams& S, fold::ConstFold F0, V3 p, unsigned long long lanes) {
    const fold::ConstFold F = fold::anew(F0);
    const int n = F->iterations;  // uniform
    float acc = 1.0f;
    if (n > 0) {
        const uint32_t stages = F->stages;
        // The loop's constants, read once here and held in scalar registers for the length of the loop alone (the empty
        // asm keeps the compiler from sinking the loads back into it: a scalar load and its wait per round otherwise);
        // they are dead again when the base estimate starts.
        float s = F->scale, t0 = F->t[0], t1 = F->t[1], t2 = F->t[2], h = F->h;
        asm volatile("" : "+s"(s), "+s"(t0), "+s"(t1), "+s"(t2), "+s"(h));
        float R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (stages & fold::ROTATE) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = F->R[i];
        }
        asm volatile("" : "+s"(R[0]), "+s"(R[1]), "+s"(R[2]), "+s"(R[3]), "+s"(R[4]), "+s"(R[5]), "+s"(R[6]), "+s"(R[7]), "+s"(R[8]));
        bool run = true;
        for (int j = 0; j < n; ++j) {
            run = run && (dot(p, p) < S.fold_n2_stop);
            if ((__builtin_amdgcn_ballot_w64(run) & lanes) == 0ull) break;
            V3 q = p;
            if (stages & fold::ABS) q = V3{abs_(q.x), abs_(q.y), abs_(q.z)};
            if (stages & fold::SORT) {
                const bool a = q.x < q.y;
                const float x1 = a ? q.y : q.x, y1 = a ? q.x : q.y;
                const bool b = x1 < q.z;
                const float x2 = b ? q.z : x1, z2 = b ? x1 : q.z;
                const bool c = y1 < z2;
                q = V3{x2, c ? z2 : y1, c ? y1 : z2};
            }
            if (stages & fold::TETRA) q = tetrahedral_fold(q);
            if (stages & fold::ROTATE) {
                q = V3{fmaf_(R[2], q.z, fmaf_(R[1], q.y, R[0] * q.x)), fmaf_(R[5], q.z, fmaf_(R[4], q.y, R[3] * q.x)),
                       fmaf_(R[8], q.z, fmaf_(R[7], q.y, R[6] * q.x))};
            }
            q = V3{fmaf_(s, q.x, t0), fmaf_(s, q.y, t1), fmaf_(s, q.z, t2)};
            if (stages & fold::MIRROR_Z) q.z = abs_(q.z - h) + h;
            p = V3{run ? q.x : p.x, run ? q.y : p.y, run ? q.z : p.z};
            acc = run ? acc * s : acc;
        }
    }
    return kifs_sdf<PRIM>(S, p, lanes) / acc;
}

// raymarch_lit for the folded launch (kifs_fold_kernels.hip): the same whole ray per lane through the view P, with the
// folded estimate wherever the lit call takes the scene's -- the march, the normal, the shadow ray and the probes.  The
// shading is lit_shade itself: fold::Params carries light::Params' fields at their offsets.  The launch runs with every
// cull off (kifs_fold.cpp): a folded scene reaches beyond the base primitive's bounding sphere.
template <int PRIM, class Dir>
KIFS_DEV V3 raymarch_folded(const FrameParams& P, fold::ConstParams K, V3 dir, bool valid, Dir redo_dir) {
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations,
                 [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return folded_sdf<PRIM>(P, &K->fold, q, lanes); });
    __builtin_amdgcn_s_setprio(0);
    const light::ConstParams KL = (light::ConstParams)K;
    const light::ConstParams L = light::anew(KL);
    const FrameParams S = *(const FrameParams*)&L->B.frame;  // the scene, as every view of the launch shares it
    V3 colour = S.background_color;
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {  // wave-uniform
        const auto sdf = [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) { return folded_sdf<PRIM>(S, &K->fold, q, lanes); };
        colour = lit_shade(
            S, KL, p, hit, S.background_color, sdf,
            [&](V3 q) __attribute__((always_inline)) {
                return normal_fd(S.epsilon, q, [&](V3 e) __attribute__((always_inline)) { return folded_sdf<PRIM>(S, &K->fold, e, ~0ull); });
            },
            redo_dir);
    }
    if (S.is_heatmap) colour = heatmap_colour(S, i_final);
    return colour;
}

// ---- extension: orbit-trap colouring of folded scenes (kifs_render_folded_trapped_async, include/kifs_hip.h) --------
// The two extensions above composed: the folded estimate wherever the folded call puts it, and a hit's colour from the
// orbit that the estimate iterates -- the point after each round -- continued by the base primitive's own.  The fold
// system and the trap are read from a record in device memory, through a pointer cast to the constant address space
// (foldorbit::Record, kifs_params.hpp): scalar loads of a uniform address, like the kernel argument's own.
namespace foldorbit {
typedef const Params __attribute__((address_space(4))) * ConstParams;
typedef const Record __attribute__((address_space(4))) * ConstRecord;
KIFS_DEV ConstParams anew(ConstParams K) {
    asm volatile("" : "+s"(K));
    return K;
}
KIFS_DEV ConstRecord anew(ConstRecord R) {
    asm volatile("" : "+s"(R));
    return R;
}
// The launch's record: the pointer is read from the kernel argument where it is asked for.
KIFS_DEV ConstRecord record_of(ConstParams K) { return (ConstRecord)anew(K)->record; }
}  // namespace foldorbit

// u of the position p on a folded scene: folded_sdf's loop restated with the running minimum.  Orbit point j + 1 is the
// point after round j (w = 0) and takes part while j + 1 <= K, K the trap's iterations; with the Sierpinski estimate as
// the base the orbit goes on from the folded p with orbit_trap's Sierpinski rule for max(K - N, 0) points.  So
// min(N, K) rounds are all the orbit needs: beyond them no fold point takes part, and the base part runs only with
// K > N, when every round has run.  The fold constants and the trap's centre and axes sit in scalar registers for the
// length of the loop only; the trip count and the exit -- once no lane still folds -- are wave-uniform (called from a
// divergent region, the ballot is of the region's lanes); a lane that has stopped takes no further fold point and keeps
// its p.  The trap's gradient fields are not read.
template <int PRIM>
KIFS_DEV float folded_orbit_trap(const FrameParams& S, fold::ConstFold F0, trap::ConstTrap T0, V3 p) {
    const fold::ConstFold F = fold::anew(F0);
    const trap::ConstTrap Tc = T0;
    const int n = F->iterations;       // uniform
    const int K = Tc->iterations;      // uniform
    trap::Trap T{};
    T.axes = Tc->axes;
    float cx = Tc->centre.x, cy = Tc->centre.y, cz = Tc->centre.z, cw = Tc->centre.w;
    asm volatile("" : "+s"(cx), "+s"(cy), "+s"(cz), "+s"(cw));
    T.centre = V4{cx, cy, cz, cw};
    float m = trap_distance(T, V4{p.x, p.y, p.z, 0.0f});
    const int rounds = n < K ? n : K;
    if (rounds > 0) {
        const uint32_t stages = F->stages;
        float s = F->scale, t0 = F->t[0], t1 = F->t[1], t2 = F->t[2], h = F->h;
        asm volatile("" : "+s"(s), "+s"(t0), "+s"(t1), "+s"(t2), "+s"(h));
        float R[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (stages & fold::ROTATE) {
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = F->R[i];
        }
        asm volatile("" : "+s"(R[0]), "+s"(R[1]), "+s"(R[2]), "+s"(R[3]), "+s"(R[4]), "+s"(R[5]), "+s"(R[6]), "+s"(R[7]), "+s"(R[8]));
        bool run = true;
        for (int j = 0; j < rounds; ++j) {
            run = run && (dot(p, p) < S.fold_n2_stop);
            if (__builtin_amdgcn_ballot_w64(run) == 0ull) break;
            V3 q = p;
            if (stages & fold::ABS) q = V3{abs_(q.x), abs_(q.y), abs_(q.z)};
            if (stages & fold::SORT) {
                const bool a = q.x < q.y;
                const float x1 = a ? q.y : q.x, y1 = a ? q.x : q.y;
                const bool b = x1 < q.z;
                const float x2 = b ? q.z : x1, z2 = b ? x1 : q.z;
                const bool c = y1 < z2;
                q = V3{x2, c ? z2 : y1, c ? y1 : z2};
            }
            if (stages & fold::TETRA) q = tetrahedral_fold(q);
            if (stages & fold::ROTATE) {
                q = V3{fmaf_(R[2], q.z, fmaf_(R[1], q.y, R[0] * q.x)), fmaf_(R[5], q.z, fmaf_(R[4], q.y, R[3] * q.x)),
                       fmaf_(R[8], q.z, fmaf_(R[7], q.y, R[6] * q.x))};
            }
            q = V3{fmaf_(s, q.x, t0), fmaf_(s, q.y, t1), fmaf_(s, q.z, t2)};
            if (stages & fold::MIRROR_Z) q.z = abs_(q.z - h) + h;
            p = V3{run ? q.x : p.x, run ? q.y : p.y, run ? q.z : p.z};
            const float d = trap_distance(T, V4{q.x, q.y, q.z, 0.0f});
            m = (run && (d < m)) ? d : m;
        }
    }
    if constexpr (PRIM == PRIM_SIERPINSKI) {
        V3 q = p;
        for (int k = n; k < K; ++k) {  // uniform: max(K - N, 0) points, from N and not from the rounds that ran
            q = tetrahedral_fold(q);
            q = V3{fmaf_(2.0f, q.x, -1.0f), fmaf_(2.0f, q.y, -1.0f), fmaf_(2.0f, q.z, -1.0f)};
            const float d = trap_distance(T, V4{q.x, q.y, q.z, 0.0f});
            m = (d < m) ? d : m;
        }
    }
    return sqrt_(m);
}

// raymarch_folded for the folded trapped launch (kifs_fold_trap_kernels.hip): the same whole ray per lane through the
// view P with the folded estimate in the march, the normal, the shadow ray and the probes, and trapped_shade's colour of
// a hit from folded_orbit_trap (foldorbit::Params carries light::Params' fields at their offsets, which is all that
// trapped_shade reads of its argument).  `u`: the hit's trap distance, written when the launch has a plane -- then for
// every hit, heatmap frames included -- or when the colour needs it; a lane that did not hit leaves it alone.
template <int PRIM, class Dir>
KIFS_DEV V3 raymarch_folded_trapped(const FrameParams& P, foldorbit::ConstParams K, V3 dir, bool valid, float& u, Dir redo_dir) {
    float t = 0.0f;
    V3 p = P.origin;
    bool hit = false;
    int trips = 0;
    int i_final = 0;
    bool marching = whole_ray_sets_out(P, dir, valid);
    generic_loop(P, dir, t, p, hit, marching, trips, i_final, P.max_iterations, [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) {
        return folded_sdf<PRIM>(P, &foldorbit::record_of(K)->fold, q, lanes);
    });
    __builtin_amdgcn_s_setprio(0);
    const trap::ConstParams KT = (trap::ConstParams)K;
    const foldorbit::ConstParams L = foldorbit::anew(K);
    const FrameParams S = *(const FrameParams*)&L->B.frame;  // the scene, as every view of the launch shares it
    V3 colour = S.background_color;
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {  // wave-uniform
        const auto sdf = [&](V3 q, unsigned long long lanes) __attribute__((always_inline)) {
            return folded_sdf<PRIM>(S, &foldorbit::record_of(K)->fold, q, lanes);
        };
        colour = trapped_shade(
            S, KT, p, hit, S.background_color, sdf,
            [&](V3 q) __attribute__((always_inline)) {
                return normal_fd(S.epsilon, q, [&](V3 e) __attribute__((always_inline)) {
                    return folded_sdf<PRIM>(S, &foldorbit::record_of(K)->fold, e, ~0ull);
                });
            },
            redo_dir,
            [&](V3 q) __attribute__((always_inline)) {
                // (the scene's constants anew: what the gradient and the counter's colour read of them need not cross
                // the normal's and the shadow ray's estimates, which leave the bunny few scalar registers)
                const foldorbit::ConstParams A = foldorbit::anew(K);
                const bool heatmap = A->B.frame.is_heatmap != 0u, planed = A->plane != nullptr;  // uniform
                V3 col{A->B.frame.fractal_color.x, A->B.frame.fractal_color.y, A->B.frame.fractal_color.z};
                if (heatmap && !planed) return col;  // the colour is the counter's
                const foldorbit::ConstRecord R = foldorbit::record_of(K);
                u = folded_orbit_trap<PRIM>(S, &R->fold, &R->trap, q);
                if (!heatmap) {
                    const foldorbit::ConstParams B = foldorbit::anew(K);
                    const FrameParams G = *(const FrameParams*)&B->B.frame;
                    const trap::Trap T = trap::load(&foldorbit::anew(R)->trap);
                    col = trap_colour(G, T, u);
                }
                return col;
            });
    }
    const foldorbit::ConstParams E = foldorbit::anew(K);
    const FrameParams H = *(const FrameParams*)&E->B.frame;
    if (H.is_heatmap) colour = heatmap_colour(H, i_final);
    return colour;
}

}  // namespace kifs
