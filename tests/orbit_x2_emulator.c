/* The Julia orbit trip of the throughput kernel in its two forms, emulated on the CPU operation for operation
 * (kifs_scene.hpp: KIFS_JULIA_PROLOGUE_SCALAR + KIFS_FAST_TRIP_SCALAR, and KIFS_JULIA_PROLOGUE_X2 +
 * KIFS_FAST_TRIP_X2_), compared bit for bit: |q|^2 and dqs after the loop, the trip a lane escapes on and the class
 * test that decides whether the step is handed back.  Where the two differ, the host's orbit_x2_eligible()
 * (kifs_schedule.cpp) must have kept the scene on the plain trip.  Built by tests/test_orbit_x2_emulator.py with -ffp-contract=off.
 *
 *     orbit_x2_emulator N SEED   ->  "orbits N differ D differ_eligible U ineligible G"
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ok: the value the kernel's class test reads (|q|^2, or 4|q|^2 in the doubled form) is a positive normal number --
 * otherwise the step goes back to the general loop and nothing else of the trip is used */
typedef struct { float qq, dqs; int escaped_at, ok; } Out;

static int positive_normal(float f) { return isnormal(f) && f > 0.0f; }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* KIFS_JULIA_PROLOGUE_SCALAR + iters x KIFS_FAST_TRIP_SCALAR, then dqs = dq * (4|q_last|^2) */
static Out plain(const float p[3], const float c[4], float maxd, int iters) {
    float v46 = 2.0f * p[0], v47 = 1.0f, y = p[1], z = p[2], w = 0.1f, dq = 1.0f;
    float s = y * y + z * z;  /* v_mul, v_mul, v_add */
    float d = fmaf(w, w, s);
    float n = fmaf(p[0], p[0], d);
    float xn = fmaf(p[0], p[0], -d);
    xn = c[0] + xn;
    Out o = {0, 0, -1, 0};
    for (int k = 1; k <= iters; ++k) {
        y = fmaf(v46, y, c[1]);
        z = fmaf(v46, z, c[2]);
        w = fmaf(v46, w, c[3]);
        dq = fmaf(v47, dq, 0.0f);
        v46 = 2.0f * xn;
        v47 = 4.0f * n;
        float a = y * y, b = z * z;
        s = a + b;
        d = fmaf(w, w, s);
        n = fmaf(xn, xn, d);
        float r = fmaf(xn, xn, -d);
        xn = c[0] + r;
        if (maxd < n) { o.escaped_at = k; break; } /* v_cmpx_nlt: the lane stays while !(maxd < |q|^2) */
    }
    o.qq = n;
    o.dqs = dq * v47;
    o.ok = positive_normal(n);
    return o;
}

/* KIFS_JULIA_PROLOGUE_X2 + iters x KIFS_FAST_TRIP_X2_ (A / B alternate: the same arithmetic), |q|^2 = 0.25 N4 */
static Out doubled(const float p[3], const float c2[4], float maxd4, int iters) {
    float xk = p[0] + p[0], Y = p[1] + p[1], Z = p[2] + p[2], W = 2.0f * 0.1f, DQ = 1.0f;
    float s = Y * Y + Z * Z;
    float D = fmaf(W, W, s);
    float N4 = fmaf(xk, xk, D);
    float R = fmaf(xk, xk, -D);
    float xk1 = fmaf(R, 0.5f, c2[0]);
    Out o = {0, 0, -1, 0};
    for (int k = 1; k <= iters; ++k) {
        Y = fmaf(xk, Y, c2[1]);
        Z = fmaf(xk, Z, c2[2]);
        W = fmaf(xk, W, c2[3]);
        DQ = fmaf(N4, DQ, 0.0f);
        float a = Y * Y, b = Z * Z;
        s = a + b;
        D = fmaf(W, W, s);
        N4 = fmaf(xk1, xk1, D);
        R = fmaf(xk1, xk1, -D);
        float x2 = fmaf(R, 0.5f, c2[0]);
        xk = xk1;
        xk1 = x2;
        if (maxd4 < N4) { o.escaped_at = k; break; }
    }
    o.ok = positive_normal(N4);
    o.qq = 0.25f * N4;
    o.dqs = DQ;
    return o;
}

/* orbit_x2_eligible() of kifs_schedule.cpp (bound_n2 = 4.04, eligible for every scene drawn here) */
static int eligible(const float c[4], float maxd) {
    for (int i = 0; i < 4; ++i)
        if (!(fabsf(c[i]) >= 0x1p-14f && fabsf(c[i]) <= 0x1p10f)) return 0;
    return maxd > 0.0f && maxd <= 0x1p60f;
}

/* xorshift64* */
static uint64_t rng_state;
static uint64_t rnd(void) {
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}
static float unif(void) { return (float)(rnd() >> 40) * 0x1p-24f; }           /* [0, 1) */
static float sym(float a) { return (2.0f * unif() - 1.0f) * a; }
static float sign(void) { return (rnd() & 1) ? -1.0f : 1.0f; }
static float tiny(int lo, int hi) { return sign() * ldexpf(1.0f + unif(), lo + (int)(rnd() % (uint64_t)(hi - lo + 1))); }

/* one random orbit; `kind` picks the family */
static void draw(int kind, float p[3], float c[4], float* maxd, int* iters) {
    const float cfg2[4] = {-0.2f, 0.6f, 0.2f, 0.2f};
    for (int i = 0; i < 3; ++i) p[i] = sym(2.0f);
    for (int i = 0; i < 4; ++i) c[i] = (kind % 3 == 0) ? cfg2[i] : sym(1.0f);
    *maxd = (rnd() & 3) ? 1000.0f : 4.0f + unif() * 1e4f;
    *iters = (rnd() & 1) ? 12 : 1 + (int)(rnd() % 100);
    switch (kind % 8) {
    case 3:  /* start point near the fractal of cfg2: small perturbations of a few seeds */
        p[0] = sym(0.6f); p[1] = sym(0.6f); p[2] = sym(0.6f); break;
    case 4:  /* tiny or zero start components: squares in the denormal range, absorbed by w_0^2 */
        p[1 + (int)(rnd() & 1)] = tiny(-100, -55);
        if (rnd() & 1) p[(rnd() & 1) ? 1 : 2] = (rnd() & 1) ? 0.0f : tiny(-149, -60);
        if (rnd() & 1) p[0] = tiny(-149, -40);
        break;
    case 5:  /* tiny or zero constants (outside the host condition) */
        c[1 + (int)(rnd() % 3)] = (rnd() & 1) ? 0.0f : tiny(-40, -12);
        if (rnd() & 1) c[0] = tiny(-40, -12);
        break;
    case 6: {  /* near-cancelling real part: x0^2 ~ d0 */
        float s = p[1] * p[1] + p[2] * p[2];
        float d = fmaf(0.1f, 0.1f, s);
        p[0] = sign() * from_bits(bits(sqrtf(d)) + (uint32_t)(rnd() % 5) - 2u);
        break;
    }
    case 7:  /* constants at the edges of the host condition, and far escape radii */
        for (int i = 0; i < 4; ++i) c[i] = sign() * ldexpf(1.0f + unif(), -14 + (int)(rnd() % 4));
        if (rnd() & 1) *maxd = (rnd() & 1) ? 0x1p60f : 0x1p70f;
        *iters = 12 + (int)(rnd() % 40);
        break;
    default: break;
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000000;
    rng_state = argc > 2 ? strtoull(argv[2], 0, 10) * 0x9E3779B97F4A7C15ULL + 1 : 1;
    long differ = 0, eligible_diff = 0, ineligible = 0;
    for (long i = 0; i < n; ++i) {
        float p[3], c[4], maxd;
        int iters;
        draw((int)(i % 8), p, c, &maxd, &iters);
        const float c2[4] = {2.0f * c[0], 2.0f * c[1], 2.0f * c[2], 2.0f * c[3]};
        const Out a = plain(p, c, maxd, iters), b = doubled(p, c2, 4.0f * maxd, iters);
        const int off = !eligible(c, maxd);
        ineligible += off;
        /* a step that fails the class test is redone by the general loop in both forms: then nothing else counts */
        const int same = a.ok == b.ok && (!a.ok || (bits(a.qq) == bits(b.qq) && bits(a.dqs) == bits(b.dqs) &&
                                                    a.escaped_at == b.escaped_at));
        if (!same) {
            ++differ;
            if (!off) {
                if (++eligible_diff <= 5)
                    fprintf(stderr, "difference in an eligible scene: p=(%a,%a,%a) c=(%a,%a,%a,%a) maxd=%a iters=%d qq %a/%a dqs %a/%a esc %d/%d\n",
                            p[0], p[1], p[2], c[0], c[1], c[2], c[3], maxd, iters, a.qq, b.qq, a.dqs, b.dqs,
                            a.escaped_at, b.escaped_at);
            }
        }
    }
    printf("orbits %ld differ %ld differ_eligible %ld ineligible %ld\n", n, differ, eligible_diff, ineligible);
    return eligible_diff != 0;
}
