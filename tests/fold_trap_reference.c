/*
 * fold_trap_reference.c -- the expected frame and plane of kifs_render_folded_trapped_async and the expected u of
 * kifs_eval_fold_trap (include/kifs_hip.h), on the CPU.  TEST INFRASTRUCTURE ONLY.
 *
 * The contract on the oracle's PUBLIC pieces and on tests/fold_reference.c, which this file includes: the round of the
 * fold (fold_round), the host-side constants, the folded estimate and its normal, the shadow march and the occlusion
 * probes over it are that file's; the orbit, the trap distance and the gradient are restated here, and so are the march
 * and the shading with the hit's own colour in the place of fractal_color.  tests/test_fold_trap_reference.py holds this
 * file to tests/fold_reference.c (a neutral trap) and to tests/trap_reference.c (no iterations of the fold).  This file is
 * normative where the header's text and it could be read differently.
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/fold_trap_reference.py).
 */
#include "fold_reference.c"

typedef struct {
    float centre[4];
    uint32_t axes;
    int32_t iterations;
    float scale, bias;
    float mid[3];
    float far[3];
} KftTrap; /* KifsOrbitTrap */

/* d(z): the components of `axes` in the order x, y, z, w */
static float trap_distance(const KftTrap* trap, const float z[4]) {
    float d = 0.0f;
    for (int i = 0; i < 4; i++)
        if (trap->axes & (1u << i)) {
            const float e = z[i] - trap->centre[i];
            d = fmaf(e, e, d);
        }
    return d;
}

/* u of the position p.  info (NULL: not wanted): info[0] = where the least distance was attained -- 0 at z_0, 1 at a fold
 * point, 2 at a base point; info[1] = 1 if the stop rule cut the orbit, that is a stop test failed before round
 * min(N, K), where a fold point would still have taken part (or, K > N, the base part would have started elsewhere);
 * info[2] = the rounds of the fold that ran among the first min(N, K). */
float kft_trap_u(const KorOptions* options, const KfrFold* f, const KftTrap* trap, const float p[3], int32_t* info) {
    const int N = f->iterations, K = trap->iterations;
    float t[3], h;
    kfr_constants(f, t, &h);
    float q[3] = {p[0], p[1], p[2]};
    float z[4] = {p[0], p[1], p[2], 0.0f};
    float m = trap_distance(trap, z);
    int where = 0, cut = 0, ran = 0;
    for (int j = 0; j < N; j++) {
        if (!(sqrtf(dot3(q, q)) < options->max_distance)) { /* stops for good and keeps its p */
            if (j < K) cut = 1;
            break;
        }
        fold_round(f, t, h, q);
        if (j + 1 <= K) { /* fold point j + 1 takes part */
            ran++;
            z[0] = q[0];
            z[1] = q[1];
            z[2] = q[2];
            const float d = trap_distance(trap, z);
            if (d < m) {
                m = d;
                where = 1;
            }
        }
    }
    const int Kb = (K - N > 0) ? K - N : 0; /* from N, not from the rounds that ran */
    if (options->fractal_group_id == 0u && options->primitive_id == 4u) /* Sierpinski */
        for (int k = 0; k < Kb; k++) {
            float r[3];
            kor_tetrahedral_fold(q, r);
            q[0] = fmaf(2.0f, r[0], -1.0f);
            q[1] = fmaf(2.0f, r[1], -1.0f);
            q[2] = fmaf(2.0f, r[2], -1.0f);
            z[0] = q[0];
            z[1] = q[1];
            z[2] = q[2];
            const float d = trap_distance(trap, z);
            if (d < m) {
                m = d;
                where = 2;
            }
        }
    if (info) {
        info[0] = where;
        info[1] = cut;
        info[2] = ran;
    }
    return sqrtf(m);
}

void kft_trap_u_many(const KorOptions* options, const KfrFold* f, const KftTrap* trap, const float* points, int n, float* u,
                     int32_t* info) {
    for (int i = 0; i < n; i++) u[i] = kft_trap_u(options, f, trap, points + 3 * i, info ? info + 3 * i : NULL);
}

/* The gradient at u; returns t. */
float kft_colour(const KorOptions* options, const KftTrap* trap, float u, float col[3]) {
    const float v = fmaf(trap->scale, u, trap->bias);
    float t = (v > 0.0f) ? v : 0.0f;
    t = (t < 1.0f) ? t : 1.0f;
    const float x = t * 2.0f;
    const int j = (x >= 1.0f) ? 1 : 0;
    const float g = x - (float)j;
    const float* stops[3] = {options->fractal_color, trap->mid, trap->far};
    for (int i = 0; i < 3; i++) col[i] = fmaf(g, stops[j + 1][i] - stops[j][i], stops[j][i]);
    return t;
}

/* Rows [y0, y1) of the frame `screen` describes (a virtual screen for a supersampled launch's samples), as
 * kfr_march_rows.  u_out (NULL: not wanted): one float per pixel, the plane -- u of a hit, in heatmap mode too, +inf on a
 * miss.  Returns 0, or -1 on bad arguments. */
int kft_march_rows(const KorScreen* screen, const KorCamera* camera, const KorOptions* options, const KorIters* iters,
                   const KorExt* ext, const KfrFold* fold, const KftTrap* trap, const KfrLight* light, const KfrTerm* ao, int y0,
                   int y1, float* rgb, uint8_t* hit_out, float* pos_out, float* u_out) {
    static const KfrLight reference = {{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 0};
    if (!screen || !camera || !options || !iters || !fold || !trap || !rgb || y0 < 0 || y1 < y0 || (float)y1 > screen->height)
        return -1;
    if (!light) light = &reference;
    const int w = (int)screen->width;
    const float origin[3] = {camera->origin[0], camera->origin[1], camera->origin[2]};
    float Lh[3];
    normalize3(light->direction, Lh);
    const int has_spec = light->specular[0] != 0.0f || light->specular[1] != 0.0f || light->specular[2] != 0.0f;
    for (int y = y0; y < y1; y++)
        for (int x = 0; x < w; x++) {
            float dir[3];
            kor_ray_direction(screen, camera, x, y, dir);
            float t = 0.0f;
            float p[3] = {origin[0], origin[1], origin[2]};
            float n[3] = {0.0f, 0.0f, 0.0f};
            float c[3] = {options->background_color[0], options->background_color[1], options->background_color[2]};
            float u = INFINITY;
            int hit = 0;
            int i;
            for (i = 0; i < options->max_iterations && t < options->max_distance; i++) { /* kifs_oracle.c:raymarch */
                const float d = kfr_sdf(options, iters, fold, p);
                if (d < options->epsilon) {
                    kfr_normal(options, iters, fold, p, n);
                    hit = 1;
                    break;
                }
                t = t + d;
                p[0] = fmaf(t, dir[0], origin[0]);
                p[1] = fmaf(t, dir[1], origin[1]);
                p[2] = fmaf(t, dir[2], origin[2]);
            }
            if (hit) u = kft_trap_u(options, fold, trap, p, NULL);
            if (hit && !options->is_heatmap) {
                float col[3];
                kft_colour(options, trap, u, col);
                const float lit0 = clamp01(dot3(n, light->direction));
                float sh = 1.0f, lit = lit0;
                if (ext && ext->soft_shadow) {
                    if (lit0 > 0.0f) sh = shadow(options, iters, fold, ext, Lh, p, n);
                    lit = lit0 * sh;
                }
                const float k = fmaf(light->diffuse, lit, light->ambient);
                c[0] = k * col[0];
                c[1] = k * col[1];
                c[2] = k * col[2];
                if (has_spec) {
                    const float s = highlight(light, n, dir);
                    const float spec = (lit0 > 0.0f) ? s * sh : 0.0f;
                    c[0] = fmaf(light->specular[0], spec, c[0]);
                    c[1] = fmaf(light->specular[1], spec, c[1]);
                    c[2] = fmaf(light->specular[2], spec, c[2]);
                }
                if (ao) {
                    const float a = factor(options, iters, fold, ao, p, n);
                    c[0] = a * c[0];
                    c[1] = a * c[1];
                    c[2] = a * c[2];
                }
            }
            if (options->is_heatmap) { /* entry.wgsl:27-29: the counter's colour */
                const float g = (float)i / (float)options->max_iterations;
                c[0] = g * options->fractal_color[0];
                c[1] = g * options->fractal_color[1];
                c[2] = g * options->fractal_color[2];
            }
            const size_t k = (size_t)(y - y0) * (size_t)w + (size_t)x;
            memcpy(rgb + 3 * k, c, sizeof c);
            if (hit_out) hit_out[k] = (uint8_t)hit;
            if (pos_out) memcpy(pos_out + 3 * k, p, sizeof p);
            if (u_out) u_out[k] = u;
        }
    return 0;
}
