/*
 * trap_reference.c -- the expected frame of kifs_render_trapped_async and the expected u of kifs_eval_trap
 * (include/kifs_hip.h), on the CPU.  TEST INFRASTRUCTURE ONLY.
 *
 * The contract on the oracle's PUBLIC pieces -- kor_ray_direction, kor_scene_sdf, kor_get_normal, kor_tetrahedral_fold,
 * kor_encode_channel, the kor_* elementary functions (for quat_pow) -- and fmaf: the march and the shading of
 * tests/lighting_reference.c, restated here with the hit's own colour in the place of fractal_color, and the orbit, the
 * trap distance and the gradient that make that colour.  Nothing of the oracle's own shading is called, so
 * tests/test_trap_reference.py can hold this file to it and to tests/lighting_reference.c: with scale = bias = 0 the frame
 * is theirs.  This file is normative where the header's text and it could be read differently.
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/trap_reference.py).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kifs_oracle.h"

typedef struct {
    float direction[3];
    float ambient, diffuse;
    float specular[3];
    int32_t shininess_log2;
} KtrLight; /* KifsLight */

typedef struct {
    int32_t samples;
    float step, decay, strength;
} KtrTerm; /* KifsAmbientOcclusion */

typedef struct {
    float centre[4];
    uint32_t axes;
    int32_t iterations;
    float scale, bias;
    float mid[3];
    float far[3];
} KtrTrap; /* KifsOrbitTrap */

static float dot3(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
static void normalize3(const float v[3], float out[3]) {
    const float l = sqrtf(dot3(v, v));
    out[0] = v[0] / l;
    out[1] = v[1] / l;
    out[2] = v[2] / l;
}
static float clamp01(float e) { /* clamp_ of kifs_oracle.c: its comparisons pass a NaN through */
    const float lo = (e < 0.0f) ? 0.0f : e;
    return (1.0f < lo) ? 1.0f : lo;
}

/* ---- the orbit ------------------------------------------------------------------------------------------------------ */
static float quat_ijk2(const float q[4]) { return fmaf(q[3], q[3], q[1] * q[1] + q[2] * q[2]); }
static float quat_norm2(const float q[4]) { return fmaf(q[0], q[0], quat_ijk2(q)); }

/* kifs_oracle.c:quat_sq_add */
static void quat_sq_add(const float q[4], const float c[4], float out[4]) {
    const float tr = 2.0f * q[0];
    const float r0 = fmaf(q[0], q[0], -quat_ijk2(q)) + c[0];
    const float r1 = fmaf(tr, q[1], c[1]), r2 = fmaf(tr, q[2], c[2]), r3 = fmaf(tr, q[3], c[3]);
    out[0] = r0;
    out[1] = r1;
    out[2] = r2;
    out[3] = r3;
}

/* kifs_oracle.c:quat_pow (the form genjulia_normal uses), on the public elementary functions */
static void quat_pow(const float q[4], float x, float out[4]) {
    const float d = quat_ijk2(q);
    const float qs = fmaf(q[0], q[0], d);
    const float L = kor_log2f(qs);
    const float inv = 1.0f / sqrtf(qs);
    const float phi = kor_acosf(q[0] * inv);
    const float ninv = 1.0f / sqrtf(d);
    const float n[3] = {q[1] * ninv, q[2] * ninv, q[3] * ninv};
    const float pw = kor_exp2f(x * (0.5f * L));
    const float a = x * phi;
    const float cs = kor_cosf(a), sn = kor_sinf(a);
    out[0] = pw * cs;
    out[1] = pw * (n[0] * sn);
    out[2] = pw * (n[1] * sn);
    out[3] = pw * (n[2] * sn);
}

/* d(z): the components of `axes` in the order x, y, z, w */
static float trap_distance(const KtrTrap* trap, const float z[4]) {
    float d = 0.0f;
    for (int i = 0; i < 4; i++)
        if (trap->axes & (1u << i)) {
            const float e = z[i] - trap->centre[i];
            d = fmaf(e, e, d);
        }
    return d;
}

/* u of the position p: sqrt of the least d over z_0 .. z_K as far as the orbit ran. */
float ktr_trap_u(const KorOptions* options, const KtrTrap* trap, const float p[3]) {
    const int julia = options->fractal_group_id == 1u, genjulia = options->fractal_group_id == 2u;
    float z[4] = {p[0], p[1], p[2], (julia || genjulia) ? 0.1f : 0.0f};
    float m = trap_distance(trap, z);
    if (julia || genjulia) {
        for (int k = 0; k < trap->iterations; k++) {
            float n[4];
            if (julia) {
                quat_sq_add(z, options->constant, n);
            } else {
                quat_pow(z, options->power, n);
                for (int i = 0; i < 4; i++) n[i] = n[i] + options->constant[i];
            }
            memcpy(z, n, sizeof z);
            const float d = trap_distance(trap, z);
            m = (d < m) ? d : m;
            if (quat_norm2(z) > options->max_distance) break;
        }
    } else if (options->fractal_group_id == 0u && options->primitive_id == 4u) { /* Sierpinski */
        for (int k = 0; k < trap->iterations; k++) {
            float f[3];
            kor_tetrahedral_fold(z, f);
            z[0] = fmaf(2.0f, f[0], -1.0f);
            z[1] = fmaf(2.0f, f[1], -1.0f);
            z[2] = fmaf(2.0f, f[2], -1.0f);
            const float d = trap_distance(trap, z);
            m = (d < m) ? d : m;
        }
    }
    return sqrtf(m);
}

void ktr_trap_u_many(const KorOptions* options, const KtrTrap* trap, const float* points, int n, float* u) {
    for (int i = 0; i < n; i++) u[i] = ktr_trap_u(options, trap, points + 3 * i);
}

/* The gradient at u; returns t. */
float ktr_colour(const KorOptions* options, const KtrTrap* trap, float u, float col[3]) {
    const float v = fmaf(trap->scale, u, trap->bias);
    float t = (v > 0.0f) ? v : 0.0f;
    t = (t < 1.0f) ? t : 1.0f;
    const float x = t * 2.0f;
    const int j = (x >= 1.0f) ? 1 : 0;
    const float f = x - (float)j;
    const float* stops[3] = {options->fractal_color, trap->mid, trap->far};
    for (int i = 0; i < 3; i++) col[i] = fmaf(f, stops[j + 1][i] - stops[j][i], stops[j][i]);
    return t;
}

/* ---- the shading of tests/lighting_reference.c ------------------------------------------------------------------------ */
static float highlight(const KtrLight* light, const float n[3], const float dir[3]) {
    float Lh[3], h[3];
    normalize3(light->direction, Lh);
    const float hv[3] = {Lh[0] - dir[0], Lh[1] - dir[1], Lh[2] - dir[2]};
    normalize3(hv, h);
    float s = clamp01(dot3(n, h));
    for (int i = 0; i < light->shininess_log2; i++) s = s * s;
    return s;
}

static float shadow(const KorOptions* options, const KorIters* iters, const KorExt* ext, const float L[3], const float p[3],
                    const float n[3]) {
    const float off = 2.0f * options->epsilon;
    const float start[3] = {fmaf(off, n[0], p[0]), fmaf(off, n[1], p[1]), fmaf(off, n[2], p[2])};
    float res = 1.0f;
    float t = ext->shadow_t0;
    for (int j = 0; j < ext->shadow_steps; j++) {
        const float q[3] = {fmaf(t, L[0], start[0]), fmaf(t, L[1], start[1]), fmaf(t, L[2], start[2])};
        const float h = kor_scene_sdf(options, iters, q);
        if (h < options->epsilon) return 0.0f;
        const float r = (ext->shadow_k * h) / t;
        res = (r < res) ? r : res;
        t = t + h;
        if (t > ext->shadow_max_t) break;
    }
    return res;
}

static float factor(const KorOptions* options, const KorIters* iters, const KtrTerm* ao, const float p[3], const float n[3]) {
    float occ = 0.0f, w = 1.0f;
    for (int i = 1; i <= ao->samples; i++) {
        const float h = ao->step * (float)i;
        const float q[3] = {fmaf(h, n[0], p[0]), fmaf(h, n[1], p[1]), fmaf(h, n[2], p[2])};
        const float d = kor_scene_sdf(options, iters, q);
        occ = occ + w * (h - d);
        w = w * ao->decay;
    }
    return clamp01(1.0f - ao->strength * occ);
}

/* Rows [y0, y1) of the frame `screen` describes (a virtual screen for a supersampled launch's samples).  rgb: three
 * floats per pixel, the linear colour before the resolve and the encode.  Optional outputs (NULL: not wanted), per pixel:
 * hit; pos (three floats, the tested position); ut: two floats (u, t) of a hit outside heatmap mode, (0, 0) otherwise.
 * light NULL: the reference's light; ext and ao may be NULL.  Returns 0, or -1 on bad arguments. */
int ktr_march_rows(const KorScreen* screen, const KorCamera* camera, const KorOptions* options, const KorIters* iters,
                   const KorExt* ext, const KtrTrap* trap, const KtrLight* light, const KtrTerm* ao, int y0, int y1, float* rgb,
                   uint8_t* hit_out, float* pos_out, float* ut_out) {
    static const KtrLight reference = {{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 0};
    if (!screen || !camera || !options || !iters || !trap || !rgb || y0 < 0 || y1 < y0 || (float)y1 > screen->height) return -1;
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
            float ut[2] = {0.0f, 0.0f};
            int hit = 0;
            int i;
            for (i = 0; i < options->max_iterations && t < options->max_distance; i++) { /* kifs_oracle.c:raymarch */
                const float d = kor_scene_sdf(options, iters, p);
                if (d < options->epsilon) {
                    kor_get_normal(options, iters, p, n);
                    hit = 1;
                    break;
                }
                t = t + d;
                p[0] = fmaf(t, dir[0], origin[0]);
                p[1] = fmaf(t, dir[1], origin[1]);
                p[2] = fmaf(t, dir[2], origin[2]);
            }
            if (hit && !options->is_heatmap) {
                float col[3];
                ut[0] = ktr_trap_u(options, trap, p);
                ut[1] = ktr_colour(options, trap, ut[0], col);
                const float lit0 = clamp01(dot3(n, light->direction));
                float sh = 1.0f, lit = lit0;
                if (ext && ext->soft_shadow) {
                    if (lit0 > 0.0f) sh = shadow(options, iters, ext, Lh, p, n);
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
                    const float a = factor(options, iters, ao, p, n);
                    c[0] = a * c[0];
                    c[1] = a * c[1];
                    c[2] = a * c[2];
                }
            }
            if (options->is_heatmap) { /* entry.wgsl:27-29: the counter's colour; no trap is evaluated */
                const float f = (float)i / (float)options->max_iterations;
                c[0] = f * options->fractal_color[0];
                c[1] = f * options->fractal_color[1];
                c[2] = f * options->fractal_color[2];
            }
            const size_t k = (size_t)(y - y0) * (size_t)w + (size_t)x;
            memcpy(rgb + 3 * k, c, sizeof c);
            if (hit_out) hit_out[k] = (uint8_t)hit;
            if (pos_out) memcpy(pos_out + 3 * k, p, sizeof p);
            if (ut_out) memcpy(ut_out + 2 * k, ut, sizeof ut);
        }
    return 0;
}

/* Linear colours to RGBA8 through the oracle's encoder, alpha 255. */
void ktr_encode(const float* rgb, size_t pixels, int encode, uint8_t* rgba) {
    for (size_t k = 0; k < pixels; k++) {
        rgba[4 * k + 0] = kor_encode_channel(rgb[3 * k + 0], encode);
        rgba[4 * k + 1] = kor_encode_channel(rgb[3 * k + 1], encode);
        rgba[4 * k + 2] = kor_encode_channel(rgb[3 * k + 2], encode);
        rgba[4 * k + 3] = 255;
    }
}
