/*
 * fold_reference.c -- the expected frame of kifs_render_folded_async and the expected values of kifs_eval_fold
 * (include/kifs_hip.h), on the CPU.  TEST INFRASTRUCTURE ONLY.
 *
 * The contract on the oracle's PUBLIC pieces -- kor_ray_direction, kor_scene_sdf (the base primitive's estimate),
 * kor_tetrahedral_fold, kor_encode_channel -- and fmaf: the folded estimate, its central-difference normal, and the march
 * and the shading of tests/lighting_reference.c restated here with the folded estimate in the place of the scene's
 * everywhere -- the primary march, the normal, the soft-shadow march and the occlusion probes.  Nothing of the oracle's
 * own march or shading is called, so tests/test_fold_reference.py can hold this file to it and to
 * tests/lighting_reference.c: with iterations = 0 the frame is theirs.  This file is normative where the header's text
 * and it could be read differently.
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/fold_reference.py).
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
} KfrLight; /* KifsLight */

typedef struct {
    int32_t samples;
    float step, decay, strength;
} KfrTerm; /* KifsAmbientOcclusion */

typedef struct {
    uint32_t stages;
    int32_t iterations;
    float scale;
    float offset[3];
    float rotation[9];
} KfrFold; /* KifsFoldSystem */

enum { FOLD_ABS = 1, FOLD_SORT = 2, FOLD_TETRA = 4, FOLD_ROTATE = 8, FOLD_MIRROR_Z = 16 };

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

/* ---- the folded estimate ---------------------------------------------------------------------------------------------- */
static void swap_if_less(float* a, float* b) { /* if (a < b) swap(a, b): a NaN is not moved */
    if (*a < *b) {
        const float t = *a;
        *a = *b;
        *b = t;
    }
}

/* One round of the stages at q, in the contract's order; t and h are the host-side constants. */
static void fold_round(const KfrFold* f, const float t[3], float h, float q[3]) {
    if (f->stages & FOLD_ABS) {
        q[0] = fabsf(q[0]);
        q[1] = fabsf(q[1]);
        q[2] = fabsf(q[2]);
    }
    if (f->stages & FOLD_SORT) {
        swap_if_less(&q[0], &q[1]);
        swap_if_less(&q[0], &q[2]);
        swap_if_less(&q[1], &q[2]);
    }
    if (f->stages & FOLD_TETRA) {
        float r[3];
        kor_tetrahedral_fold(q, r);
        memcpy(q, r, sizeof r);
    }
    if (f->stages & FOLD_ROTATE) {
        const float* R = f->rotation;
        const float r[3] = {fmaf(R[2], q[2], fmaf(R[1], q[1], R[0] * q[0])), fmaf(R[5], q[2], fmaf(R[4], q[1], R[3] * q[0])),
                            fmaf(R[8], q[2], fmaf(R[7], q[1], R[6] * q[0]))};
        memcpy(q, r, sizeof r);
    }
    q[0] = fmaf(f->scale, q[0], t[0]);
    q[1] = fmaf(f->scale, q[1], t[1]);
    q[2] = fmaf(f->scale, q[2], t[2]);
    if (f->stages & FOLD_MIRROR_Z) q[2] = fabsf(q[2] - h) + h;
}

/* The host-side constants: k = s - 1, t_i = -(k c_i), h = 0.5 t_z. */
void kfr_constants(const KfrFold* f, float t[3], float* h) {
    const float k = f->scale - 1.0f;
    for (int i = 0; i < 3; i++) t[i] = -(k * f->offset[i]);
    *h = 0.5f * t[2];
}

/* The folded point and acc of p. */
void kfr_fold_point(const KorOptions* options, const KfrFold* f, const float p[3], float q[3], float* acc_out) {
    float t[3], h;
    kfr_constants(f, t, &h);
    float acc = 1.0f;
    memcpy(q, p, 3 * sizeof(float));
    for (int j = 0; j < f->iterations; j++) {
        if (!(sqrtf(dot3(q, q)) < options->max_distance)) break;
        fold_round(f, t, h, q);
        acc = acc * f->scale;
    }
    *acc_out = acc;
}

float kfr_sdf(const KorOptions* options, const KorIters* iters, const KfrFold* f, const float p[3]) {
    float q[3], acc;
    kfr_fold_point(options, f, p, q, &acc);
    return kor_scene_sdf(options, iters, q) / acc;
}

/* get_normal's central differences with h = epsilon over the folded estimate (kifs_oracle.c:kifs_normal). */
void kfr_normal(const KorOptions* options, const KorIters* iters, const KfrFold* f, const float p[3], float n[3]) {
    const float h = options->epsilon;
    const float xp[3] = {p[0] + h, p[1] + 0.0f, p[2] + 0.0f}, xm[3] = {p[0] - h, p[1] - 0.0f, p[2] - 0.0f};
    const float yp[3] = {p[0] + 0.0f, p[1] + h, p[2] + 0.0f}, ym[3] = {p[0] - 0.0f, p[1] - h, p[2] - 0.0f};
    const float zp[3] = {p[0] + 0.0f, p[1] + 0.0f, p[2] + h}, zm[3] = {p[0] - 0.0f, p[1] - 0.0f, p[2] - h};
    const float d[3] = {kfr_sdf(options, iters, f, xp) - kfr_sdf(options, iters, f, xm),
                        kfr_sdf(options, iters, f, yp) - kfr_sdf(options, iters, f, ym),
                        kfr_sdf(options, iters, f, zp) - kfr_sdf(options, iters, f, zm)};
    normalize3(d, n);
}

/* sdf and/or normal (NULL: not wanted) of n positions. */
void kfr_eval_many(const KorOptions* options, const KorIters* iters, const KfrFold* f, const float* points, int n, float* sdf,
                   float* normal) {
    for (int i = 0; i < n; i++) {
        if (sdf) sdf[i] = kfr_sdf(options, iters, f, points + 3 * i);
        if (normal) kfr_normal(options, iters, f, points + 3 * i, normal + 3 * i);
    }
}

/* ---- the shading of tests/lighting_reference.c over the folded estimate ----------------------------------------------- */
static float highlight(const KfrLight* light, const float n[3], const float dir[3]) {
    float Lh[3], h[3];
    normalize3(light->direction, Lh);
    const float hv[3] = {Lh[0] - dir[0], Lh[1] - dir[1], Lh[2] - dir[2]};
    normalize3(hv, h);
    float s = clamp01(dot3(n, h));
    for (int i = 0; i < light->shininess_log2; i++) s = s * s;
    return s;
}

static float shadow(const KorOptions* options, const KorIters* iters, const KfrFold* f, const KorExt* ext, const float L[3],
                    const float p[3], const float n[3]) {
    const float off = 2.0f * options->epsilon;
    const float start[3] = {fmaf(off, n[0], p[0]), fmaf(off, n[1], p[1]), fmaf(off, n[2], p[2])};
    float res = 1.0f;
    float t = ext->shadow_t0;
    for (int j = 0; j < ext->shadow_steps; j++) {
        const float q[3] = {fmaf(t, L[0], start[0]), fmaf(t, L[1], start[1]), fmaf(t, L[2], start[2])};
        const float h = kfr_sdf(options, iters, f, q);
        if (h < options->epsilon) return 0.0f;
        const float r = (ext->shadow_k * h) / t;
        res = (r < res) ? r : res;
        t = t + h;
        if (t > ext->shadow_max_t) break;
    }
    return res;
}

static float factor(const KorOptions* options, const KorIters* iters, const KfrFold* f, const KfrTerm* ao, const float p[3],
                    const float n[3]) {
    float occ = 0.0f, w = 1.0f;
    for (int i = 1; i <= ao->samples; i++) {
        const float h = ao->step * (float)i;
        const float q[3] = {fmaf(h, n[0], p[0]), fmaf(h, n[1], p[1]), fmaf(h, n[2], p[2])};
        const float d = kfr_sdf(options, iters, f, q);
        occ = occ + w * (h - d);
        w = w * ao->decay;
    }
    return clamp01(1.0f - ao->strength * occ);
}

/* Rows [y0, y1) of the frame `screen` describes (a virtual screen for a supersampled launch's samples).  rgb: three
 * floats per pixel, the linear colour before the resolve and the encode.  Optional outputs (NULL: not wanted), per pixel:
 * hit; pos (three floats, the tested position).  light NULL: the reference's light; ext and ao may be NULL.  Returns 0, or
 * -1 on bad arguments. */
int kfr_march_rows(const KorScreen* screen, const KorCamera* camera, const KorOptions* options, const KorIters* iters,
                   const KorExt* ext, const KfrFold* fold, const KfrLight* light, const KfrTerm* ao, int y0, int y1, float* rgb,
                   uint8_t* hit_out, float* pos_out) {
    static const KfrLight reference = {{1.0f, 1.0f, 1.0f}, 0.1f, 0.9f, {0.0f, 0.0f, 0.0f}, 0};
    if (!screen || !camera || !options || !iters || !fold || !rgb || y0 < 0 || y1 < y0 || (float)y1 > screen->height) return -1;
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
            if (hit && !options->is_heatmap) {
                const float lit0 = clamp01(dot3(n, light->direction));
                float sh = 1.0f, lit = lit0;
                if (ext && ext->soft_shadow) {
                    if (lit0 > 0.0f) sh = shadow(options, iters, fold, ext, Lh, p, n);
                    lit = lit0 * sh;
                }
                const float k = fmaf(light->diffuse, lit, light->ambient);
                c[0] = k * options->fractal_color[0];
                c[1] = k * options->fractal_color[1];
                c[2] = k * options->fractal_color[2];
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
                const float f = (float)i / (float)options->max_iterations;
                c[0] = f * options->fractal_color[0];
                c[1] = f * options->fractal_color[1];
                c[2] = f * options->fractal_color[2];
            }
            const size_t k = (size_t)(y - y0) * (size_t)w + (size_t)x;
            memcpy(rgb + 3 * k, c, sizeof c);
            if (hit_out) hit_out[k] = (uint8_t)hit;
            if (pos_out) memcpy(pos_out + 3 * k, p, sizeof p);
        }
    return 0;
}

/* Linear colours to RGBA8 through the oracle's encoder, alpha 255. */
void kfr_encode(const float* rgb, size_t pixels, int encode, uint8_t* rgba) {
    for (size_t k = 0; k < pixels; k++) {
        rgba[4 * k + 0] = kor_encode_channel(rgb[3 * k + 0], encode);
        rgba[4 * k + 1] = kor_encode_channel(rgb[3 * k + 1], encode);
        rgba[4 * k + 2] = kor_encode_channel(rgb[3 * k + 2], encode);
        rgba[4 * k + 3] = 255;
    }
}
