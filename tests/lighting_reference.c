/*
 * lighting_reference.c -- the expected frame of kifs_render_lit_async (include/kifs_hip.h), on the CPU.
 * TEST INFRASTRUCTURE ONLY.
 *
 * The contract on the oracle's PUBLIC pieces -- kor_ray_direction, kor_scene_sdf, kor_get_normal, kor_encode_channel --
 * and fmaf: the march (kifs_oracle.c:raymarch, as tests/occlusion_reference.c restates it), the direct term with a light
 * vector, the soft-shadow march of KifsExtensions towards the normalised light vector (kifs_oracle.c:soft_shadow with L
 * replaced), the Blinn-Phong highlight, the factor of kifs_render_occlusion_async and the heatmap's counter.  Nothing of
 * the oracle's own shading is called, so tests/test_lighting_reference.py can hold this file to it: with the reference's
 * light the frame is kor_render_ext's.  This file is normative where the header's text and it could be read differently.
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/lighting_reference.py).
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
} KlrLight; /* KifsLight */

typedef struct {
    int32_t samples;
    float step, decay, strength;
} KlrTerm; /* KifsAmbientOcclusion */

static float dot3(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
static void normalize3(const float v[3], float out[3]) {
    const float l = sqrtf(dot3(v, v));
    out[0] = v[0] / l;
    out[1] = v[1] / l;
    out[2] = v[2] / l;
}
static float clamp01(float e) { /* clamp_ of kifs_oracle.c: min_(max_(e, 0), 1), whose comparisons pass a NaN through */
    const float lo = (e < 0.0f) ? 0.0f : e;
    return (1.0f < lo) ? 1.0f : lo;
}

/* Lh of the contract. */
void klr_unit(const KlrLight* light, float out[3]) { normalize3(light->direction, out); }

/* lit0: the direct term with the light vector as given. */
float klr_direct(const KlrLight* light, const float n[3]) { return clamp01(dot3(n, light->direction)); }

/* s: the highlight before its attenuation, e squarings. */
float klr_highlight(const KlrLight* light, const float n[3], const float dir[3]) {
    float Lh[3], h[3];
    normalize3(light->direction, Lh);
    const float hv[3] = {Lh[0] - dir[0], Lh[1] - dir[1], Lh[2] - dir[2]};
    normalize3(hv, h);
    float s = clamp01(dot3(n, h));
    for (int i = 0; i < light->shininess_log2; i++) s = s * s;
    return s;
}

/* The secondary march of KifsExtensions from the hit at p with normal n towards the unit vector L. */
float klr_shadow(const KorOptions* options, const KorIters* iters, const KorExt* ext, const float L[3], const float p[3],
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
        res = (r < res) ? r : res; /* min_(res, r) */
        t = t + h;
        if (t > ext->shadow_max_t) break;
    }
    return res;
}

/* The factor of kifs_render_occlusion_async at (p, n) (tests/occlusion_reference.c:koc_factor). */
float klr_factor(const KorOptions* options, const KorIters* iters, const KlrTerm* ao, const float p[3], const float n[3]) {
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
 * hit; normal and pos (three floats, the tested position; zero normal on a miss); terms: four floats (lit0, s, sh, a) of a
 * hit -- s is 0 without a highlight, a is 1 without a term -- and (0, 0, 1, 1) on a miss.  ext and ao may be NULL.
 * Returns 0, or -1 on bad arguments. */
int klr_march_rows(const KorScreen* screen, const KorCamera* camera, const KorOptions* options, const KorIters* iters,
                   const KorExt* ext, const KlrLight* light, const KlrTerm* ao, int y0, int y1, float* rgb, uint8_t* hit_out,
                   float* normal_out, float* pos_out, float* terms_out) {
    if (!screen || !camera || !options || !iters || !light || !rgb || y0 < 0 || y1 < y0 || (float)y1 > screen->height) return -1;
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
            float terms[4] = {0.0f, 0.0f, 1.0f, 1.0f};
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
            if (hit) {
                const float lit0 = clamp01(dot3(n, light->direction));
                float sh = 1.0f, lit = lit0;
                if (ext && ext->soft_shadow) {
                    if (lit0 > 0.0f) sh = klr_shadow(options, iters, ext, Lh, p, n);
                    lit = lit0 * sh;
                }
                const float k = fmaf(light->diffuse, lit, light->ambient);
                c[0] = k * options->fractal_color[0];
                c[1] = k * options->fractal_color[1];
                c[2] = k * options->fractal_color[2];
                terms[0] = lit0;
                terms[2] = sh;
                if (has_spec) {
                    const float s = klr_highlight(light, n, dir);
                    const float spec = (lit0 > 0.0f) ? s * sh : 0.0f;
                    c[0] = fmaf(light->specular[0], spec, c[0]);
                    c[1] = fmaf(light->specular[1], spec, c[1]);
                    c[2] = fmaf(light->specular[2], spec, c[2]);
                    terms[1] = s;
                }
                if (ao) {
                    const float a = klr_factor(options, iters, ao, p, n);
                    c[0] = a * c[0];
                    c[1] = a * c[1];
                    c[2] = a * c[2];
                    terms[3] = a;
                }
            }
            if (options->is_heatmap) { /* entry.wgsl:27-29: the counter's colour, unlit and unattenuated */
                const float f = (float)i / (float)options->max_iterations;
                c[0] = f * options->fractal_color[0];
                c[1] = f * options->fractal_color[1];
                c[2] = f * options->fractal_color[2];
            }
            const size_t k = (size_t)(y - y0) * (size_t)w + (size_t)x;
            memcpy(rgb + 3 * k, c, sizeof c);
            if (hit_out) hit_out[k] = (uint8_t)hit;
            if (normal_out) memcpy(normal_out + 3 * k, n, sizeof n);
            if (pos_out) memcpy(pos_out + 3 * k, p, sizeof p);
            if (terms_out) memcpy(terms_out + 4 * k, terms, sizeof terms);
        }
    return 0;
}

/* Linear colours to RGBA8 through the oracle's encoder, alpha 255. */
void klr_encode(const float* rgb, size_t pixels, int encode, uint8_t* rgba) {
    for (size_t k = 0; k < pixels; k++) {
        rgba[4 * k + 0] = kor_encode_channel(rgb[3 * k + 0], encode);
        rgba[4 * k + 1] = kor_encode_channel(rgb[3 * k + 1], encode);
        rgba[4 * k + 2] = kor_encode_channel(rgb[3 * k + 2], encode);
        rgba[4 * k + 3] = 255;
    }
}
