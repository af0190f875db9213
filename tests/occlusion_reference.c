/*
 * occlusion_reference.c -- the expected frame and plane of kifs_render_occlusion_async (include/kifs_hip.h), on the CPU.
 * TEST INFRASTRUCTURE ONLY.
 *
 * The factor of the contract on the oracle's PUBLIC pieces -- kor_scene_sdf, kor_get_normal -- and fmaf, for the hits of
 * the march tests/geometry_reference.c restates (the same loop, kept here because the factor needs the tested position,
 * which that file's texel does not carry; tests/test_occlusion_reference.py holds the two to each other).  The colour of
 * a hit is the factor times the oracle's own linear colour of the pixel, kor_shade_pixel_ext -- soft shadows included
 * when the extension block says so; a miss and a heatmap pixel are the oracle's colour as it is.  This file is normative
 * where the header's text and it could be read differently.
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/occlusion_reference.py).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kifs_oracle.h"

typedef struct {
    int32_t samples;
    float step, decay, strength;
} KocTerm; /* KifsAmbientOcclusion */

/* The factor of a hit at the tested position p with the shading's normal n. */
float koc_factor(const KorOptions* options, const KorIters* iters, const KocTerm* ao, const float p[3], const float n[3]) {
    float occ = 0.0f, w = 1.0f;
    for (int i = 1; i <= ao->samples; i++) {
        const float h = ao->step * (float)i;
        const float q[3] = {fmaf(h, n[0], p[0]), fmaf(h, n[1], p[1]), fmaf(h, n[2], p[2])};
        const float d = kor_scene_sdf(options, iters, q);
        occ = occ + w * (h - d);
        w = w * ao->decay;
    }
    const float e = 1.0f - ao->strength * occ;
    const float lo = (e < 0.0f) ? 0.0f : e; /* clamp_ of kifs_oracle.c: min_(max_(e, 0), 1), */
    return (1.0f < lo) ? 1.0f : lo;         /* whose comparisons pass a NaN through */
}

/* Rows [y0, y1) of the frame `screen` describes (a virtual screen for a supersampled launch's samples).  rgb: three
 * floats per pixel, the linear colour before the resolve and the encode; plane: one float per pixel, the factor of a hit
 * and 1.0f on a miss; hit, normal (three floats per pixel, zero on a miss) and pos (the tested position) may be NULL.
 * ext may be NULL.  Returns 0, or -1 on bad arguments. */
int koc_march_rows(const KorScreen* screen, const KorCamera* camera, const KorOptions* options, const KorIters* iters,
                   const KorExt* ext, const KocTerm* ao, int y0, int y1, float* rgb, float* plane, uint8_t* hit_out,
                   float* normal_out, float* pos_out) {
    if (!screen || !camera || !options || !iters || !ao || !rgb || !plane || y0 < 0 || y1 < y0 || (float)y1 > screen->height)
        return -1;
    const int w = (int)screen->width;
    const float origin[3] = {camera->origin[0], camera->origin[1], camera->origin[2]};
    for (int y = y0; y < y1; y++)
        for (int x = 0; x < w; x++) {
            float dir[3];
            kor_ray_direction(screen, camera, x, y, dir);
            float t = 0.0f;
            float p[3] = {origin[0], origin[1], origin[2]};
            float n[3] = {0.0f, 0.0f, 0.0f};
            int hit = 0;
            for (int i = 0; i < options->max_iterations && t < options->max_distance; i++) { /* kifs_oracle.c:raymarch */
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
            const size_t k = (size_t)(y - y0) * (size_t)w + (size_t)x;
            float shade[4];
            kor_shade_pixel_ext(screen, camera, options, iters, ext, x, y, shade);
            float a = 1.0f;
            if (hit) a = koc_factor(options, iters, ao, p, n);
            plane[k] = a;
            if (hit && !options->is_heatmap) {
                rgb[3 * k + 0] = a * shade[0];
                rgb[3 * k + 1] = a * shade[1];
                rgb[3 * k + 2] = a * shade[2];
            } else {
                rgb[3 * k + 0] = shade[0];
                rgb[3 * k + 1] = shade[1];
                rgb[3 * k + 2] = shade[2];
            }
            if (hit_out) hit_out[k] = (uint8_t)hit;
            if (normal_out) memcpy(normal_out + 3 * k, n, sizeof n);
            if (pos_out) memcpy(pos_out + 3 * k, p, sizeof p);
        }
    return 0;
}

/* Linear colours to RGBA8 through the oracle's encoder, alpha 255. */
void koc_encode(const float* rgb, size_t pixels, int encode, uint8_t* rgba) {
    for (size_t k = 0; k < pixels; k++) {
        rgba[4 * k + 0] = kor_encode_channel(rgb[3 * k + 0], encode);
        rgba[4 * k + 1] = kor_encode_channel(rgb[3 * k + 1], encode);
        rgba[4 * k + 2] = kor_encode_channel(rgb[3 * k + 2], encode);
        rgba[4 * k + 3] = 255;
    }
}
