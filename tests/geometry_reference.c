/*
 * geometry_reference.c -- the expected geometry plane of kifs_render_geometry_async (include/kifs_hip.h), on the CPU.
 * TEST INFRASTRUCTURE ONLY.
 *
 * The oracle's raymarch() (oracle/kifs_oracle.c) keeps hit, t and the normal to itself, so this file restates its loop
 * on the oracle's PUBLIC pieces -- kor_ray_direction, kor_scene_sdf, kor_get_normal -- with fmaf for the position, and
 * hands out what the loop held: per pixel whether it broke at d < epsilon, the ray parameter t at the break, the
 * normal get_normal returned there, and the loop counter i.  tests/test_geometry_reference.py holds the restatement to
 * the oracle itself (the counter against kor_render_stats, the colour rebuilt from n against kor_shade_pixel).
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/geometry_reference.py).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kifs_oracle.h"

/* Rows [y0, y1) of the frame.  geom: (y1 - y0) * W texels of four floats (n.x, n.y, n.z, t), the miss texel being
 * (0, 0, 0, +inf); hit: one byte per pixel; steps: the loop counter i of entry.wgsl:11-27 (saturated at 65535, as
 * kor_render_stats').  hit and steps may be NULL.  Returns 0, or -1 on bad arguments. */
int kgr_march_rows(const KorScreen* screen, const KorCamera* camera, const KorOptions* options, const KorIters* iters,
                   int y0, int y1, float* geom, uint8_t* hit_out, uint16_t* steps_out) {
    if (!screen || !camera || !options || !iters || !geom || y0 < 0 || y1 < y0 || (float)y1 > screen->height) return -1;
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
            const size_t k = (size_t)(y - y0) * (size_t)w + (size_t)x;
            float* texel = geom + 4 * k;
            if (hit) {
                texel[0] = n[0]; texel[1] = n[1]; texel[2] = n[2]; texel[3] = t;
            } else {
                texel[0] = 0.0f; texel[1] = 0.0f; texel[2] = 0.0f; texel[3] = INFINITY;
            }
            if (hit_out) hit_out[k] = (uint8_t)hit;
            if (steps_out) steps_out[k] = (uint16_t)(i > 65535 ? 65535 : i);
        }
    return 0;
}

/* The linear colour the contract's shading makes of a texel, no heatmap, no shadows (entry.wgsl:16-19 as
 * kifs_oracle.c:raymarch writes it): fma(0.9, clamp((n.x + n.y) + n.z, 0, 1), 0.1) times the fractal colour, or the
 * background on a miss.  rgb: three floats per pixel. */
void kgr_colour_from_geometry(const KorOptions* options, const float* geom, const uint8_t* hit, size_t pixels,
                              float* rgb) {
    for (size_t k = 0; k < pixels; k++) {
        const float* n = geom + 4 * k;
        float* c = rgb + 3 * k;
        if (!hit[k]) {
            c[0] = options->background_color[0]; c[1] = options->background_color[1]; c[2] = options->background_color[2];
            continue;
        }
        const float ndl = (n[0] + n[1]) + n[2];                 /* dot(n, (1,1,1)) */
        const float lo = (ndl < 0.0f) ? 0.0f : ndl;             /* clamp_ of kifs_oracle.c: min_(max_(e, 0), 1), */
        const float lit = (1.0f < lo) ? 1.0f : lo;              /* whose comparisons pass a NaN through */
        const float diffuse = fmaf(0.9f, lit, 0.1f);
        c[0] = diffuse * options->fractal_color[0];
        c[1] = diffuse * options->fractal_color[1];
        c[2] = diffuse * options->fractal_color[2];
    }
}
