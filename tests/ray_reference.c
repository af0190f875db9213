/*
 * ray_reference.c -- the expected output of kifs_trace_rays_async (include/kifs_hip.h), on the CPU.
 * TEST INFRASTRUCTURE ONLY.
 *
 * The oracle marches the pixels of its pinhole camera and nothing else, so this file restates its loop
 * (oracle/kifs_oracle.c:raymarch, as tests/geometry_reference.c does) on the oracle's PUBLIC pieces -- kor_scene_sdf,
 * kor_get_normal, kor_encode_channel -- for a ray record: its own origin and direction in place of the camera's and
 * kor_ray_direction's, with fmaf for the position.  Per ray it hands out the geometry texel, the loop counter i and the
 * RGBA8 pixel: the unshadowed shading of the normal as kgr_colour_from_geometry states it, the heatmap colour from i, the
 * background on a miss.  Soft shadows are not restated here: the oracle's own frames speak for them
 * (tests/test_gpu_rays.py).  tests/test_ray_reference.py holds the restatement to the oracle itself.
 *
 * Built at test time with -ffp-contract=off and linked against the oracle's shared library (tests/ray_reference.py).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "kifs_oracle.h"

/* rays: n records of eight floats (origin.xyz, -, direction.xyz, -).  geom: n texels of four floats; rgba: n pixels of
 * four bytes; steps: the loop counter i (saturated at 65535).  geom, rgba and steps may each be NULL.  Returns 0, or -1
 * on bad arguments. */
int krr_trace(const KorOptions* options, const KorIters* iters, int encode, const float* rays, size_t n, float* geom,
              uint8_t* rgba, uint16_t* steps_out) {
    if (!options || !iters || !rays) return -1;
    for (size_t k = 0; k < n; k++) {
        const float* origin = rays + 8 * k;
        const float* dir = rays + 8 * k + 4;
        float t = 0.0f;
        float p[3] = {origin[0], origin[1], origin[2]};
        float nrm[3] = {0.0f, 0.0f, 0.0f};
        int hit = 0;
        int i;
        for (i = 0; i < options->max_iterations && t < options->max_distance; i++) { /* kifs_oracle.c:raymarch */
            const float d = kor_scene_sdf(options, iters, p);
            if (d < options->epsilon) {
                kor_get_normal(options, iters, p, nrm);
                hit = 1;
                break;
            }
            t = t + d;
            p[0] = fmaf(t, dir[0], origin[0]);
            p[1] = fmaf(t, dir[1], origin[1]);
            p[2] = fmaf(t, dir[2], origin[2]);
        }
        if (geom) {
            float* texel = geom + 4 * k;
            if (hit) {
                texel[0] = nrm[0]; texel[1] = nrm[1]; texel[2] = nrm[2]; texel[3] = t;
            } else {
                texel[0] = 0.0f; texel[1] = 0.0f; texel[2] = 0.0f; texel[3] = INFINITY;
            }
        }
        if (steps_out) steps_out[k] = (uint16_t)(i > 65535 ? 65535 : i);
        if (rgba) {
            float c[3] = {options->background_color[0], options->background_color[1], options->background_color[2]};
            if (hit) { /* entry.wgsl:16-19 as kgr_colour_from_geometry states it */
                const float ndl = (nrm[0] + nrm[1]) + nrm[2];
                const float lo = (ndl < 0.0f) ? 0.0f : ndl;
                const float lit = (1.0f < lo) ? 1.0f : lo;
                const float diffuse = fmaf(0.9f, lit, 0.1f);
                c[0] = diffuse * options->fractal_color[0];
                c[1] = diffuse * options->fractal_color[1];
                c[2] = diffuse * options->fractal_color[2];
            }
            if (options->is_heatmap) { /* entry.wgsl:27-29: the counter as a fraction of max_iterations */
                const float f = (float)i / (float)options->max_iterations;
                c[0] = f * options->fractal_color[0];
                c[1] = f * options->fractal_color[1];
                c[2] = f * options->fractal_color[2];
            }
            uint8_t* px = rgba + 4 * k;
            px[0] = kor_encode_channel(c[0], encode);
            px[1] = kor_encode_channel(c[1], encode);
            px[2] = kor_encode_channel(c[2], encode);
            px[3] = 255;
        }
    }
    return 0;
}
