// accumulate_driver_common.hpp -- TEST INFRASTRUCTURE: what the four drivers of the accumulated calls share
// (accumulate_driver.cpp, accumulate_jitter_driver.cpp, progressive_driver.cpp, converge_driver.cpp): the hooks of
// hip_stub.cpp and accumulate_family_stub.cpp, and the helpers that make a scene, cameras, options, cells and a context
// and restate a view and a scene record for the model.  Included AFTER the driver defines CHECK: the helpers' checks
// count as the driver's.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "../../include/kifs_hip.h"
#include "accumulate_model.hpp"

extern "C" {
void stub_fail_in(long n);
long stub_calls();
long stub_launches();
long stub_stream_waits();
long stub_event_synchronizes();
size_t stub_live_device_allocations();
size_t stub_live_streams_and_events();
void family_stub_fail_next();
void family_stub_expect_grid(int grid);
long family_stub_launches();  // of any kind
long family_stub_carries();
long family_stub_converges();
}
// what the last launch that was not made to fail carried: any launch's, a carried pass's, a converging pass's
const kifs::accum::Params& family_stub_last_params();
const std::vector<kifs::anim::SceneView>& family_stub_last_scenes();
const kifs::accum::CarryParams& family_stub_last_carry();
const kifs::accum::ConvergeParams& family_stub_last_converge();

struct Scene {
    KifsScreenUniform screen;
    KifsOptionsUniform options;
    int w, h;
};

inline Scene scene(int w, int h, uint8_t bg) {
    Scene s{};
    s.w = w;
    s.h = h;
    CHECK(kifs_host_screen(uint32_t(w), uint32_t(h), &s.screen) == KIFS_OK);
    KifsGuiData gui;
    kifs_host_gui_default(&gui);
    gui.fractal_group = 1;  // Julia
    gui.background_color[0] = bg;
    CHECK(kifs_host_options(&gui, &s.options) == KIFS_OK);
    return s;
}

inline std::vector<KifsCameraUniform> cameras(int n, int first) {
    std::vector<KifsCameraUniform> out(static_cast<size_t>(n), KifsCameraUniform{});
    for (int i = 0; i < n; ++i) {
        KifsCameraData c;
        kifs_host_camera_default(&c);
        c.origin_distance = 3.0f + 0.25f * float((first + i) % 7);
        c.phi = 0.37f * float(first + i);
        c.theta = 0.2f * float((first + i) % 5) - 0.4f;
        CHECK(kifs_host_camera(&c, &out[size_t(i)]) == KIFS_OK);
    }
    return out;
}

// Option images that differ where they may: constant, power and both colours (`fourth`: the constant's w too).
inline std::vector<KifsOptionsUniform> morph(const KifsOptionsUniform& base, int n, bool fourth = false) {
    std::vector<KifsOptionsUniform> out(static_cast<size_t>(n), base);
    for (int i = 0; i < n; ++i) {
        KifsOptionsUniform& o = out[size_t(i)];
        o.constant[0] += 0.01f * float(i);
        if (fourth) o.constant[3] -= 0.02f * float(i % 9);
        o.power = 2.0f + 0.125f * float(i % 16);
        o.fractal_color[1] = 0.25f + 0.001f * float(i);
        o.background_color[2] = 0.002f * float(i);
    }
    return out;
}

// Cells that differ from view to view (`corner`: and view 1 in the grid's far corner).
inline std::vector<KifsSubpixel> cells_for(int views, int g, bool corner = true) {
    std::vector<KifsSubpixel> out(static_cast<size_t>(views));
    for (int v = 0; v < views; ++v) out[size_t(v)] = KifsSubpixel{uint8_t((5 * v + 2) % g), uint8_t((g - 1 - (3 * v) % g))};
    if (corner && views > 1) out[1] = KifsSubpixel{uint8_t(g - 1), uint8_t(g - 1)};
    return out;
}

inline uint8_t* dev_alloc(size_t bytes) {
    void* p = nullptr;
    CHECK(hipMalloc(&p, bytes) == hipSuccess);
    return static_cast<uint8_t*>(p);
}

inline kifs_ctx* context_for(const Scene& s, bool with_options) {
    int st = 0;
    kifs_ctx* c = kifs_create(0, &st);
    CHECK(c && st == KIFS_OK);
    CHECK(kifs_set_screen(c, &s.screen) == KIFS_OK);
    if (with_options) CHECK(kifs_set_options(c, &s.options) == KIFS_OK);
    return c;
}

inline kifs::BatchView view_of(const KifsCameraUniform& cam) {
    kifs::BatchView v{};
    v.origin = {cam.origin[0], cam.origin[1], cam.origin[2]};
    v.m0 = {cam.matrix[0][0], cam.matrix[0][1], cam.matrix[0][2]};
    v.m1 = {cam.matrix[1][0], cam.matrix[1][1], cam.matrix[1][2]};
    v.m2 = {cam.matrix[2][0], cam.matrix[2][1], cam.matrix[2][2]};
    return v;
}

inline kifs::anim::SceneView scene_of(const KifsOptionsUniform& o) {
    kifs::anim::SceneView s{};
    s.c = {o.constant[0], o.constant[1], o.constant[2], o.constant[3]};
    s.power = o.power;
    s.fractal_color = {o.fractal_color[0], o.fractal_color[1], o.fractal_color[2]};
    s.background_color = {o.background_color[0], o.background_color[1], o.background_color[2]};
    return s;
}
