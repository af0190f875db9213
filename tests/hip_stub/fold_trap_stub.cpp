// fold_trap_stub.cpp -- TEST INFRASTRUCTURE, never shipped: a stand-in for launch_folded_trapped and launch_eval_fold_trap
// (kifs_fold_trap_kernels.hip) for fold_trap_driver.cpp (`make asan-fold-trap`).  It RECORDS what a launch carries -- the
// foldorbit::Params with its frame constants (the driver reads the culls there), THE RECORD'S CONTENTS AS THE COPY LEFT
// THEM AT LAUNCH TIME (read through Params::record, which must be device memory), the pipeline and the stream -- refuses
// what the API must have refused before it got here, and models the launch's stores: every row of every view's band
// receives a word pattern of (view, row, column) in the colour destination and, with a plane, a value per pixel there,
// through need_device, so that a byte outside the caller's arrays aborts.
// fold_trap_stub_fail_next(): the next launch fails once.
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kifs_raymarching_amd/csrc/kifs_internal.hpp"
#include "fold_trap_model.hpp"

namespace {

bool g_fail_next = false;
long g_launches = 0, g_evals = 0;
FoldTrapStubLaunch g_last{};
FoldTrapStubEval g_last_eval{};

void need_device(const void* p, size_t bytes, const char* what) {
    if (!bytes) return;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice ||
        hipPointerGetAttributes(&b, static_cast<const char*>(p) + bytes - 1) != hipSuccess || b.type != hipMemoryTypeDevice) {
        std::fprintf(stderr, "fold_trap_stub: %s touches %zu bytes at %p outside device memory\n", what, bytes, p);
        std::abort();
    }
}

void refuse(const char* what) {
    std::fprintf(stderr, "fold_trap_stub: %s\n", what);
    std::abort();
}

bool finite(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }

// What both launchers must never see of a system or a trap: the API refuses it.
void need_system(const kifs::fold::Fold& F, uint32_t group) {
    const float fv[14] = {F.scale, F.t[0], F.t[1], F.t[2], F.h, F.R[0], F.R[1], F.R[2], F.R[3], F.R[4], F.R[5], F.R[6], F.R[7], F.R[8]};
    for (float v : fv)
        if (!finite(v)) refuse("a fold system with a value that is not finite");
    if (F.stages > 31u || F.iterations < 0 || F.iterations > 24 || !(F.scale >= 1.0f) || !(F.scale <= 16.0f))
        refuse("a fold system outside its ranges");
    if (group != 0u) refuse("a Julia pipeline has no folded form");
}
void need_orbit(const kifs::trap::Trap& T) {
    if (!finite(T.centre.x) || !finite(T.centre.y) || !finite(T.centre.z) || !finite(T.centre.w)) refuse("a trap centre that is not finite");
    if (T.axes < 1u || T.axes > 15u || T.iterations < 0 || T.iterations > 32) refuse("a trap outside its ranges");
}
void need_trap(const kifs::trap::Trap& T) {
    need_orbit(T);
    const float tv[8] = {T.scale, T.bias, T.mid.x, T.mid.y, T.mid.z, T.far.x, T.far.y, T.far.z};
    for (float v : tv)
        if (!finite(v)) refuse("a trap with a value that is not finite");
    for (int i = 2; i < 8; ++i)
        if (!(tv[i] >= 0.0f)) refuse("a negative colour");
}

}  // namespace

extern "C" {
void fold_trap_stub_fail_next() { g_fail_next = true; }
long fold_trap_stub_launches() { return g_launches; }
long fold_trap_stub_evals() { return g_evals; }
}
const FoldTrapStubLaunch& fold_trap_stub_last() { return g_last; }
const FoldTrapStubEval& fold_trap_stub_last_eval() { return g_last_eval; }

namespace kifs {

hipError_t launch_folded_trapped(const foldorbit::Params& O, uint32_t group, uint32_t primitive, hipStream_t stream) {
    ++g_launches;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    const FrameParams& P = O.B.frame;
    // what the API must have refused before it got here
    if (O.B.count < 1 || O.B.count > MAX_BATCH_INLINE || O.B.table) refuse("a count the kernel argument cannot hold");
    if (P.ssaa < 1 || P.ssaa > 4) refuse("a bad supersampling factor");
    if (O.has_ao > 1u) refuse("a flag that is neither 0 nor 1");
    if (O.has_ao && (O.ao.samples < 1 || O.ao.samples > 16 || !(O.ao.step > 0.0f) || !(O.ao.decay > 0.0f) || !(O.ao.decay <= 1.0f) ||
                     !(O.ao.strength >= 0.0f) || !(O.ao.step <= FLT_MAX) || !(O.ao.strength <= FLT_MAX)))
        refuse("a term outside its ranges");
    const light::Light& L = O.light;
    const float lv[11] = {L.direction.x, L.direction.y, L.direction.z, L.unit.x, L.unit.y, L.unit.z, L.ambient, L.diffuse,
                          L.specular.x, L.specular.y, L.specular.z};
    for (float v : lv)
        if (!finite(v)) refuse("a light with a value that is not finite");
    if (!(L.ambient >= 0.0f) || !(L.diffuse >= 0.0f) || !(L.specular.x >= 0.0f) || !(L.specular.y >= 0.0f) || !(L.specular.z >= 0.0f))
        refuse("a negative weight");
    if (L.shininess_log2 < 0 || L.shininess_log2 > 10) refuse("a shininess outside its range");
    if (L.highlight != ((L.specular.x != 0.0f || L.specular.y != 0.0f || L.specular.z != 0.0f) ? 1u : 0u)) refuse("a wrong highlight flag");
    const float u2 = L.unit.x * L.unit.x + L.unit.y * L.unit.y + L.unit.z * L.unit.z;
    if (!(u2 > 0.999f && u2 < 1.001f)) refuse("a unit vector that is none");
    // the record: in device memory, 128 bytes, as the copy on this stream left it
    if (!O.record || (reinterpret_cast<uintptr_t>(O.record) & 15u)) refuse("a null or misaligned record");
    need_device(O.record, sizeof(foldorbit::Record), "the record");
    foldorbit::Record R;
    std::memcpy(&R, O.record, sizeof R);
    need_system(R.fold, group);
    need_trap(R.trap);
    if (R.pad[0] || R.pad[1]) refuse("padding that is not zero");
    if (P.encode != 0 && P.encode != 1) refuse("a bad encode");
    if (P.y0 < 0 || P.y1 <= P.y0 || P.width < 1) refuse("an empty or inverted band");
    if (P.stripe_rows || P.geom || P.tile_cost || P.counters || P.round_steps || P.workgroups_per_cu) refuse("not the fixed launch shape");
    if (!P.tile_order || P.tile_count != uint32_t((P.width + 31) / 32) * uint32_t((P.y1 - P.y0 + 7) / 8)) refuse("not the band's tile table");
    if (P.pitch_words < uint32_t(P.width)) refuse("a colour pitch below the width");
    if (O.plane && (P.ssaa > 1 || (reinterpret_cast<uintptr_t>(O.plane) & 3u) || O.pitch_words < uint32_t(P.width))) refuse("a plane the API refuses");
    need_device(P.srgb_table, 256 * sizeof(float), "the sRGB table");
    need_device(P.tile_order, size_t(P.tile_count) * 4, "the tile order");
    g_last = FoldTrapStubLaunch{O, R, group, primitive, stream};
    const int rows = P.y1 - P.y0;
    for (int v = 0; v < O.B.count; ++v) {
        uint32_t* out = O.B.count > 1 ? O.B.view[v].out : P.out;
        if (!out || (reinterpret_cast<uintptr_t>(out) & 3u)) refuse("a null or misaligned destination");
        for (int r = 0; r < rows; ++r) {
            uint32_t* row = out + size_t(r) * P.pitch_words;
            need_device(row, size_t(P.width) * 4, "a colour row");
            for (int x = 0; x < P.width; ++x)
                row[x] = fold_trap_model::pixel(v, P.y0 + r, x, P.encode, P.ssaa, O.has_ao != 0u, L.shininess_log2, R.fold.iterations, R.trap.iterations);
            if (O.plane) {
                float* prow = O.plane + size_t(v) * O.stride_words + size_t(r) * O.pitch_words;
                need_device(prow, size_t(P.width) * 4, "a row of the plane");
                for (int x = 0; x < P.width; ++x) prow[x] = fold_trap_model::u_of(v, P.y0 + r, x, R.fold.iterations, R.trap.iterations);
            }
        }
    }
    return hipSuccess;
}

// kifs_eval_fold_trap's launch: the scene's constants, the two records, n positions up and the values down.
hipError_t launch_eval_fold_trap(const foldorbit::EvalParams& E, uint32_t group, uint32_t primitive, hipStream_t stream) {
    ++g_evals;
    if (g_fail_next) {
        g_fail_next = false;
        return hipErrorLaunchFailure;
    }
    if (E.n < 1) refuse("an empty evaluation reached the launcher");
    need_system(E.fold, group);
    need_orbit(E.trap);
    need_device(E.points, size_t(E.n) * 12, "the positions");
    need_device(E.u, size_t(E.n) * 4, "the values");
    g_last_eval = FoldTrapStubEval{E, group, primitive, stream};
    for (int i = 0; i < E.n; ++i) E.u[i] = fold_trap_model::eval_of(i, E.fold.iterations, E.trap.iterations) + E.points[3 * i];
    return hipSuccess;
}

}  // namespace kifs
