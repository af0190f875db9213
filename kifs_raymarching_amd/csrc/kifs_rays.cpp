// kifs_rays.cpp -- the host side of ray queries (kifs_trace_rays_async, include/kifs_hip.h): validate, fill the frame
// constants the SCENE needs -- options, iteration counts, extensions, the bounding radius' cull constant -- without a
// screen or a camera, and launch rays::trace_render_kernel (kifs_rays_kernels.hip), one ray per lane.  It is not a render
// launch: no tile table, no feedback, no profiling record, and the kifs_debug_last_* values stay as they were.
#include "kifs_context.hpp"

namespace kifs {
namespace rays {

// fill_params reads the context's screen, camera and supersampling factor; a ray query reads none of them.  For the
// length of the fill the context holds a 1 x 1 screen, a camera at the origin with the identity matrix and factor 1,
// and gets its own back at the end, set or not (as anim::OptionsOfFrame0 does for the options).
struct NoCamera {
    kifs_ctx* c;
    KifsScreenUniform screen;
    KifsCameraUniform camera;
    int supersampling;
    explicit NoCamera(kifs_ctx* ctx) : c(ctx), screen(ctx->screen), camera(ctx->camera), supersampling(ctx->supersampling) {
        c->screen = KifsScreenUniform{1.0f, 1.0f, 1.0f};
        c->camera = KifsCameraUniform{};
        for (int k = 0; k < 3; ++k) c->camera.matrix[k][k] = 1.0f;
        c->supersampling = 1;
    }
    ~NoCamera() {
        c->screen = screen;
        c->camera = camera;
        c->supersampling = supersampling;
    }
    NoCamera(const NoCamera&) = delete;
    NoCamera& operator=(const NoCamera&) = delete;
};

static int fill(kifs_ctx* c, int encode, Params* R) {
    FrameParams& P = R->frame;
    {
        NoCamera scope(c);
        if (const int st = host::fill_params(c, &P); st != KIFS_OK) return st;
    }
    // nothing derived from a camera: the wave and tile exits assume one origin, the ray queue a tile
    P.quick_cull_n2 = 0.0f;
    P.tile_cull_beta = 0.0f;
    P.tile_cull_sqrtk = 0.0f;
    P.round_steps = 0;
    P.counters = nullptr;
    P.encode = encode;
    return KIFS_OK;
}

}  // namespace rays
}  // namespace kifs

extern "C" int kifs_trace_rays_async(kifs_ctx* c, void* hip_stream, const KifsRay* dev_rays, int n, float* dev_geometry,
                                     uint8_t* dev_rgba8, int encode) {
    using namespace kifs;
    static_assert(sizeof(KifsRay) == 32, "a ray record is two 16-byte rows");
    static_assert((long long)KIFS_MAX_RAYS * 32 > 0 && KIFS_MAX_RAYS / 256 * 256 == KIFS_MAX_RAYS, "the grid of the largest call");
    if (!c) return KIFS_ERR_BAD_ARG;
    if (n < 0 || n > KIFS_MAX_RAYS) return KIFS_ERR_BAD_ARG;
    if (!dev_rays || (reinterpret_cast<uintptr_t>(dev_rays) & 15u) != 0) return KIFS_ERR_BAD_ARG;
    if (!dev_geometry && !dev_rgba8) return KIFS_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(dev_geometry) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dev_rgba8) & 3u) != 0)
        return KIFS_ERR_BAD_ARG;
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    if (!c->have_options) return KIFS_ERR_UNCONFIGURED;
    if (n == 0) return KIFS_OK;
    host::DeviceGuard g(c->device);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    rays::Params R{};
    if (const int st = rays::fill(c, encode, &R); st != KIFS_OK) return st;
    R.rays = reinterpret_cast<const float*>(dev_rays);
    R.n = n;
    R.geom = dev_geometry;
    R.rgba = reinterpret_cast<uint32_t*>(dev_rgba8);
    return host::hip_ok(launch_trace_rays(R, c->options.fractal_group_id, c->options.primitive_id, s), "launch(trace_rays)")
               ? KIFS_OK : KIFS_ERR_RUNTIME;
}
