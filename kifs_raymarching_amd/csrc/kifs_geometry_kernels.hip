// kifs_geometry_kernels.hip -- the geometry output (kifs_render_geometry_async, include/kifs_hip.h): beside the frame's
// RGBA8 pixels, one 16-byte texel (n.x, n.y, n.z, t) per pixel -- whether the primary ray hit, its parameter at the hit
// and the normal the shading used.  Only the kernel holds these values, so only here can they be handed out.
//
//   geom::render_kernel<GROUP, PRIM>  256 threads per 32 x 8 tile of the launch's tile order, exactly as
//                                     kifs::render_kernel takes them: wave w owns 8 x 8 block w and marches its 64 rays
//                                     from start to finish.  The colour goes through the LDS tile as everywhere else;
//                                     the texel is one 16-byte store per lane, straight from registers: the eight lanes
//                                     of a block row write 128 contiguous bytes.
// Tile table, bands, views and order are the plain launch's; a miss -- culled waves included -- stores (0, 0, 0, +inf).
#include "kifs_render_common.hpp"

// The plane is written once and not read by the launch: 1 = non-temporal stores, 0 = plain ones (the default; the
// other form is unmeasured -- DESIGN 5.8).
#ifndef KIFS_GEOM_NONTEMPORAL
#define KIFS_GEOM_NONTEMPORAL 0
#endif

namespace kifs {
namespace geom {

typedef float Texel __attribute__((ext_vector_type(4)));

// (amdgpu_waves_per_eu: as ssaa::render_kernel -- the normal and t held across the encode otherwise cost the Julia
// march its sixth wave per SIMD)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const BatchParams B) {
    __shared__ float s_srgb[256];
    __shared__ uint32_t s_tile[TILE_H][TILE_W];

    const TileFrame F = tile_frame(B, s_srgb);
    const FrameParams& P = F.P;
    const int x = F.x, y = F.y;
    const bool valid = F.valid;

    const bool culled = wave_is_culled(P, x, y, valid);  // wave-uniform

    V3 colour{0.0f, 0.0f, 0.0f};
    V3 n{0.0f, 0.0f, 0.0f};
    float t = __builtin_inff();  // the miss texel: (0, 0, 0, +inf)
    if (!culled && __ballot(valid) != 0ull) {
        bool hit = false;
        const V3 dir = ray_direction(P, x, y);
        colour = raymarch_geometry<GROUP, PRIM>(P, dir, valid, hit, t, n);
    }
    // the texel of pixel (x, y): row y - y0 of view `view`'s plane (rows of a band are packed, as the colour's)
    if (valid) {
        Texel* const row = reinterpret_cast<Texel*>(P.geom) + size_t(F.view) * P.geom_stride_texels +
                           size_t(F.tile_y + F.ly) * P.geom_pitch_texels;
        const Texel v{n.x, n.y, n.z, t};
#if KIFS_GEOM_NONTEMPORAL
        __builtin_nontemporal_store(v, row + x);
#else
        row[x] = v;
#endif
    }
    __syncthreads();  // s_srgb visible
    uint32_t rgba = P.background_rgba;
    if (!culled) rgba = encode_rgba(colour, F.srgb, s_srgb);
    s_tile[F.ly][F.lx] = rgba;
    __syncthreads();
    store_tile(P, F.tile_x, F.tile_y, F.frame_y, s_tile, int(threadIdx.x));
}

template <int GROUP, int PRIM>
static hipError_t launch(const BatchParams& B, hipStream_t stream) {
    // the lone frame's residency cap, as kifs::render_kernel's (launch_variant in kifs_kernels.hip)
    const unsigned pad = residency_pad_bytes(B.frame.workgroups_per_cu);
    if (hipError_t e = ensure_dynamic_lds<&render_kernel<GROUP, PRIM>>(pad); e != hipSuccess) return e;
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(B.frame.tile_count * uint32_t(B.count)), dim3(BLOCK), pad, stream,
                       B);
    return hipGetLastError();
}

}  // namespace geom

hipError_t launch_geometry(const BatchParams& B, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = B.frame;
    if (!P.geom || P.ssaa > 1 || P.stripe_rows) return hipErrorInvalidValue;  // (refused by the API before it gets here)
    // Julia: the short divide / square root by sdf_iters.  The bunny: per-lane bunny_sdf -- slow, correct.
    return dispatch_pipeline<2>(group, primitive, uint32_t(P.sdf_iters <= 24), [&](auto g, auto prim) {
        return geom::launch<decltype(g)::value, decltype(prim)::value>(B, stream);
    });
}

}  // namespace kifs
