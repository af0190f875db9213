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
#include <atomic>

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

    const uint32_t batch = uint32_t(B.count);
    const uint32_t view = batch > 1 ? blockIdx.x % batch : 0u;
    const uint32_t slot = batch > 1 ? blockIdx.x / batch : blockIdx.x;
    const FrameParams P = batch_frame(B, view);
    const int tid = threadIdx.x;
    const bool srgb = (P.encode == 1);
    if (srgb) s_srgb[tid] = P.srgb_table[tid];

    const int wave = tid >> 6, lane = tid & 63;
    const int lx = (wave << 3) | (lane & 7);
    const int ly = lane >> 3;
    const uint32_t tile = P.tile_order[slot];  // scalar load: uniform per workgroup
    const int tile_x = int(tile & 0xffffu) * TILE_W;
    const int tile_y = int(tile >> 16) * TILE_H;        // row offset within the launch's rows
    const int frame_y = tile_frame_row(P, tile >> 16);  // the tile's first frame row
    const int x = tile_x + lx;
    const int y = frame_y + ly;
    const bool valid = (x < P.width) && (y < P.y1);

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
        Texel* const row = reinterpret_cast<Texel*>(P.geom) + size_t(view) * P.geom_stride_texels +
                           size_t(tile_y + ly) * P.geom_pitch_texels;
        const Texel v{n.x, n.y, n.z, t};
#if KIFS_GEOM_NONTEMPORAL
        __builtin_nontemporal_store(v, row + x);
#else
        row[x] = v;
#endif
    }
    __syncthreads();  // s_srgb visible
    uint32_t rgba = P.background_rgba;
    if (!culled) rgba = encode_rgba(colour, srgb, s_srgb);
    s_tile[ly][lx] = rgba;
    __syncthreads();

    // store mapping: thread -> (tid & 31, tid >> 5): linear rows of 128 bytes
    const int sx = tid & (TILE_W - 1), sy = tid >> 5;
    const int ox = tile_x + sx;
    if (ox < P.width && (frame_y + sy) < P.y1)
        P.out[out_row(P, frame_y + sy, tile_y + sy) * P.pitch_words + ox] = s_tile[sy][sx];
}

template <int GROUP, int PRIM>
static hipError_t launch(const BatchParams& B, hipStream_t stream) {
    // the lone frame's residency cap, as kifs::render_kernel's (launch_variant in kifs_kernels.hip)
    const unsigned pad = residency_pad_bytes(B.frame.workgroups_per_cu);
    if (pad > 48 * 1024) {
        static std::atomic<bool> opted_in[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
        if (dev < 0 || dev >= 64 || !opted_in[dev].load(std::memory_order_acquire)) {
            hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&render_kernel<GROUP, PRIM>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
            if (attr != hipSuccess) return attr;
            if (dev >= 0 && dev < 64) opted_in[dev].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(B.frame.tile_count * uint32_t(B.count)), dim3(BLOCK), pad, stream,
                       B);
    return hipGetLastError();
}

}  // namespace geom

hipError_t launch_geometry(const BatchParams& B, uint32_t group, uint32_t primitive, hipStream_t stream) {
    const FrameParams& P = B.frame;
    if (!P.geom || P.ssaa > 1 || P.stripe_rows) return hipErrorInvalidValue;  // (refused by the API before it gets here)
    switch (group) {
    case GROUP_JULIA:  // the short divide / square root by sdf_iters, as launch_render
        return P.sdf_iters <= 24 ? geom::launch<GROUP_JULIA, 1>(B, stream) : geom::launch<GROUP_JULIA, 0>(B, stream);
    case GROUP_GENJULIA: return geom::launch<GROUP_GENJULIA, 0>(B, stream);
    case GROUP_KIFS:
        switch (primitive) {
        case PRIM_SPHERE: return geom::launch<GROUP_KIFS, PRIM_SPHERE>(B, stream);
        case PRIM_CYLINDER: return geom::launch<GROUP_KIFS, PRIM_CYLINDER>(B, stream);
        case PRIM_BOX: return geom::launch<GROUP_KIFS, PRIM_BOX>(B, stream);
        case PRIM_TORUS: return geom::launch<GROUP_KIFS, PRIM_TORUS>(B, stream);
        case PRIM_SIERPINSKI: return geom::launch<GROUP_KIFS, PRIM_SIERPINSKI>(B, stream);
        case PRIM_BUNNY: return geom::launch<GROUP_KIFS, PRIM_BUNNY>(B, stream);  // per-lane bunny_sdf: slow, correct
        default: return geom::launch<GROUP_KIFS, PRIM_OTHER>(B, stream);  // kifs.wgsl:154
        }
    default: return hipErrorInvalidValue;
    }
}

}  // namespace kifs
