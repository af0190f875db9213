// kifs_animation_kernels.hip -- animated batches (kifs_render_animation_async, include/kifs_hip.h): the frames of one
// launch differ not only in camera but in the Julia constant, the power and the two colours -- a morph, rendered with the
// long rays of all its frames side by side as kifs_render_batch_async renders an orbit.
//
//   anim::render_kernel<GROUP, PRIM>  256 threads per 32 x 8 tile of the launch's tile order, exactly as
//                                     kifs::render_kernel takes them: wave w owns 8 x 8 block w and marches its 64 rays
//                                     from start to finish.  What is new is the view's SCENE: a 64-byte record per view in
//                                     a device table (c, power, the colours, the encoded background), read with scalar
//                                     loads -- the view index is workgroup-uniform -- and laid over the launch's frame
//                                     constants before anything uses them.
// Cameras and destinations travel as in every batch: inline in the kernel argument up to MAX_BATCH_INLINE views, through
// the context's view-table ring beyond.  Tile table, bands and order are the plain launch's.
// The entry point's host side is kifs_animation.cpp; it reaches the kernel through launch_animation_render at the end of
// this file (kifs_internal.hpp).
#include "kifs_render_common.hpp"

namespace kifs {
namespace anim {

// View `view`'s scene over its frame constants.  The table is read through the constant address space, as batch_frame
// reads a view table: the index is uniform, so these are scalar loads like the kernel argument's own.
__device__ __forceinline__ void overlay_scene(FrameParams& P, const SceneView* scenes, uint32_t view) {
    typedef const SceneView __attribute__((address_space(4))) * ConstScene;
    const ConstScene s = (ConstScene)(scenes + view);
    P.c = V4{s->c.x, s->c.y, s->c.z, s->c.w};
    P.power = s->power;
    P.fractal_color = V3{s->fractal_color.x, s->fractal_color.y, s->fractal_color.z};
    P.background_color = V3{s->background_color.x, s->background_color.y, s->background_color.z};
    P.background_rgba = s->background_rgba;
}

// (amdgpu_waves_per_eu: as geom::render_kernel)
template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void render_kernel(const Params A) {
    __shared__ float s_srgb[256];
    __shared__ uint32_t s_tile[TILE_H][TILE_W];

    TileFrame F = tile_frame(A.B, s_srgb);  // (the prologue reads no field of the scene)
    overlay_scene(F.P, A.scenes, F.view);
    const FrameParams& P = F.P;

    const bool culled = wave_is_culled(P, F.x, F.y, F.valid);  // wave-uniform

    V3 colour{0.0f, 0.0f, 0.0f};
    if (!culled && __ballot(F.valid) != 0ull) {
        int steps = 0;
        const V3 dir = ray_direction(P, F.x, F.y);
        colour = raymarch<GROUP, PRIM>(P, dir, F.valid, steps);
    }
    __syncthreads();  // s_srgb visible
    uint32_t rgba = P.background_rgba;  // the view's own
    if (!culled) rgba = encode_rgba(colour, F.srgb, s_srgb);
    s_tile[F.ly][F.lx] = rgba;
    __syncthreads();
    store_tile(P, F.tile_x, F.tile_y, F.frame_y, s_tile, int(threadIdx.x));
}

template <int GROUP, int PRIM>
static hipError_t launch(const Params& A, hipStream_t stream) {
    hipLaunchKernelGGL((render_kernel<GROUP, PRIM>), dim3(A.B.frame.tile_count * uint32_t(A.B.count)), dim3(BLOCK), 0, stream, A);
    return hipGetLastError();
}

}  // namespace anim

hipError_t launch_animation_render(const anim::Params& A, uint32_t group, uint32_t primitive, hipStream_t stream) {
    // Julia: the short divide / square root by sdf_iters; the doubled orbit trip is the throughput kernels' only.
    // The bunny: per-lane bunny_sdf -- slow, correct.
    return dispatch_pipeline<2>(group, primitive, uint32_t(A.B.frame.sdf_iters <= 24), [&](auto g, auto prim) {
        return anim::launch<decltype(g)::value, decltype(prim)::value>(A, stream);
    });
}

}  // namespace kifs
