// kifs_rays_kernels.hip -- ray queries (kifs_trace_rays_async, include/kifs_hip.h): the march, the shading and the
// geometry texel of every other entry point, for rays the CALLER supplies instead of the pixels of a pinhole camera.
//
//   rays::trace_render_kernel<GROUP, PRIM>  256 threads, one ray per lane, ceil(n / 256) workgroups; lanes at or beyond
//                                           n are invalid, as out-of-frame lanes are elsewhere.  A lane loads its ray
//                                           with two 16-byte loads, stores its texel with one (1 KB contiguous per
//                                           wave) and its pixel as one dword.
// The origin is PER LANE: the march is generic_loop of kifs_scene.hpp on a copy of the frame constants whose origin is
// the lane's (vector registers), for every pipeline -- the Julia set too, through the plain scene_sdf<GROUP_JULIA, ...>
// eval_points_kernel uses: the hand-written Julia loop keeps its origin in pinned scalars and has no place here (the two
// Julia slots of dispatch_pipeline<2> therefore hold the same code).  Shading is shade_hit, which depends on the hit
// position only.  The wave and tile culls assume one origin and do not apply; the ray-level cull does, in a form that
// holds for any direction length (never_inside below); generic_loop's own per-step test is sign-only.
#include "kifs_render_common.hpp"

namespace kifs {
namespace rays {

typedef float Row __attribute__((ext_vector_type(4)));

// ray_never_inside of kifs_scene.hpp for any origin and a direction of any length, zero included: the closest approach
// of the ray's line, c^2 = |o|^2 - (o.d)^2 / |d|^2, exceeds K = cull_n2  <=>  (|o|^2 - K) |d|^2 > (o.d)^2 while the ray
// approaches (o.d < 0); a ray that does not approach -- or stands still -- stays outside iff it starts there.  The
// rounding of this arithmetic is a few ulps of |o|^2, and K keeps 1.5 % and more over the radius it certifies
// (fill_params, julia_culls), so the test is made only for |o|^2 <= 1024, where that is below 1e-3; a ray from further
// away is simply marched.  A comparison with a NaN is false: such a ray is marched too.
KIFS_DEV bool never_inside(const FrameParams& P, V3 o, V3 d) {
    const float oo = dot(o, o), od = dot(o, d), dd = dot(d, d);
    const float room = oo - P.cull_n2;
    const bool never = (od < 0.0f) ? (room * dd > od * od) : (room > 0.0f);
    return never && (oo <= 1024.0f);
}

// The kernel argument again, through a pointer the compiler cannot see through (as accum::reloaded): what only the
// shading and the stores read is then loaded behind the march instead of being held in SGPRs across it -- held, it cost
// the bunny, whose estimate streams its weights through scalar registers, 13 parked SGPRs.
typedef const Params __attribute__((address_space(4))) * ConstParams;
__device__ __forceinline__ const Params& reloaded(ConstParams kp) {
    asm volatile("" : "+s"(kp));
    return *(const Params*)kp;
}

template <int GROUP, int PRIM>
__global__ __launch_bounds__(BLOCK) void trace_render_kernel(const Params R) {
    __shared__ float s_srgb[256];
    const ConstParams kp = (ConstParams)__builtin_amdgcn_kernarg_segment_ptr();  // = &R
    constexpr int NPRIM = GROUP == GROUP_JULIA ? 0 : PRIM;  // (Julia: the PRIM slot is not a primitive)
    const FrameParams& P = R.frame;
    const int tid = threadIdx.x;
    const bool colours = R.rgba != nullptr;  // uniform, and so is the barrier below
    const bool srgb = (P.encode == 1);
    if (colours && srgb) s_srgb[tid] = P.srgb_table[tid];

    const size_t k = size_t(blockIdx.x) * BLOCK + size_t(tid);
    const bool valid = k < size_t(R.n);
    Row ro{0.0f, 0.0f, 0.0f, 0.0f}, rd{0.0f, 0.0f, 0.0f, 0.0f};  // an invalid lane: a ray that stands still at the origin
    if (valid) {
        const Row* const rec = reinterpret_cast<const Row*>(R.rays) + 2 * k;
        ro = rec[0];
        rd = rec[1];
    }
    const V3 origin{ro.x, ro.y, ro.z}, dir{rd.x, rd.y, rd.z};
    FrameParams L = P;  // the frame constants with this lane's origin: what generic_loop reads
    L.origin = origin;

    float t = 0.0f;
    V3 p = origin;
    bool hit = false;
    int trips = 0;  // == the loop counter i of entry.wgsl:11 for every marching lane
    int i_final = 0;
    bool marching = valid && (0 < P.max_iterations) && (0.0f < P.max_distance);
    if (P.is_heatmap == 0u && P.cull_n2 > 0.0f) marching = marching && !never_inside(P, origin, dir);
    generic_loop(L, dir, t, p, hit, marching, trips, i_final, P.max_iterations,
                 [&](V3 q, unsigned long long lanes) { return scene_sdf<GROUP, NPRIM>(P, q, lanes); });
    __builtin_amdgcn_s_setprio(0);

    const Params& S = reloaded(kp);
    const FrameParams& Q = S.frame;
    V3 n{0.0f, 0.0f, 0.0f};
    float t_hit = __builtin_inff();  // the miss texel: (0, 0, 0, +inf)
    const V3 colour = whole_ray_colour(Q, hit, i_final, [&] {
        t_hit = t;
        return shade_hit<GROUP, PRIM>(Q, p, &n);
    });
    if (valid && S.geom) reinterpret_cast<Row*>(S.geom)[k] = Row{n.x, n.y, n.z, t_hit};
    if (S.rgba != nullptr) {
        __syncthreads();  // s_srgb visible
        if (valid) S.rgba[k] = encode_rgba(colour, Q.encode == 1, s_srgb);
    }
}

template <int GROUP, int PRIM>
static hipError_t launch(const Params& R, hipStream_t stream) {
    static_assert(RAYS_PER_WORKGROUP == uint32_t(BLOCK), "one ray per lane");
    hipLaunchKernelGGL((trace_render_kernel<GROUP, PRIM>), dim3(workgroups(R.n)), dim3(BLOCK), 0, stream, R);
    return hipGetLastError();
}

}  // namespace rays

hipError_t launch_trace_rays(const rays::Params& R, uint32_t group, uint32_t primitive, hipStream_t stream) {
    if (!R.rays || R.n < 1 || (!R.geom && !R.rgba)) return hipErrorInvalidValue;  // (refused by the API before it gets here)
    return dispatch_pipeline<2>(group, primitive, uint32_t(R.frame.sdf_iters <= 24), [&](auto g, auto prim) {
        return rays::launch<decltype(g)::value, decltype(prim)::value>(R, stream);
    });
}

}  // namespace kifs
