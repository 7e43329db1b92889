// lasgun_amd/csrc/k_gather.hip -- radiance gathers (include/lasgun_hip.h, lg_radiance_gather*): li() along K shared directions from N poses,
// LEVEL 0 of the level-by-level pipeline (k_wavefront.hip) a third time.  k_radiance.hip is level 0 for rays the caller wrote out; here the
// rays are never written out: ray (i, k) has the origin origins[i] as given and the direction dirs[k] as given, or, with frames, the pose's
// 3 x 3 matrix applied to it -- d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z, f64, in this order, nothing fused (-ffp-contract=off): the
// range scans' rule (k_scan.hip).  The three passes are level0.h's bodies over GatherSource, which says the three things a source says:
//   * the tile -> (pose, direction) mapping (gather_item).  Work item i = tile * 64 + lane of a chunk belongs to tile T = base_tile + tile of
//     the call (a chunk holds whole tiles), and there are two work items (POSE):
//       direction lanes (POSE = false): T = pose * ceil(n_dirs / 64) + block, lane l owns direction 64 block + l.  The origin and the frame are
//         the same address in every lane: the rays of a wave share an origin, like a camera's;
//       pose lanes (POSE = true): T = pose_block * n_dirs + k, lane l owns pose 64 pose_block + l.  The direction is the same address in
//         every lane: without frames the wave walks 64 parallel rays;
//   * the ray: origin + frame x direction (gather_ray);
//   * the finish: (0 + value) * 1.0 at RAY INDEX r = pose * n_dirs + k of an li array -- the caller's radiance plane, or the context's parked
//     buffer until the resolve pass.  Every r is written exactly once, whichever form and however the chunks are cut.
// Levels >= 1 and every shadow pass are the render's own kernels.
//
// gather_resolve_kernel: sums[(i*C + c)*3 + ch] = the sequential sum over k = 0 .. n_dirs-1 of li(i,k)[ch] * W[k*C + c] from +0.0, one f64
// product then one f64 sum a step, nothing fused, a zero weight not skipped.  One lane per (i, c), consecutive lanes consecutive c of one
// pose: the W reads coalesce, the li reads are one address a pose.  No atomics: element (i, c) has one lane.
#include "wflevel.h"
#include "travform.h"
#include "level0.h"

namespace lg {

// work item j of the chunk -> (pose, direction); false: the item stands behind n_dirs (direction lanes) or n_poses (pose lanes)
template <bool POSE> __device__ __forceinline__ bool gather_item(const GatherArgs &Q, unsigned long long j, unsigned long long &pose, unsigned long long &k) {
    const uint32_t T = (uint32_t)(Q.base_tile + (j >> 6)), lane = (uint32_t)j & 63u; // (the call's tiles are counted in 32 bits: gather_host.h)
    const uint32_t hi = T / Q.tiles_per, lo = T - hi * Q.tiles_per;
    if (POSE) { pose = 64ull * hi + lane; k = lo; return pose < Q.n_poses; }
    pose = hi; k = 64ull * lo + lane;
    return k < Q.n_dirs;
}
// the ray of (pose, direction): the direction's bits, or the frame applied in the header's order
__device__ __forceinline__ Ray gather_ray(const GatherArgs &Q, unsigned long long pose, unsigned long long k) {
    const double *po = Q.origins + 3ull * pose, *bk = Q.dirs + 3ull * k;
    const V3 b{bk[0], bk[1], bk[2]};
    if (!Q.frames) return ray_new(V3{po[0], po[1], po[2]}, b); // Ray3::new: the direction as given
    const double *M = Q.frames + 9ull * pose;
    return ray_new(V3{po[0], po[1], po[2]}, V3{(M[0] * b.x + M[1] * b.y) + M[2] * b.z, (M[3] * b.x + M[4] * b.y) + M[5] * b.z, (M[6] * b.x + M[7] * b.y) + M[8] * b.z});
}
// The source: the item is (pose, direction), finished as (0 + value) * 1.0 at RAY INDEX r = pose * n_dirs + k of an li array
template <bool POSE> struct GatherSource {
    const GatherArgs &Q;
    struct Item { unsigned long long pose, k; };
    __device__ __forceinline__ bool work_item(const DParams &, unsigned long long j, Item &it) const { return gather_item<POSE>(Q, j, it.pose, it.k); }
    __device__ __forceinline__ bool tile_item(const DParams &P, uint32_t tile, uint32_t lane, Item &it) const { return work_item(P, (unsigned long long)tile * 64ull + lane, it); }
    __device__ __forceinline__ Ray ray(const DParams &, const Item &it) const { return gather_ray(Q, it.pose, it.k); }
    __device__ __forceinline__ void finish(const DParams &, const Item &it, unsigned long long, V3 value) const { l0_finish_at(Q.li + 3ull * (it.pose * Q.n_dirs + it.k), value); }
};

// W1, W3 and W4 of level 0
template <bool FAST, bool LDSS, bool PRUNE, bool POSE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) gather_closest_kernel(const DParams P, const GatherArgs Q) {
    l0_closest_body<FAST, LDSS, PRUNE>(P, GatherSource<POSE>{Q});
}
template <int KIND, bool POSE> __global__ void __launch_bounds__(LG_BLOCK, 3) gather_shade_kernel(const DParams P, const GatherArgs Q) { l0_shade_body<KIND>(P, GatherSource<POSE>{Q}); }
template <bool POSE> __global__ void __launch_bounds__(LG_BLOCK) gather_combine_kernel(const DParams P, const GatherArgs Q) { l0_combine_body(P, GatherSource<POSE>{Q}); }

// The reduction: one lane per (pose, c), the directions in their order
__global__ void __launch_bounds__(LG_BLOCK) gather_resolve_kernel(const double *li, const double *W, double *sums, unsigned long long n_poses, unsigned long long n_dirs,
                                                                  unsigned long long n_weights) {
    const unsigned long long items = n_poses * n_weights;
    for (unsigned long long g = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; g < items; g += (unsigned long long)gridDim.x * LG_BLOCK) {
        const unsigned long long pose = g / n_weights, c = g - pose * n_weights;
        const double *l = li + 3ull * (pose * n_dirs), *w = W + c;
        V3 acc = vzero();
        for (unsigned long long k = 0; k < n_dirs; ++k, l += 3, w += n_weights) acc = acc + V3{l[0], l[1], l[2]} * w[0];
        double *o = sums + 3ull * g;
        o[0] = acc.x; o[1] = acc.y; o[2] = acc.z;
    }
}

// ---- host-callable launchers (launch.cpp, enqueue_radiance_gather).  The closest pass: the forms and their operations are travform.h's.
// Variants: direction lanes, pose lanes
template <bool F, bool L, bool Z> struct GatherKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(gather_closest_kernel<F, L, Z, false>), reinterpret_cast<const void *>(gather_closest_kernel<F, L, Z, true>)};
        return k[v];
    }
};
hipError_t launch_gather_closest(const DParams &P, const GatherArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<GatherArgs *>(&Q)};
    return trav_launch<GatherKernels>(P, fast, Q.pose_lanes ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t launch_gather_shade(const DParams &P, const GatherArgs &Q, uint32_t blocks, hipStream_t stream) {
    static const L0Kernel<GatherArgs> k[2][2] = {{gather_shade_kernel<0, false>, gather_shade_kernel<0, true>}, {gather_shade_kernel<1, false>, gather_shade_kernel<1, true>}};
    return l0_launch_shade(k, P, Q, Q.pose_lanes != 0u, blocks, stream);
}
hipError_t launch_gather_combine(const DParams &P, const GatherArgs &Q, uint32_t blocks, hipStream_t stream) {
    static const L0Kernel<GatherArgs> k[2] = {gather_combine_kernel<false>, gather_combine_kernel<true>};
    return l0_launch_combine(k, P, Q, Q.pose_lanes != 0u, blocks, stream);
}
hipError_t launch_gather_resolve(const double *li, const double *weights, double *sums, unsigned long long n_poses, unsigned long long n_dirs, unsigned long long n_weights,
                                 uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(gather_resolve_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, li, weights, sums, n_poses, n_dirs, n_weights);
    return hipGetLastError();
}
hipError_t gather_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<GatherKernels>(bytes, ldss); }

} // namespace lg
