// lasgun_amd/csrc/k_gather.hip -- radiance gathers (include/lasgun_hip.h, lg_radiance_gather*): li() along K shared directions from N poses,
// LEVEL 0 of the level-by-level pipeline (k_wavefront.hip) a third time.  k_radiance.hip is level 0 for rays the caller wrote out; here the
// rays are never written out: ray (i, k) has the origin origins[i] as given and the direction dirs[k] as given, or, with frames, the pose's
// 3 x 3 matrix applied to it -- d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z, f64, in this order, nothing fused (-ffp-contract=off): the
// range scans' rule (k_scan.hip).  The three passes are k_radiance.hip's radiance forms (and rq_closest_body.h) with exactly three things
// replaced -- read them side by side:
//   * "slot base + i is active while < n" by the tile -> (pose, direction) mapping (gather_item).  Work item i = tile * 64 + lane of a chunk
//     belongs to tile T = base_tile + tile of the call (a chunk holds whole tiles), and there are two work items (POSE):
//       direction lanes (POSE = false): T = pose * ceil(n_dirs / 64) + block, lane l owns direction 64 block + l.  The origin and the frame are
//         the same address in every lane: the rays of a wave share an origin, like a camera's;
//       pose lanes (POSE = true): T = pose_block * n_dirs + k, lane l owns pose 64 pose_block + l.  The direction is the same address in
//         every lane: without frames the wave walks 64 parallel rays;
//   * rq_load_ray by origin + frame x direction (gather_ray), in the closest pass and again in the shade pass (wo depends on it; the same
//     expression gives the same bits);
//   * rq_finish writing (0 + value) * 1.0 at RAY INDEX r = pose * n_dirs + k of an li array (gather_finish) -- the caller's radiance plane,
//     or the context's parked buffer until the resolve pass.  Every r is written exactly once, whichever form and however the chunks are cut.
// The walk, the hit queue, the parked frame, wave_append and every f64 expression are kept as they are there; levels >= 1 and every shadow
// pass are the render's own kernels.  The bodies are repeated, not shared: the radiance and film kernels sit at their register budget and
// compile to exactly what they were before this file existed (profiles/r16_kernel_resources_diff.txt).
//
// gather_resolve_kernel: sums[(i*C + c)*3 + ch] = the sequential sum over k = 0 .. n_dirs-1 of li(i,k)[ch] * W[k*C + c] from +0.0, one f64
// product then one f64 sum a step, nothing fused, a zero weight not skipped.  One lane per (i, c), consecutive lanes consecutive c of one
// pose: the W reads coalesce, the li reads are one address a pose.  No atomics: element (i, c) has one lane.
#include "wflevel.h"
#include "travform.h"

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
// integrate() for a pixel whose one sample is this ray (k_radiance.hip, rq_finish), at the ray's index of li
__device__ __forceinline__ void gather_finish(const GatherArgs &Q, unsigned long long r, V3 value) {
    const V3 color = (vzero() + value) * 1.0;
    double *o = Q.li + 3ull * r;
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}

// W1 of level 0: rq_closest_body.h with the three replacements
template <bool FAST, bool LDSS, bool PRUNE, bool POSE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) gather_closest_kernel(const DParams P, const GatherArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ntiles = P.ntiles;
    if (ntiles == 0u) return; // (uniform: before the LDS copy and its barrier)
    uint32_t *stack = lds_stack + tid;
    constexpr uint32_t stride = LDSS ? LG_LDSS_BLOCK : LG_BLOCK;
    const uint4 *scn = nullptr;
    if (LDSS) {
        uint4 *dst = reinterpret_cast<uint4 *>(lds_stack + P.stack_depth * stride);
        copy_to_lds(dst, reinterpret_cast<const uint4 *>(P.lds_image), P.lds_image_n16, tid, stride);
        __syncthreads(); // the only workgroup-wide step; every wave reaches it before pulling tiles
        scn = dst;
    }
    const uint4 *const arec = (LDSS || FAST) ? nullptr : load_accel_image(P, P.stack_depth * LG_BLOCK);
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    if (!wave_has_work(ntiles)) return;
    uint32_t band = LDSS ? xcc_id() : 0u, bands_left = TILE_HEADS;
    for (bool final = false; !final;) {
        uint32_t tile;
        if (LDSS) tile = claim_tile(P.tile_counter, ntiles, band, bands_left, final);
        else tile = claim_tile_single(P.tile_counter, ntiles, final);
        if (tile == NO_TILE) break;
        const unsigned long long i = (unsigned long long)tile * 64ull + lane; // the chunk's work item: index of level 0's arrays
        unsigned long long pose = 0, k = 0;
        const bool active = gather_item<POSE>(Q, i, pose, k);
        Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
        if (active) ray = gather_ray(Q, pose, k);
        Best b;
        b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
        if (active) walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
        const bool hit = active && b.ref != NO_HIT;
        // ---- this wave's slots in the level's hit queue (wflevel.h: dense where most lanes hit, appended otherwise)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        const uint32_t nhit = (uint32_t)__builtin_popcountll(mask);
        unsigned long long h = i;
        if (nhit < WF_FULL_MIN) {
            P.wf_hq[i] = WF_NONE; // (every lane stands for slot i of the dense part, a ray or a slot of no ray: the chunk's arrays hold whole tiles)
            if (nhit != 0u) {
                uint32_t base_v = 0u;
                if (lane == 0u) base_v = atomicAdd(P.wf_counts + P.wf_levels, nhit);
                h = P.wf_hit_cap + (uint32_t)__builtin_amdgcn_readfirstlane((int)base_v) + lanes_below(mask);
            }
        } else if (!hit) P.wf_hq[i] = WF_NONE; // a hole of a dense block
        if (hit) {
            P.wf_hq[h] = (uint32_t)i; // a bare index below 2^31, as in rq_closest_body.h: the chunks come from the same ChunkPlan
            Shade sh;
            shade_frame(P, ray, b, sh);
            const unsigned long long n = P.wf_hit_stride;
            double *f = P.frame + h;
            f[0 * n] = sh.praw.x; f[1 * n] = sh.praw.y; f[2 * n] = sh.praw.z;
            f[3 * n] = sh.ng.x; f[4 * n] = sh.ng.y; f[5 * n] = sh.ng.z;
            f[6 * n] = sh.ns.x; f[7 * n] = sh.ns.y; f[8 * n] = sh.ns.z;
            f[9 * n] = sh.ss.x; f[10 * n] = sh.ss.y; f[11 * n] = sh.ss.z;
            f[12 * n] = (double)sh.mat;
        } else if (active) { // integrate.rs:26-28
            const V3 value = background(P, normalize(ray.d));
            if (P.wf_levels == 1u) gather_finish(Q, pose * Q.n_dirs + k, value);
            else {
                const unsigned long long n = P.wf_cap;
                P.wf_out[i] = value.x; P.wf_out[n + i] = value.y; P.wf_out[2 * n + i] = value.z;
                P.wf_child[i] = WF_MISS;
            }
        }
    }
}

// W3 of level 0: rq_shade_body with the ray made again from the hit's work item
template <int KIND, bool POSE>
__global__ void __launch_bounds__(LG_BLOCK, 3) gather_shade_kernel(const DParams P, const GatherArgs Q) {
    const HitSlots hs = hit_slots(P, 0u, 64u);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long t = (unsigned long long)blockIdx.x * (LG_BLOCK / 64u) + wave;
    if (t >= hs.tiles) return; // (whole waves stay together: the appends of KIND 1 are wave-wide)
    unsigned long long h = 0;
    const bool valid = hit_of(P, hs, (uint32_t)t, lane, h);
    unsigned long long j = 0, r = 0;
    bool has_r = false, has_t = false;
    Sample sr, st;
    Shade sh;
    V3 output = vzero();
    if (valid) {
        j = P.wf_hq[h];
        unsigned long long pose = 0, k = 0;
        (void)gather_item<POSE>(Q, j, pose, k); // (a hit's item is active)
        r = pose * Q.n_dirs + k;
        const Ray ray = gather_ray(Q, pose, k);
        const unsigned long long n = P.wf_hit_stride;
        const double *f = P.frame + h;
        V3 p{f[0 * n], f[1 * n], f[2 * n]};
        sh.ng = V3{f[3 * n], f[4 * n], f[5 * n]};
        sh.ns = V3{f[6 * n], f[7 * n], f[8 * n]};
        sh.ss = V3{f[9 * n], f[10 * n], f[11 * n]};
        sh.mat = (int32_t)f[12 * n];
        sh.wo = -normalize(ray.d);
        const double err = 2.220446049250313e-16 * 65536.0;
        V3 p_err = sh.ng * err;
        sh.praw = p; sh.p = p + p_err; sh.pm = p - p_err;
        sh.ts = cross(sh.ns, sh.ss);
        const DMaterial m = P.materials[sh.mat];
        const uint32_t vis = P.nlights ? P.vis[h] : 0u;
        output = shade_lights(P, m, sh, vis); // integrate.rs:47-67
        if (KIND == 1 && (m.kind == MAT_GLASS || m.kind == MAT_MIRROR)) { // depth < max recursion (integrate.rs:69-77)
            if (sample_specular_transmission(m, sh, st))
                has_t = !(st.pdf <= 0.0 || veq(st.spectrum, vzero()) || fabs(dot(st.wi, sh.ns)) == 0.0);
            if (sample_specular_reflection(m, sh, sr))
                has_r = !(sr.pdf <= 0.0 || veq(sr.spectrum, vzero()) || dot(sr.wi, sh.ns) <= 0.0);
        }
    }
    if (KIND == 0) { // integrate.rs:79 with no children
        if (valid) gather_finish(Q, r, output + vzero() + vzero());
        return;
    }
    // children: consecutive slots of level 1's ray queue per wavefront and kind
    const uint32_t cr = wave_append(P.wf_counts + 1u, has_r);
    const uint32_t ct = wave_append(P.wf_counts + 1u, has_t);
    if (!valid) return;
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    P.wf_out[j] = output.x; P.wf_out[n + j] = output.y; P.wf_out[2 * n + j] = output.z;
    P.wf_child[j] = has_r ? cr : WF_NONE;
    P.wf_child[n + j] = has_t ? ct : WF_NONE;
    double *sp = P.wf_spec + j;
    if (has_r) {
        sp[0 * n] = sr.spectrum.x; sp[1 * n] = sr.spectrum.y; sp[2 * n] = sr.spectrum.z;
        const V3 wr = -1.0 * sh.wo + 2.0 * dot(sh.wo, sh.ns) * sh.ns; // bxdf::util::reflect (integrate.rs:100)
        double *q = P.wf_q_next + cr;
        q[0 * nn] = sh.p.x; q[1 * nn] = sh.p.y; q[2 * nn] = sh.p.z; q[3 * nn] = wr.x; q[4 * nn] = wr.y; q[5 * nn] = wr.z;
    }
    if (has_t) {
        sp[3 * n] = st.spectrum.x; sp[4 * n] = st.spectrum.y; sp[5 * n] = st.spectrum.z;
        sp[6 * n] = fabs(dot(st.wi, sh.ns)); sp[7 * n] = st.pdf;
        double *q = P.wf_q_next + ct;
        q[0 * nn] = sh.pm.x; q[1 * nn] = sh.pm.y; q[2 * nn] = sh.pm.z; q[3 * nn] = st.wi.x; q[4 * nn] = st.wi.y; q[5 * nn] = st.wi.z;
    }
}

// W4 of level 0: rq_combine_body over the chunk's work items
template <bool POSE>
__global__ void __launch_bounds__(LG_BLOCK) gather_combine_kernel(const DParams P, const GatherArgs Q) {
    const unsigned long long n_work = (unsigned long long)P.ntiles * 64ull;
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    for (unsigned long long j = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; j < n_work; j += (unsigned long long)gridDim.x * LG_BLOCK) {
        unsigned long long pose = 0, k = 0;
        if (!gather_item<POSE>(Q, j, pose, k)) continue;
        V3 value{P.wf_out[j], P.wf_out[n + j], P.wf_out[2 * n + j]};
        const uint32_t c0 = P.wf_child[j];
        if (c0 != WF_MISS) {
            const uint32_t c1 = P.wf_child[n + j];
            const double *sp = P.wf_spec + j;
            V3 reflected = vzero(), refracted = vzero();
            if (c0 != WF_NONE) {
                const V3 l{P.wf_out_next[c0], P.wf_out_next[nn + c0], P.wf_out_next[2 * nn + c0]};
                reflected = mul_ew(V3{sp[0 * n], sp[1 * n], sp[2 * n]}, l); // integrate.rs:103
            }
            if (c1 != WF_NONE) {
                const V3 l{P.wf_out_next[c1], P.wf_out_next[nn + c1], P.wf_out_next[2 * nn + c1]};
                refracted = mul_ew(V3{sp[3 * n], sp[4 * n], sp[5 * n]}, l) * sp[6 * n] / sp[7 * n]; // integrate.rs:129
            }
            value = value + reflected + refracted; // integrate.rs:79
        }
        gather_finish(Q, pose * Q.n_dirs + k, value);
    }
}

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
    if (P.wf_levels == 1u) {
        if (Q.pose_lanes) hipLaunchKernelGGL((gather_shade_kernel<0, true>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
        else hipLaunchKernelGGL((gather_shade_kernel<0, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    } else {
        if (Q.pose_lanes) hipLaunchKernelGGL((gather_shade_kernel<1, true>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
        else hipLaunchKernelGGL((gather_shade_kernel<1, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    }
    return hipGetLastError();
}
hipError_t launch_gather_combine(const DParams &P, const GatherArgs &Q, uint32_t blocks, hipStream_t stream) {
    if (Q.pose_lanes) hipLaunchKernelGGL((gather_combine_kernel<true>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else hipLaunchKernelGGL((gather_combine_kernel<false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t launch_gather_resolve(const double *li, const double *weights, double *sums, unsigned long long n_poses, unsigned long long n_dirs, unsigned long long n_weights,
                                 uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(gather_resolve_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, li, weights, sums, n_poses, n_dirs, n_weights);
    return hipGetLastError();
}
hipError_t gather_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<GatherKernels>(bytes, ldss); }

} // namespace lg
