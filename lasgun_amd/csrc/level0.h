// lasgun_amd/csrc/level0.h -- LEVEL 0 of the level-by-level pipeline (k_wavefront.hip) for rays that are not the scene camera's: the three
// passes as bodies over a SOURCE, for light groups' closest pass (k_light_groups.hip), radiance gathers (k_gather.hip) and view batches
// (k_views.hip); and the slots, rays and finish of a query's rays, which k_radiance.hip and k_light_groups.hip share.
//
// The pipeline's levels >= 1 never knew where level 0's rays came from: they read a ray queue and leave li in a per-level array, so the
// shadow pass of every level, the closest / shade passes of the levels below and every combine above level 0 are the render's own kernels.
// What is welded to the camera in k_wavefront.hip is level 0 -- camera_ray() / pixel_of() / finish_pixel() -- and the bodies below are its
// three passes with exactly that replaced by a source; the walk, the hit queue, the parked frame, wave_append and every f64 expression are
// kept as they are there (read the two side by side; k_wavefront.hip is not touched).  A source is a small struct around the kernel's
// argument struct that says three things and nothing else:
//   * which work item is active, and what it stands for (`Item`): tile_item(P, tile, lane, item) for the closest pass, where the claimed tile
//     is the same in every lane, and work_item(P, j, item) for the shade and combine passes, where a lane's work item j comes from the hit
//     queue or the grid.  Both return whether the item is active;
//   * ray(P, item): the item's ray, in the closest pass and again in the shade pass (wo depends on it; the same expression gives the same
//     bits) -- no transposed copy of the rays, no gather pass over the results;
//   * finish(P, item, j, value): where a finished li goes.
// Each kernel file keeps its __global__ kernels -- names, template parameters and launch bounds as they were -- as one-line calls into the
// bodies.  The bodies were once repeated per family for the register budget of these kernels; measured on the shared form
// (profiles/level0_shared_kernel_resources_diff.txt): every kernel over them keeps its vgpr, sgpr, LDS and workgroup size.  The radiance
// and film kernels (k_radiance.hip) keep the text these bodies were made from: over the bodies three of their rows measured slower
// than the parent's by more than its own spread (profiles/level0_shared_ab.jsonl).  The closest body's prologue and tile loop are what
// tilewalk.h holds for the tiled query kernels, in this file's own text: over the shared header gather, scatter and lit rows measured
// slower than the parent's by more than its spread (profiles/tilewalk_account.md), and the body is one for all its families.
#pragma once
#include "wflevel.h"

namespace lg {

// ---- the rays of a query: slot s of the query is ray r = perm ? perm[s] : s (lg_accel_set_query_order(1): the chunks are cut from the
// sorted order, k_sort.hip), read from the caller's AoS buffer (48 bytes, three 16-byte loads, as k_query.hip reads it)
template <bool PERM> __device__ __forceinline__ unsigned long long rq_ray_index(const RadianceArgs &Q, unsigned long long slot) {
    return PERM ? (unsigned long long)Q.perm[slot] : slot;
}
__device__ __forceinline__ Ray rq_load_ray(const RadianceArgs &Q, unsigned long long r) {
    const double2 *p = reinterpret_cast<const double2 *>(Q.rays + 6ull * r);
    const double2 a = p[0], b = p[1], c = p[2];
    return ray_new(V3{a.x, a.y, b.x}, V3{b.y, c.x, c.y}); // Ray3::new: the direction as given
}
// integrate() for a pixel whose one sample is this ray: Color::zero() + li, then * weight with weight = 1 / 1 (integrate.rs:16-20).
// (The sum is what turns a -0.0 of li into the +0.0 a rendered pixel holds; the product by one is exact.)
__device__ __forceinline__ V3 l0_finished(V3 value) { return (vzero() + value) * 1.0; }
// ... as three doubles at `o`: radiance[3r ..] of a query, and every other array of li that is indexed by the ray
__device__ __forceinline__ void l0_finish_at(double *o, V3 value) {
    const V3 color = l0_finished(value);
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}
__device__ __forceinline__ void rq_finish(const RadianceArgs &Q, unsigned long long r, V3 value) {
    const V3 color = l0_finished(value);
    double *o = Q.radiance + 3ull * r;
    o[0] = color.x; o[1] = color.y; o[2] = color.z;
}
// ... and into a film (FilmArgs, ViewArgs): the same value as one RGBA8 word (to_byte per channel, A = 255; img.rs:46-67, as write_pixel)
// and / or three doubles at the pixel's film offset
template <class FILM> __device__ __forceinline__ void film_store(const FILM &Q, unsigned long long off, V3 color) {
    if (Q.rgba) Q.rgba[off] = to_byte(color.x) | (to_byte(color.y) << 8) | (to_byte(color.z) << 16) | (255u << 24);
    if (Q.rgb) {
        double *o = Q.rgb + 3ull * off;
        o[0] = color.x; o[1] = color.y; o[2] = color.z;
    }
}
// the ray is pixel slot r of one sample; a slot whose offset lies behind the film writes nothing
__device__ __forceinline__ void rq_finish(const FilmArgs &Q, unsigned long long r, V3 value) {
    const unsigned long long off = Q.offsets ? Q.offsets[r] : r;
    if (off >= Q.npix) return;
    film_store(Q, off, l0_finished(value));
}

// A hook of the closest pass for a source that wants the hit itself (k_scatter.hip: t, kind, prim and instance are known only here): called by
// every lane that hit, behind its frame's stores.  Empty for every source that does not overload it for its own type -- their kernels are
// the code they were (profiles/r22_kernel_resources_diff.txt).
template <class SRC> __device__ __forceinline__ void l0_closest_hit(const SRC &, const DParams &, const typename SRC::Item &, const Best &, const Shade &) {}

// W1 of level 0 (wf_trace_kernel<FAST, false, LDSS, true, PRUNE>)
template <bool FAST, bool LDSS, bool PRUNE, class SRC>
__device__ __forceinline__ void l0_closest_body(const DParams &P, const SRC src) {
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
        typename SRC::Item it{};
        const bool active = src.tile_item(P, tile, lane, it);
        Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
        if (active) ray = src.ray(P, it);
        Best b;
        b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
        if (active) walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
        const bool hit = active && b.ref != NO_HIT;
        // ---- this wave's slots in the level's hit queue (wflevel.h: dense where most lanes hit, appended otherwise)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        const uint32_t nhit = (uint32_t)__builtin_popcountll(mask);
        unsigned long long h = i;
        if (nhit < WF_FULL_MIN) {
            P.wf_hq[i] = WF_NONE; // (every lane stands for slot i of the dense part, an active item or not: the chunk's arrays hold whole tiles)
            if (nhit != 0u) {
                uint32_t base_v = 0u;
                if (lane == 0u) base_v = atomicAdd(P.wf_counts + P.wf_levels, nhit);
                h = P.wf_hit_cap + (uint32_t)__builtin_amdgcn_readfirstlane((int)base_v) + lanes_below(mask);
            }
        } else if (!hit) P.wf_hq[i] = WF_NONE; // a hole of a dense block
        if (hit) {
            // A bare work-item index: bit 31 of this word is WF_SKIP to the shadow pass (wflevel.h, hit_of), which would then neither walk the hit nor
            // write its vis word.  i stays below 2^31 because these chunks come from the same ChunkPlan as a render's (launch.cpp: cap_limit,
            // 0x7FFFFFF0 rays for the level-by-level pipeline) -- raise that cap for queries and this store has to mask or flag like k_wavefront.hip's.
            P.wf_hq[h] = (uint32_t)i;
            Shade sh;
            shade_frame(P, ray, b, sh);
            const unsigned long long n = P.wf_hit_stride;
            double *f = P.frame + h;
            f[0 * n] = sh.praw.x; f[1 * n] = sh.praw.y; f[2 * n] = sh.praw.z;
            f[3 * n] = sh.ng.x; f[4 * n] = sh.ng.y; f[5 * n] = sh.ng.z;
            f[6 * n] = sh.ns.x; f[7 * n] = sh.ns.y; f[8 * n] = sh.ns.z;
            f[9 * n] = sh.ss.x; f[10 * n] = sh.ss.y; f[11 * n] = sh.ss.z;
            f[12 * n] = (double)sh.mat;
            l0_closest_hit(src, P, it, b, sh);
        } else if (active) { // integrate.rs:26-28
            const V3 value = background(P, normalize(ray.d));
            if (P.wf_levels == 1u) src.finish(P, it, i, value);
            else {
                const unsigned long long n = P.wf_cap;
                P.wf_out[i] = value.x; P.wf_out[n + i] = value.y; P.wf_out[2 * n + i] = value.z;
                P.wf_child[i] = WF_MISS;
            }
        }
    }
}

// W3 of level 0 (wf_shade_kernel<KIND, true>).  KIND 0: the scene has no recursion at all, li = output + 0 + 0 is the ray's radiance;
// KIND 1: there is a level below, the specular children are appended to its ray queue (integrate.rs:69-77).
// The grid covers the chunk's dense tiles AND the most hits that can be appended behind them, one wave per tile, no loop.
template <int KIND, class SRC>
__device__ __forceinline__ void l0_shade_body(const DParams &P, const SRC src) {
    const HitSlots hs = hit_slots(P, 0u, 64u);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long t = (unsigned long long)blockIdx.x * (LG_BLOCK / 64u) + wave;
    if (t >= hs.tiles) return; // (whole waves stay together: the appends of KIND 1 are wave-wide)
    unsigned long long h = 0;
    const bool valid = hit_of(P, hs, (uint32_t)t, lane, h);
    unsigned long long j = 0;
    typename SRC::Item it{};
    bool has_r = false, has_t = false;
    Sample sr, st;
    Shade sh;
    V3 output = vzero();
    if (valid) {
        j = P.wf_hq[h];
        (void)src.work_item(P, j, it); // (a hit's item is active)
        const Ray ray = src.ray(P, it);
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
        if (valid) src.finish(P, it, j, output + vzero() + vzero());
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

// W4 of level 0 (wf_combine_kernel at level 0): li of the chunk's work items from their children's (integrate.rs:79, 103, 129), finished
template <class SRC>
__device__ __forceinline__ void l0_combine_body(const DParams &P, const SRC src) {
    const unsigned long long n_work = (unsigned long long)P.ntiles * 64ull;
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    for (unsigned long long j = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; j < n_work; j += (unsigned long long)gridDim.x * LG_BLOCK) {
        typename SRC::Item it{};
        if (!src.work_item(P, j, it)) continue;
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
        src.finish(P, it, j, value);
    }
}

// ---- host side: the shade and combine kernel of level 0 that a launch takes.  A family names its kernels once, shade[KIND][variant] and
// combine[variant] (the variant: PERM, POSE); KIND 0 where the scene has no recursion at all.
template <class ARGS> using L0Kernel = void (*)(const DParams, const ARGS);
template <class ARGS> hipError_t l0_launch(L0Kernel<ARGS> kernel, const DParams &P, const ARGS &Q, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
template <class ARGS> hipError_t l0_launch_shade(const L0Kernel<ARGS> (&shade)[2][2], const DParams &P, const ARGS &Q, bool variant, uint32_t blocks, hipStream_t stream) {
    return l0_launch(shade[P.wf_levels == 1u ? 0 : 1][variant ? 1 : 0], P, Q, blocks, stream);
}
template <class ARGS> hipError_t l0_launch_combine(const L0Kernel<ARGS> (&combine)[2], const DParams &P, const ARGS &Q, bool variant, uint32_t blocks, hipStream_t stream) {
    return l0_launch(combine[variant ? 1 : 0], P, Q, blocks, stream);
}

} // namespace lg
