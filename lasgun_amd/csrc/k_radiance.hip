// lasgun_amd/csrc/k_radiance.hip -- radiance queries (include/lasgun_hip.h, lg_radiance*): LEVEL 0 of the level-by-level pipeline
// (k_wavefront.hip) for rays the caller supplies instead of the rays a camera generates for a film.
//
// A query is li() of n rays.  These are level 0's three passes (level0.h says what they are and what a source replaces in them) in this
// family's OWN text: rq_closest_body.h, rq_shade_body, rq_combine_body -- the text level0.h's bodies were made from, with the query's slots,
// rays and finish (level0.h: rq_ray_index, rq_load_ray, rq_finish, film_store) written in place:
//   * work item i = tile * 64 + lane of a chunk stands for SLOT s = base + i of the query, active while s < n, and walks
//     ray r = perm ? perm[s] : s (lg_accel_set_query_order(1): the chunks are cut from the sorted order, k_sort.hip);
//   * the ray is read from the caller's AoS buffer in the closest pass and again in the shade pass (wo depends on it);
//   * a finished ray is radiance[3r ..] = (0 + li) * 1.0 (rq_) or pixel slot r of a film (rf_, FilmArgs).
// Why not the shared bodies: measured over them against the parent's library, three alternations in one session, one radiance row and two
// sorted-order film rows were slower by 0.2-0.5 % with ranges that did not overlap (profiles/level0_shared_ab.jsonl), so by the rule set
// for sharing this family keeps its text, and its kernels are the code they were (profiles/level0_shared_kernel_resources_diff.txt).
#include "wflevel.h"
#include "travform.h"
#include "level0.h"

namespace lg {

// W1 of level 0 (wf_trace_kernel<FAST, false, LDSS, true, PRUNE>): rq_closest_body.h, into radiance[] (rq_) or into a film (rf_)
template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) rq_closest_kernel(const DParams P, const RadianceArgs Q) {
#include "rq_closest_body.h"
}
template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) rf_closest_kernel(const DParams P, const FilmArgs Q) {
#include "rq_closest_body.h"
}

// W3 of level 0 (wf_shade_kernel<KIND, true>).  KIND 0: the scene has no recursion at all, li = output + 0 + 0 is the ray's radiance;
// KIND 1: there is a level below, the specular children are appended to its ray queue (integrate.rs:69-77).
// The grid covers the chunk's dense tiles AND the most hits that can be appended behind them, one wave per tile, no loop.
template <int KIND, bool PERM, class ARGS>
__device__ __forceinline__ void rq_shade_body(const DParams &P, const ARGS &Q) {
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
        r = rq_ray_index<PERM>(Q, Q.base + j);
        const Ray ray = rq_load_ray(Q, r);
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
        if (valid) rq_finish(Q, r, output + vzero() + vzero());
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
template <int KIND, bool PERM> __global__ void __launch_bounds__(LG_BLOCK, 3) rq_shade_kernel(const DParams P, const RadianceArgs Q) { rq_shade_body<KIND, PERM>(P, Q); }
template <int KIND, bool PERM> __global__ void __launch_bounds__(LG_BLOCK, 3) rf_shade_kernel(const DParams P, const FilmArgs Q) { rq_shade_body<KIND, PERM>(P, Q); }

// W4 of level 0 (wf_combine_kernel at level 0): li of the query's rays from their children's (integrate.rs:79, 103, 129), finished
template <bool PERM, class ARGS>
__device__ __forceinline__ void rq_combine_body(const DParams &P, const ARGS &Q) {
    const unsigned long long n_work = (unsigned long long)P.ntiles * 64ull;
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    for (unsigned long long j = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; j < n_work; j += (unsigned long long)gridDim.x * LG_BLOCK) {
        if (Q.base + j >= Q.n) continue;
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
        rq_finish(Q, rq_ray_index<PERM>(Q, Q.base + j), value);
    }
}
template <bool PERM> __global__ void __launch_bounds__(LG_BLOCK) rq_combine_kernel(const DParams P, const RadianceArgs Q) { rq_combine_body<PERM>(P, Q); }
template <bool PERM> __global__ void __launch_bounds__(LG_BLOCK) rf_combine_kernel(const DParams P, const FilmArgs Q) { rq_combine_body<PERM>(P, Q); }

// The resolve pass of a ray film of several samples per pixel slot (lg_capture_rays*, samples > 1): every ray's li is parked ray-indexed
// in `li` by the radiance forms above -- so neither the chunks' boundaries nor the sorted order touch it --, and one lane per slot g sums
// li[g*S .. g*S+S) in that order from zero, scales by 1 / S and writes the pixel: integrate.rs:16-20, as wf_resolve_kernel does it.
// (A parked value is (0 + li) * 1: the sum from zero gives the same bits from it as from li itself.)
__global__ void __launch_bounds__(LG_BLOCK) rf_resolve_kernel(const FilmArgs Q, const double *li, unsigned long long slots, uint32_t S) {
    const double weight = 1. / (double)S;
    for (unsigned long long g = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; g < slots; g += (unsigned long long)gridDim.x * LG_BLOCK) {
        const unsigned long long off = Q.offsets ? Q.offsets[g] : g;
        if (off >= Q.npix) continue;
        const double *p = li + 3ull * (g * S);
        V3 color = vzero();
        for (uint32_t s = 0; s < S; ++s, p += 3) color = color + V3{p[0], p[1], p[2]};
        film_store(Q, off, color * weight);
    }
}

// ---- host-callable launchers (launch.cpp, enqueue_radiance).  The closest pass: the forms and their operations are travform.h's.
// Variants: into radiance[] (rq_, a RadianceArgs) / into a film (rf_, a FilmArgs) x PERM (Q.perm != nullptr)
template <bool F, bool L, bool Z> struct ClosestKernels {
    static constexpr int variants = 4;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(rq_closest_kernel<F, L, Z, false>), reinterpret_cast<const void *>(rq_closest_kernel<F, L, Z, true>),
                                   reinterpret_cast<const void *>(rf_closest_kernel<F, L, Z, false>), reinterpret_cast<const void *>(rf_closest_kernel<F, L, Z, true>)};
        return k[v];
    }
};
hipError_t launch_rq_closest(const DParams &P, const RadianceArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<RadianceArgs *>(&Q)};
    return trav_launch<ClosestKernels>(P, fast, Q.perm ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t launch_rf_closest(const DParams &P, const FilmArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<FilmArgs *>(&Q)};
    return trav_launch<ClosestKernels>(P, fast, Q.perm ? 3 : 2, blocks, stack_depth, args, stream);
}
hipError_t launch_rq_shade(const DParams &P, const RadianceArgs &Q, uint32_t blocks, hipStream_t stream) {
    static const L0Kernel<RadianceArgs> k[2][2] = {{rq_shade_kernel<0, false>, rq_shade_kernel<0, true>}, {rq_shade_kernel<1, false>, rq_shade_kernel<1, true>}};
    return l0_launch_shade(k, P, Q, Q.perm != nullptr, blocks, stream);
}
hipError_t launch_rf_shade(const DParams &P, const FilmArgs &Q, uint32_t blocks, hipStream_t stream) {
    static const L0Kernel<FilmArgs> k[2][2] = {{rf_shade_kernel<0, false>, rf_shade_kernel<0, true>}, {rf_shade_kernel<1, false>, rf_shade_kernel<1, true>}};
    return l0_launch_shade(k, P, Q, Q.perm != nullptr, blocks, stream);
}
hipError_t launch_rq_combine(const DParams &P, const RadianceArgs &Q, uint32_t blocks, hipStream_t stream) {
    static const L0Kernel<RadianceArgs> k[2] = {rq_combine_kernel<false>, rq_combine_kernel<true>};
    return l0_launch_combine(k, P, Q, Q.perm != nullptr, blocks, stream);
}
hipError_t launch_rf_combine(const DParams &P, const FilmArgs &Q, uint32_t blocks, hipStream_t stream) {
    static const L0Kernel<FilmArgs> k[2] = {rf_combine_kernel<false>, rf_combine_kernel<true>};
    return l0_launch_combine(k, P, Q, Q.perm != nullptr, blocks, stream);
}
hipError_t launch_rf_resolve(const FilmArgs &Q, const double *li, unsigned long long slots, uint32_t samples, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rf_resolve_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, Q, li, slots, samples);
    return hipGetLastError();
}
hipError_t rq_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<ClosestKernels>(bytes, ldss); }

} // namespace lg
