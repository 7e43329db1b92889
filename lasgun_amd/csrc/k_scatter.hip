// lasgun_amd/csrc/k_scatter.hip -- surface scatter (include/lasgun_hip.h, lg_scatter*): ONE level of li()'s tree, opened.  For each of the
// caller's rays: lg_intersect's record of its hit, the light and ambient sum there (shade_lights, integrate.rs:47-67), and the two specular
// children with the factors the combine pass multiplies their li by -- what wf_shade_kernel<1, .> / l0_shade_body<1> append to level 1's ray
// queue and park in wf_spec, written instead to the caller's planes at the ray's own index.
//
// It is level 0 of the level-by-level pipeline (level0.h) run as a chain of ONE level, whatever depth the accel was built at:
//   * the closest pass is l0_closest_body over ScatterSource (scatter_source.h, shared with k_lit.hip).  With one level the body finishes a miss through the source, whose finish()
//     writes ALL of a miss's planes; a hit's lg_hit is written there too, through the body's hook (l0_closest_hit), because t, kind, prim
//     and instance are known only in that pass (the parked frame holds p, ng, ns, ss and the material);
//   * the shadow pass is the render's own kernel (wf_trace_kernel, shadow form), unchanged -- that is where the time goes;
//   * scatter_emit_kernel stands where the shade pass stands: one wave per tile of the hit queue, no loop.  It restores the frame as
//     l0_shade_body does, calls shade_lights and both sample_specular_*, applies KIND 1's presence tests and writes the hit's planes.
//     No wave_append, no level-1 arrays, no combine pass: the chain ends here.
// Every element of every plane asked for is written by exactly one lane: a miss's by the closest pass, a hit's `hits` by the closest
// pass and its other planes by the emit pass.
//
// Stores: a ray's planes are AoS rows of 4 .. 96 bytes, up to 284 bytes a ray.  Lane l of a tile writes ray base + l (as given) so a
// wave's 64 rows of a plane are one contiguous piece of 0.25 .. 6 KiB and every cache line of it is filled by the same wave, whatever
// the order of the stores inside a lane (a wave of the hit queue's appended part holds the compacted hits of sparse tiles and writes
// their rows, runs of a few tiles); with the sorted order the rows are the rays' own, scattered as lg_intersect's answers are.
// `hits` is 16-byte aligned by contract and written as six 16-byte stores (k_query.hip); the double planes are 8-byte aligned by contract
// and their rows are 24, 40 or 48 bytes, so they are written as 8-byte stores (a 16-byte store would need 16-byte rows).  No transposing
// through LDS: the emit kernel's lanes hold one ray each and the row is what a lane holds.
#include "wflevel.h"
#include "travform.h"
#include "level0.h"
#include "scatter_source.h"

namespace lg {

static_assert(sizeof(DParams) + sizeof(ScatterArgs) <= 4096, "both are passed by value: a kernel's arguments are at most 4 KB");

// W1: level0.h's closest body over the query's rays
template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) scatter_closest_kernel(const DParams P, const ScatterArgs Q) {
    l0_closest_body<FAST, LDSS, PRUNE>(P, ScatterSource<PERM>{Q});
}

// In the shade pass's place (l0_shade_body<1>, read the two side by side): the grid covers the chunk's dense tiles and the most hits that
// can be appended behind them, one wave per tile, no loop.  The launch bounds are the shade kernels': the body holds the same frame, the
// same two Samples and shade_lights' registers; what it adds is stores.
template <bool PERM>
__global__ void __launch_bounds__(LG_BLOCK, 3) scatter_emit_kernel(const DParams P, const ScatterArgs Q) {
    const HitSlots hs = hit_slots(P, 0u, 64u);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long t = (unsigned long long)blockIdx.x * (LG_BLOCK / 64u) + wave;
    if (t >= hs.tiles) return;
    unsigned long long h = 0;
    if (!hit_of(P, hs, (uint32_t)t, lane, h)) return;
    const unsigned long long j = P.wf_hq[h];
    const unsigned long long r = rq_ray_index<PERM>(Q, Q.base + j);
    const Ray ray = rq_load_ray(Q, r);
    Shade sh;
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
    const V3 output = shade_lights(P, m, sh, vis); // integrate.rs:47-67
    bool has_r = false, has_t = false;
    Sample sr, st;
    if (m.kind == MAT_GLASS || m.kind == MAT_MIRROR) { // integrate.rs:69-77, as at a depth below the maximum
        if (sample_specular_transmission(m, sh, st))
            has_t = !(st.pdf <= 0.0 || veq(st.spectrum, vzero()) || fabs(dot(st.wi, sh.ns)) == 0.0);
        if (sample_specular_reflection(m, sh, sr))
            has_r = !(sr.pdf <= 0.0 || veq(sr.spectrum, vzero()) || dot(sr.wi, sh.ns) <= 0.0);
    }
    if (Q.direct) sc_store3(Q.direct + 3ull * r, output);
    if (Q.flags) Q.flags[r] = SCATTER_HIT | (has_r ? SCATTER_REFLECT : 0u) | (has_t ? SCATTER_REFRACT : 0u);
    V3 wr = vzero(), sr_spectrum = vzero();
    if (has_r) {
        wr = -1.0 * sh.wo + 2.0 * dot(sh.wo, sh.ns) * sh.ns; // bxdf::util::reflect (integrate.rs:100)
        sr_spectrum = sr.spectrum;
    }
    sc_store_reflect(Q, r, has_r, sh.p, wr, sr_spectrum);
    V3 wt = vzero(), st_spectrum = vzero();
    double cosv = 0.0, pdf = 0.0;
    if (has_t) {
        wt = st.wi; st_spectrum = st.spectrum;
        cosv = fabs(dot(st.wi, sh.ns)); pdf = st.pdf;
    }
    sc_store_refract(Q, r, has_t, sh.pm, wt, st_spectrum, cosv, pdf);
}

// ---- host-callable launchers (launch.cpp, enqueue_scatter).  The closest pass: the forms and their operations are travform.h's.
// Variants: PERM (Q.perm != nullptr)
template <bool F, bool L, bool Z> struct ScatterClosestKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(scatter_closest_kernel<F, L, Z, false>), reinterpret_cast<const void *>(scatter_closest_kernel<F, L, Z, true>)};
        return k[v];
    }
};
hipError_t launch_scatter_closest(const DParams &P, const ScatterArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<ScatterArgs *>(&Q)};
    return trav_launch<ScatterClosestKernels>(P, fast, Q.perm ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t launch_scatter_emit(const DParams &P, const ScatterArgs &Q, uint32_t blocks, hipStream_t stream) {
    if (Q.perm) hipLaunchKernelGGL(scatter_emit_kernel<true>, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else hipLaunchKernelGGL(scatter_emit_kernel<false>, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t scatter_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<ScatterClosestKernels>(bytes, ldss); }

} // namespace lg
