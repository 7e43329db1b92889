// lasgun_amd/csrc/k_lit.hip -- lit scatter (include/lasgun_hip.h, lg_scatter_lit*): surface scatter (k_scatter.hip) with the lights of the
// CALL in place of the scene's.  The call brings K point lights -- one table shared by every ray, or a table per ray -- and an ambient
// colour; the scene's own lights and ambient play no part in any plane.  Beside lg_scatter's seven planes there are two more: every
// light's own term of `direct`, and the visibility bits.
//
// Level 0 of the level-by-level pipeline (level0.h) as a chain of ONE level, as k_scatter.hip runs it, with all three passes its own:
//   * the closest pass is l0_closest_body over LitSource, which is ScatterSource (scatter_source.h) with a finish() that also writes a
//     miss's rows of `terms` and `visible`;
//   * the shadow pass, lit_shadow_kernel, is new: the hot path.  Its lights come from the call, and a hit has W = ceil(K / 32) visibility
//     words instead of one.  A work tile is (hit tile t, word w): the 64 hits of tile t of the level's two-part hit queue x the up to 32
//     lights of word w, claimed from the launch's tile counter over hs.tiles * W as id = t * W + w -- the W words of a hit tile are claimed
//     one behind the other, so the waves that walk them read the same frames at about the same time (nothing has been measured for the
//     other order).  A lane loads its hit's p + ng * 2^-36 once, walks one any-hit ray per light of the word and writes ONE word,
//     P.vis[w * P.wf_hit_stride + h]: exactly one lane writes each word.  Shared lights: light k's record is read through an index that is
//     the same in every lane, so it arrives in scalar registers and a tile's 64 shadow rays converge on one point.  Per-ray lights: a lane
//     reads its own ray's 72-byte record at (r * K + k), r from P.wf_hq[h] and the permutation;
//   * lit_emit_kernel stands where scatter_emit_kernel stands.  Its light loop is shade_lights' (shade.h) restated with three differences:
//     the light comes from the call's table, its bit from word k >> 5, and the term is stored where `terms` is asked for.  The children are
//     formed and stored as there.  Restated, not shared: see level0.h on why the project repeats such bodies.
// The skip (Q.skip: `visible` is not asked for): a (hit, light) pair whose term cannot depend on the light being visible is not walked and
// counts as not visible -- light_irrelevant (shade.h) with PI * intensity finite: the term is +-0 in every channel whether the light is
// visible or not, and adding it changes no bit of a sum that starts at +0; or f_att == 0: the emit pass leaves that light out whatever its
// bit.  One wave-uniform test guards all of it; with `visible` asked for every pair is walked.
// Every element of every plane asked for is written by exactly one lane: a miss's by the closest pass, a hit's `hits` by the closest pass
// and its other planes by the emit pass.  No atomics, no pre-fill.
#include "wflevel.h"
#include "travform.h"
#include "level0.h"
#include "scatter_source.h"

namespace lg {

static_assert(sizeof(DParams) + sizeof(LitArgs) <= 4096, "both are passed by value: a kernel's arguments are at most 4 KB");
static_assert(sizeof(DLight) == 72, "a light record is lg_light: 72 bytes");

// Level 0's source: ScatterSource's items and rays; a miss also gets +0.0 in its K rows of `terms` and 0 in its W words of `visible`
template <bool PERM> struct LitSource : ScatterSource<PERM> {
    const LitArgs &L;
    __device__ __forceinline__ void finish(const DParams &P, const typename ScatterSource<PERM>::Item &it, unsigned long long j, V3 value) const {
        ScatterSource<PERM>::finish(P, it, j, value);
        const unsigned long long r = rq_ray_index<PERM>(L, it.slot);
        if (L.terms) {
            double *o = L.terms + 3ull * L.n_lights * r;
            for (uint32_t k = 0; k < 3u * L.n_lights; ++k) o[k] = 0.0;
        }
        if (L.visible) {
            uint32_t *o = L.visible + (unsigned long long)L.vis_words * r;
            for (uint32_t w = 0; w < L.vis_words; ++w) o[w] = 0u;
        }
    }
};
// the closest body's hook: ScatterSource's (the generic empty hook would otherwise be the better match for the derived type)
template <bool PERM>
__device__ __forceinline__ void l0_closest_hit(const LitSource<PERM> &src, const DParams &P, const typename ScatterSource<PERM>::Item &it, const Best &b, const Shade &sh) {
    l0_closest_hit(static_cast<const ScatterSource<PERM> &>(src), P, it, b, sh);
}

// W1: level0.h's closest body over the query's rays
template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) lit_closest_kernel(const DParams P, const LitArgs Q) {
    l0_closest_body<FAST, LDSS, PRUNE>(P, LitSource<PERM>{{Q}, Q});
}

// W2: the shadow pass under the call's lights.  The prologue, the LDS stacks and images and the launch bounds are the shadow form's of
// wf_trace_kernel (k_wavefront.hip, SHADOW branch; read the two side by side), in this file's own text and not over tilewalk.h: over it five
// rows of this family measured slower than the parent's by more than its spread (profiles/tilewalk_account.md).  Q.n_lights >= 1 (the host launches nothing for K == 0).
template <bool FAST, bool LDSS, bool PRUNE, bool PER_RAY>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) lit_shadow_kernel(const DParams P, const LitArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const HitSlots hs = hit_slots(P, 0u, 64u);
    const uint32_t W = Q.vis_words, K = Q.n_lights;
    const uint32_t ntiles = hs.tiles * W; // (fits 32 bits: launch.cpp, WfChunk::run)
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
    const unsigned long long n = P.wf_hit_stride;
    uint32_t band = LDSS ? xcc_id() : 0u, bands_left = TILE_HEADS;
    for (bool final = false; !final;) {
        uint32_t id;
        if (LDSS) id = claim_tile(P.tile_counter, ntiles, band, bands_left, final);
        else id = claim_tile_single(P.tile_counter, ntiles, final);
        if (id == NO_TILE) break;
        const uint32_t tile = id / W, w = id - tile * W; // (the same in every lane)
        unsigned long long h;
        if (!hit_of(P, hs, tile, lane, h)) continue;
        // interaction.p + p_err, recomputed from the parked frame exactly as the emit pass does
        const V3 praw{P.frame[0 * n + h], P.frame[1 * n + h], P.frame[2 * n + h]};
        const V3 ng{P.frame[3 * n + h], P.frame[4 * n + h], P.frame[5 * n + h]};
        const double err = 2.220446049250313e-16 * 65536.0;
        const V3 hit_p = praw + ng * err;
        unsigned long long r = 0;
        if (PER_RAY || Q.skip) r = Q.perm ? (unsigned long long)Q.perm[Q.base + P.wf_hq[h]] : Q.base + P.wf_hq[h];
        const DLight *const row = PER_RAY ? Q.lights + (unsigned long long)K * r : Q.lights;
        const uint32_t k0 = w * 32u, kn = K - k0 < 32u ? K - k0 : 32u;
        // the lights of the word this lane walks: all of them, or (the skip) those whose term can depend on the walk's answer.  Made AHEAD of
        // the walks, so that what light_term reads of the emit pass's frame -- made here by that pass's expressions -- holds no register
        // across them.
        uint32_t todo = kn < 32u ? (1u << kn) - 1u : ~0u;
        if (Q.skip) { // (wave-uniform)
            Shade sh;
            sh.p = hit_p; sh.ng = ng;
            sh.ns = V3{P.frame[6 * n + h], P.frame[7 * n + h], P.frame[8 * n + h]};
            sh.wo = -normalize(rq_load_ray(Q, r).d);
            todo = 0u;
            for (uint32_t k = 0; k < kn; ++k) {
                const DLight L = row[k0 + k];
                const LightTerm t = light_term(L, sh);
                const bool finite = isfinite(PI * L.intensity[0]) && isfinite(PI * L.intensity[1]) && isfinite(PI * L.intensity[2]);
                if (!(t.f_att == 0.0 || (finite && light_irrelevant(t)))) todo |= 1u << k; // otherwise the bit stays 0: the term is left out, or is a zero either way
            }
        }
        uint32_t vis = 0u;
        for (uint32_t k = 0; k < kn; ++k) {
            if (!((todo >> k) & 1u)) continue;
            const DLight *const L = row + (k0 + k);
            const Ray sray = ray_new(hit_p, V3{L->pos[0], L->pos[1], L->pos[2]} - hit_p); // point.rs:43-44
            Best b;
            walk<LDSS, FAST, PRUNE>(P, sray, true, stack, stride, b, scn, cnt, arec);
            if (!(b.t < 1.0)) vis |= 1u << k; // point.rs:49
        }
        P.vis[(unsigned long long)w * n + h] = vis;
    }
}

// In scatter_emit_kernel's place, with its grid and bounds (k_scatter.hip; read the two side by side)
template <bool PERM>
__global__ void __launch_bounds__(LG_BLOCK, 3) lit_emit_kernel(const DParams P, const LitArgs Q) {
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
    // shade_lights (shade.h; integrate.rs:47-67) under the call's lights: the light from the call's table, its bit from word k >> 5, its term stored
    const uint32_t K = Q.n_lights;
    const DLight *const row = Q.per_ray ? Q.lights + (unsigned long long)K * r : Q.lights;
    double *const trow = Q.terms ? Q.terms + 3ull * K * r : nullptr;
    V3 output = vzero();
    const V3 nrm = sh.ns;
    const WoTerms wt = wo_terms(m, sh, sh.wo);
    uint32_t vis = 0u;
    for (uint32_t k = 0; k < K; ++k) { // integrate.rs:47-66
        if ((k & 31u) == 0u) {
            vis = P.vis[(unsigned long long)(k >> 5) * n + h];
            if (Q.visible) Q.visible[(unsigned long long)Q.vis_words * r + (k >> 5)] = vis;
        }
        V3 term = vzero(); // +0.0 where the light's term is not added
        if ((vis >> (k & 31u)) & 1u) {
            const DLight L = row[k];
            const LightTerm lt = light_term(L, sh);
            if (lt.f_att != 0.0) {
                V3 fr = bsdf_f(m, sh, wt, lt.wi, lt.reflect);
                V3 li_col{L.intensity[0], L.intensity[1], L.intensity[2]};
                const V3 added = mul_ew(PI * li_col, fr) * lt.wi_dot_n / lt.f_att;
                output = output + added;
                term = vzero() + added; // (the sum from zero: a -0.0 becomes +0.0, as a single-light group's plane holds it)
            }
        }
        if (trow) sc_store3(trow + 3ull * k, term);
    }
    output = output + mul_ew(V3{Q.ambient[0], Q.ambient[1], Q.ambient[2]}, bsdf_f(m, sh, wt, nrm, bsdf_reflect(sh, sh.wo, nrm))); // integrate.rs:67
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
    V3 wt_dir = vzero(), st_spectrum = vzero();
    double cosv = 0.0, pdf = 0.0;
    if (has_t) {
        wt_dir = st.wi; st_spectrum = st.spectrum;
        cosv = fabs(dot(st.wi, sh.ns)); pdf = st.pdf;
    }
    sc_store_refract(Q, r, has_t, sh.pm, wt_dir, st_spectrum, cosv, pdf);
}

// ---- host-callable launchers (launch.cpp, enqueue_scatter_lit).  The forms and their operations are travform.h's.
// Variants: closest PERM (Q.perm != nullptr); shadow PER_RAY (Q.per_ray != 0)
template <bool F, bool L, bool Z> struct LitClosestKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(lit_closest_kernel<F, L, Z, false>), reinterpret_cast<const void *>(lit_closest_kernel<F, L, Z, true>)};
        return k[v];
    }
};
template <bool F, bool L, bool Z> struct LitShadowKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(lit_shadow_kernel<F, L, Z, false>), reinterpret_cast<const void *>(lit_shadow_kernel<F, L, Z, true>)};
        return k[v];
    }
};
hipError_t launch_lit_closest(const DParams &P, const LitArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<LitArgs *>(&Q)};
    return trav_launch<LitClosestKernels>(P, fast, Q.perm ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t launch_lit_shadow(const DParams &P, const LitArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<LitArgs *>(&Q)};
    return trav_launch<LitShadowKernels>(P, fast, Q.per_ray ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t launch_lit_emit(const DParams &P, const LitArgs &Q, uint32_t blocks, hipStream_t stream) {
    if (Q.perm) hipLaunchKernelGGL(lit_emit_kernel<true>, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else hipLaunchKernelGGL(lit_emit_kernel<false>, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t lit_set_lds_limit(size_t bytes, bool ldss) {
    const hipError_t e = trav_set_lds_limit<LitClosestKernels>(bytes, ldss);
    return e != hipSuccess ? e : trav_set_lds_limit<LitShadowKernels>(bytes, ldss);
}

} // namespace lg
