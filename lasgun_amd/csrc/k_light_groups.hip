// lasgun_amd/csrc/k_light_groups.hip -- light groups (include/lasgun_hip.h, lg_radiance_groups*): li() of the caller's rays split by
// subsets of the scene's lights, G planes from ONE chain of walks.
//
// Nothing a walk finds depends on which lights are counted: the closest hit of every level, each hit's specular children and their
// weights, and the shadow pass's visibility word (one bit per light) are the same for every subset.  So the call is k_radiance.hip's
// pipeline -- the caller's rays as level 0, the render's own wf_trace_kernels for the shadow pass of every level and the closest pass of
// the levels below -- and only what SUMS lights carries G planes, at every level: the shade pass (lg_shade_kernel: wf_shade_kernel /
// l0_shade_body with the group loop) and the combine pass (lg_combine_kernel: wf_combine_kernel / l0_combine_body per group).  Plane g is
// what lg_radiance returns on an accel rebuilt with the lights of groups[g].lights alone and, without LG_GROUP_AMBIENT, an ambient
// colour of +0: shade_lights' expression where a light outside the mask is skipped as an invisible one is and P.ambient becomes
// vzero() (the product is still formed).  Each group's additions run in light order from vzero(): groups outside, lights inside, the
// light's term evaluated again per group that names it -- the sums stay in the registers the model holds one in, and a call's cost in
// light terms is the sum of the groups' light counts (per-light groups: about twice a render's).
//
// Where a plane lives (dscene.h, GroupArgs): plane 0 of level d is the pipeline's wf_out, planes 1 .. G-1 the chunk's xout.  The render's
// closest pass writes a miss's background into wf_out alone.  Above the deepest level the miss is marked WF_MISS in wf_child and the
// combine pass hands plane 0 to every group; at the DEEPEST level there is no wf_child, so lg_spread_kernel copies plane 0 of the level's
// rays into the other planes between that level's closest and shade passes (the shade pass then overwrites the hits).
#include "wflevel.h"
#include "travform.h"
#include "level0.h"

namespace lg {

static_assert(sizeof(DLightGroup) == 8 && sizeof(GroupArgs) == sizeof(RadianceArgs) + 24 + 8 * MAX_LIGHT_GROUPS, "GroupArgs: the query, two plane pointers, the count, the table");
static_assert(sizeof(DParams) + sizeof(GroupArgs) <= 4096, "both are passed by value: a kernel's arguments are at most 4 KB");

// integrate() for a pixel whose one sample is this ray, into plane g: radiance[(g*n + r)*3 ..] = (0 + li) * 1.0 (integrate.rs:16-20)
__device__ __forceinline__ void lg_finish(const GroupArgs &Q, unsigned long long r, uint32_t g, V3 value) {
    l0_finish_at(Q.radiance + ((unsigned long long)g * Q.n + r) * 3ull, value);
}
// Level 0's source (level0.h) for the closest pass: work item i = tile * 64 + lane of a chunk stands for SLOT s = Q.base + i of the query,
// active while s < Q.n; the item is the slot, and the ray's index is read where it is used, not carried across the walk.  The finish is a
// ray that missed with no recursion at all: the background belongs to every group.
template <bool PERM> struct GroupRaySource {
    const GroupArgs &Q;
    struct Item { unsigned long long slot; };
    __device__ __forceinline__ bool work_item(const DParams &, unsigned long long j, Item &it) const {
        it.slot = Q.base + j;
        return it.slot < Q.n;
    }
    __device__ __forceinline__ bool tile_item(const DParams &P, uint32_t tile, uint32_t lane, Item &it) const { return work_item(P, (unsigned long long)tile * 64ull + lane, it); }
    __device__ __forceinline__ Ray ray(const DParams &, const Item &it) const { return rq_load_ray(Q, rq_ray_index<PERM>(Q, it.slot)); }
    __device__ __forceinline__ void finish(const DParams &, const Item &it, unsigned long long, V3 value) const {
        const unsigned long long r = rq_ray_index<PERM>(Q, it.slot);
        for (uint32_t g = 0; g < Q.n_groups; ++g) lg_finish(Q, r, g, value);
    }
};
// plane g of a level's li: channel c of ray j at [c * cap + j]
__device__ __forceinline__ double *lg_plane(double *plane0, double *xplanes, unsigned long long cap, uint32_t g) {
    return g == 0u ? plane0 : xplanes + (unsigned long long)(g - 1u) * 3ull * cap;
}
__device__ __forceinline__ void lg_store(double *plane, unsigned long long cap, unsigned long long j, V3 v) {
    plane[j] = v.x; plane[cap + j] = v.y; plane[2 * cap + j] = v.z;
}
__device__ __forceinline__ V3 lg_load(const double *plane, unsigned long long cap, unsigned long long j) { return V3{plane[j], plane[cap + j], plane[2 * cap + j]}; }

// W1 of level 0: level0.h's closest body over the query's rays (the source above writes a finished miss into all G planes)
template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) lg_closest_kernel(const DParams P, const GroupArgs Q) {
    l0_closest_body<FAST, LDSS, PRUNE>(P, GroupRaySource<PERM>{Q});
}

// shade_lights (shade.h, integrate.rs:47-67) for one group: `vis` is the shadow pass's word AND the group's mask -- a light outside the
// mask is skipped exactly as an invisible light is --, `ambient` the scene's or vzero(), `amb_f` BSDF::f towards the normal (no group changes it)
__device__ __forceinline__ V3 lg_shade_group(const DParams &P, const DMaterial &m, const Shade &sh, const WoTerms &wt, const uint32_t vis, const V3 ambient, const V3 amb_f) {
    V3 output = vzero();
    for (uint32_t l = 0; l < P.nlights; ++l) { // integrate.rs:47-66
        if (!((vis >> l) & 1u)) continue;
        const DLight L = P.lights[l];
        const LightTerm t = light_term(L, sh);
        if (t.f_att == 0.0) continue;
        V3 fr = bsdf_f(m, sh, wt, t.wi, t.reflect);
        V3 li_col{L.intensity[0], L.intensity[1], L.intensity[2]};
        output = output + (mul_ew(PI * li_col, fr) * t.wi_dot_n / t.f_att);
    }
    return output + mul_ew(ambient, amb_f); // integrate.rs:67
}

// W3 of every level.  KIND 0: no recursion at all (level 0 alone), li = output + 0 + 0 is finished into the G planes of radiance[];
// KIND 1: a level with a level below, the specular children appended ONCE to its ray queue; KIND 2: the deepest level of a recursive
// scene, li stored for the level above.  L0: the ray is the caller's (PERM: through the sorted order), otherwise the level's queue's.
// Level 0's grid covers the dense tiles and the most hits that can be appended, one wave per tile; deeper levels stride (wf_shade_kernel).
template <int KIND, bool L0, bool PERM>
__global__ void __launch_bounds__(LG_BLOCK, 3) lg_shade_kernel(const DParams P, const GroupArgs Q) {
    static_assert((KIND != 0 || L0) && (KIND != 2 || !L0) && (L0 || !PERM), "KIND 0 is level 0's, KIND 2 a level below it; the sorted order is level 0's");
    const uint32_t level = L0 ? 0u : P.wf_level;
    const HitSlots hs = hit_slots(P, level, 64u);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long t_step = L0 ? ~0ull >> 1 : (unsigned long long)gridDim.x * (LG_BLOCK / 64u);
    for (unsigned long long t = (unsigned long long)blockIdx.x * (LG_BLOCK / 64u) + wave; t < hs.tiles; t += t_step) { // (whole waves stay together: the appends of KIND 1 are wave-wide)
        unsigned long long h = 0;
        const bool valid = hit_of(P, hs, (uint32_t)t, lane, h);
        unsigned long long j = 0, r = 0;
        bool has_r = false, has_t = false;
        Sample sr, st;
        Shade sh;
        DMaterial m;
        if (valid) {
            j = hq_ray(P.wf_hq[h]);
            Ray ray;
            if (L0) {
                r = rq_ray_index<PERM>(Q, Q.base + j);
                ray = rq_load_ray(Q, r);
            } else ray = wf_load_ray(P, j);
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
            m = P.materials[sh.mat];
            if (KIND == 1 && (m.kind == MAT_GLASS || m.kind == MAT_MIRROR)) { // depth < max recursion (integrate.rs:69-77)
                if (sample_specular_transmission(m, sh, st))
                    has_t = !(st.pdf <= 0.0 || veq(st.spectrum, vzero()) || fabs(dot(st.wi, sh.ns)) == 0.0);
                if (sample_specular_reflection(m, sh, sr))
                    has_r = !(sr.pdf <= 0.0 || veq(sr.spectrum, vzero()) || dot(sr.wi, sh.ns) <= 0.0);
            }
        }
        const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
        if (KIND == 1) { // children: consecutive slots of the next level's ray queue per wavefront and kind -- no group changes them
            const uint32_t cr = wave_append(P.wf_counts + level + 1u, has_r);
            const uint32_t ct = wave_append(P.wf_counts + level + 1u, has_t);
            if (valid) {
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
        }
        if (!valid) continue;
        // the G planes of the hit: integrate.rs:47-67 per group
        const uint32_t vis = P.nlights ? P.vis[h] : 0u;
        const WoTerms wt = wo_terms(m, sh, sh.wo);
        const V3 amb_f = bsdf_f(m, sh, wt, sh.ns, bsdf_reflect(sh, sh.wo, sh.ns));
        for (uint32_t g = 0; g < Q.n_groups; ++g) {
            const DLightGroup grp = Q.groups[g];
            const V3 output = lg_shade_group(P, m, sh, wt, vis & grp.lights, (grp.flags & GROUP_AMBIENT) ? P.ambient : vzero(), amb_f);
            if (KIND == 0) lg_finish(Q, r, g, output + vzero() + vzero()); // integrate.rs:79 with no children
            else lg_store(lg_plane(P.wf_out, Q.xout, n, g), n, j, KIND == 2 ? output + vzero() + vzero() : output);
        }
    }
}

// W4 of every level above the deepest: li of the level's rays from their children's, per group (integrate.rs:79, 103, 129); wf_child and
// wf_spec are read once.  A ray that missed (WF_MISS) holds its background in plane 0, which is its value in every group.
// L0: finished into radiance[]; otherwise stored for the level above.
template <bool L0, bool PERM>
__global__ void __launch_bounds__(LG_BLOCK) lg_combine_kernel(const DParams P, const GroupArgs Q) {
    static_assert(L0 || !PERM, "the sorted order is level 0's");
    const unsigned long long n_work = L0 ? (unsigned long long)P.ntiles * 64ull : wf_level_rays(P, P.wf_level);
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    const uint32_t G = Q.n_groups;
    for (unsigned long long j = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; j < n_work; j += (unsigned long long)gridDim.x * LG_BLOCK) {
        if (L0 && Q.base + j >= Q.n) continue;
        const unsigned long long r = L0 ? rq_ray_index<PERM>(Q, Q.base + j) : 0ull;
        const uint32_t c0 = P.wf_child[j];
        if (c0 == WF_MISS) {
            const V3 value = lg_load(P.wf_out, n, j);
            for (uint32_t g = L0 ? 0u : 1u; g < G; ++g) {
                if (L0) lg_finish(Q, r, g, value);
                else lg_store(lg_plane(P.wf_out, Q.xout, n, g), n, j, value);
            }
            continue;
        }
        const uint32_t c1 = P.wf_child[n + j];
        const double *sp = P.wf_spec + j;
        V3 wr = vzero(), wt = vzero();
        double cosv = 0.0, pdf = 0.0;
        if (c0 != WF_NONE) wr = V3{sp[0 * n], sp[1 * n], sp[2 * n]};
        if (c1 != WF_NONE) { wt = V3{sp[3 * n], sp[4 * n], sp[5 * n]}; cosv = sp[6 * n]; pdf = sp[7 * n]; }
        for (uint32_t g = 0; g < G; ++g) {
            double *mine = lg_plane(P.wf_out, Q.xout, n, g);
            const double *below = lg_plane(P.wf_out_next, Q.xout_next, nn, g);
            V3 value = lg_load(mine, n, j);
            V3 reflected = vzero(), refracted = vzero();
            if (c0 != WF_NONE) reflected = mul_ew(wr, lg_load(below, nn, c0)); // integrate.rs:103
            if (c1 != WF_NONE) refracted = mul_ew(wt, lg_load(below, nn, c1)) * cosv / pdf; // integrate.rs:129
            value = value + reflected + refracted; // integrate.rs:79
            if (L0) lg_finish(Q, r, g, value);
            else lg_store(mine, n, j, value);
        }
    }
}

// The deepest level of a recursive scene, between its closest and shade passes: plane 0 of the level's rays (where the render's closest
// pass left every miss's background) into planes 1 .. G-1.  A hit's slot carries whatever plane 0 held; the shade pass overwrites it in every plane.
__global__ void __launch_bounds__(LG_BLOCK) lg_spread_kernel(const DParams P, const GroupArgs Q) {
    const unsigned long long n_work = wf_level_rays(P, P.wf_level), n = P.wf_cap;
    for (unsigned long long j = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; j < n_work; j += (unsigned long long)gridDim.x * LG_BLOCK) {
        const V3 value = lg_load(P.wf_out, n, j);
        for (uint32_t g = 1; g < Q.n_groups; ++g) lg_store(lg_plane(P.wf_out, Q.xout, n, g), n, j, value);
    }
}

// ---- host-callable launchers (launch.cpp, enqueue_radiance_groups).  The closest pass: the forms and their operations are travform.h's.
// Variants: PERM (Q.perm != nullptr)
template <bool F, bool L, bool Z> struct GroupClosestKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(lg_closest_kernel<F, L, Z, false>), reinterpret_cast<const void *>(lg_closest_kernel<F, L, Z, true>)};
        return k[v];
    }
};
hipError_t launch_lg_closest(const DParams &P, const GroupArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<GroupArgs *>(&Q)};
    return trav_launch<GroupClosestKernels>(P, fast, Q.perm ? 1 : 0, blocks, stack_depth, args, stream);
}
// the shade pass of level P.wf_level (level 0: Q's rays)
hipError_t launch_lg_shade(const DParams &P, const GroupArgs &Q, uint32_t blocks, hipStream_t stream) {
    const bool l0 = P.wf_level == 0u;
    if (P.wf_levels == 1u) {
        if (Q.perm) hipLaunchKernelGGL((lg_shade_kernel<0, true, true>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
        else hipLaunchKernelGGL((lg_shade_kernel<0, true, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    } else if (P.wf_level + 1u >= P.wf_levels) hipLaunchKernelGGL((lg_shade_kernel<2, false, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else if (l0) {
        if (Q.perm) hipLaunchKernelGGL((lg_shade_kernel<1, true, true>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
        else hipLaunchKernelGGL((lg_shade_kernel<1, true, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    } else hipLaunchKernelGGL((lg_shade_kernel<1, false, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
// the combine pass of level P.wf_level
hipError_t launch_lg_combine(const DParams &P, const GroupArgs &Q, uint32_t blocks, hipStream_t stream) {
    if (P.wf_level != 0u) hipLaunchKernelGGL((lg_combine_kernel<false, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else if (Q.perm) hipLaunchKernelGGL((lg_combine_kernel<true, true>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else hipLaunchKernelGGL((lg_combine_kernel<true, false>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t launch_lg_spread(const DParams &P, const GroupArgs &Q, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(lg_spread_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t light_groups_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<GroupClosestKernels>(bytes, ldss); }

} // namespace lg
