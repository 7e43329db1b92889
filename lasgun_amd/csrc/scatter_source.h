// lasgun_amd/csrc/scatter_source.h -- level 0's source of surface scatter (k_scatter.hip) and the stores of its planes, shared with lit
// scatter (k_lit.hip), whose source is derived from it: the same rays, the same hit records, the same miss rows of the seven planes.
#pragma once
#include "wflevel.h"
#include "level0.h"

namespace lg {

__device__ __forceinline__ uint4 sc_bits2(double a, double b) {
    const unsigned long long x = (unsigned long long)__double_as_longlong(a), y = (unsigned long long)__double_as_longlong(b);
    return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}
__device__ __forceinline__ void sc_store3(double *o, V3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
__device__ __forceinline__ void sc_store_ray(double *o, V3 origin, V3 d) {
    o[0] = origin.x; o[1] = origin.y; o[2] = origin.z; o[3] = d.x; o[4] = d.y; o[5] = d.z;
}
// the reflected child's planes of ray r, or the +0.0s of an absent one
__device__ __forceinline__ void sc_store_reflect(const ScatterArgs &Q, unsigned long long r, bool has, V3 origin, V3 d, V3 spectrum) {
    if (Q.reflect) sc_store_ray(Q.reflect + 6ull * r, has ? origin : vzero(), has ? d : vzero());
    if (Q.reflect_weight) sc_store3(Q.reflect_weight + 3ull * r, has ? spectrum : vzero());
}
// ... and the transmitted child's: spectrum[3], |wi . ns|, pdf -- the last five doubles of wf_spec
__device__ __forceinline__ void sc_store_refract(const ScatterArgs &Q, unsigned long long r, bool has, V3 origin, V3 d, V3 spectrum, double cosv, double pdf) {
    if (Q.refract) sc_store_ray(Q.refract + 6ull * r, has ? origin : vzero(), has ? d : vzero());
    if (Q.refract_weight) {
        double *o = Q.refract_weight + 5ull * r;
        sc_store3(o, has ? spectrum : vzero());
        o[3] = has ? cosv : 0.0; o[4] = has ? pdf : 0.0;
    }
}

// Level 0's source (level0.h): work item i = tile * 64 + lane of a chunk stands for SLOT s = Q.base + i of the query, active while
// s < Q.n; the item is the slot, and the ray's index is read where it is used.  finish() is a ray that missed: with a chain of one level the
// closest body hands every miss here, and all of its planes are written -- lg_intersect's miss record, the background, no flags, no children.
template <bool PERM> struct ScatterSource {
    const ScatterArgs &Q;
    struct Item { unsigned long long slot; };
    __device__ __forceinline__ bool work_item(const DParams &, unsigned long long j, Item &it) const {
        it.slot = Q.base + j;
        return it.slot < Q.n;
    }
    __device__ __forceinline__ bool tile_item(const DParams &P, uint32_t tile, uint32_t lane, Item &it) const { return work_item(P, (unsigned long long)tile * 64ull + lane, it); }
    __device__ __forceinline__ Ray ray(const DParams &, const Item &it) const { return rq_load_ray(Q, rq_ray_index<PERM>(Q, it.slot)); }
    __device__ __forceinline__ void finish(const DParams &, const Item &it, unsigned long long, V3 value) const {
        const unsigned long long r = rq_ray_index<PERM>(Q, it.slot);
        if (Q.hits) {
            uint4 *out = reinterpret_cast<uint4 *>(Q.hits) + 6ull * r;
            out[0] = sc_bits2(INFINITY, 0.0); out[1] = sc_bits2(0.0, 0.0); out[2] = sc_bits2(0.0, 0.0);
            out[3] = sc_bits2(0.0, 0.0); out[4] = sc_bits2(0.0, 0.0);
            out[5] = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu); // kind 0, prim / instance ~0, material -1
        }
        if (Q.direct) sc_store3(Q.direct + 3ull * r, value); // background(normalize(d)) (integrate.rs:26-28)
        if (Q.flags) Q.flags[r] = 0u;
        sc_store_reflect(Q, r, false, vzero(), vzero(), vzero());
        sc_store_refract(Q, r, false, vzero(), vzero(), vzero(), 0.0, 0.0);
    }
};
// the closest body's hook: lg_intersect's record of a hit (k_query.hip, query_kernel: the same expressions on the same Best and Shade)
template <bool PERM>
__device__ __forceinline__ void l0_closest_hit(const ScatterSource<PERM> &src, const DParams &, const typename ScatterSource<PERM>::Item &it, const Best &b, const Shade &sh) {
    const ScatterArgs &Q = src.Q;
    if (!Q.hits) return;
    uint4 *out = reinterpret_cast<uint4 *>(Q.hits) + 6ull * rq_ray_index<PERM>(Q, it.slot);
    const uint32_t pk = b.ref >> 30, idx = b.ref & PRIM_INDEX_MASK;
    const uint32_t prim = pk == PK_TRIANGLE ? idx - Q.tri_base[b.accel] : idx;
    out[0] = sc_bits2(b.t, sh.praw.x); out[1] = sc_bits2(sh.praw.y, sh.praw.z);
    out[2] = sc_bits2(sh.ng.x, sh.ng.y); out[3] = sc_bits2(sh.ng.z, sh.ns.x); out[4] = sc_bits2(sh.ns.y, sh.ns.z);
    out[5] = make_uint4(pk + 1u, prim, b.accel, (uint32_t)sh.mat); // lg_hit::kind: 1 sphere, 2 box, 3 triangle
}

} // namespace lg
