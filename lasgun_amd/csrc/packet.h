// lasgun_amd/csrc/packet.h -- the packet form of the plain exact walk over the pair image: the 64 rays of a wave walked with ONE
// cursor, ONE stack and ONE slot counter, all scalar; a lane keeps its ray and its best hit and nothing else.  Used by the level-0 closest
// launch of the level-by-level pipeline where it passes the gate (packet_host.h, launch.cpp) and by nothing else.  (The shadow pass in this
// form was measured and not kept: DESIGN.md 3.5.)
//
// Why it is the reference's walk for every lane: in the plain exact walk nothing depends on best.t but the accept of a primitive -- no node
// is culled by t -- so a lane's visit sequence is fixed by its box-test outcomes and by dir_is_neg[axis] at each interior node.  The wave is
// split into groups of lanes with the same (sign triple of dinv, plain or not); within a group dir_is_neg is the group's, the packet visits
// the tree in that one order, and a lane takes part at a record exactly when every ancestor of the record was hit by it.  Restricted to
// one lane the packet's sequence of (leaf, slot) tests is that lane's own: every box tested at most once, every primitive against the
// best.t the lane would have had, ties first-come.  Groups run one after the other; a lane belongs to one.
//
// A nested accel (the gate admits trees that are a single root record, entered from the root accel) is handled in place, under the mask
// of the slot: door probe, local ray, root record, the lone-mesh rule, the one leaf -- per-lane expressions, the ones traverse_ref uses.
#pragma once
#include "walk.h"

namespace lg {

__device__ __forceinline__ uint32_t pk_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); } // (a value every lane holds)

// Called by EVERY lane of the wave in wave-uniform control flow; `active`: this lane has a ray.  `wstack`: the wave's slice of the LDS stacks
// (entry e at wstack + e * stride, 16 bytes of it used: the typed word and the 64-bit lane mask); the host checked its depth (packet_host.h).
template <bool REL>
__device__ __forceinline__ void packet_walk(const DParams &P, const Ray &wray, const bool active, uint32_t *wstack, const uint32_t stride, Best &best,
                                            const uint4 *scn) {
    best.t = INFINITY; best.ref = NO_HIT; best.accel = 0;
    const uint4 *const arec = scn + P.lds_accel_off;
    const char *const img = reinterpret_cast<const char *>(scn);
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 info0 = lds_u4(arec + 6u);
    const uint32_t root_base = pk_uniform(info0.x), root_flags = pk_uniform(info0.w);
    Ray ray = wray; // the root accel's local ray (bvh.rs:462)
    if (!((root_flags & AF_IDENTITY) && ray_plain(wray))) ray = accel_local_ray<true>(P, arec, 0u, wray);
    const double dd = dot(ray.d, ray.d), four_a = 4.0 * dd;
    const uint32_t key = neg_mask_x(ray); // dir_is_neg (bvh.rs:463), + SIGNS_NOT_PLAIN
    uint32_t sp = 0u;
    unsigned long long m = 0ull; // the lanes for which the current record is reachable
    uint32_t word = 0u;          // the current typed word: a pair record's offset, or PAIR_LEAF | slots
    auto lane_of = [&](const unsigned long long mask) { return ((mask >> lane) & 1ull) != 0ull; };
    auto push = [&](const uint32_t w, const unsigned long long mask) __attribute__((always_inline)) {
        if (lane == 0u) *reinterpret_cast<uint4 *>(wstack + sp * stride) = uint4{w, (uint32_t)mask, (uint32_t)(mask >> 32), 0u};
        ++sp;
    };
    // the next pending (word, mask); false: the stack is empty.  (No lane ever leaves a closest-hit walk: an entry's mask is as it was pushed, never empty.)
    auto pop = [&]() __attribute__((always_inline)) {
        if (sp == 0u) { m = 0ull; return false; }
        --sp;
        __builtin_amdgcn_wave_barrier();
        const uint4 e = lds_u4(reinterpret_cast<const uint4 *>(wstack + sp * stride));
        word = pk_uniform(e.x);
        m = (unsigned long long)pk_uniform(e.y) | ((unsigned long long)pk_uniform(e.z) << 32);
        return true;
    };
    // node 0 of accel level `base` (its root record) for this lane's ray `r` (bvh.rs:472-473); the level's word comes back in `w`
    auto root_hit = [&](const uint32_t base, const Ray &r, uint32_t &w) __attribute__((always_inline)) {
        const char *rec = img + base;
        const double2 a = lds_d2(rec), b = lds_d2(rec + 16), c = lds_d2(rec + 32);
        w = *reinterpret_cast<const uint32_t *>(rec + PAIR_ROOT_WORD_OFF);
        const double bmin[3] = {a.x, a.y, b.x}, bmax[3] = {b.y, c.x, c.y};
        return REL ? slab_intersects_nc_rel(bmin, bmax, r) : slab_intersects_nc(bmin, bmax, r);
    };
    // one sphere or cuboid slot of accel `accel` for the lanes `go`, whose ray at that level is r (dd_, fa_ its dot(d, d) and 4 * that)
    auto prim_slot = [&](const uint32_t ref, const uint32_t slot, const Ray &r, const double dd_, const double fa_, const uint32_t accel, const bool go) __attribute__((always_inline)) {
        const uint4 *q = scn + (P.lds_soup_off + slot * 3u);
        const LeafRec g{lds_u4(q), lds_u4(q + 1), lds_u4(q + 2)};
        if (go) {
            double t = 0.0;
            bool accepted = false;
            if (ref < (1u << 30)) accepted = sphere_slot_accept<REL>(g, r, dd_, fa_, best.t, t);
            else { // PK_CUBOID
                double mn[3] = {rec_f64(g.a.x, g.a.y), rec_f64(g.a.z, g.a.w), rec_f64(g.b.x, g.b.y)};
                double mx[3] = {rec_f64(g.b.z, g.b.w), rec_f64(g.c.x, g.c.y), rec_f64(g.c.z, g.c.w)};
                V3 d0, d1;
                if (cuboid_hit<false>(mn, mx, r, t, d0, d1)) accepted = !(t >= best.t);
            }
            if (accepted) { best.t = t; best.ref = ref; best.accel = accel; }
        }
    };
    // the single fat leaf of mesh accel `mid` for the lanes `go`, whose ray in the mesh is r
    auto mesh_level = [&](const uint32_t mid, const Ray &r, bool go) __attribute__((always_inline)) {
        const uint4 info = lds_u4(arec + (mid * LDS_ACCEL_UNITS + 6u));
        const uint32_t base = pk_uniform(info.x), soup_delta = pk_uniform(info.z);
        uint32_t w;
        const bool hit = root_hit(base, r, w);
        go = go && hit;
        w = pk_uniform(w);
        const uint32_t li = w & PAIR_SLOT_MAX, le = li + ((w >> PAIR_SLOT_BITS) & PAIR_COUNT_MAX);
        if (go) {
            const TriSetup tri = tri_setup(r); // per fat leaf (triangle.rs:186-201)
            bool tie = false;
            Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            const LeafCull lc{INFINITY, INFINITY, 0.0, 0u, 0.0f, 0.0f, 0.0f};
            if (tri.kz == 0) mesh_leaf2<0, true>(P, scn, r, tri, li, le, soup_delta, mid, false, false, best, tie, cnt, lc);
            else if (tri.kz == 1) mesh_leaf2<1, true>(P, scn, r, tri, li, le, soup_delta, mid, false, false, best, tie, cnt, lc);
            else mesh_leaf2<2, true>(P, scn, r, tri, li, le, soup_delta, mid, false, false, best, tie, cnt, lc);
        }
    };
    // A slot of the root accel that is nested accel `idx` (wave-uniform), for the lanes `go`: what traverse_ref's ST_ENTER block and the
    // walk of a level that is one root record come to -- the probe at the door, the local ray, the lone-mesh rule, node 0, the leaf.
    auto nested = [&](const uint32_t idx, bool go) __attribute__((always_inline)) {
        if ((P.level_door & LEVEL_DOOR_PROBE) && door_shut<true>(P, arec, idx, ray)) go = false;
        if (__builtin_amdgcn_ballot_w64(go) == 0ull) return;
        const uint4 info = lds_u4(arec + (idx * LDS_ACCEL_UNITS + 6u));
        const uint32_t base = pk_uniform(info.x), flags = pk_uniform(info.w);
        const bool same = (flags & AF_IDENTITY) != 0u && ray_plain(ray);
        Ray r1 = ray;
        if (go && !same) r1 = accel_local_ray<true>(P, arec, idx, ray);
        if (flags & AF_MESH) { mesh_level(idx, r1, go); return; }
        uint32_t lone = NO_HIT;
        if (P.level_door & LEVEL_DOOR_LONE) lone = pk_uniform(lds_u4(arec + (idx * LDS_ACCEL_UNITS + 7u)).z);
        // the group and its lone mesh as one level: the lanes whose local ray is plain (the mesh's entry keeps it)
        const bool as_one = lone != NO_HIT && ray_plain(r1);
        bool go_mesh = go && as_one, go_group = go && !as_one;
        Ray rm = r1;
        if (__builtin_amdgcn_ballot_w64(go_group) != 0ull) { // the group as a level of its own: node 0, then its leaf's slots in order[]
            uint32_t w;
            const bool hit = root_hit(base, r1, w);
            go_group = go_group && hit;
            w = pk_uniform(w);
            const uint32_t li = w & PAIR_SLOT_MAX, le = li + ((w >> PAIR_SLOT_BITS) & PAIR_COUNT_MAX);
            const double dd1 = dot(r1.d, r1.d), fa1 = 4.0 * dd1;
            for (uint32_t s = li; s < le; ++s) {
                const uint32_t ref = pk_uniform(load_primref<true>(P, scn, s));
                if (ref >= (3u << 30)) { // the group's one slot, its lone mesh (packet_host.h), entered as a level: probe, local ray; its leaf below
                    const uint32_t mesh = ref & PRIM_INDEX_MASK;
                    bool in2 = go_group;
                    if ((P.level_door & LEVEL_DOOR_PROBE) && door_shut<true>(P, arec, mesh, r1)) in2 = false;
                    const uint32_t mflags = pk_uniform(lds_u4(arec + (mesh * LDS_ACCEL_UNITS + 6u)).w);
                    const bool same2 = (mflags & AF_IDENTITY) != 0u && ray_plain(r1);
                    if (in2 && !same2) rm = accel_local_ray<true>(P, arec, mesh, r1);
                    go_mesh = go_mesh || in2;
                    lone = mesh;
                } else prim_slot(ref, s, r1, dd1, fa1, idx, go_group);
            }
        }
        if (lone != NO_HIT && __builtin_amdgcn_ballot_w64(go_mesh) != 0ull) mesh_level(lone, rm, go_mesh);
    };

    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    while (todo != 0ull) { // one octant group at a time
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)__builtin_ctzll(todo));
        const unsigned long long group = __builtin_amdgcn_ballot_w64(active && key == k);
        todo &= ~group;
        const uint32_t sg = (P.boxes_finite && k < SIGNS_NOT_PLAIN) ? k : SIGNS_NOT_PLAIN, negbits = k & 7u;
        sp = 0u;
        {
            uint32_t w;
            const bool hit = root_hit(root_base, ray, w);
            m = __builtin_amdgcn_ballot_w64(hit) & group;
            word = pk_uniform(w);
        }
        // interior nodes (bvh.rs:471-505): pair trips until the current word is a leaf's, or the group has nothing pending
        auto node_trips = [&](auto sgc) __attribute__((always_inline)) {
            constexpr int SG = decltype(sgc)::value;
            do {
                // one pair record through a wave-uniform address: both children's boxes, their words, 1 << split axis
                const char *rec = img + word;
                const double2 a0 = lds_d2(rec), a1 = lds_d2(rec + 16), a2 = lds_d2(rec + 32), b0 = lds_d2(rec + 48), b1 = lds_d2(rec + 64), b2 = lds_d2(rec + 80);
                const uint4 w = lds_u4(reinterpret_cast<const uint4 *>(rec + PAIR_WORDS_OFF));
                const double amin[3] = {a0.x, a0.y, a1.x}, amax[3] = {a1.y, a2.x, a2.y}, bmin[3] = {b0.x, b0.y, b1.x}, bmax[3] = {b1.y, b2.x, b2.y};
                unsigned long long ma, mb;
                if (SG < 8) {
                    // the two comparisons of the test voted on one by one: a vote on a comparison is the comparison's own lane mask,
                    // a vote on their conjunction is rebuilt from a register (two more vector instructions per box)
                    double tx, ty, tz, an, af, bn, bf;
                    if (REL) { slab_sg_rel_t<SG & 7>(amin, amax, ray, an, af); slab_sg_rel_t<SG & 7>(bmin, bmax, ray, bn, bf); }
                    else { slab_sg_t<SG & 7>(amin, amax, ray, tx, ty, tz, an, af); slab_sg_t<SG & 7>(bmin, bmax, ray, tx, ty, tz, bn, bf); }
                    ma = __builtin_amdgcn_ballot_w64(!(an > af)) & __builtin_amdgcn_ballot_w64(!(af <= 0.0)) & m;
                    mb = __builtin_amdgcn_ballot_w64(!(bn > bf)) & __builtin_amdgcn_ballot_w64(!(bf <= 0.0)) & m;
                } else {
                    bool hit_a, hit_b;
                    if (REL) { hit_a = slab_intersects_nc_rel(amin, amax, ray); hit_b = slab_intersects_nc_rel(bmin, bmax, ray); }
                    else { hit_a = slab_intersects_nc(amin, amax, ray); hit_b = slab_intersects_nc(bmin, bmax, ray); }
                    ma = __builtin_amdgcn_ballot_w64(hit_a) & m; mb = __builtin_amdgcn_ballot_w64(hit_b) & m;
                }
                const uint32_t wa = pk_uniform(w.x), wb = pk_uniform(w.y), axis = pk_uniform(w.z);
                const bool neg = ((SG < 8 ? (uint32_t)SG : negbits) & axis) != 0u; // dir_is_neg[axis] (bvh.rs:496): the group's
                const uint32_t near_w = neg ? wb : wa, far_w = neg ? wa : wb;
                const unsigned long long near_m = neg ? mb : ma, far_m = neg ? ma : mb;
                if (near_m != 0ull) {
                    if (far_m != 0ull) push(far_w, far_m); // (bvh.rs:493-504)
                    word = near_w; m = near_m;
                } else if (far_m != 0ull) { word = far_w; m = far_m; }
                else if (!pop()) break;
            } while ((int32_t)word >= 0);
        };
        while (m != 0ull) {
            if ((int32_t)word >= 0) {
                switch (sg) {
                case 0u: node_trips(IntC<0>{}); break;
                case 1u: node_trips(IntC<1>{}); break;
                case 2u: node_trips(IntC<2>{}); break;
                case 3u: node_trips(IntC<3>{}); break;
                case 4u: node_trips(IntC<4>{}); break;
                case 5u: node_trips(IntC<5>{}); break;
                case 6u: node_trips(IntC<6>{}); break;
                case 7u: node_trips(IntC<7>{}); break;
                default: node_trips(IntC<8>{}); break;
                }
                if (m == 0ull) break;
            }
            // leaf primitives in order[] sequence (bvh.rs:481-488): the slot, and with it the primitive's kind, is the wave's
            const uint32_t li = word & PAIR_SLOT_MAX, le = li + ((word >> PAIR_SLOT_BITS) & PAIR_COUNT_MAX);
            const bool in = lane_of(m);
            for (uint32_t s = li; s < le; ++s) {
                const uint32_t ref = pk_uniform(load_primref<true>(P, scn, s));
                if (ref >= (3u << 30)) nested(ref & PRIM_INDEX_MASK, in);
                else prim_slot(ref, s, ray, dd, four_a, 0u, in);
            }
            if (!pop()) break;
        }
    }
}

} // namespace lg
