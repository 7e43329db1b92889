// lasgun_amd/csrc/k_nearest.hip -- proximity queries (include/lasgun_hip.h, lg_nearest*): for each of the caller's points, under a radius of
// its own, the k nearest primitives in ascending (d2, key) order, how many primitives lie within the radius at all, and whether any does.
// A candidate is lg_closest_points' own -- one per primitive, closest_prim.h's arithmetic through k_closest.hip's closest_candidate --, so
// the answer is the brute force's over ALL primitives, bit for bit, and slot 0 under a shared radius is lg_closest_points' planes.
//
// nearest_kernel<FORM>: one point per lane, 64-point tiles claimed as closest_kernel claims them, LG_BLOCK lanes per workgroup, and
// closest_kernel's distance-ordered walk of the REFERENCE trees with its (node, accel) stack in dynamic LDS: the walk's pieces are
// k_closest.hip's text itself (included below without its kernel), the loop around them differs only in the limit it prunes against and in
// where it ends.  Three forms, by what the planes asked for need:
//   NEAREST_TOUCH  `touch` alone: the lane leaves the walk at its first admissible candidate.  Limit: r_i^2.
//   NEAREST_LIST   no `count`: the lane keeps the k best (nearest_list.h).  Limit: min(the k-th entry's d2 once the list is full, r_i^2),
//                  through the unchanged closest_skip -- strict and with its margin, so a subtree that may hold a candidate TYING the k-th d2
//                  is still walked, and nearest_insert lets the key decide.
//   NEAREST_COUNT  `count`, with or without slot planes: every admissible candidate has to be met, so the limit is r_i^2 alone; at an
//                  infinite radius this walks every primitive for every point, by definition.
//
// Dynamic LDS: the stack as closest_kernel lays it out -- entry e of lane t at words (2e) * LG_BLOCK + t and (2e + 1) * LG_BLOCK + t --, and
// behind it the lists: word w (0 .. 4: d2 low, d2 high, key low, key high, leaf slot) of entry e of lane t at
// stack_depth * 2 * LG_BLOCK + (5e + w) * LG_BLOCK + t.  A wave's 64 lanes read 64 consecutive words: conflict-free.  LG_BLOCK * (8 *
// stack_depth + 20 * k) bytes in all (nearest_host.h, nearest_lds_bytes); no per-lane array lives in registers or scratch.  A winner's x is
// not carried: at the end closest_candidate runs again on the entry's leaf slot -- the same inputs, the same bits.
//
// Every element of every plane asked for is written by exactly one lane: no atomics, no pre-fill.  Lanes past the last point walk nothing
// and write nothing.
#define LG_CLOSEST_WALK_ONLY
#include "k_closest.hip"
#include "nearest_host.h"
#include "nearest_list.h"

#if LG_NEAREST_FAULT != 0
#error "LG_NEAREST_FAULT seeds a fault into nearest_list.h for tools/nearest_list_check.cpp alone: the kernel is never built with it"
#endif

namespace lg {

static_assert(NEAREST_BLOCK == LG_BLOCK && NEAREST_STACK_ENTRY_BYTES == 2 * sizeof(uint32_t) && NEAREST_LIST_ENTRY_BYTES == 5 * sizeof(uint32_t),
              "nearest_lds_bytes (nearest_host.h) states the layout below");

extern __shared__ uint32_t nearest_lds[];

enum { NEAREST_TOUCH = 0, NEAREST_LIST = 1, NEAREST_COUNT = 2 };

struct NearestArgs {
    ClosestArgs c;         // the walk's: points, n, qmax, tri_base, cl, tile_counter, ntiles, stack_depth; r2 the SHARED radius squared; its planes unused
    const double *radii;   // [n] or nullptr: the shared radius for every point
    uint32_t k;            // list entries a lane keeps: 0 where no slot plane is asked for
    uint8_t *touch;        // [n]; may be nullptr (as every plane)
    uint32_t *count;       // [n]
    double *distance;      // [k][n]
    double *point;         // [k][n][3]
    uint4 *id;             // [k][n]
};

// a lane's list in LDS (header comment): `base` is the lists' first word plus the lane's number in the workgroup
struct NearestLds {
    uint32_t *base;
    __device__ __forceinline__ NearestEntry get(uint32_t e) const {
        const uint32_t *w = base + (5u * e) * LG_BLOCK;
        NearestEntry r;
        r.d2 = __hiloint2double((int)w[LG_BLOCK], (int)w[0]);
        r.key = ((unsigned long long)w[3u * LG_BLOCK] << 32) | (unsigned long long)w[2u * LG_BLOCK];
        r.slot = w[4u * LG_BLOCK];
        return r;
    }
    __device__ __forceinline__ void set(uint32_t e, const NearestEntry &v) {
        uint32_t *w = base + (5u * e) * LG_BLOCK;
        w[0] = (uint32_t)__double2loint(v.d2);
        w[LG_BLOCK] = (uint32_t)__double2hiint(v.d2);
        w[2u * LG_BLOCK] = (uint32_t)v.key;
        w[3u * LG_BLOCK] = (uint32_t)(v.key >> 32);
        w[4u * LG_BLOCK] = v.slot;
    }
};

template <int FORM> __global__ void __launch_bounds__(LG_BLOCK) nearest_kernel(const DParams P, const NearestArgs N) {
    const ClosestArgs &Q = N.c;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ntiles = Q.ntiles;
    if (!closest_begin(ntiles)) return;
    uint32_t *stack = nearest_lds + tid;
    NearestLds list{nearest_lds + Q.stack_depth * 2u * LG_BLOCK + tid};
    const uint32_t kcap = FORM == NEAREST_TOUCH ? 0u : N.k;
    for (bool final = false; !final;) {
        const uint32_t tile = closest_next_tile(Q, ntiles, final);
        if (tile == NO_TILE) break;
        const unsigned long long i = (unsigned long long)tile * 64ull + lane;
        if (i >= Q.n) continue;
        const double *pq = Q.points + 3ull * i;
        const V3 qw{pq[0], pq[1], pq[2]};
        const double r = N.radii ? N.radii[i] : 0.0;
        const double r2 = N.radii ? r * r : Q.r2; // one f64 product; a NaN or negative r: the point is a miss (-0.0 is zero)
        uint32_t m = 0u;
        unsigned long long total = 0ull; // admissible candidates met.  (64 bits wide on purpose: as a 32-bit word its increment is merged with the leaf's ++sp into one store through a selected address, and both words then live in scratch)
        double worst = INFINITY; // the d2 of the list's last entry once it is full
        if (__builtin_isfinite(qw.x) && __builtin_isfinite(qw.y) && __builtin_isfinite(qw.z) && r >= 0.0) {
            const double qinf = fmax(fabs(qw.x), fmax(fabs(qw.y), fabs(qw.z)));
            const bool prune = qinf <= Q.qmax;
            const double eta = 0x1p-44 * qinf;
            ClosestLevel L;
            closest_enter(P, Q, qw, 0u, L);
            uint32_t sp = 0u, node = 0u;
            bool have = true; // a node in registers whose own box has been measured (the root: never skipped)
            for (;;) {
                if (FORM == NEAREST_TOUCH && total != 0ull) break;
                if (!have) {
                    if (sp == 0u) break;
                    --sp;
                    node = stack[(2u * sp) * LG_BLOCK];
                    const uint32_t accel = stack[(2u * sp + 1u) * LG_BLOCK];
                    if (accel != L.accel) closest_enter(P, Q, qw, accel, L);
                    const double lim = FORM == NEAREST_LIST ? fmin(worst, r2) : r2;
                    if (closest_skip(L, closest_box_d2(L, P.nodes + (L.node_base + node)), lim, eta, prune)) continue;
                }
                have = false;
                const DNode *n = P.nodes + (L.node_base + node);
                const uint32_t meta = n->meta;
                if (meta & NODE_LEAF) {
                    closest_leaf(P, Q, L, qw, n, stack, sp, [&](const ClosestPt &c, uint32_t kind, uint32_t prim, uint32_t slot) {
                        const bool admissible = nearest_admissible(c.d2, r2);
                        total += admissible ? 1ull : 0ull;
                        if (FORM == NEAREST_TOUCH || !admissible) return;
                        nearest_insert(list, m, kcap, NearestEntry{c.d2, closest_key(L.accel, kind + 1u, prim), slot});
                        worst = nearest_worst(list, m, kcap); // (in the count form too, which never reads it: see `total`)
                    });
                    continue;
                }
                const uint32_t c0 = node + 1u, c1 = n->link;
                const double d0 = closest_box_d2(L, P.nodes + (L.node_base + c0)), d1 = closest_box_d2(L, P.nodes + (L.node_base + c1));
                const double lim = FORM == NEAREST_LIST ? fmin(worst, r2) : r2;
                const bool s0 = closest_skip(L, d0, lim, eta, prune), s1 = closest_skip(L, d1, lim, eta, prune);
                if (s0 && s1) continue;
                const bool near1 = s0 || (!s1 && d1 < d0); // the nearer child first; the first on a tie
                if (!s0 && !s1) {
                    stack[(2u * sp) * LG_BLOCK] = near1 ? c0 : c1;
                    stack[(2u * sp + 1u) * LG_BLOCK] = L.accel;
                    ++sp;
                }
                node = near1 ? c1 : c0;
                have = true;
            }
        }
        if (N.touch) N.touch[i] = total != 0ull ? 1u : 0u;
        if (N.count) N.count[i] = (uint32_t)total; // (a scene holds fewer than 2^32 primitives)
        for (uint32_t j = 0; j < kcap; ++j) { // (kcap is the wave's; m the lane's)
            double dist = INFINITY;
            V3 x{0.0, 0.0, 0.0};
            uint4 id = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu);
            if (j < m) {
                const NearestEntry e = list.get(j);
                const uint32_t instance = (uint32_t)(e.key >> 34), kind = (uint32_t)(e.key >> 32) & 3u;
                const uint32_t ref = P.primref[e.slot];
                uint32_t prim;
                x = closest_candidate(P, Q, instance, e.slot, ref >> 30, ref & PRIM_INDEX_MASK, qw, prim).x;
                dist = sqrt(e.d2);
                id = make_uint4(kind, prim, instance, (uint32_t)closest_material(P, kind, prim, instance));
            }
            const unsigned long long row = (unsigned long long)j * Q.n + i;
            if (N.distance) N.distance[row] = dist;
            if (N.point) { double *o = N.point + 3ull * row; o[0] = x.x; o[1] = x.y; o[2] = x.z; }
            if (N.id) N.id[row] = id;
        }
    }
}

// ---- host-callable launchers (query.cpp)
static const void *nearest_function(int form) {
    return form == NEAREST_TOUCH  ? reinterpret_cast<const void *>(nearest_kernel<NEAREST_TOUCH>)
           : form == NEAREST_LIST ? reinterpret_cast<const void *>(nearest_kernel<NEAREST_LIST>)
                                  : reinterpret_cast<const void *>(nearest_kernel<NEAREST_COUNT>);
}
// The form the planes asked for need, and the entries a lane keeps
int nearest_form(bool count, bool slots) { return count ? NEAREST_COUNT : slots ? NEAREST_LIST : NEAREST_TOUCH; }
hipError_t launch_nearest(const DParams &P, int form, const double *points, const double *radii, unsigned long long n, double r2, double qmax, uint32_t k, uint8_t *touch,
                          uint32_t *count, double *distance, double *point, void *id, const uint32_t *tri_base, const void *cl, uint32_t *tile_counter, uint32_t blocks,
                          uint32_t stack_depth, hipStream_t stream) {
    const ClosestArgs Q{points, n, r2, qmax, nullptr, nullptr, nullptr, tri_base, reinterpret_cast<const ClosestAccel *>(cl), tile_counter, (uint32_t)((n + 63ull) / 64ull), stack_depth};
    const NearestArgs N{Q, radii, k, touch, count, distance, point, reinterpret_cast<uint4 *>(id)};
    const size_t lds = nearest_lds_bytes(stack_depth, k);
    if (form == NEAREST_TOUCH) hipLaunchKernelGGL(nearest_kernel<NEAREST_TOUCH>, dim3(blocks), dim3(LG_BLOCK), lds, stream, P, N);
    else if (form == NEAREST_LIST) hipLaunchKernelGGL(nearest_kernel<NEAREST_LIST>, dim3(blocks), dim3(LG_BLOCK), lds, stream, P, N);
    else hipLaunchKernelGGL(nearest_kernel<NEAREST_COUNT>, dim3(blocks), dim3(LG_BLOCK), lds, stream, P, N);
    return hipGetLastError();
}
hipError_t nearest_occupancy(int form, uint32_t stack_depth, uint32_t k, int *blocks_per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, nearest_function(form), LG_BLOCK, nearest_lds_bytes(stack_depth, k));
}
// the dynamic LDS a launch of any form may ask for, raised once per device where stack and lists need more than the default 64 KiB
hipError_t nearest_set_lds_limit(size_t bytes) {
    for (int form = NEAREST_TOUCH; form <= NEAREST_COUNT; ++form) {
        const hipError_t e = hipFuncSetAttribute(nearest_function(form), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace lg
