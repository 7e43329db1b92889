// lasgun_amd/csrc/k_closest.hip -- closest points (include/lasgun_hip.h, lg_closest_points*): for each of the caller's points the nearest
// surface point of the scene, its distance and the primitive it lies on.  The contract is arithmetic over ALL primitives (closest_prim.h:
// the candidate of a triangle, a box, a sphere; the rule between two candidates); this walk only leaves out subtrees that provably hold no
// candidate at or below the best so far, so its answer is the brute force's, bit for bit, whatever the trees look like.
//
// closest_kernel: one point per lane, 64-point tiles of the caller's array claimed as query_kernel claims its tiles (claim_tile_single),
// LG_BLOCK lanes per workgroup.  ONE form for every accel and every traversal mode: it reads the REFERENCE trees from the global tables
// (P.nodes, P.primref, P.leaf_soup, P.accels, tri_base) -- the LDS image, the pair records, the fast trees and the culling records play no
// part.  Nothing of walk.h or shade.h is used, and DParams only for its table pointers; the query's own arguments are ClosestArgs.
//
// The walk is ordered by distance, not by ray parameter.  A lane holds one node in registers; at an interior node it measures both children's
// boxes against the point in the accel's local space, goes on with the nearer and pushes the farther, each unless its lower bound rules it
// out (closest_skip); a pushed node is measured again when it is taken, against the best of that moment.  A nested accel in a leaf is
// pushed as (node 0, that accel).  Stack entries are (node, accel) word pairs in dynamic LDS, entry e of lane t at words
// (2e) * LG_BLOCK + t and (2e + 1) * LG_BLOCK + t -- conflict-free --, as deep as the host computed for this push rule (closest_host.h).
// Entering an accel re-expresses the point through the chain's stored inverses, root first, as accel_local_ray does for an origin, and
// carries a bound e of that point's rounding along.
//
// The lower bound (closest_host.h, ClosestAccel):
//   LB = shrink * ((dist(q_A, box) * (1 - 2^-40) - 2 e) - delta) - omega - 2^-44 |q|_inf,   skipped iff LB > 0 and LB * LB > lim * (1 + 2^-40),
// lim the smaller of the best squared distance so far and radius^2.  Strict, so exact ties survive and the key decides them; a NaN anywhere
// makes the test false: walking without skipping is always correct.  A point beyond Q.qmax is walked unpruned.
//
// Every element of every plane asked for is written by exactly one lane: no atomics, no pre-fill.  Lanes past the last point walk nothing
// and write nothing.
//
// The walk's pieces -- ClosestArgs, closest_world, ClosestLevel, closest_enter, closest_box_d2, closest_skip, closest_candidate, closest_leaf,
// closest_material, closest_begin, closest_next_tile -- are k_nearest.hip's too (lg_nearest*: the k nearest, counts, per-point radii): it includes THIS text with
// LG_CLOSEST_WALK_ONLY defined, which leaves out the kernel, its stack and its launchers.  One text, no copy: the tests that pin these
// lines read them here.
#include "closest_host.h"
#include "closest_prim.h"
#include "kcommon.h"

#if LG_CLOSEST_FAULT != 0
#error "LG_CLOSEST_FAULT seeds a fault into closest_prim.h for tools/closest_prim_check.cpp alone: the kernel is never built with it"
#endif

namespace lg {

#ifndef LG_CLOSEST_WALK_ONLY
extern __shared__ uint32_t closest_stack[];
#endif

struct ClosestArgs {
    const double *points;      // [n][3]
    unsigned long long n;
    double r2;                 // radius * radius
    double qmax;               // the walk prunes for |q|_inf <= qmax
    double *distance;          // [n]; may be nullptr (as every plane)
    double *point;             // [n][3]
    uint4 *id;                 // [n]: kind, prim, instance, material
    const uint32_t *tri_base;  // per accel, its mesh's first triangle in the triangle tables
    const ClosestAccel *cl;    // per accel, the pruning test's constants
    uint32_t *tile_counter;
    uint32_t ntiles;
    uint32_t stack_depth;      // entries; the launch's dynamic LDS is stack_depth * 2 * LG_BLOCK words
};

// W_A(x): the accel's own transform, then its parent's, up to the root's
__device__ __forceinline__ V3 closest_world(const DParams &P, uint32_t accel, V3 x) {
    for (int32_t a = (int32_t)accel; a >= 0;) {
        const DAccel *A = P.accels + a;
        x = xf_point(A->m, x);
        a = A->parent;
    }
    return x;
}

// the lane's state in one accel: the point in its local space with the bound of its rounding, the accel's table bases and constants
struct ClosestLevel {
    V3 q;
    double e;
    uint32_t accel, node_base, prim_base;
    double shrink, delta, omega;
};
__device__ __forceinline__ void closest_enter(const DParams &P, const ClosestArgs &Q, V3 qw, uint32_t accel, ClosestLevel &L) {
    const DAccel *A = P.accels + accel;
    const uint32_t nchain = A->nchain;
    V3 q = qw;
    double e = 0.0;
    for (uint32_t s = 0; s < nchain; ++s) {
        const Affine &m = P.accels[A->chain[s]].minv;
        // the rounding of this stage is at most 4u of the sum of the products' magnitudes, component by component (2^-50: twice that); what
        // the point carried is stretched by the linear part's infinity norm at most
        const double ax = fabs(q.x), ay = fabs(q.y), az = fabs(q.z);
        const double m0 = ((fabs(m.c[0][0]) * ax + fabs(m.c[1][0]) * ay) + fabs(m.c[2][0]) * az) + fabs(m.c[3][0]);
        const double m1 = ((fabs(m.c[0][1]) * ax + fabs(m.c[1][1]) * ay) + fabs(m.c[2][1]) * az) + fabs(m.c[3][1]);
        const double m2 = ((fabs(m.c[0][2]) * ax + fabs(m.c[1][2]) * ay) + fabs(m.c[2][2]) * az) + fabs(m.c[3][2]);
        const double r0 = (fabs(m.c[0][0]) + fabs(m.c[1][0])) + fabs(m.c[2][0]);
        const double r1 = (fabs(m.c[0][1]) + fabs(m.c[1][1])) + fabs(m.c[2][1]);
        const double r2 = (fabs(m.c[0][2]) + fabs(m.c[1][2])) + fabs(m.c[2][2]);
        e = fmax(r0, fmax(r1, r2)) * e * (1.0 + 0x1p-40) + 0x1p-50 * fmax(m0, fmax(m1, m2));
        q = xf_point(m, q);
    }
    L.q = q; L.e = e;
    L.accel = accel; L.node_base = A->node_base; L.prim_base = A->prim_base;
    const ClosestAccel c = Q.cl[accel];
    L.shrink = c.shrink; L.delta = c.delta; L.omega = c.omega;
}

// squared distance from the level's point to a node's box (0 inside; a NaN bound counts as no excess)
__device__ __forceinline__ double closest_box_d2(const ClosestLevel &L, const DNode *n) {
    const double lx = n->bmin[0] - L.q.x, hx = L.q.x - n->bmax[0];
    const double ly = n->bmin[1] - L.q.y, hy = L.q.y - n->bmax[1];
    const double lz = n->bmin[2] - L.q.z, hz = L.q.z - n->bmax[2];
    const double ex = lx > 0.0 ? lx : (hx > 0.0 ? hx : 0.0);
    const double ey = ly > 0.0 ? ly : (hy > 0.0 ? hy : 0.0);
    const double ez = lz > 0.0 ? lz : (hz > 0.0 ? hz : 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}
// may everything below a box at squared local distance `box_d2` be left out?  (header comment)
__device__ __forceinline__ bool closest_skip(const ClosestLevel &L, double box_d2, double lim, double eta, bool prune) {
    if (!prune) return false;
    const double lb = L.shrink * ((sqrt(box_d2) * (1.0 - 0x1p-40) - 2.0 * L.e) - L.delta) - L.omega - eta;
    return lb > 0.0 && lb * lb > lim * (1.0 + 0x1p-40);
}

// The candidate of one leaf slot (`slot` indexes P.leaf_soup; kind, idx: the halves of its primref; never a nested accel) of accel `accel`,
// and its prim in lg_hit's numbering.  It reads nothing of the walk's state: the same slot gives the same bits whenever it is asked
// (k_nearest.hip evaluates a list's winners again at the end).
__device__ __forceinline__ ClosestPt closest_candidate(const DParams &P, const ClosestArgs &Q, uint32_t accel, uint32_t slot, uint32_t kind, uint32_t idx, V3 qw, uint32_t &prim) {
    const uint4 *rec = reinterpret_cast<const uint4 *>(P.leaf_soup + slot);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    ClosestPt c;
    prim = idx;
    if (kind == PK_TRIANGLE) {
        const V3 a = closest_world(P, accel, V3{(double)__uint_as_float(r0.x), (double)__uint_as_float(r0.y), (double)__uint_as_float(r0.z)});
        const V3 b = closest_world(P, accel, V3{(double)__uint_as_float(r0.w), (double)__uint_as_float(r1.x), (double)__uint_as_float(r1.y)});
        const V3 cc = closest_world(P, accel, V3{(double)__uint_as_float(r1.z), (double)__uint_as_float(r1.w), (double)__uint_as_float(r2.x)});
        c = closest_triangle(qw, a, b, cc);
        prim = idx - Q.tri_base[accel];
    } else if (kind == PK_SPHERE) {
        const double cx = __hiloint2double((int)r0.y, (int)r0.x), cy = __hiloint2double((int)r0.w, (int)r0.z);
        const double cz = __hiloint2double((int)r1.y, (int)r1.x), r = __hiloint2double((int)r1.w, (int)r1.z);
        c = closest_sphere(qw, closest_world(P, accel, V3{cx, cy, cz}), closest_world(P, accel, V3{cx + r, cy + 0.0, cz + 0.0}));
    } else {
        const double mn[3] = {__hiloint2double((int)r0.y, (int)r0.x), __hiloint2double((int)r0.w, (int)r0.z), __hiloint2double((int)r1.y, (int)r1.x)};
        const double mx[3] = {__hiloint2double((int)r1.w, (int)r1.z), __hiloint2double((int)r2.y, (int)r2.x), __hiloint2double((int)r2.w, (int)r2.z)};
        V3 w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = closest_world(P, accel, V3{(q & 1) ? mx[0] : mn[0], (q & 2) ? mx[1] : mn[1], (q & 4) ? mx[2] : mn[2]});
        c = closest_box(qw, w);
    }
    return c;
}
// A leaf: its nested accels pushed as (node 0, that accel), every other slot's candidate handed to offer(c, kind, prim, slot) -- kind the
// primref's (lg_hit's less one)
template <class Offer>
__device__ __forceinline__ void closest_leaf(const DParams &P, const ClosestArgs &Q, const ClosestLevel &L, V3 qw, const DNode *n, uint32_t *stack, uint32_t &sp, Offer &&offer) {
    const uint32_t count = n->meta & 0xFFFFu, first = L.prim_base + n->link;
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t ref = P.primref[first + k], kind = ref >> 30, idx = ref & PRIM_INDEX_MASK;
        if (kind == PK_ACCEL) {
            stack[(2u * sp) * LG_BLOCK] = 0u;
            stack[(2u * sp + 1u) * LG_BLOCK] = idx;
            ++sp;
            continue;
        }
        uint32_t prim;
        const ClosestPt c = closest_candidate(P, Q, L.accel, first + k, kind, idx, qw, prim);
        offer(c, kind, prim, first + k);
    }
}

// lg_intersect's material for a hit on the winner (walk.h, resolve_hit): the primitive's own, else the outermost accel's on the way up, else the default
__device__ __forceinline__ int32_t closest_material(const DParams &P, uint32_t kind, uint32_t prim, uint32_t instance) {
    int32_t prim_mat = -1;
    if (kind == 1u) prim_mat = P.sphere_mat[prim];
    else if (kind == 2u) prim_mat = P.cuboid_mat[prim];
    int32_t mat = P.default_material;
    for (int32_t a = (int32_t)instance; a >= 0;) {
        const DAccel *A = P.accels + a;
        if (A->material >= 0) mat = A->material;
        a = A->parent;
    }
    return prim_mat >= 0 ? prim_mat : mat;
}

// The prologue and the tile cursor of a kernel of this family: has the wave anything to do (a launch of n tiles is claimed by its first n
// waves), and its next 64-point tile, the same in every lane, or NO_TILE (kcommon.h says how a launch ends)
__device__ __forceinline__ bool closest_begin(uint32_t ntiles) { return ntiles != 0u && wave_has_work(ntiles); }
__device__ __forceinline__ uint32_t closest_next_tile(const ClosestArgs &Q, uint32_t ntiles, bool &final) { return claim_tile_single(Q.tile_counter, ntiles, final); }

#ifndef LG_CLOSEST_WALK_ONLY
__global__ void __launch_bounds__(LG_BLOCK) closest_kernel(const DParams P, const ClosestArgs Q) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ntiles = Q.ntiles;
    if (!closest_begin(ntiles)) return;
    uint32_t *stack = closest_stack + tid;
    for (bool final = false; !final;) {
        const uint32_t tile = closest_next_tile(Q, ntiles, final);
        if (tile == NO_TILE) break;
        const unsigned long long i = (unsigned long long)tile * 64ull + lane;
        if (i >= Q.n) continue;
        const double *pq = Q.points + 3ull * i;
        const V3 qw{pq[0], pq[1], pq[2]};
        ClosestBest best = closest_none();
        if (__builtin_isfinite(qw.x) && __builtin_isfinite(qw.y) && __builtin_isfinite(qw.z)) {
            const double qinf = fmax(fabs(qw.x), fmax(fabs(qw.y), fabs(qw.z)));
            const bool prune = qinf <= Q.qmax;
            const double eta = 0x1p-44 * qinf;
            ClosestLevel L;
            closest_enter(P, Q, qw, 0u, L);
            uint32_t sp = 0u, node = 0u;
            bool have = true; // a node in registers whose own box has been measured (the root: never skipped)
            for (;;) {
                if (!have) {
                    if (sp == 0u) break;
                    --sp;
                    node = stack[(2u * sp) * LG_BLOCK];
                    const uint32_t accel = stack[(2u * sp + 1u) * LG_BLOCK];
                    if (accel != L.accel) closest_enter(P, Q, qw, accel, L);
                    const double lim = fmin(best.d2, Q.r2);
                    if (closest_skip(L, closest_box_d2(L, P.nodes + (L.node_base + node)), lim, eta, prune)) continue;
                }
                have = false;
                const DNode *n = P.nodes + (L.node_base + node);
                const uint32_t meta = n->meta;
                if (meta & NODE_LEAF) {
                    closest_leaf(P, Q, L, qw, n, stack, sp, [&](const ClosestPt &c, uint32_t kind, uint32_t prim, uint32_t) {
                        closest_offer(best, c, Q.r2, closest_key(L.accel, kind + 1u, prim));
                    });
                    continue;
                }
                const uint32_t c0 = node + 1u, c1 = n->link;
                const double d0 = closest_box_d2(L, P.nodes + (L.node_base + c0)), d1 = closest_box_d2(L, P.nodes + (L.node_base + c1));
                const double lim = fmin(best.d2, Q.r2);
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
        uint4 id = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu);
        if (best.key != ~0ull) {
            const uint32_t instance = (uint32_t)(best.key >> 34), kind = (uint32_t)(best.key >> 32) & 3u, prim = (uint32_t)best.key;
            id = make_uint4(kind, prim, instance, (uint32_t)closest_material(P, kind, prim, instance));
        }
        if (Q.distance) Q.distance[i] = sqrt(best.d2);
        if (Q.point) { double *o = Q.point + 3ull * i; o[0] = best.x.x; o[1] = best.x.y; o[2] = best.x.z; }
        if (Q.id) Q.id[i] = id;
    }
}

// ---- host-callable launchers (query.cpp)
static size_t closest_lds_bytes(uint32_t stack_depth) { return (size_t)stack_depth * 2u * LG_BLOCK * sizeof(uint32_t); }
hipError_t launch_closest(const DParams &P, const double *points, unsigned long long n, double r2, double qmax, double *distance, double *point, void *id,
                          const uint32_t *tri_base, const void *cl, uint32_t *tile_counter, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const ClosestArgs Q{points, n, r2, qmax, distance, point, reinterpret_cast<uint4 *>(id), tri_base, reinterpret_cast<const ClosestAccel *>(cl), tile_counter,
                        (uint32_t)((n + 63ull) / 64ull), stack_depth};
    hipLaunchKernelGGL(closest_kernel, dim3(blocks), dim3(LG_BLOCK), closest_lds_bytes(stack_depth), stream, P, Q);
    return hipGetLastError();
}
hipError_t closest_occupancy(uint32_t stack_depth, int *blocks_per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, closest_kernel, LG_BLOCK, closest_lds_bytes(stack_depth));
}
// the dynamic LDS a launch may ask for, raised once per device where the stack needs more than the default 64 KiB
hipError_t closest_set_lds_limit(size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(closest_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
size_t closest_stack_bytes(uint32_t stack_depth) { return closest_lds_bytes(stack_depth); }
#endif // LG_CLOSEST_WALK_ONLY

} // namespace lg
