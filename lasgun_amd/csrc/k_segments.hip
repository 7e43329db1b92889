// lasgun_amd/csrc/k_segments.hip -- segment proximity (include/lasgun_hip.h, lg_closest_segments*): for each of the caller's segments
// p0 .. p1, under a radius of its own, the nearest surface point of the scene to the segment, the segment's parameter there, the distance
// and the primitive -- capsules and swept spheres against the world.  A candidate is segment_prim.h's, one per primitive, over world geometry
// formed exactly as k_closest.hip's closest_candidate forms it, so the answer is the brute force's over ALL primitives, bit for bit.
//
// segments_kernel<FORM>: one segment per lane, 64-segment tiles claimed as closest_kernel claims them, LG_BLOCK lanes per workgroup, and
// closest_kernel's distance-ordered walk of the REFERENCE trees with its (node, accel) stack in dynamic LDS -- the stack alone,
// stack_depth * 2 * LG_BLOCK words, closest_kernel's layout.  The walk's pieces are k_closest.hip's text itself (included below without its
// kernel): closest_enter for both endpoints, closest_skip unchanged, closest_leaf for a leaf's slots (the point candidate it forms for p0 is
// not used and falls away), closest_material, the tile cursor.  Two forms, by the planes asked for:
//   SEGMENTS_TOUCH  `touch` alone: the lane leaves the walk at its first admissible candidate.  Limit: r_i^2.
//   SEGMENTS_BEST   every other plane set: the lane keeps the best (d2, key).  Limit: min(best d2, r_i^2).
//
// Pruning is a segment against a box in the accel's local space, where the segment's image is the straight segment between the images of
// its endpoints q0, q1 (an affine map), each known up to its own rounding bound; the walk carries e = max(e0, e1).  Two stages (DESIGN.md
// section 3.7, "Segment proximity"):
//   1  the gap between the node's box and the local segment's own bounding box, squared, through the UNCHANGED closest_skip: the same
//      strictness, the same margins, a NaN means walk.  The segment lies in its bounding box, so the gap is a lower bound of its distance.
//   2  where stage 1 does not skip and the limit is finite: does the local segment miss the node's box grown on every side by rho, the local
//      distance at which closest_skip's inequality holds for the current limit --
//        rho = ((((sqrt(lim * (1 + 2^-40)) + omega) + eta) / shrink + delta) + 2 e) / (1 - 2^-40), times (1 + 2^-40) twice --,
//      by a slab test that errs towards "not missed" (2^-40 of the parameter).  A miss of the grown box is an L-infinity distance above rho
//      at every point of the segment, hence a Euclidean distance above rho.  Any NaN or non-finite word means walk.
// Children are ordered by stage 1's gap, the first on a tie.  eta = 2^-44 max(|p0|_inf, |p1|_inf); both endpoints within qmax, or no pruning.
//
// Every element of every plane asked for is written by exactly one lane: no atomics, no pre-fill.  Lanes past the last segment walk nothing
// and write nothing.
#define LG_CLOSEST_WALK_ONLY
#include "k_closest.hip"
#include "segment_prim.h"
#include "segments_host.h"

#if LG_SEGMENT_FAULT != 0
#error "LG_SEGMENT_FAULT seeds a fault into segment_prim.h for tools/segment_prim_check.cpp alone: the kernel is never built with it"
#endif

namespace lg {

extern __shared__ uint32_t segments_stack[];

enum { SEGMENTS_TOUCH = 0, SEGMENTS_BEST = 1 };

struct SegmentsArgs {
    ClosestArgs c;         // the walk's: n, qmax, tri_base, cl, tile_counter, ntiles, stack_depth; r2 the SHARED radius squared; points and its planes unused
    const double *segments; // [n][6]: p0, p1
    const double *radii;   // [n] or nullptr: the shared radius for every segment
    uint8_t *touch;        // [n]; may be nullptr (as every plane)
    double *distance;      // [n]
    double *param;         // [n]
    double *point;         // [n][3]
    uint4 *id;             // [n]
};

// the lane's state in one accel: closest points' level for p0 (its e: the larger of the two endpoints' bounds; a NaN stays), and q1
struct SegLevel {
    ClosestLevel L;
    V3 q1;
};
__device__ __forceinline__ void segments_enter(const DParams &P, const ClosestArgs &Q, V3 p0, V3 p1, uint32_t accel, SegLevel &S) {
    ClosestLevel L1;
    closest_enter(P, Q, p0, accel, S.L);
    closest_enter(P, Q, p1, accel, L1);
    S.q1 = L1.q;
    S.L.e = (L1.e > S.L.e || L1.e != L1.e) ? L1.e : S.L.e;
}

// stage 1: the squared gap between a node's box and the local segment's bounding box (0 where they overlap; a NaN bound counts as no excess)
__device__ __forceinline__ double segments_box_d2(const SegLevel &S, const DNode *n) {
    const V3 a = S.L.q, b = S.q1;
    const double sx0 = a.x < b.x ? a.x : b.x, sx1 = a.x < b.x ? b.x : a.x;
    const double sy0 = a.y < b.y ? a.y : b.y, sy1 = a.y < b.y ? b.y : a.y;
    const double sz0 = a.z < b.z ? a.z : b.z, sz1 = a.z < b.z ? b.z : a.z;
    const double lx = n->bmin[0] - sx1, hx = sx0 - n->bmax[0];
    const double ly = n->bmin[1] - sy1, hy = sy0 - n->bmax[1];
    const double lz = n->bmin[2] - sz1, hz = sz0 - n->bmax[2];
    const double ex = lx > 0.0 ? lx : (hx > 0.0 ? hx : 0.0);
    const double ey = ly > 0.0 ? ly : (hy > 0.0 ? hy : 0.0);
    const double ez = lz > 0.0 ? lz : (hz > 0.0 ? hz : 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}
// stage 2's distance for a limit (header comment): +INF or a NaN where nothing may be skipped
__device__ __forceinline__ double segments_rho(const ClosestLevel &L, double lim, double eta, bool prune) {
#ifdef LG_SEGMENTS_NO_STAGE2
    return INFINITY;
#else
    if (!prune || !(lim < INFINITY) || !(L.shrink > 0.0)) return INFINITY;
    const double need = (sqrt(lim * (1.0 + 0x1p-40)) + L.omega) + eta;
    const double rho = (((need / L.shrink + L.delta) + 2.0 * L.e) / (1.0 - 0x1p-40)) * (1.0 + 0x1p-40);
    return rho * (1.0 + 0x1p-40);
#endif
}
// one axis of the slab test against the box grown by rho: false where a word is not finite
__device__ __forceinline__ bool segments_slab_axis(double q0, double q1, double bmin, double bmax, double rho, double &tmin, double &tmax, bool &miss) {
    const double lo = (bmin - q0) - rho, hi = (bmax - q0) + rho, d = q1 - q0;
    if (!(__builtin_isfinite(lo) && __builtin_isfinite(hi) && __builtin_isfinite(d))) return false;
    if (d == 0.0) {
        miss = miss || lo > 0.0 || hi < 0.0;
        return true;
    }
    const double t1 = lo / d, t2 = hi / d;
    const double tn = d > 0.0 ? t1 : t2, tf = d > 0.0 ? t2 : t1;
    tmin = tn > tmin ? tn : tmin;
    tmax = tf < tmax ? tf : tmax;
    return true;
}
// does the local segment provably miss the node's box grown by rho?
__device__ __forceinline__ bool segments_slab_miss(const SegLevel &S, const DNode *n, double rho) {
    if (!(rho < INFINITY)) return false;
    double tmin = 0.0, tmax = 1.0;
    bool miss = false;
    const bool ok = segments_slab_axis(S.L.q.x, S.q1.x, n->bmin[0], n->bmax[0], rho, tmin, tmax, miss) &&
                    segments_slab_axis(S.L.q.y, S.q1.y, n->bmin[1], n->bmax[1], rho, tmin, tmax, miss) &&
                    segments_slab_axis(S.L.q.z, S.q1.z, n->bmin[2], n->bmax[2], rho, tmin, tmax, miss);
    return ok && (miss || tmin > tmax + 0x1p-40);
}

// The candidate of one leaf slot for the segment: the primitive's world geometry formed as closest_candidate forms it
__device__ __forceinline__ SegPt segments_candidate(const DParams &P, uint32_t accel, uint32_t slot, uint32_t kind, V3 p0, V3 p1) {
    const uint4 *rec = reinterpret_cast<const uint4 *>(P.leaf_soup + slot);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    if (kind == PK_TRIANGLE) {
        const V3 a = closest_world(P, accel, V3{(double)__uint_as_float(r0.x), (double)__uint_as_float(r0.y), (double)__uint_as_float(r0.z)});
        const V3 b = closest_world(P, accel, V3{(double)__uint_as_float(r0.w), (double)__uint_as_float(r1.x), (double)__uint_as_float(r1.y)});
        const V3 cc = closest_world(P, accel, V3{(double)__uint_as_float(r1.z), (double)__uint_as_float(r1.w), (double)__uint_as_float(r2.x)});
        return seg_triangle(p0, p1, a, b, cc);
    }
    if (kind == PK_SPHERE) {
        const double cx = __hiloint2double((int)r0.y, (int)r0.x), cy = __hiloint2double((int)r0.w, (int)r0.z);
        const double cz = __hiloint2double((int)r1.y, (int)r1.x), r = __hiloint2double((int)r1.w, (int)r1.z);
        return seg_sphere(p0, p1, closest_world(P, accel, V3{cx, cy, cz}), closest_world(P, accel, V3{cx + r, cy + 0.0, cz + 0.0}));
    }
    const double mn[3] = {__hiloint2double((int)r0.y, (int)r0.x), __hiloint2double((int)r0.w, (int)r0.z), __hiloint2double((int)r1.y, (int)r1.x)};
    const double mx[3] = {__hiloint2double((int)r1.w, (int)r1.z), __hiloint2double((int)r2.y, (int)r2.x), __hiloint2double((int)r2.w, (int)r2.z)};
    const V3 w0 = closest_world(P, accel, V3{mn[0], mn[1], mn[2]}), w1 = closest_world(P, accel, V3{mx[0], mn[1], mn[2]});
    const V3 w2 = closest_world(P, accel, V3{mn[0], mx[1], mn[2]}), w3 = closest_world(P, accel, V3{mx[0], mx[1], mn[2]});
    const V3 w4 = closest_world(P, accel, V3{mn[0], mn[1], mx[2]}), w5 = closest_world(P, accel, V3{mx[0], mn[1], mx[2]});
    const V3 w6 = closest_world(P, accel, V3{mn[0], mx[1], mx[2]}), w7 = closest_world(P, accel, V3{mx[0], mx[1], mx[2]});
    return seg_box(p0, p1, w0, w1, w2, w3, w4, w5, w6, w7);
}

template <int FORM> __global__ void __launch_bounds__(LG_BLOCK) segments_kernel(const DParams P, const SegmentsArgs N) {
    const ClosestArgs &Q = N.c;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ntiles = Q.ntiles;
    if (!closest_begin(ntiles)) return;
    uint32_t *stack = segments_stack + tid;
    for (bool final = false; !final;) {
        const uint32_t tile = closest_next_tile(Q, ntiles, final);
        if (tile == NO_TILE) break;
        const unsigned long long i = (unsigned long long)tile * 64ull + lane;
        if (i >= Q.n) continue;
        const double *ps = N.segments + 6ull * i;
        const V3 p0{ps[0], ps[1], ps[2]}, p1{ps[3], ps[4], ps[5]};
        const double r = N.radii ? N.radii[i] : 0.0;
        const double r2 = N.radii ? r * r : Q.r2; // one f64 product; a NaN or negative r: the segment is a miss (-0.0 is zero)
        SegBest best = seg_none();
        bool touched = false;
        if (__builtin_isfinite(p0.x) && __builtin_isfinite(p0.y) && __builtin_isfinite(p0.z) && __builtin_isfinite(p1.x) && __builtin_isfinite(p1.y) &&
            __builtin_isfinite(p1.z) && r >= 0.0) {
            const double qinf = fmax(fmax(fabs(p0.x), fmax(fabs(p0.y), fabs(p0.z))), fmax(fabs(p1.x), fmax(fabs(p1.y), fabs(p1.z))));
            const bool prune = qinf <= Q.qmax;
            const double eta = 0x1p-44 * qinf;
            SegLevel S;
            segments_enter(P, Q, p0, p1, 0u, S);
            uint32_t sp = 0u, node = 0u;
            bool have = true; // a node in registers whose own box has been measured (the root: never skipped)
            for (;;) {
                if (FORM == SEGMENTS_TOUCH && touched) break;
                if (!have) {
                    if (sp == 0u) break;
                    --sp;
                    node = stack[(2u * sp) * LG_BLOCK];
                    const uint32_t accel = stack[(2u * sp + 1u) * LG_BLOCK];
                    if (accel != S.L.accel) segments_enter(P, Q, p0, p1, accel, S);
                    const double lim = FORM == SEGMENTS_BEST ? fmin(best.d2, r2) : r2;
                    const DNode *n = P.nodes + (S.L.node_base + node);
                    if (closest_skip(S.L, segments_box_d2(S, n), lim, eta, prune)) continue;
                    if (segments_slab_miss(S, n, segments_rho(S.L, lim, eta, prune))) continue;
                }
                have = false;
                const DNode *n = P.nodes + (S.L.node_base + node);
                const uint32_t meta = n->meta;
                if (meta & NODE_LEAF) {
                    closest_leaf(P, Q, S.L, p0, n, stack, sp, [&](const ClosestPt &, uint32_t kind, uint32_t prim, uint32_t slot) {
                        const SegPt c = segments_candidate(P, S.L.accel, slot, kind, p0, p1);
                        if (FORM == SEGMENTS_TOUCH) touched = touched || seg_admissible(c.d2, r2);
                        else seg_offer(best, c, r2, closest_key(S.L.accel, kind + 1u, prim));
                    });
                    continue;
                }
                const uint32_t c0 = node + 1u, c1 = n->link;
                const DNode *n0 = P.nodes + (S.L.node_base + c0), *n1 = P.nodes + (S.L.node_base + c1);
                const double d0 = segments_box_d2(S, n0), d1 = segments_box_d2(S, n1);
                const double lim = FORM == SEGMENTS_BEST ? fmin(best.d2, r2) : r2;
                const double rho = segments_rho(S.L, lim, eta, prune);
                const bool s0 = closest_skip(S.L, d0, lim, eta, prune) || segments_slab_miss(S, n0, rho);
                const bool s1 = closest_skip(S.L, d1, lim, eta, prune) || segments_slab_miss(S, n1, rho);
                if (s0 && s1) continue;
                const bool near1 = s0 || (!s1 && d1 < d0); // the nearer child first; the first on a tie
                if (!s0 && !s1) {
                    stack[(2u * sp) * LG_BLOCK] = near1 ? c0 : c1;
                    stack[(2u * sp + 1u) * LG_BLOCK] = S.L.accel;
                    ++sp;
                }
                node = near1 ? c1 : c0;
                have = true;
            }
        }
        if (FORM == SEGMENTS_TOUCH) {
            N.touch[i] = touched ? 1u : 0u;
            continue;
        }
        uint4 id = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu);
        if (best.key != ~0ull) {
            const uint32_t instance = (uint32_t)(best.key >> 34), kind = (uint32_t)(best.key >> 32) & 3u, prim = (uint32_t)best.key;
            id = make_uint4(kind, prim, instance, (uint32_t)closest_material(P, kind, prim, instance));
        }
        if (N.touch) N.touch[i] = best.key != ~0ull ? 1u : 0u;
        if (N.distance) N.distance[i] = sqrt(best.d2);
        if (N.param) N.param[i] = best.s;
        if (N.point) { double *o = N.point + 3ull * i; o[0] = best.x.x; o[1] = best.x.y; o[2] = best.x.z; }
        if (N.id) N.id[i] = id;
    }
}

// ---- host-callable launchers (query.cpp)
static size_t segments_lds_bytes(uint32_t stack_depth) { return (size_t)stack_depth * 2u * LG_BLOCK * sizeof(uint32_t); }
static const void *segments_function(bool touch_only) {
    return touch_only ? reinterpret_cast<const void *>(segments_kernel<SEGMENTS_TOUCH>) : reinterpret_cast<const void *>(segments_kernel<SEGMENTS_BEST>);
}
hipError_t launch_segments(const DParams &P, bool touch_only, const double *segments, const double *radii, unsigned long long n, double r2, double qmax, uint8_t *touch,
                           double *distance, double *param, double *point, void *id, const uint32_t *tri_base, const void *cl, uint32_t *tile_counter, uint32_t blocks,
                           uint32_t stack_depth, hipStream_t stream) {
    const ClosestArgs Q{nullptr, n, r2, qmax, nullptr, nullptr, nullptr, tri_base, reinterpret_cast<const ClosestAccel *>(cl), tile_counter, (uint32_t)((n + 63ull) / 64ull), stack_depth};
    const SegmentsArgs N{Q, segments, radii, touch, distance, param, point, reinterpret_cast<uint4 *>(id)};
    const size_t lds = segments_lds_bytes(stack_depth);
    if (touch_only) hipLaunchKernelGGL(segments_kernel<SEGMENTS_TOUCH>, dim3(blocks), dim3(LG_BLOCK), lds, stream, P, N);
    else hipLaunchKernelGGL(segments_kernel<SEGMENTS_BEST>, dim3(blocks), dim3(LG_BLOCK), lds, stream, P, N);
    return hipGetLastError();
}
hipError_t segments_occupancy(bool touch_only, uint32_t stack_depth, int *blocks_per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, segments_function(touch_only), LG_BLOCK, segments_lds_bytes(stack_depth));
}
// the dynamic LDS a launch of either form may ask for, raised once per device where the stack needs more than the default 64 KiB
hipError_t segments_set_lds_limit(size_t bytes) {
    for (int t = 0; t < 2; ++t) {
        const hipError_t e = hipFuncSetAttribute(segments_function(t != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace lg
