// lasgun_amd/csrc/closest_host.h -- the part of lg_closest_points* (query.cpp; k_closest.hip) that touches no device: the one table of
// lg_closest_out's planes (closest_planes) with the NULL and alignment rules that follow from it (the rules themselves and the host form's
// staging are planes_host.h's), the call's checks in their refusal order (check_closest), the sphere gate (lg_scene_closest_gate), and what
// the kernel's walk is given beside the scene's tables: per accel the three constants of its pruning test -- shrink, delta, omega, derived in
// DESIGN.md section 3.7 --, the largest point magnitude the walk prunes for (qmax) and the depth of its per-lane stack for ITS push rule.
// Arithmetic on size_t that can overflow, tree walks over indices and bounds that have to hold, so kept free of HIP:
// tools/closest_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and the entry points call it.
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/lasgun_hip.h"
#include "dscene.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_closest_out) == 24 && offsetof(lg_closest_out, distance) == 0 && offsetof(lg_closest_out, point) == 8 && offsetof(lg_closest_out, id) == 16,
              "lg_closest_out: three pointers, 24 bytes");

// The three planes of lg_closest_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order
template <class Out, class F> inline void closest_planes(Out &out, size_t n, F &&f) {
    f(out.distance, n, 8, "distance");
    f(out.point, n * 3, 8, "point");
    f(out.id, n * 4, 16, "id");
}

// Everything the contract calls an error that needs neither a device nor the scene, thrown here in the contract's order; n is not 0 (an
// empty set is answered before this).  After it no count or size of closest_planes wraps.
inline void check_closest(const void *accel, const double *points, size_t n, double radius, const lg_closest_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!points) throw std::runtime_error("points is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { closest_planes(*out, 0, f); });
    if (!(radius >= 0.0)) throw std::runtime_error("radius is NaN or negative (+INF: no limit)");
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many points in one query");
    (void)checked_bytes(n, 3 * sizeof(double), "points"); // 24 bytes a row: the widest (points, point)
}
// The device form's alignment rule: points 8 bytes, the planes theirs (distance and point 8; id 16); NULL is not misaligned
inline void check_closest_alignment(const double *points, const lg_closest_out &out) {
    check_alignment(points, 8, "points");
    check_planes_alignment([&](auto &&f) { closest_planes(out, 0, f); });
}

// ---- what the kernel is given ---------------------------------------------------------------------------------------------------------
// Per accel A, for a point q whose coordinates in A's local space are q_A (the stored inverse transforms applied root first, each with a
// running rounding bound e the walk carries): no primitive below a box B of A's tree yields a candidate of squared distance below LB^2,
//   LB = shrink * ((dist(q_A, B) * (1 - 2^-40) - 2 e) - delta) - omega - 2^-44 |q|_inf
// (k_closest.hip, closest_skip; DESIGN.md section 3.7 has the derivation).  shrink = 0: nothing of this accel's own tree is ever skipped.
struct ClosestAccel {
    double shrink; // <= 1 / ||K||_2, K the linear part of world -> local as the walk applies it; also <= sigma_min of local -> world
    double delta;  // local units: how far world -> local after local -> world may move a point of A's root box, plus the boxes' own rounding
    double omega;  // world units: rounding of the transformed vertices, of the closest-point arithmetic on them and of a sphere's radius, of A and of every accel below it
    double pad;
};
constexpr uint32_t CLOSEST_MAX_DEPTH = LG_CLOSEST_MAX_DEPTH;       // entries of the per-lane stack that fit (2 words x 256 lanes each: 2 KiB an entry, 128 KiB)
constexpr double CLOSEST_GATE_REL = 0x1p-40;      // the sphere gate: L^T L within this, relative, of s^2 I
constexpr double CLOSEST_COND_MAX = 0x1p20;       // a chain worse conditioned than this proves no shrink
constexpr double CLOSEST_ALTITUDE_RANGE = 0x1p28; // the walk prunes for |q|_inf + (the scene's magnitude) <= this * (the smallest altitude of any triangle)
constexpr double CLOSEST_RANGE = 0x1p100;         // magnitudes beyond [1 / this, this] -- the scene's coordinates, a triangle's altitude, a sphere's world radius --: walked unpruned (as PRUNE_RANGE)

struct ClosestTables {
    std::vector<ClosestAccel> accel; // one per accel
    double qmax = -1.0;              // the walk prunes for points with |q|_inf <= qmax (-1: never)
    uint32_t depth = 1;              // per-lane stack entries, for the kernel's push rule
    int refused = -1;                // the gate: the first accel that holds a sphere under a chain that is no similarity; -1 none
};

namespace closest_detail {
typedef long double ld;
struct Aff { ld m[3][4]; }; // row-major 3 x 4: x' = m[i][0..2] . x + m[i][3]
inline Aff aff_of(const Affine &a) {
    Aff r;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) r.m[i][j] = (ld)a.c[j][i];
    return r;
}
inline Aff aff_identity() { Aff r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) r.m[i][j] = i == j ? 1.0L : 0.0L; return r; }
// a after b: x -> a(b(x))
inline Aff aff_mul(const Aff &a, const Aff &b) {
    Aff r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            ld s = j == 3 ? a.m[i][3] : 0.0L;
            for (int k = 0; k < 3; ++k) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
inline Aff aff_abs(const Aff &a) { Aff r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) r.m[i][j] = fabsl(a.m[i][j]); return r; }
inline ld frob3(const Aff &a) { ld s = 0; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) s += a.m[i][j] * a.m[i][j]; return sqrtl(s); }
inline bool inverse3(const Aff &a, Aff &inv) {
    const ld (*m)[4] = a.m;
    const ld c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const ld det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    if (!(det != 0.0L) || !std::isfinite((double)det)) return false;
    inv = aff_identity();
    inv.m[0][0] = c00 / det; inv.m[1][0] = c01 / det; inv.m[2][0] = c02 / det;
    inv.m[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; inv.m[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; inv.m[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    inv.m[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det; inv.m[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det; inv.m[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    return true;
}
// local -> world of accel a as one matrix (root's transform outermost), in long double
inline Aff world_of(const DAccel *accels, size_t n_accels, uint32_t a) {
    Aff w = aff_identity();
    const DAccel &A = accels[a];
    if (A.nchain < 1 || A.nchain > (uint32_t)MAX_CHAIN) throw std::runtime_error("closest tables: an accel's chain length is out of range");
    for (uint32_t s = 0; s < A.nchain; ++s) {
        if (A.chain[s] >= n_accels) throw std::runtime_error("closest tables: an accel's chain names no accel");
        w = aff_mul(w, aff_of(accels[A.chain[s]].m));
    }
    return w;
}
// Is the 3 x 3 part of `w` a similarity: w^T w within CLOSEST_GATE_REL, relative, of s2 * I?  Every singular value of it then lies within
// sqrt(s2) * (1 -+ 2^-39) (Weyl: the eigenvalues of w^T w move by at most 3 * 2^-40 s2).
inline bool similarity(const Aff &w, ld *scale2 = nullptr) {
    ld s[3][3], big = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            s[i][j] = 0;
            for (int k = 0; k < 3; ++k) s[i][j] += w.m[k][i] * w.m[k][j];
        }
    const ld s2 = (s[0][0] + s[1][1] + s[2][2]) / 3.0L;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) big = fmaxl(big, fabsl(s[i][j] - (i == j ? s2 : 0.0L)));
    if (scale2) *scale2 = s2;
    return s2 > 0.0L && big <= (ld)CLOSEST_GATE_REL * s2; // (a NaN fails)
}
// An upper bound of the largest singular value of the 3 x 3 part of `a`: its scale where it is a similarity, its Frobenius norm otherwise
inline ld norm2_above(const Aff &a) {
    ld s2 = 0;
    return similarity(a, &s2) ? sqrtl(s2) * (1.0L + 0x1p-30L) : frob3(a);
}
// A lower bound of the smallest singular value of the 3 x 3 part of `w`, rounded down: sigma_min(w) = 1 / ||w^-1||_2 >= 1 / ||w^-1||_F (its
// scale where `w` is a similarity), and never above 1 / ||k||_2 for `k` (may be null) the stored inverse chain; 0 where nothing is proven
inline double shrink_of(const Aff &w, const Aff *k) {
    Aff inv;
    if (!inverse3(w, inv)) return 0.0;
    const ld cond = frob3(w) * frob3(inv);
    if (!(cond <= (ld)CLOSEST_COND_MAX)) return 0.0;
    ld f = norm2_above(inv);
    if (k) { const ld fk = norm2_above(*k); if (!(fk == fk)) return 0.0; if (fk > f) f = fk; }
    const double s = (double)((1.0L - 0x1p-20L) / f);
    return std::isfinite(s) && s > 0.0 ? s : 0.0;
}
inline V3 to_world(const DAccel *accels, uint32_t a, V3 x) { // W_A as the kernel applies it
    for (int32_t i = (int32_t)a; i >= 0; i = accels[i].parent) x = xf_point(accels[i].m, x);
    return x;
}
// the smallest altitude of triangle (a, b, c): 2 area / longest edge; +INF for a triangle with a repeated vertex (harmless to the walk:
// the header's steps 1-3 answer it with a vertex, an edge point or NaN)
inline double altitude(V3 a, V3 b, V3 c) {
    if (veq(a, b) || veq(b, c) || veq(a, c)) return INFINITY;
    const V3 ab = b - a, ac = c - a, bc = c - b;
    const double e2 = std::fmax(dot(ab, ab), std::fmax(dot(ac, ac), dot(bc, bc)));
    const V3 n = cross(ab, ac);
    const double h = std::sqrt(dot(n, n)) / std::sqrt(e2);
    return h == h ? h : 0.0;
}
} // namespace closest_detail

// A view of the flattened scene's tables (host.h, FlatScene), so that this header needs no more than dscene.h
struct ClosestScene {
    const DAccel *accels; size_t n_accels;
    const DNode *nodes; size_t n_nodes;
    const uint32_t *primref; size_t n_primref;
    const DLeafRec *leaf_soup; size_t n_soup;
};

// Everything of ClosestTables; throws where a table names something out of range (nothing is read beyond the counts given)
inline ClosestTables closest_tables(const ClosestScene &S) {
    using namespace closest_detail;
    ClosestTables T;
    const size_t na = S.n_accels;
    if (na == 0 || na > PRIM_INDEX_MASK) throw std::runtime_error("closest tables: no accel");
    T.accel.assign(na, ClosestAccel{0.0, 0.0, 0.0, 0.0});
    std::vector<double> own_omega(na, 0.0), wmag(na, 0.0);
    std::vector<uint32_t> need(na, 0u);
    std::vector<char> done(na, 0);
    double hmin = INFINITY, scene_mag = 0.0, rw_min = INFINITY; // rw_min: the smallest world radius of any sphere (its scale: ||W||_F / sqrt(3), exact under a similarity)
    bool ranges_ok = true;

    // one accel: its tree walked once -- the stack need of its own tree (children's added below), its spheres' largest radius, its
    // primitives' smallest world-space altitude -- then its constants
    struct Walk { uint32_t node, depth; };
    // children first: accels are numbered parents first, so from the last to the first every child is done before its parent
    for (size_t ai = na; ai-- > 0;) {
        const uint32_t a = (uint32_t)ai;
        const DAccel &A = S.accels[a];
        if (A.node_base >= S.n_nodes) throw std::runtime_error("closest tables: an accel's tree lies outside the node table");
        if (A.parent >= (int32_t)a) throw std::runtime_error("closest tables: an accel's parent does not precede it");
        double rmax = 0.0, rmin = INFINITY;
        bool has_sphere = false;
        // need(node): the most entries the walk holds above its base while it works on the subtree of `node` (held in registers).
        // Interior: one pushed sibling while it is in either child.  Leaf: every nested accel of it pushed, then taken last first.
        // Iterative, over (node, entries already on the stack): the answer is the largest sum seen.
        uint32_t worst = 0;
        std::vector<Walk> todo{Walk{0u, 0u}};
        size_t visited = 0;
        while (!todo.empty()) {
            const Walk w = todo.back();
            todo.pop_back();
            if (++visited > S.n_nodes) throw std::runtime_error("closest tables: a tree does not end");
            const size_t ni = (size_t)A.node_base + w.node;
            if (ni >= S.n_nodes) throw std::runtime_error("closest tables: a node lies outside the node table");
            const DNode &N = S.nodes[ni];
            if (!(N.meta & NODE_LEAF)) {
                worst = std::max(worst, w.depth + 1u);
                todo.push_back(Walk{w.node + 1u, w.depth + 1u});
                todo.push_back(Walk{N.link, w.depth + 1u});
                continue;
            }
            const uint32_t count = N.meta & 0xFFFFu;
            uint32_t nested = 0;
            for (uint32_t k = 0; k < count; ++k) {
                const size_t slot = (size_t)A.prim_base + N.link + k;
                if (slot >= S.n_primref || slot >= S.n_soup) throw std::runtime_error("closest tables: a leaf lies outside the primitive table");
                const uint32_t ref = S.primref[slot], kind = ref >> 30, idx = ref & PRIM_INDEX_MASK;
                const DLeafRec &rec = S.leaf_soup[slot];
                if (kind == PK_ACCEL) {
                    if (idx >= na || idx <= a || !done[idx]) throw std::runtime_error("closest tables: a nested accel does not follow its parent");
                    worst = std::max(worst, w.depth + nested + 1u + need[idx]); // `nested` entries of this leaf stay below it while it is walked
                    ++nested;
                } else if (kind == PK_SPHERE) {
                    double d[4];
                    std::memcpy(d, rec.w, sizeof d);
                    has_sphere = true;
                    rmax = std::fmax(rmax, std::fabs(d[3]));
                    rmin = std::fmin(rmin, std::fabs(d[3]));
                } else if (kind == PK_CUBOID) {
                    double d[6];
                    std::memcpy(d, rec.w, sizeof d);
                    V3 c[8];
                    for (int q = 0; q < 8; ++q) c[q] = to_world(S.accels, a, V3{d[(q & 1) ? 3 : 0], d[(q & 2) ? 4 : 1], d[(q & 4) ? 5 : 2]});
                    static const int tri[12][3] = {{0, 2, 6}, {0, 6, 4}, {1, 3, 7}, {1, 7, 5}, {0, 1, 5}, {0, 5, 4}, {2, 3, 7}, {2, 7, 6}, {0, 1, 3}, {0, 3, 2}, {4, 5, 7}, {4, 7, 6}};
                    for (const auto &t : tri) hmin = std::fmin(hmin, altitude(c[t[0]], c[t[1]], c[t[2]]));
                } else {
                    float f[9];
                    std::memcpy(f, rec.w, sizeof f);
                    V3 v[3];
                    for (int q = 0; q < 3; ++q) v[q] = to_world(S.accels, a, V3{(double)f[3 * q], (double)f[3 * q + 1], (double)f[3 * q + 2]});
                    hmin = std::fmin(hmin, altitude(v[0], v[1], v[2]));
                }
            }
            worst = std::max(worst, w.depth + nested);
        }
        need[a] = worst;
        done[a] = 1;

        // ---- the gate
        const Aff W = world_of(S.accels, na, a);
        if (has_sphere && !similarity(W)) T.refused = (int)a; // (descending: the last one set is the first offender)

        // ---- the constants.  G: world -> local as the walk applies it (the STORED inverses, root first)
        Aff G = aff_identity(), Gabs = aff_identity(), Wabs = aff_identity();
        for (uint32_t s = 0; s < A.nchain; ++s) {
            const Aff n = aff_of(S.accels[A.chain[s]].minv);
            G = aff_mul(n, G);
            Gabs = aff_mul(aff_abs(n), Gabs);
            Wabs = aff_mul(Wabs, aff_abs(aff_of(S.accels[A.chain[s]].m)));
        }
        const DNode &R = S.nodes[A.node_base];
        ld cmax[3], cbig = 0;
        for (int k = 0; k < 3; ++k) { cmax[k] = fmaxl(fabsl((ld)R.bmin[k]), fabsl((ld)R.bmax[k])); cbig = fmaxl(cbig, cmax[k]); }
        // delta: sup over the root box of |G(W(y)) - y|_2 <= sqrt(3) max_i (sum_j |D_ij| cmax_j + |D_i3|), D = G W - I, plus what long
        // double arithmetic may have lost of D (2^-58 of the same product taken over absolute values), plus the boxes' own rounding
        const Aff D = aff_mul(G, W), Dabs = aff_mul(Gabs, Wabs);
        ld drow = 0, arow = 0;
        for (int i = 0; i < 3; ++i) {
            ld d = fabsl(D.m[i][3]), m = Dabs.m[i][3];
            for (int j = 0; j < 3; ++j) { d += fabsl(D.m[i][j] - (i == j ? 1.0L : 0.0L)) * cmax[j]; m += Dabs.m[i][j] * cmax[j]; }
            drow = fmaxl(drow, d); arow = fmaxl(arow, m);
        }
        const double delta = (double)(2.0L * (drow + 0x1p-58L * arow) + 0x1p-48L * cbig);
        // omega: the rounding of W_A(x) as the kernel forms it, one xf_point a stage from A up to the root: err' = ||M||_inf err + 2^-50 mag',
        // mag' = |M| mag + |t| the componentwise bound of the stage's result; then 2^-44 of the world magnitude for the closest-point
        // arithmetic, and a sphere's radius under a chain the gate let pass (2^-38 of it)
        ld mag[3] = {cmax[0], cmax[1], cmax[2]}, err = 0;
        for (int32_t i = (int32_t)a; i >= 0; i = S.accels[i].parent) {
            const Aff m = aff_abs(aff_of(S.accels[i].m));
            ld next[3], rn = 0, big = 0;
            for (int r = 0; r < 3; ++r) {
                next[r] = (m.m[r][0] * mag[0] + m.m[r][1] * mag[1] + m.m[r][2] * mag[2]) + m.m[r][3];
                rn = fmaxl(rn, m.m[r][0] + m.m[r][1] + m.m[r][2]);
                big = fmaxl(big, next[r]);
            }
            err = rn * err + 0x1p-50L * big;
            for (int r = 0; r < 3; ++r) mag[r] = next[r];
        }
        const ld wm = fmaxl(mag[0], fmaxl(mag[1], mag[2]));
        wmag[a] = (double)wm;
        own_omega[a] = (double)(4.0L * err + 0x1p-44L * wm + 0x1p-38L * frob3(W) * (ld)rmax);
        if (has_sphere) rw_min = std::fmin(rw_min, (double)(frob3(W) / sqrtl(3.0L)) * rmin);
        const double shrink = shrink_of(W, &G);
        T.accel[a] = ClosestAccel{shrink, delta, own_omega[a], 0.0};
        scene_mag = std::fmax(scene_mag, wmag[a]);
        if (!(std::isfinite(delta) && std::isfinite(own_omega[a]) && wmag[a] <= CLOSEST_RANGE)) ranges_ok = false;
    }
    // omega of an accel covers every accel below it: parents follow their children from the last to the first
    for (size_t ai = na; ai-- > 1;) {
        const int32_t p = S.accels[ai].parent;
        if (p >= 0) T.accel[(size_t)p].omega = std::fmax(T.accel[(size_t)p].omega, T.accel[ai].omega);
    }
    T.depth = need[0] + 1u; // ... and the root's own entry
    if (ranges_ok && hmin >= 1.0 / CLOSEST_RANGE && rw_min >= 1.0 / CLOSEST_RANGE) { // (a scene without spheres: rw_min = +INF)
        const double q = std::fmin(CLOSEST_RANGE, CLOSEST_ALTITUDE_RANGE * hmin) - scene_mag;
        T.qmax = q > 0.0 ? q : -1.0;
    }
    return T;
}

// The gate alone with the shrink bound, for lg_scene_closest_gate: shrink[a] for a < min(cap, accels)
inline int closest_gate(const ClosestScene &S, double *shrink, int cap) {
    const ClosestTables T = closest_tables(S);
    for (size_t a = 0; shrink && a < S.n_accels && (long long)a < (long long)cap; ++a) shrink[a] = T.accel[a].shrink;
    return T.refused;
}

} // namespace lg
