// lasgun_amd/csrc/closest_prim.h -- the per-primitive arithmetic of lg_closest_points* (include/lasgun_hip.h has the contract): the closest
// point of a triangle, of a box taken as twelve triangles, of a sphere, and the rule that decides between two candidates.  All f64, nothing
// fused (the whole product is built with -ffp-contract=off), dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as everywhere.  Host and device: ONE
// text for k_closest.hip and for tools/closest_prim_check.cpp, which runs it under AddressSanitizer / UBSan on the CPU against the numpy
// restatement (tests/closest_ref.py) word for word.
#pragma once
#include "vecmath.h"

// tools/closest_prim_check.cpp alone is also built with 1, 2 and 3: one seeded fault each (a `<` for a `<=` in a region test, a fused
// product, a swapped tie), which tests/test_closest_prim_host.py must see caught.  The product is built with 0.
#ifndef LG_CLOSEST_FAULT
#define LG_CLOSEST_FAULT 0
#endif

namespace lg {

struct ClosestPt {
    V3 x;      // the closest point
    double d2; // dot(q - x, q - x)
};

// Ericson, Real-Time Collision Detection, section 5.1.5, in the header's operation order: the seven regions in turn
LG_HD V3 closest_on_triangle(V3 q, V3 a, V3 b, V3 c) {
    const V3 ab = b - a, ac = c - a, ap = q - a;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return a;
    const V3 bp = q - b;
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
#if LG_CLOSEST_FAULT == 1
    if (d3 >= 0.0 && d4 < d3) return b;
#else
    if (d3 >= 0.0 && d4 <= d3) return b;
#endif
#if LG_CLOSEST_FAULT == 2
    const double vc = fma(d1, d4, -(d3 * d2));
#else
    const double vc = d1 * d4 - d3 * d2;
#endif
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return a + ab * (d1 / (d1 - d3));
    const V3 cp = q - c;
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return c;
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return a + ac * (d2 / (d2 - d6));
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) return b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)));
    const double den = 1.0 / ((va + vb) + vc);
    return (a + ab * (vb * den)) + ac * (vc * den);
}
LG_HD ClosestPt closest_triangle(V3 q, V3 a, V3 b, V3 c) {
    const V3 x = closest_on_triangle(q, a, b, c);
    const V3 e = q - x;
    return ClosestPt{x, dot(e, e)};
}

// A box: corner k of w[] has the box's max on axis x / y / z where bit 0 / 1 / 2 of k is set (its min otherwise), taken to world space.  The
// faces in the order -x, +x, -y, +y, -z, +z, each cut by the diagonal from its lowest-numbered corner to its highest; the lowest d2 wins,
// the first triangle a tie.  A d2 that is NaN never replaces anything; all twelve NaN: d2 = NaN.
LG_HD void closest_box_triangle(int t, int &i, int &j, int &k) {
    // (written as arithmetic, not as a table: a constant array indexed at run time would live in scratch on the device)
    const int face = t >> 1, axis = face >> 1, hi = face & 1, second = t & 1;
    // the face's two other axes as corner bits, lower bit first: x: (y, z) = (2, 4); y: (x, z) = (1, 4); z: (x, y) = (1, 2)
    const int ub = axis == 0 ? 2 : 1, vb = axis == 2 ? 2 : 4;
    const int base = hi << axis;
    i = base;
    j = second ? base + ub + vb : base + ub;
    k = second ? base + vb : base + ub + vb;
}
LG_HD ClosestPt closest_box(V3 q, const V3 w[8]) {
    ClosestPt best{V3{0.0, 0.0, 0.0}, NAN};
    bool have = false;
    for (int t = 0; t < 12; ++t) {
        int i, j, k;
        closest_box_triangle(t, i, j, k);
        const ClosestPt c = closest_triangle(q, w[i], w[j], w[k]);
        if (!(c.d2 == c.d2)) continue;
        if (!have || c.d2 < best.d2) { best = c; have = true; }
    }
    return best;
}

// A sphere under a similarity: cw the world centre, pw the world image of centre + (r, 0, 0)
LG_HD ClosestPt closest_sphere(V3 q, V3 cw, V3 pw) {
    const V3 pc = pw - cw;
    const double rw = sqrt(dot(pc, pc));
    const V3 v = q - cw;
    const double l = sqrt(dot(v, v));
    const double d = fabs(l - rw);
    ClosestPt c;
    c.d2 = d * d;
    c.x = l == 0.0 ? pw : cw + v * (rw / l);
    return c;
}

// The winner so far and the rule between two candidates.  `key` orders exact ties: instance, then kind (lg_hit's: 1 sphere, 2 box,
// 3 triangle), then prim -- one 64-bit word compares all three (an instance is below 2^30, a kind below 4, prim fills the low 32 bits).
struct ClosestBest {
    double d2;              // +INF: nothing admissible yet
    V3 x;
    unsigned long long key; // instance << 34 | kind << 32 | prim
};
LG_HD unsigned long long closest_key(uint32_t instance, uint32_t kind, uint32_t prim) {
    return ((unsigned long long)instance << 34) | ((unsigned long long)kind << 32) | (unsigned long long)prim;
}
LG_HD ClosestBest closest_none() { return ClosestBest{INFINITY, V3{0.0, 0.0, 0.0}, ~0ull}; }
// admissible iff d2 <= r2 and d2 < +INF (a NaN fails both); smaller d2 wins, an exact tie goes to the smaller key
LG_HD void closest_offer(ClosestBest &b, const ClosestPt &c, double r2, unsigned long long key) {
    if (!(c.d2 <= r2 && c.d2 < INFINITY)) return;
#if LG_CLOSEST_FAULT == 3
    if (c.d2 < b.d2 || (c.d2 == b.d2 && key > b.key)) { b.d2 = c.d2; b.x = c.x; b.key = key; }
#else
    if (c.d2 < b.d2 || (c.d2 == b.d2 && key < b.key)) { b.d2 = c.d2; b.x = c.x; b.key = key; }
#endif
}

} // namespace lg
