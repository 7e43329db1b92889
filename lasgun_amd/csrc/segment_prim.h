// lasgun_amd/csrc/segment_prim.h -- the per-primitive arithmetic of lg_closest_segments* (include/lasgun_hip.h has the contract): the
// candidate (d2, s, x) of a segment p0 .. p1 against a triangle, against a box taken as closest_prim.h's twelve triangles, against a sphere,
// and the rule that decides between two candidates.  x lies ON THE PRIMITIVE, s is the parameter of the segment's own closest point
// p0 + (p1 - p0) * s.  All f64, nothing fused, dot and cross are vecmath.h's.  Host and device: ONE text for k_segments.hip and for
// tools/segment_prim_check.cpp, which runs it under AddressSanitizer / UBSan on the CPU against the numpy restatement
// (tests/segment_ref.py) word for word.
//
// Apart from the exact +0.0 of a crossing (a pierced triangle, a sphere's surface between lmin and lmax), every d2 is the squared length
// between a FORMED point of the segment and a FORMED point of the primitive, never an algebraic shortcut: such a value can fall below the
// true distance of segment and primitive only by the forward rounding of forming the two points and their difference, whatever the
// conditioning (parallel segments included).  The walk's pruning rests on this ("Segment proximity").
//
// A segment with p0 == p1 in all three components is a point: its candidate is closest_prim.h's own for p0, with s = +0.0.
#pragma once
#include "closest_prim.h"

// tools/segment_prim_check.cpp alone is also built with 1, 2 and 3: one seeded fault each (a `<` for a `<=` in the parameter clamp, a fused
// product in the segment-segment denominator, a swapped tie between sub-candidates), which tests/test_segment_prim_host.py must see caught.
// The product is built with 0.
#ifndef LG_SEGMENT_FAULT
#define LG_SEGMENT_FAULT 0
#endif

#if defined(__HIPCC__)
#define LG_SEG_LOOP _Pragma("unroll 1")
#else
#define LG_SEG_LOOP
#endif

namespace lg {

struct SegPt {
    V3 x;      // the candidate's point on the primitive
    double s;  // the segment's parameter, +0.0 .. 1.0 (never -0.0: every parameter leaves through seg_clamp01 or is a literal)
    double d2; // the squared distance; NaN: no candidate
};

// a parameter clamped to [0, 1]; a NaN stays a NaN; -0.0 becomes +0.0
LG_HD double seg_clamp01(double x) {
#if LG_SEGMENT_FAULT == 1
    return x < 0.0 ? 0.0 : (x >= 1.0 ? 1.0 : x);
#else
    return x <= 0.0 ? 0.0 : (x >= 1.0 ? 1.0 : x);
#endif
}

// lowest d2 wins, the first a tie, a NaN never replaces anything
LG_HD bool seg_take(SegPt &best, bool &have, const SegPt &c) {
    if (!(c.d2 == c.d2)) return false;
#if LG_SEGMENT_FAULT == 3
    if (!(!have || c.d2 <= best.d2)) return false;
#else
    if (!(!have || c.d2 < best.d2)) return false;
#endif
    best = c;
    have = true;
    return true;
}

// Ericson, Real-Time Collision Detection, section 5.1.9 (ClosestPtSegmentSegment) with EPSILON = 0, the segment p0 .. p1 against the edge
// e0 .. e1, in this order:
//   d1=p1-p0, d2=e1-e0, r=p0-e0; a=dot(d1,d1), e=dot(d2,d2), f=dot(d2,r).
//   a<=0 && e<=0: s=0, t=0.   a<=0: s=0, t=clamp(f/e).   otherwise c=dot(d1,r) and
//     e<=0: t=0, s=clamp(-c/a).
//     otherwise b=dot(d1,d2), denom=a*e-b*b; s = denom!=0 ? clamp((b*f-c*e)/denom) : 0; t=(b*s+f)/e;
//       t<0: t=0, s=clamp(-c/a);   t>1: t=1, s=clamp((b-c)/a).
//   c1=p0+d1*s, c2=e0+d2*t, w=c1-c2: d2 = dot(w,w), x = c2.
LG_HD SegPt seg_edge(V3 p0, V3 p1, V3 e0, V3 e1) {
    const V3 d1 = p1 - p0, d2 = e1 - e0, r = p0 - e0;
    const double a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r);
    double s, t;
    if (a <= 0.0 && e <= 0.0) { s = 0.0; t = 0.0; }
    else if (a <= 0.0) { s = 0.0; t = seg_clamp01(f / e); }
    else {
        const double c = dot(d1, r);
        if (e <= 0.0) { t = 0.0; s = seg_clamp01(-c / a); }
        else {
            const double b = dot(d1, d2);
#if LG_SEGMENT_FAULT == 2
            const double denom = fma(a, e, -(b * b));
#else
            const double denom = a * e - b * b;
#endif
            s = denom != 0.0 ? seg_clamp01((b * f - c * e) / denom) : 0.0;
            t = (b * s + f) / e;
            if (t < 0.0) { t = 0.0; s = seg_clamp01(-c / a); }
            else if (t > 1.0) { t = 1.0; s = seg_clamp01((b - c) / a); }
        }
    }
    const V3 c1 = p0 + d1 * s, c2 = e0 + d2 * t, w = c1 - c2;
    return SegPt{c2, s, dot(w, w)};
}

// Does the segment cross the triangle?  Ericson 5.3.6 (IntersectSegmentTriangle) made two-sided, then CONFIRMED on formed points, in this order:
//   ab=b-a, ac=c-a, qp=p0-p1; n=cross(ab,ac); d=dot(qp,n); ap=p0-a; t=dot(ap,n); e=cross(qp,ap); v=dot(ac,e); w=-dot(ab,e);
//   d<0: d, t, v, w all negated (d<+INF: a normal that overflowed proves nothing).
//   verdict: d>0 && d<+INF && t>=0 && t<=d && v>=0 && w>=0 && v+w<=d;   s=clamp(t/d), y=p0+(p1-p0)*s.
//   confirmed: closest_triangle(y, a, b, c).d2 <= g*g, g = 2^-46 * M, M the largest |component| of y, a, b, c (fmax: a NaN is ignored).
//   crosses iff verdict && confirmed: d2=+0.0, x=y.
// The signs alone are noise for a segment that lies (nearly) in the triangle's plane, wherever it lies there; the confirmation makes a
// false "crosses" a statement about formed points: the segment's point y is within 2^-46 M of the triangle.  A true crossing at a grazing
// angle may fail it (y is off by about 2^-52 |p0-a| / sin(angle)): the other five sub-candidates then answer, with a d2 above zero that is
// a formed distance.
LG_HD double seg_inf3(V3 v) { return fmax(fabs(v.x), fmax(fabs(v.y), fabs(v.z))); }
LG_HD bool seg_pierce(V3 p0, V3 p1, V3 a, V3 b, V3 c, SegPt &out) {
    const V3 ab = b - a, ac = c - a, qp = p0 - p1;
    const V3 n = cross(ab, ac);
    double d = dot(qp, n);
    const V3 ap = p0 - a;
    double t = dot(ap, n);
    const V3 e = cross(qp, ap);
    double v = dot(ac, e), w = -dot(ab, e);
    if (d < 0.0) { d = -d; t = -t; v = -v; w = -w; }
    if (!(d > 0.0 && d < INFINITY && t >= 0.0 && t <= d && v >= 0.0 && w >= 0.0 && (v + w) <= d)) return false;
    const double s = seg_clamp01(t / d);
    const V3 y = p0 + (p1 - p0) * s;
    const double g = 0x1p-46 * fmax(fmax(seg_inf3(y), seg_inf3(a)), fmax(seg_inf3(b), seg_inf3(c)));
    if (!(closest_triangle(y, a, b, c).d2 <= g * g)) return false;
    out = SegPt{y, s, 0.0};
    return true;
}

// A triangle: six sub-candidates in a fixed order -- 1 the crossing; 2, 3 closest_triangle of p0 (s = 0) and of p1 (s = 1); 4, 5, 6 the
// segment against the edges ab, bc, ca --, the lowest d2 wins, the first a tie.  `which` (1 .. 6; 0: the point form; -1: all NaN) is for
// the tests alone.
LG_HD SegPt seg_triangle(V3 p0, V3 p1, V3 a, V3 b, V3 c, int *which = nullptr) {
    if (veq(p0, p1)) {
        const ClosestPt cp = closest_triangle(p0, a, b, c);
        if (which) *which = 0;
        return SegPt{cp.x, 0.0, cp.d2};
    }
    SegPt best{V3{0.0, 0.0, 0.0}, 0.0, NAN}, cand;
    bool have = false;
    int w = -1;
    if (seg_pierce(p0, p1, a, b, c, cand) && seg_take(best, have, cand)) w = 1;
    LG_SEG_LOOP
    for (int i = 0; i < 2; ++i) {
        const ClosestPt cp = closest_triangle(i ? p1 : p0, a, b, c);
        if (seg_take(best, have, SegPt{cp.x, i ? 1.0 : 0.0, cp.d2})) w = 2 + i;
    }
    LG_SEG_LOOP
    for (int j = 0; j < 3; ++j) {
        const V3 e0 = j == 0 ? a : (j == 1 ? b : c), e1 = j == 0 ? b : (j == 1 ? c : a);
        if (seg_take(best, have, seg_edge(p0, p1, e0, e1))) w = 4 + j;
    }
    if (which) *which = w;
    return best;
}

// A box: w0 .. w7 are closest_prim.h's corners 0 .. 7 in world space; its twelve triangles in closest_box_triangle's order, the lowest d2
// wins, the first triangle a tie, a NaN never replaces anything; all twelve NaN: d2 = NaN.  A loop, not a table: twelve times six
// sub-candidates; the corners are eight values chosen by selects, not an array indexed by the loop's counter (which would live in scratch
// on the device).  A segment wholly inside a box gets the distance to its surface.
LG_HD V3 seg_corner(int k, V3 w0, V3 w1, V3 w2, V3 w3, V3 w4, V3 w5, V3 w6, V3 w7) {
    const V3 lo = (k & 2) ? ((k & 1) ? w3 : w2) : ((k & 1) ? w1 : w0), hi = (k & 2) ? ((k & 1) ? w7 : w6) : ((k & 1) ? w5 : w4);
    return (k & 4) ? hi : lo;
}
LG_HD SegPt seg_box(V3 p0, V3 p1, V3 w0, V3 w1, V3 w2, V3 w3, V3 w4, V3 w5, V3 w6, V3 w7) {
    SegPt best{V3{0.0, 0.0, 0.0}, 0.0, NAN};
    bool have = false;
    LG_SEG_LOOP
    for (int t = 0; t < 12; ++t) {
        int i, j, k;
        closest_box_triangle(t, i, j, k);
        const SegPt c = seg_triangle(p0, p1, seg_corner(i, w0, w1, w2, w3, w4, w5, w6, w7), seg_corner(j, w0, w1, w2, w3, w4, w5, w6, w7),
                                     seg_corner(k, w0, w1, w2, w3, w4, w5, w6, w7));
        if (!(c.d2 == c.d2)) continue;
        if (!have || c.d2 < best.d2) { best = c; have = true; } // (not seg_take: the seeded tie fault is the sub-candidates')
    }
    return best;
}

// A sphere under a similarity: cw the world centre, pw the world image of centre + (r, 0, 0), rw as closest_sphere forms it.
//   pc=pw-cw, rw=sqrt(dot(pc,pc)); u=p1-p0, uu=dot(u,u); v0=p0-cw, v1=p1-cw; tt=dot(cw-p0,u); s* = uu>0 ? clamp(tt/uu) : 0;
//   m=p0+u*s*, vm=m-cw, lmin=sqrt(dot(vm,vm)); l0=sqrt(dot(v0,v0)), l1=sqrt(dot(v1,v1)); the far endpoint is p1 iff l1>l0 (p0 on a tie), lmax its l.
//   lmin>rw:  d=lmin-rw, d2=d*d, x=cw+vm*(rw/lmin), s=s*.
//   lmax<rw:  d=rw-lmax, d2=d*d, x=cw+v*(rw/lmax) with the far endpoint's v (pw where lmax==0), s=0 or 1.
//   lmin<=rw && lmax>=rw && lmax<+INF: the segment crosses the surface, d2=+0.0.  B=dot(v0,u), C=dot(v0,v0)-rw*rw, disc=B*B-uu*C, q=sqrt(disc),
//     s1=(-B-q)/uu, s2=(-B+q)/uu: s = clamp(s1) where 0<=s1<=1, else clamp(s2) where 0<=s2<=1, and x=p0+u*s; neither (rounding): s=s*, x=m.
//   otherwise (a NaN): d2=NaN.
LG_HD SegPt seg_sphere(V3 p0, V3 p1, V3 cw, V3 pw) {
    if (veq(p0, p1)) {
        const ClosestPt cp = closest_sphere(p0, cw, pw);
        return SegPt{cp.x, 0.0, cp.d2};
    }
    const V3 pc = pw - cw;
    const double rw = sqrt(dot(pc, pc));
    const V3 u = p1 - p0;
    const double uu = dot(u, u);
    const V3 v0 = p0 - cw, v1 = p1 - cw;
    const double tt = dot(cw - p0, u);
    const double sstar = uu > 0.0 ? seg_clamp01(tt / uu) : 0.0;
    const V3 m = p0 + u * sstar, vm = m - cw;
    const double lmin = sqrt(dot(vm, vm));
    const double l0 = sqrt(dot(v0, v0)), l1 = sqrt(dot(v1, v1));
    const bool far1 = l1 > l0;
    const double lmax = far1 ? l1 : l0;
    const V3 vf = far1 ? v1 : v0;
    if (lmin > rw) {
        const double d = lmin - rw;
        return SegPt{cw + vm * (rw / lmin), sstar, d * d};
    }
    if (lmax < rw) {
        const double d = rw - lmax;
        return SegPt{lmax == 0.0 ? pw : cw + vf * (rw / lmax), far1 ? 1.0 : 0.0, d * d};
    }
    if (!(lmin <= rw && lmax >= rw && lmax < INFINITY)) return SegPt{V3{0.0, 0.0, 0.0}, 0.0, NAN};
    const double B = dot(v0, u), C = dot(v0, v0) - rw * rw;
    const double disc = B * B - uu * C;
    const double q = sqrt(disc);
    const double s1 = (-B - q) / uu, s2 = (-B + q) / uu;
    if (s1 >= 0.0 && s1 <= 1.0) { const double s = seg_clamp01(s1); return SegPt{p0 + u * s, s, 0.0}; }
    if (s2 >= 0.0 && s2 <= 1.0) { const double s = seg_clamp01(s2); return SegPt{p0 + u * s, s, 0.0}; }
    return SegPt{m, sstar, 0.0};
}

// The winner so far and the rule between two candidates: lg_closest_points' (closest_offer), with the parameter carried along
struct SegBest {
    double d2;              // +INF: nothing admissible yet
    double s;
    V3 x;
    unsigned long long key; // closest_key
};
LG_HD SegBest seg_none() { return SegBest{INFINITY, 0.0, V3{0.0, 0.0, 0.0}, ~0ull}; }
// admissible iff d2 <= r2 and d2 < +INF (a NaN fails both)
LG_HD bool seg_admissible(double d2, double r2) { return d2 <= r2 && d2 < INFINITY; }
LG_HD void seg_offer(SegBest &b, const SegPt &c, double r2, unsigned long long key) {
    if (!seg_admissible(c.d2, r2)) return;
    if (c.d2 < b.d2 || (c.d2 == b.d2 && key < b.key)) { b.d2 = c.d2; b.s = c.s; b.x = c.x; b.key = key; }
}

} // namespace lg
