// lasgun_amd/csrc/attr_resolve.h -- hit attributes (k_attributes.hip): resolve_hit's steps (walk.h) restated with what it drops kept -- the
// triangle's barycentrics and texture coordinates, the sphere's phi and theta, the box's face axes, the local point -- and shade_frame's
// tangents (shade.h) taken from the result.  The intersectors are walk.h's own (triangle_t, sphere_t, cuboid_hit<true>) on the same local
// ray, and every expression that resolve_hit / triangle_full / sphere_full / shade_frame evaluate is written here in their operand order,
// so that gu, gv, ss and ts are the f64s the render shades with.  Nothing here is called by the render's kernels.
#pragma once
#include "shade.h"

namespace lg {

struct HitAttr {
    double b0, b1, b2; // triangle: Triangle::intersect's barycentrics; otherwise +0.0
    double u, v;
    V3 local;          // lr.o + lr.d * t
    V3 ss, ts;         // shade_frame's
    V3 gu, gv;         // is.gu, is.gv after the chain
};
__device__ __forceinline__ HitAttr attr_zero() { return HitAttr{0.0, 0.0, 0.0, 0.0, 0.0, vzero(), vzero(), vzero(), vzero(), vzero()}; }

// The attributes of the primitive (pk, idx) of `accel` -- PrimKind and table index, as Best::ref holds them -- for the world ray `wray`.
// false: the primitive's own test rejects the ray (triangle_t / cuboid_hit false, a sphere's t < 0); `at` is then not meaningful.
__device__ __forceinline__ bool attr_resolve(const DParams &P, const Ray &wray, uint32_t pk, uint32_t idx, uint32_t accel, HitAttr &at) {
    const Ray lr = local_ray(P, wray, accel);
    Isect is;
    at.b0 = 0.0; at.b1 = 0.0; at.b2 = 0.0;
    if (pk == PK_SPHERE) {
        const DSphere s = P.spheres[idx];
        bool inside;
        const double t = sphere_t(lr, V3{s.cx, s.cy, s.cz}, s.r, inside);
        if (t < 0.0) return false; // bvh.rs accepts !(t < 0)
        // sphere_full (sphere.rs:79-123), phi and theta kept
        const V3 cen{s.cx, s.cy, s.cz};
        at.local = lr.o + lr.d * t;
        V3 p = at.local - cen;
        if (p.x == 0.0 && p.y == 0.0) p.x = 1e-5 * s.r;
        double phi = p_atan2(p.y, p.x);
        if (phi < 0.0) phi += 2.0 * PI;
        const double theta = p_acos(fmin_(fmax_(p.z / s.r, -1.0), 1.0));
        at.u = phi / (2.0 * PI);
        at.v = theta / PI;
        const V3 dpdu{-2.0 * PI * p.y, 2.0 * PI * p.x, 0.0};
        double sin_phi, cos_phi, sin_theta, cos_theta;
        p_sincos(phi, sin_phi, cos_phi);
        p_sincos(theta, sin_theta, cos_theta);
        (void)cos_theta;
        const V3 dpdv = PI * V3{p.z * cos_phi, p.z * sin_phi, -s.r * sin_theta};
        if (inside) isect_set(is, t, dpdu, dpdv);
        else isect_set(is, t, dpdv, dpdu);
    } else if (pk == PK_CUBOID) {
        const DCuboid c = P.cuboids[idx];
        double t; V3 d0, d1;
        if (!cuboid_hit<true>(c.mn, c.mx, lr, t, d0, d1)) return false;
        isect_set(is, t, d0, d1);
        is.has_n = true;
        is.n = face_forward(cross(d0, d1), -lr.d);
        at.local = lr.o + lr.d * t;
        // d0 and d1 are unit axes (cube_diff): the axes they point along
        const int j = d0.x == 1.0 ? 0 : (d0.y == 1.0 ? 1 : 2), k = d1.x == 1.0 ? 0 : (d1.y == 1.0 ? 1 : 2);
        at.u = (comp(at.local, j) - c.mn[j]) / (c.mx[j] - c.mn[j]);
        at.v = (comp(at.local, k) - c.mn[k]) / (c.mx[k] - c.mn[k]);
    } else {
        // triangle_full (triangle.rs:257-304), the barycentrics and the texture coordinates kept
        const uint32_t aflags = P.accels[accel].flags;
        const uint32_t *vi = P.tri_v + 3ull * idx;
        const V3 p0 = load_f3(P.vpos, vi[0]), p1 = load_f3(P.vpos, vi[1]), p2 = load_f3(P.vpos, vi[2]);
        TriHit h;
        if (!triangle_t(p0, p1, p2, lr, h)) return false;
        double uv[3][2];
        if (aflags & AF_HAS_UV) {
            const uint32_t *ti = P.tri_t + 3ull * idx;
#pragma unroll
            for (int k = 0; k < 3; ++k) { uv[k][0] = (double)P.vtex[2ull * ti[k]]; uv[k][1] = (double)P.vtex[2ull * ti[k] + 1]; }
        } else {
            uv[0][0] = 0.0; uv[0][1] = 0.0; uv[1][0] = 1.0; uv[1][1] = 0.0; uv[2][0] = 1.0; uv[2][1] = 1.0;
        }
        at.b0 = h.b0; at.b1 = h.b1; at.b2 = h.b2;
        at.u = (h.b0 * uv[0][0] + h.b1 * uv[1][0]) + h.b2 * uv[2][0];
        at.v = (h.b0 * uv[0][1] + h.b1 * uv[1][1]) + h.b2 * uv[2][1];
        at.local = lr.o + lr.d * h.t;
        const double duv02x = uv[0][0] - uv[2][0], duv02y = uv[0][1] - uv[2][1];
        const double duv12x = uv[1][0] - uv[2][0], duv12y = uv[1][1] - uv[2][1];
        const V3 dp02 = p0 - p2, dp12 = p1 - p2;
        const double determinant = (duv02x * duv12y) - (duv02y * duv12x);
        V3 dpdu, dpdv;
        if (determinant == 0.0) {
            coordinate_system(cross(p2 - p1, p1 - p0), dpdu, dpdv);
        } else {
            const double inv = 1.0 / determinant;
            dpdu = (duv12y * dp02 - duv02y * dp12) * inv;
            dpdv = (-duv12x * dp02 - duv02x * dp12) * inv;
        }
        isect_set(is, h.t, dpdu, dpdv);
        if (aflags & AF_HAS_N) {
            const uint32_t *ni = P.tri_n + 3ull * idx;
            const V3 n0 = load_f3(P.vnorm, ni[0]), n1 = load_f3(P.vnorm, ni[1]), n2 = load_f3(P.vnorm, ni[2]);
            const V3 ns = h.b0 * n0 + h.b1 * n1 + h.b2 * n2;
            V3 ss = is.gu;
            V3 ts = cross(ns, ss);
            if (magnitude2(ts) > 0.0) ss = cross(ts, ns);
            else coordinate_system(ns, ss, ts);
            is.has_n = true; is.n = ns;
            is.su = ss; is.sv = ts;
        } else {
            is.has_n = true;
            is.n = face_forward(cross(dp02, dp12), -lr.d);
        }
    }
    // resolve_hit's way up: transform_ray_intersection (transform.rs:243-264) and the backface swap (surface.rs:88-99) of every accel
    int32_t a = (int32_t)accel;
    while (a >= 0) {
        const DAccel *A = P.accels + a;
        const V3 gu = xf_vector(A->m, is.gu), gv = xf_vector(A->m, is.gv);
        if (vne(is.gu, is.su) || vne(is.gv, is.sv)) {
            is.su = xf_vector(A->m, is.su); is.sv = xf_vector(A->m, is.sv);
        } else {
            is.su = gu; is.sv = gv;
        }
        is.gu = gu; is.gv = gv;
        if (is.has_n) is.n = xf_normal(A->minv, is.n);
        if (A->flags & AF_SWAP_BACKFACE) {
            V3 tmp = is.gu; is.gu = is.gv; is.gv = tmp;
            tmp = is.su; is.su = is.sv; is.sv = tmp;
            if (is.has_n) is.n = -is.n;
        }
        a = A->parent;
    }
    // shade_frame's ns, ss and ts (surface.rs:158-183, bsdf.rs:34-35)
    const V3 ns = is.has_n ? normalize(is.n) : normalize(cross(is.su, is.sv));
    at.gu = is.gu; at.gv = is.gv;
    at.ss = normalize(is.su);
    at.ts = cross(ns, at.ss);
    return true;
}

} // namespace lg
