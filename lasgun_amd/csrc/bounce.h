// lasgun_amd/csrc/bounce.h -- the next ray of a ray path at a vertex (include/lasgun_hip.h, lg_trace_paths*; k_paths.hip calls it per lane).
// Host and device code over vecmath.h's V3: tools/bounce_check.cpp compiles exactly this text on the CPU under AddressSanitizer / UBSan
// and tests/bounce_ref.py restates it in numpy, word for word.
//
// The header's contract, in its order.  All f64, nothing fused (the whole product is compiled with -ffp-contract=off), dot as vecmath.h
// writes it: (a.x*b.x + a.y*b.y) + a.z*b.z.  d: the segment's direction; p, ng: the vertex's lg_hit::p and ::ng; N: ::ns or ::ng, the
// caller's choice; medium: the crossing parity so far (bit 0).
//   s = dot(d, N); if s > 0.0: N = -N, s = -s
//   REFLECT  k = 2.0*s; d' = d - k*N; o' = p + ng*2^-36
//   PASS     d' = d (its bits); o' = p - ng*2^-36; medium ^= 1
//   REFRACT  L = sqrt(dot(d,d)), q = 1.0/L, u = d*q, ci = -dot(u,N), eta = medium ? ior : 1.0/ior,
//            sin2 = (eta*eta) * fmax(1.0 - ci*ci, 0.0)     (fmax: the NaN-ignoring one)
//            sin2 >= 1.0: REFLECT's two lines, no toggle (total internal reflection)
//            else ct = sqrt(1.0 - sin2), a = eta*ci - ct, w = eta*u + a*N, d' = w*L, o' = p - ng*2^-36; medium ^= 1
// The offset is always along ng, which faces -d (surface.rs: the geometric normal is turned to the ray): + keeps the next ray on the side
// it came from, - takes it through.  Inside or outside is `medium`, never a normal's sign: ns of a sphere hit from inside faces the ray.
// ABSORB has no next ray and is not asked for one here.
#pragma once
#include "vecmath.h"

namespace lg {

constexpr uint32_t PATH_ABSORB = 0u, PATH_REFLECT = 1u, PATH_PASS = 2u, PATH_REFRACT = 3u; // LG_PATH_*: lg_path_rule::action
constexpr double BOUNCE_STEP = 0x1p-36; // shade_frame's p_err scale (N::epsilon() * 2^16): the layers' step through a surface

struct Bounce {
    V3 o, d;         // the next ray
    uint32_t medium; // the parity behind the vertex
};

LG_HD bool bounce_finite(const Bounce &b) {
    return __builtin_isfinite(b.o.x) && __builtin_isfinite(b.o.y) && __builtin_isfinite(b.o.z) && __builtin_isfinite(b.d.x) && __builtin_isfinite(b.d.y) &&
           __builtin_isfinite(b.d.z);
}

// action: PATH_REFLECT, PATH_PASS or PATH_REFRACT
LG_HD Bounce bounce_next(uint32_t action, double ior, V3 d, V3 p, V3 ng, V3 N, uint32_t medium) {
    double s = dot(d, N);
    if (s > 0.0) {
        N = V3{-N.x, -N.y, -N.z};
        s = -s;
    }
    const V3 step = V3{ng.x * BOUNCE_STEP, ng.y * BOUNCE_STEP, ng.z * BOUNCE_STEP};
    const V3 back = V3{p.x + step.x, p.y + step.y, p.z + step.z}, through = V3{p.x - step.x, p.y - step.y, p.z - step.z};
    if (action == PATH_PASS) return Bounce{through, d, medium ^ 1u};
    if (action == PATH_REFRACT) {
        const double L = sqrt(dot(d, d));
        const double q = 1.0 / L;
        const V3 u = V3{d.x * q, d.y * q, d.z * q};
        const double ci = -dot(u, N);
        const double eta = (medium & 1u) ? ior : 1.0 / ior;
        const double sin2 = (eta * eta) * fmax(1.0 - ci * ci, 0.0);
        if (!(sin2 >= 1.0)) {
            const double ct = sqrt(1.0 - sin2);
            const double a = eta * ci - ct;
            const V3 w = V3{eta * u.x + a * N.x, eta * u.y + a * N.y, eta * u.z + a * N.z};
            return Bounce{through, V3{w.x * L, w.y * L, w.z * L}, medium ^ 1u};
        }
    }
    const double k = 2.0 * s;
    return Bounce{back, V3{d.x - k * N.x, d.y - k * N.y, d.z - k * N.z}, medium};
}

} // namespace lg
