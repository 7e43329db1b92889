// lasgun_amd/csrc/lit_host.h -- the part of lg_scatter_lit* (query.cpp) that touches no device: the light set's rules, W, every size with its
// overflow check, and the one table of lg_lit_out's nine planes (lit_planes) with what follows from it: the NULL and alignment rules.
// Arithmetic on size_t that can overflow, so kept free of HIP: tools/lit_host_check.cpp runs exactly this text under AddressSanitizer /
// UBSan on the CPU, and both entry points call it.  Its table begins with scatter_host.h's, whose light limit it shares; the size and
// alignment rules themselves and the host form's staging are planes_host.h's.
#pragma once
#include "scatter_host.h"

namespace lg {

static_assert(sizeof(lg_light) == 72 && offsetof(lg_light, position) == 0 && offsetof(lg_light, intensity) == 24 && offsetof(lg_light, falloff) == 48,
              "lg_light: nine doubles, 72 bytes (dscene.h, DLight)");
static_assert(sizeof(lg_light_set) == 40 && offsetof(lg_light_set, lights) == 0 && offsetof(lg_light_set, count) == 8 && offsetof(lg_light_set, per_ray) == 12 &&
                  offsetof(lg_light_set, ambient) == 16,
              "lg_light_set: 40 bytes");
static_assert(sizeof(lg_lit_out) == 72 && offsetof(lg_lit_out, scatter) == 0 && offsetof(lg_lit_out, terms) == 56 && offsetof(lg_lit_out, visible) == 64,
              "lg_lit_out: lg_scatter_out and two pointers, 72 bytes");
static_assert(LG_MAX_CALL_LIGHTS == 1024u && LG_MAX_CALL_LIGHTS % 32u == 0, "at most 32 visibility words a hit");

// W: visibility words per ray for K lights
inline size_t lit_words(uint32_t count) { return ((size_t)count + 31) / 32; }

// The sizes of a call, made once by check_lit: after it none of them wraps
struct LitSizes {
    size_t n = 0, K = 0, W = 0;
    size_t terms = 0;    // doubles of `terms`: n * K * 3
    size_t visible = 0;  // words of `visible`: n * W
    size_t lights = 0;   // records of the light table: K, or n * K per ray
};

// The nine planes of lg_lit_out (or of a copy that f may edit): the seven of scatter_planes, then the two of the lights, each written down
// here and nowhere else: f(the struct's pointer, its elements, its alignment in bytes, its name) in the struct's order.  With K == 0 terms
// and visible have no elements and are not planes.
template <class Out, class F> inline void lit_planes(Out &out, const LitSizes &z, F &&f) {
    scatter_planes(out.scatter, z.n, f);
    if (z.K) {
        f(out.terms, z.terms, 8, "terms");
        f(out.visible, z.visible, 4, "visible");
    }
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  Returns the
// call's sizes.  (The sorted order's own limit on n depends on the accel's setting: query.cpp, check_sorted_count.)
inline LitSizes check_lit(const void *accel, const double *rays, size_t n, const lg_light_set *lights, const lg_lit_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!lights) throw std::runtime_error("lights is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    if (lights->count > LG_MAX_CALL_LIGHTS)
        throw std::runtime_error("lit scatter: " + std::to_string(lights->count) + " lights in the call, at most " + std::to_string(LG_MAX_CALL_LIGHTS));
    if (lights->per_ray > 1u) throw std::runtime_error("lights->per_ray is " + std::to_string(lights->per_ray) + ": 0 (shared) or 1 (a table per ray)");
    if (lights->count && !lights->lights) throw std::runtime_error("lights->lights is NULL with count > 0");
    LitSizes z;
    z.n = n; z.K = lights->count; z.W = lit_words(lights->count);
    require_any_plane([&](auto &&f) { lit_planes(*out, z, f); });
    (void)checked_bytes(n, 6 * sizeof(double), "rays");
    (void)checked_bytes(n, sizeof(lg_hit), "a plane of n rows");
    const size_t nk = checked_bytes(n, z.K, "n * count");              // n * K
    (void)checked_bytes(nk, sizeof(lg_light), "a light table per ray"); // n * K * 72, whichever form the call takes: one rule
    (void)checked_bytes(nk, 3 * sizeof(double), "terms");              // n * K * 24
    z.terms = nk * 3;
    (void)checked_bytes(checked_bytes(n, z.W, "n * words"), sizeof(uint32_t), "visible"); // n * W * 4
    z.visible = n * z.W;
    z.lights = lights->per_ray ? nk : z.K;
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many rays in one query"); // (behind the sizes: with a 64-bit size_t none of them can wrap below this limit)
    return z;
}
// The device form's alignment rule: rays 8 bytes, the planes theirs (lg_scatter's; terms 8, visible 4), a per-ray light table 8; NULL is
// not misaligned
inline void check_lit_alignment(const double *rays, const lg_light_set &lights, const lg_lit_out &out, const LitSizes &z) {
    check_alignment(rays, 8, "rays");
    if (lights.per_ray && z.K) check_alignment(lights.lights, 8, "lights->lights");
    check_planes_alignment([&](auto &&f) { lit_planes(out, z, f); });
}

} // namespace lg
