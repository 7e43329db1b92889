// lasgun_amd/csrc/lit_host.h -- the part of lg_scatter_lit* (query.cpp) that touches no device: the light set's rules, W, every size with its
// overflow check, and the one table of lg_lit_out's nine planes (lit_planes) with what follows from it: the NULL and alignment rules, the
// host form's staging and its placement.  Arithmetic on size_t that can overflow, so kept free of HIP: tools/lit_host_check.cpp runs exactly
// this text under AddressSanitizer / UBSan on the CPU, and both entry points call it.  Shaped like scatter_host.h, whose limits and byte
// arithmetic it uses, and kept apart from it: its plane table names LitStaging's members.
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

// The host form's outputs on their way back: only what is asked for has any size
struct LitStaging {
    ScatterStaging scatter;
    std::vector<double> terms;
    std::vector<uint32_t> visible;
    LitStaging(const lg_lit_out &out, const LitSizes &z);
};
// The nine planes of lg_lit_out (or of a copy that f may edit): the seven of scatter_planes through the staging's `scatter`, then the two
// of the lights, each written down here and nowhere else: f(the struct's pointer, a function that gives the plane's staging vector, its
// elements, its alignment in bytes, its name) in the struct's order.  With K == 0 terms and visible have no elements and are not planes.
template <class Out, class F> inline void lit_planes(Out &out, const LitSizes &z, F &&f) {
    scatter_planes(out.scatter, z.n, [&](auto *&p, auto plane, size_t count, size_t align, const char *what) {
        f(p, [plane](auto &st) -> auto & { return st.scatter.*plane; }, count, align, what);
    });
    if (z.K) {
        f(out.terms, [](auto &st) -> auto & { return st.terms; }, z.terms, (size_t)8, "terms");
        f(out.visible, [](auto &st) -> auto & { return st.visible; }, z.visible, (size_t)4, "visible");
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
    bool any = false;
    {
        lg_lit_out probe = *out;
        lit_planes(probe, z, [&](auto *p, auto, size_t, size_t, const char *) { any = any || p; });
    }
    if (!any) throw std::runtime_error("every plane of out is NULL: at least one output");
    (void)scatter_bytes(n, 6 * sizeof(double), "rays");
    (void)scatter_bytes(n, sizeof(lg_hit), "a plane of n rows");
    const size_t nk = scatter_bytes(n, z.K, "n * count");              // n * K
    (void)scatter_bytes(nk, sizeof(lg_light), "a light table per ray"); // n * K * 72, whichever form the call takes: one rule
    (void)scatter_bytes(nk, 3 * sizeof(double), "terms");              // n * K * 24
    z.terms = nk * 3;
    (void)scatter_bytes(scatter_bytes(n, z.W, "n * words"), sizeof(uint32_t), "visible"); // n * W * 4
    z.visible = n * z.W;
    z.lights = lights->per_ray ? nk : z.K;
    if ((unsigned long long)n > SCATTER_MAX_RAYS) throw std::runtime_error("too many rays in one query"); // (behind the sizes: with a 64-bit size_t none of them can wrap below this limit)
    return z;
}
inline LitStaging::LitStaging(const lg_lit_out &out, const LitSizes &z) : scatter(out.scatter, 0) {
    lg_lit_out o = out;
    lit_planes(o, z, [&](auto *p, auto member, size_t count, size_t, const char *) { if (p) member(*this).resize(count); });
}
inline void place_lit(const lg_lit_out &out, const LitSizes &z, const LitStaging &st) {
    lg_lit_out o = out;
    lit_planes(o, z, [&](auto *p, auto member, size_t, size_t, const char *) {
        const auto &v = member(st);
        if (p && !v.empty()) std::memcpy(p, v.data(), v.size() * sizeof *p);
    });
}
// The device form's alignment rule: rays 8 bytes, the planes theirs (lg_scatter's; terms 8, visible 4), a per-ray light table 8; NULL is
// not misaligned
inline void check_lit_alignment(const double *rays, const lg_light_set &lights, const lg_lit_out &out, const LitSizes &z) {
    const auto aligned = [](const void *p, size_t align, const char *what) {
        if (p && (uintptr_t)p % align) throw std::runtime_error(std::string(what) + " is not " + std::to_string(align) + "-byte aligned");
    };
    aligned(rays, 8, "rays");
    if (lights.per_ray && z.K) aligned(lights.lights, 8, "lights->lights");
    lg_lit_out o = out;
    lit_planes(o, z, [&](auto *p, auto, size_t, size_t align, const char *what) { aligned(p, align, what); });
}

} // namespace lg
