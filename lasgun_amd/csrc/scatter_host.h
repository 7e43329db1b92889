// lasgun_amd/csrc/scatter_host.h -- the part of lg_scatter* (query.cpp) that touches no device: the limits, the planes' byte sizes with their
// overflow checks, and the one table of lg_scatter_out's planes (scatter_planes) with what follows from it: the NULL and alignment rules,
// (the size and alignment rules themselves and the host form's staging are planes_host.h's).  Arithmetic on size_t that can overflow, so
// kept free of HIP: tools/scatter_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and both entry points
// call it.
#pragma once
#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_scatter_out) == 56 && offsetof(lg_scatter_out, hits) == 0 && offsetof(lg_scatter_out, direct) == 8 && offsetof(lg_scatter_out, flags) == 16 &&
                  offsetof(lg_scatter_out, reflect) == 24 && offsetof(lg_scatter_out, reflect_weight) == 32 && offsetof(lg_scatter_out, refract) == 40 &&
                  offsetof(lg_scatter_out, refract_weight) == 48,
              "lg_scatter_out: seven pointers, 56 bytes");
static_assert(sizeof(lg_hit) == 96, "lg_hit: 96 bytes, the widest row of a plane");
static_assert(LG_SCATTER_HIT == 1u && LG_SCATTER_REFLECT == 2u && LG_SCATTER_REFRACT == 4u, "the flag bits k_scatter.hip writes (dscene.h, SCATTER_*)");

constexpr size_t SCATTER_MAX_LIGHTS = 32;                             // the level-by-level pipeline's visibility word, as for lg_radiance
constexpr size_t SCATTER_ROW_BYTES = 96 + 24 + 4 + 48 + 24 + 48 + 40; // a ray's rows of all seven planes: 284 bytes (280 of doubles and records + the flags word)

// The seven planes of lg_scatter_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order.  The alignment and NULL rules, the host form's staging, device
// buffers and copies and the device form's buffer checks all go through here (and lit_host.h's table begins with this one).
template <class Out, class F> inline void scatter_planes(Out &out, size_t n, F &&f) {
    f(out.hits, n, 16, "hits");
    f(out.direct, n * 3, 8, "direct");
    f(out.flags, n, 4, "flags");
    f(out.reflect, n * 6, 8, "reflect");
    f(out.reflect_weight, n * 3, 8, "reflect_weight");
    f(out.refract, n * 6, 8, "refract");
    f(out.refract_weight, n * 5, 8, "refract_weight");
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  After it no
// count or size of scatter_planes wraps.  light_count: the scene's point lights (0 for a NULL accel); the accel's recursion depth is never
// asked for.  (The sorted order's own limit on n depends on the accel's setting: query.cpp, check_sorted_count.)
inline void check_scatter(const void *accel, const double *rays, size_t n, const lg_scatter_out *out, size_t light_count) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { scatter_planes(*out, 0, f); });
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    if (light_count > SCATTER_MAX_LIGHTS)
        throw std::runtime_error("surface scatter: the scene has " + std::to_string(light_count) + " lights, the level-by-level pipeline's visibility word holds 32");
    (void)checked_bytes(n, 6 * sizeof(double), "rays");
    (void)checked_bytes(n, sizeof(lg_hit), "a plane of n rows"); // 96 bytes a row, the widest (hits)
}
// The device form's alignment rule: rays 8 bytes, the planes theirs (hits 16; the double planes 8; flags 4); NULL is not misaligned
inline void check_scatter_alignment(const double *rays, const lg_scatter_out &out) {
    check_alignment(rays, 8, "rays");
    check_planes_alignment([&](auto &&f) { scatter_planes(out, 0, f); });
}

} // namespace lg
