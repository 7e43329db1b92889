// lasgun_amd/csrc/scatter_host.h -- the part of lg_scatter* (query.cpp) that touches no device: the limits, the planes' byte sizes with their
// overflow checks, and the one table of lg_scatter_out's planes (scatter_planes) with what follows from it: the NULL and alignment rules,
// the host form's staging and its placement.  Arithmetic on size_t that can overflow, so kept free of HIP: tools/scatter_host_check.cpp runs
// exactly this text under AddressSanitizer / UBSan on the CPU, and both entry points call it.  Shaped like layers_host.h and kept apart
// from it: its plane table names LayersStaging's members, and tools/layers_host_check.cpp includes that text as it is.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lasgun_hip.h"

namespace lg {

static_assert(sizeof(lg_scatter_out) == 56 && offsetof(lg_scatter_out, hits) == 0 && offsetof(lg_scatter_out, direct) == 8 && offsetof(lg_scatter_out, flags) == 16 &&
                  offsetof(lg_scatter_out, reflect) == 24 && offsetof(lg_scatter_out, reflect_weight) == 32 && offsetof(lg_scatter_out, refract) == 40 &&
                  offsetof(lg_scatter_out, refract_weight) == 48,
              "lg_scatter_out: seven pointers, 56 bytes");
static_assert(sizeof(lg_hit) == 96, "lg_hit: 96 bytes, the widest row of a plane");
static_assert(LG_SCATTER_HIT == 1u && LG_SCATTER_REFLECT == 2u && LG_SCATTER_REFRACT == 4u, "the flag bits k_scatter.hip writes (dscene.h, SCATTER_*)");

constexpr unsigned long long SCATTER_MAX_RAYS = 0xFFFFFFFFull * 64ull; // 64-ray tiles are counted in 32 bits, as lg_radiance's are
constexpr size_t SCATTER_MAX_LIGHTS = 32;                              // the level-by-level pipeline's visibility word, as for lg_radiance
constexpr size_t SCATTER_ROW_BYTES = 96 + 24 + 4 + 48 + 24 + 48 + 40;  // a ray's rows of all seven planes: 284 bytes (280 of doubles and records + the flags word)

// count * bytes_each as a size_t, refused where it does not fit the address space
inline size_t scatter_bytes(size_t count, size_t bytes_each, const char *what) {
    if (bytes_each && count > SIZE_MAX / bytes_each) throw std::runtime_error(std::string(what) + " does not fit the address space");
    return count * bytes_each;
}

// The host form's outputs on their way back: only what is asked for has any size.  An error on the way leaves the caller's arrays as they were.
struct ScatterStaging {
    std::vector<lg_hit> hits;
    std::vector<double> direct;
    std::vector<uint32_t> flags;
    std::vector<double> reflect, reflect_weight, refract, refract_weight;
    ScatterStaging(const lg_scatter_out &out, size_t n);
};
// The seven planes of lg_scatter_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, the
// plane's staging, its elements, its alignment in bytes, its name) in the struct's order.  The alignment and NULL rules, the staging's
// sizes, the host form's device buffers and copies, the device form's buffer checks and the placement all go through here.
template <class Out, class F> inline void scatter_planes(Out &out, size_t n, F &&f) {
    f(out.hits, &ScatterStaging::hits, n, 16, "hits");
    f(out.direct, &ScatterStaging::direct, n * 3, 8, "direct");
    f(out.flags, &ScatterStaging::flags, n, 4, "flags");
    f(out.reflect, &ScatterStaging::reflect, n * 6, 8, "reflect");
    f(out.reflect_weight, &ScatterStaging::reflect_weight, n * 3, 8, "reflect_weight");
    f(out.refract, &ScatterStaging::refract, n * 6, 8, "refract");
    f(out.refract_weight, &ScatterStaging::refract_weight, n * 5, 8, "refract_weight");
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  After it no
// count or size of scatter_planes wraps.  light_count: the scene's point lights (0 for a NULL accel); the accel's recursion depth is never
// asked for.  (The sorted order's own limit on n depends on the accel's setting: query.cpp, check_sorted_count.)
inline void check_scatter(const void *accel, const double *rays, size_t n, const lg_scatter_out *out, size_t light_count) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    bool any = false;
    scatter_planes(*out, 0, [&](auto *p, auto, size_t, size_t, const char *) { any = any || p; });
    if (!any) throw std::runtime_error("every plane of out is NULL: at least one output");
    if ((unsigned long long)n > SCATTER_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    if (light_count > SCATTER_MAX_LIGHTS)
        throw std::runtime_error("surface scatter: the scene has " + std::to_string(light_count) + " lights, the level-by-level pipeline's visibility word holds 32");
    (void)scatter_bytes(n, 6 * sizeof(double), "rays");
    (void)scatter_bytes(n, sizeof(lg_hit), "a plane of n rows"); // 96 bytes a row, the widest (hits)
}
inline ScatterStaging::ScatterStaging(const lg_scatter_out &out, size_t n) {
    scatter_planes(out, n, [&](auto *p, auto plane, size_t count, size_t, const char *) { if (p) (this->*plane).resize(count); });
}
inline void place_scatter(const lg_scatter_out &out, const ScatterStaging &st) {
    scatter_planes(out, 0, [&](auto *p, auto plane, size_t, size_t, const char *) {
        if (p && !(st.*plane).empty()) std::memcpy(p, (st.*plane).data(), (st.*plane).size() * sizeof *p);
    });
}
// The device form's alignment rule: rays 8 bytes, the planes theirs (hits 16; the double planes 8; flags 4); NULL is not misaligned
inline void check_scatter_alignment(const double *rays, const lg_scatter_out &out) {
    const auto aligned = [](const void *p, size_t align, const char *what) {
        if (p && (uintptr_t)p % align) throw std::runtime_error(std::string(what) + " is not " + std::to_string(align) + "-byte aligned");
    };
    aligned(rays, 8, "rays");
    scatter_planes(out, 0, [&](auto *p, auto, size_t, size_t align, const char *what) { aligned(p, align, what); });
}

} // namespace lg
