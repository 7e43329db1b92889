// lasgun_amd/csrc/paths_host.h -- the part of lg_trace_paths* (query.cpp) that touches no device: the limits, the product n * max_bounces
// and the planes' byte sizes with their overflow checks, the rule table's validation, and the one table of lg_paths_out's planes
// (path_planes) with what follows from it: the NULL and alignment rules (the size and alignment rules themselves and the host form's
// staging are planes_host.h's).  Arithmetic on size_t that can overflow, so kept free of HIP: tools/paths_host_check.cpp runs exactly this
// text under AddressSanitizer / UBSan on the CPU, and both entry points call it.
#pragma once
#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_path_rule) == 24 && offsetof(lg_path_rule, action) == 0 && offsetof(lg_path_rule, reserved) == 4 && offsetof(lg_path_rule, ior) == 8 &&
                  offsetof(lg_path_rule, gain) == 16,
              "lg_path_rule: two words and two doubles, 24 bytes (k_paths.hip, PathRule)");
static_assert(sizeof(lg_paths_out) == 72 && offsetof(lg_paths_out, hits) == 0 && offsetof(lg_paths_out, point) == 8 && offsetof(lg_paths_out, id) == 16 &&
                  offsetof(lg_paths_out, along) == 24 && offsetof(lg_paths_out, count) == 32 && offsetof(lg_paths_out, end) == 40 && offsetof(lg_paths_out, gain) == 48 &&
                  offsetof(lg_paths_out, last) == 56 && offsetof(lg_paths_out, medium) == 64,
              "lg_paths_out: nine pointers, 72 bytes");
static_assert(sizeof(lg_hit) == 96, "lg_hit: 96 bytes, the widest element of a vertex plane");

// The nine planes of lg_paths_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order; total = n * max_bounces.  The alignment and NULL rules, the host
// form's staging, device buffers and copies and the device form's buffer checks all go through here.
template <class Out, class F> inline void path_planes(Out &out, size_t n, size_t total, F &&f) {
    f(out.hits, total, 16, "hits");
    f(out.point, total * 3, 8, "point");
    f(out.id, total * 4, 16, "id");
    f(out.along, total, 8, "along");
    f(out.count, n, 4, "count");
    f(out.end, n, 4, "end");
    f(out.gain, n, 8, "gain");
    f(out.last, n * 6, 8, "last");
    f(out.medium, n, 4, "medium");
}

// The rule table: exactly one rule per material of the accel, a known action, reserved 0
inline void check_path_rules(const lg_path_rule *rules, size_t n_rules, size_t material_count) {
    if (!rules) throw std::runtime_error("rules is NULL");
    if (n_rules != material_count)
        throw std::runtime_error("n_rules is " + std::to_string(n_rules) + ", the accel has " + std::to_string(material_count) + " materials (lg_accel_material_count)");
    for (size_t m = 0; m < n_rules; ++m) {
        if (rules[m].action > LG_PATH_REFRACT) throw std::runtime_error("rules[" + std::to_string(m) + "].action is " + std::to_string(rules[m].action) + ": LG_PATH_ABSORB .. LG_PATH_REFRACT");
        if (rules[m].reserved != 0u) throw std::runtime_error("rules[" + std::to_string(m) + "].reserved is not 0");
    }
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  Returns
// n * max_bounces, the elements of a vertex plane: no count or size of path_planes wraps.  (The sorted order's own limit on n depends on
// the accel's setting: query.cpp, check_sorted_count.  material_count: lg_accel_material_count of the accel, 0 for a NULL one.)
inline size_t check_paths(const void *accel, const double *rays, size_t n, uint32_t max_bounces, const lg_path_rule *rules, size_t n_rules, size_t material_count,
                          int normal, const lg_paths_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { path_planes(*out, 0, 0, f); });
    if (max_bounces == 0) throw std::runtime_error("max_bounces is 0: at least one vertex");
    if (normal != 0 && normal != 1) throw std::runtime_error("normal is " + std::to_string(normal) + ": 0 (lg_hit::ng) or 1 (lg_hit::ns)");
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    if (n > SIZE_MAX / max_bounces) throw std::runtime_error("n * max_bounces does not fit the address space");
    const size_t total = n * (size_t)max_bounces;
    (void)checked_bytes(n, 6 * sizeof(double), "rays");
    (void)checked_bytes(total, sizeof(lg_hit), "a plane of n * max_bounces elements"); // 96 bytes an element, the widest (hits)
    check_path_rules(rules, n_rules, material_count);
    return total;
}
// The device form's alignment rule: rays 8 bytes, start_medium 4, the planes theirs; NULL is not misaligned
inline void check_paths_alignment(const double *rays, const uint32_t *start_medium, const lg_paths_out &out) {
    check_alignment(rays, 8, "rays");
    check_alignment(start_medium, 4, "start_medium");
    check_planes_alignment([&](auto &&f) { path_planes(out, 0, 0, f); });
}

} // namespace lg
