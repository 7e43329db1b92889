// lasgun_amd/csrc/nearest_host.h -- the part of lg_nearest* (query.cpp; k_nearest.hip) that touches no device: the one table of
// lg_nearest_out's planes (nearest_planes) with the NULL and alignment rules that follow from it (the rules themselves and the host form's
// staging are planes_host.h's), the call's checks in their refusal order (check_nearest), what the planes asked for make of k
// (nearest_slots, nearest_entries), and the dynamic LDS a launch needs with the limit it is held to (nearest_lds_bytes, check_nearest_lds).
// The scene's own tables -- the sphere gate, the pruning constants, the stack depth -- are lg_closest_points' (closest_host.h), unchanged.
// Arithmetic on size_t that can overflow, so kept free of HIP: tools/nearest_host_check.cpp runs exactly this text under AddressSanitizer /
// UBSan on the CPU, and the entry points call it.
#pragma once
#include "closest_host.h"

namespace lg {

static_assert(sizeof(lg_nearest_out) == 40 && offsetof(lg_nearest_out, touch) == 0 && offsetof(lg_nearest_out, count) == 8 && offsetof(lg_nearest_out, distance) == 16 &&
                  offsetof(lg_nearest_out, point) == 24 && offsetof(lg_nearest_out, id) == 32,
              "lg_nearest_out: five pointers, 40 bytes");

constexpr uint32_t NEAREST_MAX_K = LG_NEAREST_MAX_K;
constexpr uint32_t NEAREST_BLOCK = 256;              // lanes of a workgroup (kcommon.h, LG_BLOCK: k_nearest.hip asserts they agree)
constexpr size_t NEAREST_STACK_ENTRY_BYTES = 8;      // (node, accel) a lane: closest_kernel's stack
constexpr size_t NEAREST_LIST_ENTRY_BYTES = 20;      // d2, key, leaf slot a lane (nearest_list.h, NearestEntry as k_nearest.hip stores it)
constexpr size_t NEAREST_LDS_LIMIT = (size_t)160 << 10; // the LDS of a gfx950 compute unit, all of which one workgroup may have

// The five planes of lg_nearest_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order; nk = n * k, the rows of a slot plane
template <class Out, class F> inline void nearest_planes(Out &out, size_t n, size_t nk, F &&f) {
    f(out.touch, n, 1, "touch");
    f(out.count, n, 4, "count");
    f(out.distance, nk, 8, "distance");
    f(out.point, nk * 3, 8, "point");
    f(out.id, nk * 4, 16, "id");
}
// is a slot plane (distance, point, id) asked for?  Only then does k play a part
inline bool nearest_slots(const lg_nearest_out &out) { return out.distance || out.point || out.id; }
// the list entries a lane keeps: k with a slot plane, none without
inline uint32_t nearest_entries(const lg_nearest_out &out, uint32_t k) { return nearest_slots(out) ? k : 0u; }

// The dynamic LDS of one workgroup for a stack of `depth` entries and lists of k: 256 * (8 * depth + 20 * k) bytes
inline size_t nearest_lds_bytes(uint32_t depth, uint32_t k) { return (size_t)NEAREST_BLOCK * (NEAREST_STACK_ENTRY_BYTES * depth + NEAREST_LIST_ENTRY_BYTES * k); }
// The LDS rule: stack plus lists within what a workgroup may have (refused, never truncated)
inline void check_nearest_lds(uint32_t depth, uint32_t k) {
    const size_t need = nearest_lds_bytes(depth, k);
    if (need > NEAREST_LDS_LIMIT)
        throw std::runtime_error("nearest: a stack of " + std::to_string(depth) + " entries and lists of " + std::to_string(k) + " need " + std::to_string(need) +
                                 " bytes of LDS a workgroup, the limit is " + std::to_string(NEAREST_LDS_LIMIT) + " (lg_scene_nearest_lds)");
}

// Everything the contract calls an error that needs neither a device nor the scene, thrown here in the contract's order; n is not 0 (an
// empty set is answered before this).  Returns n * k, the rows of a slot plane (0 where none is asked for); after it no count or size of
// nearest_planes wraps.
inline size_t check_nearest(const void *accel, const double *points, const double *radii, size_t n, double radius, uint32_t k, const lg_nearest_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!points) throw std::runtime_error("points is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { nearest_planes(*out, 0, 0, f); });
    if (!radii && !(radius >= 0.0)) throw std::runtime_error("radius is NaN or negative (+INF: no limit)"); // (with radii it is neither read nor checked)
    if (k > NEAREST_MAX_K) throw std::runtime_error("k is beyond LG_NEAREST_MAX_K");
    const bool slots = nearest_slots(*out);
    if (k == 0u && slots) throw std::runtime_error("k is 0 and a slot plane (distance, point, id) is asked for");
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many points in one query");
    (void)checked_bytes(n, 3 * sizeof(double), "points");
    const size_t nk = slots ? checked_bytes(n, k, "n * k") : 0;
    (void)checked_bytes(nk, 3 * sizeof(double), "point"); // 24 bytes a row: the widest slot plane
    return nk;
}
// The device form's alignment rule: points and radii 8 bytes, the planes theirs (touch 1, count 4, distance and point 8; id 16); NULL is not misaligned
inline void check_nearest_alignment(const double *points, const double *radii, const lg_nearest_out &out) {
    check_alignment(points, 8, "points");
    check_alignment(radii, 8, "radii");
    check_planes_alignment([&](auto &&f) { nearest_planes(out, 0, 0, f); });
}

} // namespace lg
