// lasgun_amd/csrc/segments_host.h -- the part of lg_closest_segments* (query.cpp; k_segments.hip) that touches no device: the one table of
// lg_segments_out's planes (segments_planes) with the NULL and alignment rules that follow from it (the rules themselves and the host form's
// staging are planes_host.h's), the call's checks in their refusal order (check_segments) -- lg_nearest's without k.  The
// scene's own tables -- the sphere gate, the pruning constants, the stack depth -- are
// lg_closest_points' (closest_host.h), unchanged; the LDS of a launch is the stack alone.  Kept free of HIP:
// tools/segments_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and the entry points call it.
#pragma once
#include "closest_host.h"

namespace lg {

static_assert(sizeof(lg_segments_out) == 40 && offsetof(lg_segments_out, touch) == 0 && offsetof(lg_segments_out, distance) == 8 && offsetof(lg_segments_out, param) == 16 &&
                  offsetof(lg_segments_out, point) == 24 && offsetof(lg_segments_out, id) == 32,
              "lg_segments_out: five pointers, 40 bytes");

// The five planes of lg_segments_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order
template <class Out, class F> inline void segments_planes(Out &out, size_t n, F &&f) {
    f(out.touch, n, 1, "touch");
    f(out.distance, n, 8, "distance");
    f(out.param, n, 8, "param");
    f(out.point, n * 3, 8, "point");
    f(out.id, n * 4, 16, "id");
}
// is `touch` the only plane asked for?  Then a lane leaves its walk at the first admissible candidate
inline bool segments_touch_only(const lg_segments_out &out) { return out.touch && !out.distance && !out.param && !out.point && !out.id; }

// Everything the contract calls an error that needs neither a device nor the scene, thrown here in the contract's order; n is not 0 (an
// empty set is answered before this).  After it no count or size of segments_planes wraps.
inline void check_segments(const void *accel, const double *segments, const double *radii, size_t n, double radius, const lg_segments_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!segments) throw std::runtime_error("segments is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { segments_planes(*out, 0, f); });
    if (!radii && !(radius >= 0.0)) throw std::runtime_error("radius is NaN or negative (+INF: no limit)"); // (with radii it is neither read nor checked)
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many segments in one query");
    (void)checked_bytes(n, 6 * sizeof(double), "segments"); // 48 bytes a row: the widest (segments; point is 24, id 16)
}
// The device form's alignment rule: segments and radii 8 bytes, the planes theirs (touch 1; distance, param and point 8; id 16); NULL is not misaligned
inline void check_segments_alignment(const double *segments, const double *radii, const lg_segments_out &out) {
    check_alignment(segments, 8, "segments");
    check_alignment(radii, 8, "radii");
    check_planes_alignment([&](auto &&f) { segments_planes(out, 0, f); });
}

} // namespace lg
