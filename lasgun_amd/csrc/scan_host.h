// lasgun_amd/csrc/scan_host.h -- the part of lg_range_scan* (query.cpp) that touches no device: the lane rule, the two tile counts with
// their 32-bit limit, the planes' byte sizes, and the one table of lg_scan_out's planes (scan_planes) with what follows from it: the NULL and
// alignment rules (the size and alignment rules themselves and the host form's staging are planes_host.h's).  Arithmetic on size_t that
// can overflow, so kept free of HIP:
// tools/scan_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and lg_range_scan_lanes and both entry points call it.
#pragma once
#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_scan_out) == 48 && offsetof(lg_scan_out, range) == 0 && offsetof(lg_scan_out, point) == 8 && offsetof(lg_scan_out, normal) == 16 &&
                  offsetof(lg_scan_out, id) == 24 && offsetof(lg_scan_out, hits) == 32 && offsetof(lg_scan_out, nearest) == 40,
              "lg_scan_out: six pointers, 48 bytes");

constexpr int SCAN_BEAM_LANES = 1, SCAN_POSE_LANES = 2;
constexpr unsigned long long SCAN_MAX_TILES = 0xFFFFFFFFull; // tiles are counted in 32 bits, as the other queries' are
constexpr unsigned long long SCAN_MAX_BEAMS = 0xFFFFFFFFull;

// The work item a call takes: 1 beam lanes, 2 pose lanes; 0 asks for the stated default, pose lanes iff n_poses >= n_beams; -1: a bad `lanes`
inline int scan_lanes(size_t n_poses, size_t n_beams, int lanes) {
    if (lanes == SCAN_BEAM_LANES || lanes == SCAN_POSE_LANES) return lanes;
    if (lanes != 0) return -1;
    return n_poses >= n_beams ? SCAN_POSE_LANES : SCAN_BEAM_LANES;
}

inline unsigned long long scan_ceil_div(size_t n, unsigned d) { return (unsigned long long)(n / d) + (n % d ? 1u : 0u); }
// The tiles of a scan in `form` (1 or 2): n_poses * ceil(n_beams / 64) of one pose x 64 beams, or ceil(n_poses / 64) * ceil(n_beams / 8) of
// 64 poses x 8 beams.  false: more than 2^32 - 1 (the product itself is never formed where it could overflow)
inline bool scan_tiles(size_t n_poses, size_t n_beams, int form, unsigned long long *tiles) {
    const unsigned long long a = form == SCAN_POSE_LANES ? scan_ceil_div(n_poses, 64) : (unsigned long long)n_poses;
    const unsigned long long b = form == SCAN_POSE_LANES ? scan_ceil_div(n_beams, 8) : scan_ceil_div(n_beams, 64);
    if (a == 0 || b == 0) { *tiles = 0; return true; }
    if (a > SCAN_MAX_TILES / b) return false;
    *tiles = a * b;
    return true;
}
// The six planes of lg_scan_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order.  The alignment and NULL rules, the host form's staging, device
// buffers and copies and the device form's buffer checks all go through here.
template <class Out, class F> inline void scan_planes(Out &out, size_t n_poses, size_t pairs, F &&f) {
    f(out.range, pairs, 4, "range");
    f(out.point, pairs * 3, 4, "point");
    f(out.normal, pairs * 3, 4, "normal");
    f(out.id, pairs * 4, 16, "id");
    f(out.hits, n_poses, 4, "hits");
    f(out.nearest, n_poses, 4, "nearest");
}

// What a checked call is: its form, its tiles and its pairs
struct ScanShape {
    int form;        // SCAN_BEAM_LANES or SCAN_POSE_LANES
    uint32_t tiles;
    size_t pairs;    // n_poses * n_beams
};
// Everything the contract calls an error that needs no device, thrown here; the counts are not 0 (an empty set is answered before this)
inline ScanShape check_scan(const void *accel, const double *origins, size_t n_poses, const double *beams, size_t n_beams, int lanes, const lg_scan_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    if (!origins) throw std::runtime_error("origins is NULL");
    if (!beams) throw std::runtime_error("beams is NULL");
    require_any_plane([&](auto &&f) { scan_planes(*out, 0, 0, f); });
    const int form = scan_lanes(n_poses, n_beams, lanes);
    if (form < 0) throw std::runtime_error("lanes is " + std::to_string(lanes) + ": 0 (auto), 1 (beam lanes) or 2 (pose lanes)");
    if ((unsigned long long)n_beams > SCAN_MAX_BEAMS) throw std::runtime_error("too many beams in one scan: at most 2^32 - 1");
    unsigned long long tiles = 0;
    if (!scan_tiles(n_poses, n_beams, form, &tiles))
        throw std::runtime_error(form == SCAN_POSE_LANES ? "too many pairs in one scan: tiles of 64 poses x 8 beams are counted in 32 bits"
                                                         : "too many pairs in one scan: tiles of one pose x 64 beams are counted in 32 bits");
    if (n_poses > SIZE_MAX / n_beams) throw std::runtime_error("n_poses * n_beams does not fit the address space");
    const size_t pairs = n_poses * n_beams;
    (void)checked_bytes(n_poses, 9 * sizeof(double), "frames");
    (void)checked_bytes(pairs, 4 * sizeof(uint32_t), "a plane of n_poses * n_beams elements"); // 16 bytes an element, the widest (id): no count or size of scan_planes wraps
    return {form, (uint32_t)tiles, pairs};
}
// The device form's alignment rule: the inputs 8 bytes, the planes theirs (id 16, the others 4)
inline void check_scan_alignment(const double *origins, const double *frames, const double *beams, const lg_scan_out &out) {
    check_alignment(origins, 8, "origins");
    check_alignment(frames, 8, "frames");
    check_alignment(beams, 8, "beams");
    check_planes_alignment([&](auto &&f) { scan_planes(out, 0, 0, f); });
}

} // namespace lg
