// lasgun_amd/csrc/gather_host.h -- the part of lg_radiance_gather* (query.cpp) that touches no device: the lane rule, the two tile counts with
// their 32-bit limit, the four byte sizes, the NULL and alignment rules, and the batch a parked call is cut into (the size and alignment
// rules themselves and the host form's staging are planes_host.h's).  Arithmetic on size_t that can overflow, so kept free of HIP: tools/gather_host_check.cpp runs exactly this text under
// AddressSanitizer / UBSan on the CPU, and lg_radiance_gather_lanes and both entry points call it.
#pragma once
#include <cstdlib>

#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_gather_out) == 16 && offsetof(lg_gather_out, radiance) == 0 && offsetof(lg_gather_out, sums) == 8, "lg_gather_out: two pointers, 16 bytes");

constexpr int GATHER_DIR_LANES = 1, GATHER_POSE_LANES = 2;
constexpr unsigned long long GATHER_MAX_TILES = 0xFFFFFFFFull; // tiles are counted in 32 bits, as the other queries' are
constexpr unsigned long long GATHER_MAX_DIRS = 0xFFFFFFFFull;
constexpr unsigned long long GATHER_PARK_MB_DEFAULT = 1024;    // LASGUN_GATHER_PARK_MB: a stated default, not a measured optimum

// The work item a call takes: 1 direction lanes, 2 pose lanes; 0 asks for the stated default, pose lanes iff n_poses >= n_dirs; -1: a bad `lanes`
inline int gather_lanes(size_t n_poses, size_t n_dirs, int lanes) {
    if (lanes == GATHER_DIR_LANES || lanes == GATHER_POSE_LANES) return lanes;
    if (lanes != 0) return -1;
    return n_poses >= n_dirs ? GATHER_POSE_LANES : GATHER_DIR_LANES;
}
// The tiles of a gather in `form` (1 or 2): n_poses * ceil(n_dirs / 64) of one pose x 64 directions, or ceil(n_poses / 64) * n_dirs of 64
// poses x one direction.  false: more than 2^32 - 1 (the product itself is never formed where it could overflow)
inline bool gather_tiles(size_t n_poses, size_t n_dirs, int form, unsigned long long *tiles) {
    const auto ceil64 = [](size_t n) { return (unsigned long long)(n / 64) + (n % 64 ? 1u : 0u); };
    const unsigned long long a = form == GATHER_POSE_LANES ? ceil64(n_poses) : (unsigned long long)n_poses;
    const unsigned long long b = form == GATHER_POSE_LANES ? (unsigned long long)n_dirs : ceil64(n_dirs);
    if (a == 0 || b == 0) { *tiles = 0; return true; }
    if (a > GATHER_MAX_TILES / b) return false;
    *tiles = a * b;
    return true;
}
// count * each * bytes as a size_t, refused where it does not fit the address space
inline size_t gather_bytes(size_t count, size_t each, size_t bytes, const char *what) { return checked_bytes(checked_bytes(count, each, what), bytes, what); }

// What a checked call is: its form, its tiles and its rays
struct GatherShape {
    int form;        // GATHER_DIR_LANES or GATHER_POSE_LANES
    uint32_t tiles;
    size_t pairs;    // n_poses * n_dirs
};
// Everything the contract calls an error that needs no device and no scene, thrown here in the contract's order; the counts are not 0 (an
// empty set is answered before this).  weights and n_weights are looked at only where sums is asked for.
inline GatherShape check_gather(const void *accel, const double *origins, size_t n_poses, const double *dirs, size_t n_dirs, const double *weights, size_t n_weights, int lanes,
                                const lg_gather_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    if (!origins) throw std::runtime_error("origins is NULL");
    if (!dirs) throw std::runtime_error("dirs is NULL");
    if (!out->radiance && !out->sums) throw std::runtime_error("radiance and sums are both NULL: at least one output");
    if (out->sums && !weights) throw std::runtime_error("sums is asked for and weights is NULL");
    if (out->sums && n_weights == 0) throw std::runtime_error("sums is asked for and n_weights is 0");
    const int form = gather_lanes(n_poses, n_dirs, lanes);
    if (form < 0) throw std::runtime_error("lanes is " + std::to_string(lanes) + ": 0 (auto), 1 (direction lanes) or 2 (pose lanes)");
    if ((unsigned long long)n_dirs > GATHER_MAX_DIRS) throw std::runtime_error("too many directions in one gather: at most 2^32 - 1");
    unsigned long long tiles = 0;
    if (!gather_tiles(n_poses, n_dirs, form, &tiles))
        throw std::runtime_error(form == GATHER_POSE_LANES ? "too many rays in one gather: tiles of 64 poses x one direction are counted in 32 bits"
                                                           : "too many rays in one gather: tiles of one pose x 64 directions are counted in 32 bits");
    (void)gather_bytes(n_poses, n_dirs, 3 * sizeof(double), "n_poses * n_dirs * 24 bytes of radiance");
    if (out->sums) {
        (void)gather_bytes(n_dirs, n_weights, sizeof(double), "n_dirs * n_weights * 8 bytes of weights");
        (void)gather_bytes(n_poses, n_weights, 3 * sizeof(double), "n_poses * n_weights * 24 bytes of sums");
    }
    (void)gather_bytes(n_poses, 9, sizeof(double), "n_poses * 72 bytes of frames");
    return {form, (uint32_t)tiles, n_poses * n_dirs};
}
// The device form's alignment rule: every pointer 8 bytes
inline void check_gather_alignment(const double *origins, const double *frames, const double *dirs, const double *weights, const lg_gather_out &out) {
    check_alignment(origins, 8, "origins"); check_alignment(frames, 8, "frames"); check_alignment(dirs, 8, "dirs");
    if (out.sums) check_alignment(weights, 8, "weights");
    check_alignment(out.radiance, 8, "radiance"); check_alignment(out.sums, 8, "sums");
}

// LASGUN_GATHER_PARK_MB as bytes a batch may park: a positive integer of MiB, anything else (and no value) the default; clamped so that
// the shift cannot wrap
inline size_t gather_park_bytes(const char *env) {
    unsigned long long mb = GATHER_PARK_MB_DEFAULT;
    if (env && env[0] >= '0' && env[0] <= '9') { // (strtoull would take a sign and wrap it)
        char *end = nullptr;
        const unsigned long long v = std::strtoull(env, &end, 10);
        if (end != env && *end == '\0' && v > 0) mb = v;
    }
    const unsigned long long most = (unsigned long long)(SIZE_MAX >> 20);
    return (size_t)(mb > most ? most : mb) << 20;
}
// The poses of one batch of a call that parks its li (no radiance plane): whole consecutive poses whose li, n_dirs * 24 bytes a pose, stays
// within `park_bytes` -- never fewer than one pose, never more than the call has; in pose lanes whole blocks of 64 poses where the cap allows
// one, so that only a call's last tile row has idle lanes.  n_dirs * 24 fits (check_gather).
inline size_t gather_batch_poses(size_t n_poses, size_t n_dirs, int form, size_t park_bytes) {
    size_t b = park_bytes / (n_dirs * 3 * sizeof(double));
    if (b < 1) b = 1;
    if (form == GATHER_POSE_LANES && b >= 64) b -= b % 64;
    return b < n_poses ? b : n_poses;
}

} // namespace lg
