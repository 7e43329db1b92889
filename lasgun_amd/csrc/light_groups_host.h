// lasgun_amd/csrc/light_groups_host.h -- the part of lg_radiance_groups* (query.cpp) that touches no device: the limits on n and n_groups,
// the rules of a group (a `lights` bit names a light of the scene, `flags` holds known bits alone), the product n * n_groups * 24 and the
// rays' byte size with their overflow checks, the NULL and alignment rules, and the table as it travels (a fixed block of
// LG_MAX_LIGHT_GROUPS entries, the caller's n_groups copied in, the rest zero).  Arithmetic on size_t that can overflow and a copy from
// a caller's array, so kept free of HIP: tools/light_groups_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the
// CPU, and both entry points call it.
#pragma once
#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_light_group) == 8 && offsetof(lg_light_group, lights) == 0 && offsetof(lg_light_group, flags) == 4, "lg_light_group: two 32-bit words");
static_assert(LG_MAX_LIGHT_GROUPS == 64 && LG_GROUP_AMBIENT == 1u, "the constants of the contract");

constexpr uint32_t GROUPS_KNOWN_FLAGS = LG_GROUP_AMBIENT;
constexpr size_t GROUPS_MAX_LIGHTS = 32; // the level-by-level pipeline's visibility word

// the checked table of a call: what every launch is handed by value
struct GroupTable {
    lg_light_group groups[LG_MAX_LIGHT_GROUPS];
    uint32_t n_groups;
};
// the sizes of a checked call, in doubles
struct GroupsShape {
    size_t ray_doubles; // n * 6
    size_t out_doubles; // n_groups * n * 3: plane g, ray r, channel c at (g*n + r)*3 + c
};

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty query is answered before this).
// n_lights: the scene's point lights (more than 32 is refused too: no mask could name them).  Fills `table` and returns the sizes: no
// count or size wraps.  (The sorted order's own limit on n and the recursion limit depend on the accel: query.cpp.)
inline GroupsShape check_light_groups(const void *accel, const double *rays, size_t n, const lg_light_group *groups, size_t n_groups, const double *radiance,
                                      size_t n_lights, GroupTable &table) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!groups) throw std::runtime_error("groups is NULL");
    if (!radiance) throw std::runtime_error("radiance is NULL");
    if (n_groups == 0) throw std::runtime_error("n_groups is 0: at least one group");
    if (n_groups > LG_MAX_LIGHT_GROUPS) throw std::runtime_error("n_groups is " + std::to_string(n_groups) + ": at most LG_MAX_LIGHT_GROUPS (64)");
    if (n_lights > GROUPS_MAX_LIGHTS) throw std::runtime_error("radiance groups: the scene has " + std::to_string(n_lights) + " lights, a group's mask holds 32");
    for (size_t g = 0; g < n_groups; ++g) {
        if (groups[g].flags & ~GROUPS_KNOWN_FLAGS) throw std::runtime_error("groups[" + std::to_string(g) + "].flags has an unknown bit");
        const uint32_t beyond = n_lights >= 32 ? 0u : groups[g].lights >> n_lights; // (a shift by 32 is not one C++ defines)
        if (beyond) throw std::runtime_error("groups[" + std::to_string(g) + "].lights names a light the scene does not have (" + std::to_string(n_lights) + " lights)");
    }
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    if (n > SIZE_MAX / (n_groups * 3 * sizeof(double))) throw std::runtime_error("n * n_groups * 24 does not fit the address space");
    if (n > SIZE_MAX / (6 * sizeof(double))) throw std::runtime_error("rays does not fit the address space");
    std::memset(&table, 0, sizeof table);
    std::memcpy(table.groups, groups, n_groups * sizeof(lg_light_group));
    table.n_groups = (uint32_t)n_groups;
    return GroupsShape{n * 6, n_groups * n * 3};
}
// The device form's alignment rule: 8 bytes for both buffers
inline void check_light_groups_alignment(const double *rays, const double *radiance) {
    check_alignment(rays, 8, "rays");
    check_alignment(radiance, 8, "radiance");
}

} // namespace lg
