// tools/light_groups_host_check.cpp -- the device-free host code of lg_radiance_groups* (lasgun_amd/csrc/light_groups_host.h: the limits
// on n and n_groups, a group's rules against the scene's light count, the product n * n_groups * 24 with its overflow check, the NULL and
// alignment rules, the table as it travels, the host form's staging) in a stand-alone program, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_light_groups_host_sanitized.py does).  The counts go up to 2^64 - 1: an
// overflow in forming a product or a size is a UBSan report or a wrong value here, not a short buffer on a card.  The launch is stubbed
// out: a "kernel" that fills the staged planes with bytes that name their place (host_check.h, staged_round); the caller's table and array are heap blocks of
// exactly their size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/light_groups_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/light_groups_host.h"
#include "host_check.h"

using namespace lg;

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
static double OUT[6];

static bool refused(const void *accel, const double *rays, size_t n, const lg_light_group *groups, size_t n_groups, const double *radiance, size_t n_lights) {
    GroupTable t;
    return throws([&] { (void)check_light_groups(accel, rays, n, groups, n_groups, radiance, n_lights, t); });
}
static bool misaligned(const void *rays, const void *radiance) {
    return throws([&] { check_light_groups_alignment((const double *)rays, (const double *)radiance); });
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of the output and every entry of
// the table is looked at
static void run(size_t n, size_t n_groups, size_t n_lights) {
    std::unique_ptr<lg_light_group[]> groups(new lg_light_group[n_groups]); // exactly n_groups entries: the copy must not read past them
    for (size_t g = 0; g < n_groups; ++g) {
        groups[g].lights = n_lights ? (uint32_t)(g * 2654435761u) & (n_lights >= 32 ? 0xFFFFFFFFu : (1u << n_lights) - 1u) : 0u;
        groups[g].flags = (uint32_t)(g & 1u);
    }
    double *radiance = (double *)ASKED;
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    GroupTable t;
    std::memset(&t, 0xAB, sizeof t);
    const GroupsShape shape = check_light_groups(&accel, D, n, groups.get(), n_groups, radiance, n_lights, t);
    EXPECT(shape.ray_doubles == n * 6 && shape.out_doubles == n_groups * n * 3);
    EXPECT(t.n_groups == n_groups);
    for (size_t g = 0; g < LG_MAX_LIGHT_GROUPS; ++g) // the caller's entries, then zeros: what every launch is handed
        EXPECT(t.groups[g].lights == (g < n_groups ? groups[g].lights : 0u) && t.groups[g].flags == (g < n_groups ? groups[g].flags : 0u));
    // the one output as query.cpp stages it: n_groups planes of 3 doubles a ray
    const StagedRound r = staged_round([&](auto &&f) { f(radiance, shape.out_doubles, 8, "radiance"); });
    EXPECT(r.bytes == n_groups * n * 24);
}

int main() {
    int accel = 0;
    const size_t TOP = ~(size_t)0;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(QUERY_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    lg_light_group many[LG_MAX_LIGHT_GROUPS + 1];
    std::memset(many, 0, sizeof many);
    const lg_light_group one[1] = {{1u, LG_GROUP_AMBIENT}};
    // ---- check_light_groups: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, one, 1, OUT, 1));
    EXPECT(refused(nullptr, D, 3, one, 1, OUT, 1));
    EXPECT(refused(&accel, nullptr, 3, one, 1, OUT, 1));
    EXPECT(refused(&accel, D, 3, nullptr, 1, OUT, 1));
    EXPECT(refused(&accel, D, 3, one, 1, nullptr, 1));
    // n_groups of 0, 1, 64, 65 and 2^64 - 1
    EXPECT(refused(&accel, D, 3, many, 0, OUT, 1));
    EXPECT(!refused(&accel, D, 3, many, 1, OUT, 0));
    EXPECT(!refused(&accel, D, 3, many, LG_MAX_LIGHT_GROUPS, OUT, 0));
    EXPECT(refused(&accel, D, 3, many, LG_MAX_LIGHT_GROUPS + 1, OUT, 0));
    EXPECT(refused(&accel, D, 3, many, TOP, OUT, 0));
    // a `lights` bit at or above the scene's light count, for every count 0 .. 32; 33 lights are refused whatever the mask
    for (size_t n_lights = 0; n_lights <= 32; ++n_lights)
        for (uint32_t bit = 0; bit < 32; ++bit) {
            const lg_light_group g[2] = {{0u, 0u}, {1u << bit, 0u}};
            EXPECT(refused(&accel, D, 3, g, 2, OUT, n_lights) == (bit >= n_lights));
            const lg_light_group all[1] = {{n_lights >= 32 ? 0xFFFFFFFFu : (1u << n_lights) - 1u, LG_GROUP_AMBIENT}};
            EXPECT(!refused(&accel, D, 3, all, 1, OUT, n_lights));
        }
    EXPECT(refused(&accel, D, 3, many, 1, OUT, 33) && refused(&accel, D, 3, many, 1, OUT, TOP));
    // an unknown `flags` bit: every bit but LG_GROUP_AMBIENT
    for (uint32_t bit = 0; bit < 32; ++bit) {
        const lg_light_group g[1] = {{0u, 1u << bit}};
        EXPECT(refused(&accel, D, 3, g, 1, OUT, 1) == (bit != 0));
    }
    // the ray limit: (2^32 - 1) * 64 and one above, with 1 and with 64 groups
    EXPECT(!refused(&accel, D, QUERY_MAX_RAYS, many, 1, OUT, 0) && !refused(&accel, D, QUERY_MAX_RAYS, many, LG_MAX_LIGHT_GROUPS, OUT, 0));
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS + 1, many, 1, OUT, 0) && refused(&accel, D, TOP, many, 1, OUT, 0) && refused(&accel, D, TOP, many, LG_MAX_LIGHT_GROUPS, OUT, 0));
    {
        GroupTable t;
        const GroupsShape s = check_light_groups(&accel, D, QUERY_MAX_RAYS, many, LG_MAX_LIGHT_GROUPS, OUT, 0, t);
        EXPECT(s.out_doubles == QUERY_MAX_RAYS * 64 * 3 && s.out_doubles <= TOP / 8 && s.ray_doubles == QUERY_MAX_RAYS * 6);
    }
    // ---- the alignment rule: 8 bytes for both; NULL is not misaligned
    alignas(16) double d[4] = {0.0};
    const char *base = reinterpret_cast<const char *>(d);
    EXPECT(!misaligned(d, d) && !misaligned(nullptr, nullptr) && !misaligned(base + 8, base + 16));
    for (int off : {1, 2, 4, 7}) EXPECT(misaligned(base + off, d) && misaligned(d, base + off));
    // ---- the table, staging and placement: partial tiles, one group and the most, no light and the most
    const size_t ns[] = {1, 63, 64, 65, 129}, gs[] = {1, 2, 5, 63, 64}, ls[] = {0, 1, 3, 31, 32};
    for (size_t n : ns)
        for (size_t g : gs)
            for (size_t l : ls) run(n, g, l);
    if (failures) { std::fprintf(stderr, "light_groups_host_check: %d failures\n", failures); return 1; }
    std::printf("light_groups_host_check: ok\n");
    return 0;
}
