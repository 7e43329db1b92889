// tools/paths_host_check.cpp -- the device-free host code of lg_trace_paths* (lasgun_amd/csrc/paths_host.h: the limits, the product
// n * max_bounces and the planes' byte sizes with their overflow checks, the rule table's validation, the NULL and alignment rules of
// lg_paths_out, the host form's staging) in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_paths_host_sanitized.py does).  The counts go up to 2^64 - 1: an overflow in forming a product or a size is a UBSan report
// or a wrong value here, not a short buffer on a card.  The launch is stubbed out: a "kernel" that fills the staged planes with bytes that
// name their place (host_check.h, staged_round); every caller's array is a heap block of exactly its size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/paths_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/paths_host.h"
#include "host_check.h"

using namespace lg;

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
static const lg_path_rule RULES[3] = {{LG_PATH_REFRACT, 0u, 1.5, 1.0}, {LG_PATH_REFLECT, 0u, 1.0, 0.5}, {LG_PATH_ABSORB, 0u, 1.0, 1.0}};

static bool refused(const void *accel, const double *rays, size_t n, uint32_t max_bounces, const lg_paths_out *out, const lg_path_rule *rules = RULES, size_t n_rules = 3,
                    size_t materials = 3, int normal = 0) {
    return throws([&] { (void)check_paths(accel, rays, n, max_bounces, rules, n_rules, materials, normal, out); });
}
static size_t checked(const void *accel, size_t n, uint32_t max_bounces, const lg_paths_out *out) { return check_paths(accel, D, n, max_bounces, RULES, 3, 3, 0, out); }
static bool misaligned(const void *rays, const void *start_medium, const lg_paths_out &out) {
    return throws([&] { check_paths_alignment((const double *)rays, (const uint32_t *)start_medium, out); });
}
// lg_paths_out with the planes of a 9-bit mask named from `all`, in the struct's order
static lg_paths_out subset(const lg_paths_out &all, unsigned planes) {
    return lg_paths_out{planes & 1u ? all.hits : nullptr,   planes & 2u ? all.point : nullptr, planes & 4u ? all.id : nullptr,
                        planes & 8u ? all.along : nullptr,  planes & 16u ? all.count : nullptr, planes & 32u ? all.end : nullptr,
                        planes & 64u ? all.gain : nullptr,  planes & 128u ? all.last : nullptr, planes & 256u ? all.medium : nullptr};
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of every output is looked at
static void run(size_t n, uint32_t max_bounces, unsigned planes) {
    const size_t total = n * max_bounces;
    const lg_paths_out all{(lg_hit *)ASKED, (double *)ASKED, (uint32_t *)ASKED, (double *)ASKED, (uint32_t *)ASKED, (uint32_t *)ASKED, (double *)ASKED, (double *)ASKED, (uint32_t *)ASKED};
    lg_paths_out out = subset(all, planes);
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    EXPECT(checked(&accel, n, max_bounces, &out) == total);
    // what the host form allocates on the device and copies back: the table's counts in the plane's own elements
    const StagedRound r = staged_round([&](auto &&f) { path_planes(out, n, total, f); });
    EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 96 * total : 0, planes & 2u ? 8 * 3 * total : 0, planes & 4u ? 4 * 4 * total : 0, planes & 8u ? 8 * total : 0, planes & 16u ? 4 * n : 0,
                                                 planes & 32u ? 4 * n : 0, planes & 64u ? 8 * n : 0, planes & 128u ? 8 * 6 * n : 0, planes & 256u ? 4 * n : 0}));
    const size_t want_bytes = (planes & 1u ? 96 * total : 0) + (planes & 2u ? 24 * total : 0) + (planes & 4u ? 16 * total : 0) + (planes & 8u ? 8 * total : 0) + (planes & 16u ? 4 * n : 0) +
                              (planes & 32u ? 4 * n : 0) + (planes & 64u ? 8 * n : 0) + (planes & 128u ? 48 * n : 0) + (planes & 256u ? 4 * n : 0);
    EXPECT(r.bytes == want_bytes);
}

int main() {
    int accel = 0;
    alignas(16) lg_hit h[2];
    alignas(16) double d[8] = {0.0};
    alignas(16) uint32_t u[8] = {0u};
    std::memset(h, 0, sizeof h);
    const lg_paths_out all{h, d, u, d, u, u, d, d, u}, none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t TOP = ~(size_t)0, EDGE = TOP / 96; // the most lg_hit records an address space holds
    const uint32_t KMAX = 0xFFFFFFFFu;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(QUERY_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    // ---- check_paths: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, 5, &all) && checked(&accel, 3, 5, &all) == 15);
    EXPECT(refused(nullptr, D, 3, 5, &all));
    EXPECT(refused(&accel, nullptr, 3, 5, &all));
    EXPECT(refused(&accel, D, 3, 5, nullptr));
    EXPECT(refused(&accel, D, 3, 5, &none));
    // max_bounces of 0, 1 and 2^32 - 1
    EXPECT(refused(&accel, D, 1, 0, &all) && refused(&accel, D, QUERY_MAX_RAYS, 0, &all));
    EXPECT(!refused(&accel, D, 1, 1, &all) && checked(&accel, 1, 1, &all) == 1);
    EXPECT(!refused(&accel, D, 1, KMAX, &all) && checked(&accel, 1, KMAX, &all) == KMAX);
    EXPECT(!refused(&accel, D, 65, KMAX, &all) && checked(&accel, 65, KMAX, &all) == 65ull * KMAX);
    // the ray limit: (2^32 - 1) * 64 and one above
    EXPECT(!refused(&accel, D, QUERY_MAX_RAYS, 1, &all) && checked(&accel, QUERY_MAX_RAYS, 1, &all) == QUERY_MAX_RAYS);
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS + 1, 1, &all) && refused(&accel, D, TOP, 1, &all) && refused(&accel, D, TOP, KMAX, &all));
    // n * max_bounces just under, at and over SIZE_MAX / 96: the hits plane's bytes fit or do not, whichever planes are asked for
    const uint32_t KS[] = {(uint32_t)1 << 20, 1000003u, KMAX};
    for (uint32_t k : KS) {
        const size_t under = EDGE / k; // under * k <= EDGE < (under + 1) * k
        EXPECT(under <= QUERY_MAX_RAYS && under * k <= EDGE && EDGE - under * k < k);
        EXPECT(!refused(&accel, D, under, k, &all) && checked(&accel, under, k, &all) == under * k);
        EXPECT(refused(&accel, D, under + 1, k, &all));
        const lg_paths_out only_count = subset(all, 16u); // the limit does not depend on the planes asked for
        EXPECT(!refused(&accel, D, under, k, &only_count) && refused(&accel, D, under + 1, k, &only_count));
        // no count of the plane table wraps at the edge: the widest in elements (id, 4 a vertex) and in bytes (hits)
        size_t most = 0;
        path_planes(all, under, under * k, [&](auto *p, size_t elems, size_t, const char *) { EXPECT(elems <= TOP / sizeof *p); most = elems > most ? elems : most; });
        EXPECT(most == 4 * under * k || most == 6 * under);
    }
    // the product itself: n * max_bounces beyond 2^64 is refused before it is formed
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS, KMAX, &all) && refused(&accel, D, (size_t)1 << 33, (uint32_t)1 << 31, &all));
    // the sizes
    EXPECT(checked_bytes(0, 96, "x") == 0 && checked_bytes(EDGE, 96, "x") == EDGE * 96 && checked_bytes(5, 0, "x") == 0);
    EXPECT(throws([&] { (void)checked_bytes(EDGE + 1, 96, "x"); }));
    // ---- the rules: NULL, a count that is not the accel's, an unknown action, reserved set; normal outside {0, 1}
    EXPECT(refused(&accel, D, 3, 5, &all, nullptr, 3, 3));
    EXPECT(refused(&accel, D, 3, 5, &all, RULES, 2, 3) && refused(&accel, D, 3, 5, &all, RULES, 3, 2) && refused(&accel, D, 3, 5, &all, RULES, 0, 3));
    EXPECT(!refused(&accel, D, 3, 5, &all, RULES, 0, 0)); // (a scene without materials: an empty table, nothing read)
    EXPECT(!refused(&accel, D, 3, 5, &all, RULES, 2, 2) && !refused(&accel, D, 3, 5, &all, RULES, 1, 1));
    for (size_t m = 0; m < 3; ++m) {
        std::unique_ptr<lg_path_rule[]> r(new lg_path_rule[3]); // (a heap block of exactly the table's size: a read past it is a report)
        for (uint32_t action = 0; action < 8; ++action) {
            std::memcpy(r.get(), RULES, sizeof RULES);
            r[m].action = action;
            EXPECT(refused(&accel, D, 3, 5, &all, r.get(), 3, 3) == (action > LG_PATH_REFRACT));
        }
        std::memcpy(r.get(), RULES, sizeof RULES);
        r[m].action = KMAX;
        EXPECT(refused(&accel, D, 3, 5, &all, r.get(), 3, 3));
        std::memcpy(r.get(), RULES, sizeof RULES);
        r[m].reserved = 1u;
        EXPECT(refused(&accel, D, 3, 5, &all, r.get(), 3, 3));
        r[m].reserved = 0u;
        r[m].ior = 0.0; r[m].gain = -1.0; // (any f64 is a value, not an error)
        EXPECT(!refused(&accel, D, 3, 5, &all, r.get(), 3, 3));
    }
    for (int normal : {-1, 2, 3, 1 << 30}) EXPECT(refused(&accel, D, 3, 5, &all, RULES, 3, 3, normal));
    EXPECT(!refused(&accel, D, 3, 5, &all, RULES, 3, 3, 1));
    // ---- the NULL rule: every combination of the nine planes; only all NULL is refused
    for (unsigned planes = 0; planes < 512; ++planes) {
        const lg_paths_out o = subset(all, planes);
        EXPECT(refused(&accel, D, 3, 5, &o) == (planes == 0));
        EXPECT(refused(nullptr, D, 3, 5, &o) && refused(&accel, nullptr, 3, 5, &o) && refused(&accel, D, 3, 0, &o));
    }
    // ---- the alignment rule: rays 8; start_medium 4; hits and id 16; point, along, gain and last 8; count, end and medium 4; NULL is not misaligned
    const char *base = reinterpret_cast<const char *>(d);
    EXPECT(!misaligned(D, u, all) && !misaligned(D, nullptr, none) && !misaligned(nullptr, nullptr, all));
    for (int off : {1, 2, 4}) EXPECT(misaligned(base + off, nullptr, all));
    EXPECT(!misaligned(base + 8, nullptr, all));
    for (int off : {1, 2, 3}) EXPECT(misaligned(D, reinterpret_cast<const char *>(u) + off, all));
    EXPECT(!misaligned(D, reinterpret_cast<const char *>(u) + 4, all));
    const size_t want_align[9] = {16, 8, 16, 8, 4, 4, 8, 8, 4};
    for (int k = 0; k < 9; ++k)
        for (int off : {1, 2, 4, 8, 16}) {
            lg_paths_out o = all;
            char *hp = reinterpret_cast<char *>(h) + off, *dp = reinterpret_cast<char *>(d) + off, *up = reinterpret_cast<char *>(u) + off;
            if (k == 0) o.hits = reinterpret_cast<lg_hit *>(hp);
            else if (k == 1) o.point = reinterpret_cast<double *>(dp);
            else if (k == 2) o.id = reinterpret_cast<uint32_t *>(up);
            else if (k == 3) o.along = reinterpret_cast<double *>(dp);
            else if (k == 4) o.count = reinterpret_cast<uint32_t *>(up);
            else if (k == 5) o.end = reinterpret_cast<uint32_t *>(up);
            else if (k == 6) o.gain = reinterpret_cast<double *>(dp);
            else if (k == 7) o.last = reinterpret_cast<double *>(dp);
            else o.medium = reinterpret_cast<uint32_t *>(up);
            EXPECT(misaligned(D, nullptr, o) == ((size_t)off % want_align[k] != 0));
        }
    // ---- staging and placement: every subset of the planes, shapes with partial tiles and more than one vertex
    const size_t shapes[][2] = {{1, 1}, {1, 8}, {63, 2}, {64, 3}, {65, 1}, {129, 8}};
    for (const auto &s : shapes)
        for (unsigned planes = 1; planes < 512; ++planes) run(s[0], (uint32_t)s[1], planes);
    if (failures) { std::fprintf(stderr, "paths_host_check: %d failures\n", failures); return 1; }
    std::printf("paths_host_check: ok\n");
    return 0;
}
