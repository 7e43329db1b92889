// tools/layers_host_check.cpp -- the device-free host code of lg_hit_layers* (lasgun_amd/csrc/layers_host.h: the limits, the product
// n * max_layers and the planes' byte sizes with their overflow checks, the NULL and alignment rules of lg_layers_out, the host form's
// staging) in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_layers_host_sanitized.py does).  The counts go up to 2^64 - 1: an overflow in forming a product or a size is a UBSan report
// or a wrong value here, not a short buffer on a card.  The launch is stubbed out: a "kernel" that fills the staged planes with bytes that
// name their place (host_check.h, staged_round); every caller's array is a heap block of exactly its size, so a copy past an end is an
// ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/layers_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/layers_host.h"
#include "host_check.h"

using namespace lg;

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};

static bool refused(const void *accel, const double *rays, size_t n, uint32_t max_layers, const lg_layers_out *out) {
    return throws([&] { (void)check_layers(accel, rays, n, max_layers, out); });
}
static bool misaligned(const void *rays, const lg_layers_out &out) {
    return throws([&] { check_layers_alignment((const double *)rays, out); });
}
// lg_layers_out with the planes of a 5-bit mask named from `all`
static lg_layers_out subset(const lg_layers_out &all, unsigned planes) {
    return lg_layers_out{planes & 1u ? all.hits : nullptr, planes & 2u ? all.along : nullptr, planes & 4u ? all.id : nullptr, planes & 8u ? all.count : nullptr,
                         planes & 16u ? all.inside : nullptr};
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of every output is looked at
static void run(size_t n, uint32_t max_layers, unsigned planes) {
    const size_t total = n * max_layers;
    const lg_layers_out all{(lg_hit *)ASKED, (double *)ASKED, (uint32_t *)ASKED, (uint32_t *)ASKED, (double *)ASKED};
    lg_layers_out out = subset(all, planes);
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    EXPECT(check_layers(&accel, D, n, max_layers, &out) == total);
    // what the host form allocates on the device and copies back: the table's counts in the plane's own elements
    const StagedRound r = staged_round([&](auto &&f) { layer_planes(out, n, total, f); });
    EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 96 * total : 0, planes & 2u ? 8 * total : 0, planes & 4u ? 4 * 4 * total : 0, planes & 8u ? 4 * n : 0, planes & 16u ? 8 * n : 0}));
    const size_t want_bytes = (planes & 1u ? 96 * total : 0) + (planes & 2u ? 8 * total : 0) + (planes & 4u ? 16 * total : 0) + (planes & 8u ? 4 * n : 0) + (planes & 16u ? 8 * n : 0);
    EXPECT(r.bytes == want_bytes);
}

int main() {
    int accel = 0;
    alignas(16) lg_hit h[2];
    alignas(16) double d[8] = {0.0};
    alignas(16) uint32_t u[8] = {0u};
    std::memset(h, 0, sizeof h);
    const lg_layers_out all{h, d, u, u, d}, none{nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t TOP = ~(size_t)0, EDGE = TOP / 96; // the most lg_hit records an address space holds
    const uint32_t KMAX = 0xFFFFFFFFu;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(QUERY_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    // ---- check_layers: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, 5, &all) && check_layers(&accel, D, 3, 5, &all) == 15);
    EXPECT(refused(nullptr, D, 3, 5, &all));
    EXPECT(refused(&accel, nullptr, 3, 5, &all));
    EXPECT(refused(&accel, D, 3, 5, nullptr));
    EXPECT(refused(&accel, D, 3, 5, &none));
    // max_layers of 0, 1 and 2^32 - 1
    EXPECT(refused(&accel, D, 1, 0, &all) && refused(&accel, D, QUERY_MAX_RAYS, 0, &all));
    EXPECT(!refused(&accel, D, 1, 1, &all) && check_layers(&accel, D, 1, 1, &all) == 1);
    EXPECT(!refused(&accel, D, 1, KMAX, &all) && check_layers(&accel, D, 1, KMAX, &all) == KMAX);
    EXPECT(!refused(&accel, D, 65, KMAX, &all) && check_layers(&accel, D, 65, KMAX, &all) == 65ull * KMAX);
    // the ray limit: (2^32 - 1) * 64 and one above
    EXPECT(!refused(&accel, D, QUERY_MAX_RAYS, 1, &all) && check_layers(&accel, D, QUERY_MAX_RAYS, 1, &all) == QUERY_MAX_RAYS);
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS + 1, 1, &all) && refused(&accel, D, TOP, 1, &all) && refused(&accel, D, TOP, KMAX, &all));
    // n * max_layers just under, at and over SIZE_MAX / 96: the hits plane's bytes fit or do not, whichever planes are asked for
    const uint32_t KS[] = {(uint32_t)1 << 20, 1000003u, KMAX};
    for (uint32_t k : KS) {
        const size_t under = EDGE / k; // under * k <= EDGE < (under + 1) * k
        EXPECT(under <= QUERY_MAX_RAYS && under * k <= EDGE && EDGE - under * k < k);
        EXPECT(!refused(&accel, D, under, k, &all) && check_layers(&accel, D, under, k, &all) == under * k);
        EXPECT(refused(&accel, D, under + 1, k, &all));
        const lg_layers_out only_count = subset(all, 8u); // the limit does not depend on the planes asked for
        EXPECT(!refused(&accel, D, under, k, &only_count) && refused(&accel, D, under + 1, k, &only_count));
    }
    // the product itself: n * max_layers beyond 2^64 is refused before it is formed
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS, KMAX, &all) && refused(&accel, D, (size_t)1 << 33, (uint32_t)1 << 31, &all));
    // the sizes
    EXPECT(checked_bytes(0, 96, "x") == 0 && checked_bytes(EDGE, 96, "x") == EDGE * 96 && checked_bytes(5, 0, "x") == 0);
    EXPECT(throws([&] { (void)checked_bytes(EDGE + 1, 96, "x"); }));
    // ---- the NULL rule: every combination of the five planes; only all NULL is refused
    for (unsigned planes = 0; planes < 32; ++planes) {
        const lg_layers_out o = subset(all, planes);
        EXPECT(refused(&accel, D, 3, 5, &o) == (planes == 0));
        EXPECT(refused(nullptr, D, 3, 5, &o) && refused(&accel, nullptr, 3, 5, &o) && refused(&accel, D, 3, 0, &o));
    }
    // ---- the alignment rule: rays 8; hits and id 16; along and inside 8; count 4; NULL is not misaligned
    const char *base = reinterpret_cast<const char *>(d);
    EXPECT(!misaligned(D, all) && !misaligned(D, none) && !misaligned(nullptr, all));
    for (int off : {1, 2, 4}) EXPECT(misaligned(base + off, all));
    EXPECT(!misaligned(base + 8, all));
    const size_t want_align[5] = {16, 8, 16, 4, 8};
    for (int k = 0; k < 5; ++k)
        for (int off : {1, 2, 4, 8, 16}) {
            lg_layers_out o = all;
            if (k == 0) o.hits = reinterpret_cast<lg_hit *>(reinterpret_cast<char *>(h) + off);
            else if (k == 1) o.along = reinterpret_cast<double *>(reinterpret_cast<char *>(d) + off);
            else if (k == 2) o.id = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(u) + off);
            else if (k == 3) o.count = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(u) + off);
            else o.inside = reinterpret_cast<double *>(reinterpret_cast<char *>(d) + off);
            EXPECT(misaligned(D, o) == ((size_t)off % want_align[k] != 0));
        }
    // ---- staging and placement: every subset of the planes, shapes with partial tiles and more than one layer
    const size_t shapes[][2] = {{1, 1}, {1, 8}, {63, 2}, {64, 3}, {65, 1}, {129, 8}};
    for (const auto &s : shapes)
        for (unsigned planes = 1; planes < 32; ++planes) run(s[0], (uint32_t)s[1], planes);
    if (failures) { std::fprintf(stderr, "layers_host_check: %d failures\n", failures); return 1; }
    std::printf("layers_host_check: ok\n");
    return 0;
}
