// tools/scatter_host_check.cpp -- the device-free host code of lg_scatter* (lasgun_amd/csrc/scatter_host.h: the limits, the planes' byte
// sizes with their overflow checks, the light count's refusal, the NULL and alignment rules of lg_scatter_out, the host form's staging) in
// a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_scatter_host_sanitized.py
// does).  The counts go up to 2^64 - 1: an overflow in forming a size is a UBSan report or a wrong value here, not a short buffer on a
// card.  The launch is stubbed out: a "kernel" that fills the staged planes with bytes that name their place (host_check.h, staged_round); every caller's array is a
// heap block of exactly its size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/scatter_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/scatter_host.h"
#include "host_check.h"

using namespace lg;

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};

static bool refused(const void *accel, const double *rays, size_t n, const lg_scatter_out *out, size_t lights = 1) {
    return throws([&] { check_scatter(accel, rays, n, out, lights); });
}
static bool misaligned(const void *rays, const lg_scatter_out &out) {
    return throws([&] { check_scatter_alignment((const double *)rays, out); });
}
// lg_scatter_out with the planes of a 7-bit mask named from `all`, in the struct's order
static lg_scatter_out subset(const lg_scatter_out &all, unsigned planes) {
    return lg_scatter_out{planes & 1u ? all.hits : nullptr,           planes & 2u ? all.direct : nullptr,   planes & 4u ? all.flags : nullptr,
                          planes & 8u ? all.reflect : nullptr,        planes & 16u ? all.reflect_weight : nullptr,
                          planes & 32u ? all.refract : nullptr,       planes & 64u ? all.refract_weight : nullptr};
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of every output is looked at
static void run(size_t n, unsigned planes) {
    const lg_scatter_out all{(lg_hit *)ASKED, (double *)ASKED, (uint32_t *)ASKED, (double *)ASKED, (double *)ASKED, (double *)ASKED, (double *)ASKED};
    lg_scatter_out out = subset(all, planes);
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    EXPECT(!refused(&accel, D, n, &out));
    // what the host form allocates on the device and copies back: the table's counts in the plane's own elements
    const StagedRound r = staged_round([&](auto &&f) { scatter_planes(out, n, f); });
    EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 96 * n : 0, planes & 2u ? 8 * 3 * n : 0, planes & 4u ? 4 * n : 0, planes & 8u ? 8 * 6 * n : 0, planes & 16u ? 8 * 3 * n : 0,
                                                 planes & 32u ? 8 * 6 * n : 0, planes & 64u ? 8 * 5 * n : 0}));
    const size_t want_bytes = n * ((planes & 1u ? 96 : 0) + (planes & 2u ? 24 : 0) + (planes & 4u ? 4 : 0) + (planes & 8u ? 48 : 0) + (planes & 16u ? 24 : 0) + (planes & 32u ? 48 : 0) +
                                   (planes & 64u ? 40 : 0));
    EXPECT(r.bytes == want_bytes);
    if (planes == 127u) EXPECT(want_bytes == n * SCATTER_ROW_BYTES);
}

int main() {
    int accel = 0;
    alignas(16) lg_hit h[2];
    alignas(16) double d[8] = {0.0};
    alignas(16) uint32_t u[8] = {0u};
    std::memset(h, 0, sizeof h);
    const lg_scatter_out all{h, d, u, d, d, d, d}, none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t TOP = ~(size_t)0, EDGE = TOP / 96; // the most lg_hit records an address space holds
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(QUERY_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    static_assert(SCATTER_ROW_BYTES == 284, "96 + 24 + 4 + 48 + 24 + 48 + 40");
    // ---- check_scatter: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, &all));
    EXPECT(refused(nullptr, D, 3, &all));
    EXPECT(refused(&accel, nullptr, 3, &all));
    EXPECT(refused(&accel, D, 3, nullptr));
    EXPECT(refused(&accel, D, 3, &none));
    // the ray limit: (2^32 - 1) * 64 and one above; it is below what an address space holds of lg_hit records, so no size wraps
    EXPECT(!refused(&accel, D, QUERY_MAX_RAYS, &all));
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS + 1, &all) && refused(&accel, D, EDGE, &all) && refused(&accel, D, EDGE + 1, &all) && refused(&accel, D, TOP, &all));
    EXPECT(QUERY_MAX_RAYS < EDGE);
    {
        size_t most = 0; // no count of the plane table wraps at the limit: the widest in elements (reflect, 6 a ray) and in bytes (hits)
        scatter_planes(all, (size_t)QUERY_MAX_RAYS, [&](auto *p, size_t elems, size_t, const char *) { EXPECT(elems <= TOP / sizeof *p); most = elems > most ? elems : most; });
        EXPECT(most == 6 * (size_t)QUERY_MAX_RAYS);
    }
    // the sizes
    EXPECT(checked_bytes(0, 96, "x") == 0 && checked_bytes(EDGE, 96, "x") == EDGE * 96 && checked_bytes(5, 0, "x") == 0);
    EXPECT(throws([&] { (void)checked_bytes(EDGE + 1, 96, "x"); }));
    // the lights: 0 .. 32 are served, 33 and more refused (lg_radiance's refusal); there is no depth to refuse
    for (size_t lights : {(size_t)0, (size_t)1, (size_t)32}) EXPECT(!refused(&accel, D, 3, &all, lights));
    for (size_t lights : {(size_t)33, (size_t)64, TOP}) EXPECT(refused(&accel, D, 3, &all, lights));
    // ---- the NULL rule: every combination of the seven planes; only all NULL is refused
    for (unsigned planes = 0; planes < 128; ++planes) {
        const lg_scatter_out o = subset(all, planes);
        EXPECT(refused(&accel, D, 3, &o) == (planes == 0));
        EXPECT(refused(nullptr, D, 3, &o) && refused(&accel, nullptr, 3, &o) && refused(&accel, D, 3, &o, 33));
    }
    // ---- the alignment rule: rays 8; hits 16; the double planes 8; flags 4; NULL is not misaligned
    const char *base = reinterpret_cast<const char *>(d);
    EXPECT(!misaligned(D, all) && !misaligned(D, none) && !misaligned(nullptr, all));
    for (int off : {1, 2, 4}) EXPECT(misaligned(base + off, all));
    EXPECT(!misaligned(base + 8, all));
    const size_t want_align[7] = {16, 8, 4, 8, 8, 8, 8};
    for (int k = 0; k < 7; ++k)
        for (int off : {1, 2, 4, 8, 16}) {
            lg_scatter_out o = all;
            char *hp = reinterpret_cast<char *>(h) + off, *up = reinterpret_cast<char *>(u) + off;
            double *dp = reinterpret_cast<double *>(reinterpret_cast<char *>(d) + off);
            if (k == 0) o.hits = reinterpret_cast<lg_hit *>(hp);
            else if (k == 1) o.direct = dp;
            else if (k == 2) o.flags = reinterpret_cast<uint32_t *>(up);
            else if (k == 3) o.reflect = dp;
            else if (k == 4) o.reflect_weight = dp;
            else if (k == 5) o.refract = dp;
            else o.refract_weight = dp;
            EXPECT(misaligned(D, o) == ((size_t)off % want_align[k] != 0));
        }
    // ---- staging and placement: every subset of the planes, shapes with partial tiles
    const size_t shapes[] = {1, 63, 64, 65, 129};
    for (size_t n : shapes)
        for (unsigned planes = 1; planes < 128; ++planes) run(n, planes);
    if (failures) { std::fprintf(stderr, "scatter_host_check: %d failures\n", failures); return 1; }
    std::printf("scatter_host_check: ok\n");
    return 0;
}
