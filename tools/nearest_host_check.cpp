// tools/nearest_host_check.cpp -- the device-free host code of lg_nearest* (lasgun_amd/csrc/nearest_host.h: the five-plane table, every check
// and every refusal in its order, what the planes asked for make of k, n * k and the sizes at their limits, the alignment rule, the LDS
// rule at its edge, the host form's staging for every subset of the planes) compiled alone for the CPU, with its own main: nothing of HIP,
// nothing loaded into python.  tests/test_nearest_host_sanitized.py builds it under AddressSanitizer and UBSan.
//
// usage: nearest_host_check               the self-checks; prints "nearest_host_check: ok"
#include <cmath>
#include <cstdio>
#include <limits>

#include "../lasgun_amd/csrc/nearest_host.h"
#include "host_check.h"

using namespace lg;

static const double INF = std::numeric_limits<double>::infinity(), QNAN = std::numeric_limits<double>::quiet_NaN();

static lg_nearest_out subset(int planes, void *p) {
    return lg_nearest_out{(planes & 1) ? (uint8_t *)p : nullptr, (planes & 2) ? (uint32_t *)p : nullptr, (planes & 4) ? (double *)p : nullptr, (planes & 8) ? (double *)p : nullptr,
                          (planes & 16) ? (uint32_t *)p : nullptr};
}

static void check_the_call() {
    int accel = 0;
    const double D[3] = {0, 0, 0};
    const lg_nearest_out all = subset(31, ASKED), none = subset(0, ASKED), flags = subset(3, ASKED);
    const size_t HUGE_N = (size_t)-1;
    EXPECT(check_nearest(&accel, D, nullptr, 5, INF, 8, &all) == 40);
    EXPECT(check_nearest(&accel, D, nullptr, 5, 0.0, 1, &all) == 5);
    EXPECT(check_nearest(&accel, D, D, 5, -0.0, 3, &all) == 15);
    // every refusal, in its order: each call has every LATER fault too, and names the first
    EXPECT(thrown([&] { check_nearest(nullptr, nullptr, nullptr, HUGE_N, -1.0, 9, nullptr); }) == "accel is NULL");
    EXPECT(thrown([&] { check_nearest(&accel, nullptr, nullptr, HUGE_N, -1.0, 9, nullptr); }) == "points is NULL");
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, -1.0, 9, nullptr); }) == "out is NULL");
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, -1.0, 9, &none); }).find("every plane of out is NULL") == 0);
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, -1.0, 9, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, QNAN, 9, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, -INF, 9, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, INF, 9, &all); }) == "k is beyond LG_NEAREST_MAX_K");
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, INF, 0, &all); }) == "k is 0 and a slot plane (distance, point, id) is asked for");
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, HUGE_N, INF, 8, &all); }) == "too many points in one query");
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, (size_t)(QUERY_MAX_RAYS + 1), 1.0, 8, &all); }) == "too many points in one query");
    EXPECT(check_nearest(&accel, D, nullptr, (size_t)QUERY_MAX_RAYS, 1.0, 8, &all) == (size_t)QUERY_MAX_RAYS * 8);
    // with radii the shared radius is neither read nor checked
    EXPECT(!throws([&] { check_nearest(&accel, D, D, 5, -1.0, 8, &all); }));
    EXPECT(!throws([&] { check_nearest(&accel, D, D, 5, QNAN, 8, &all); }));
    // k: 0 is legal iff no slot plane is asked for, and then n * k is 0 whatever k is; beyond LG_NEAREST_MAX_K never
    EXPECT(check_nearest(&accel, D, nullptr, 5, 1.0, 0, &flags) == 0 && check_nearest(&accel, D, nullptr, 5, 1.0, 8, &flags) == 0);
    EXPECT(thrown([&] { check_nearest(&accel, D, nullptr, 5, 1.0, 9, &flags); }) == "k is beyond LG_NEAREST_MAX_K");
    for (int planes = 1; planes < 32; ++planes) { // each plane alone is enough; a slot plane needs k > 0
        const lg_nearest_out o = subset(planes, ASKED);
        EXPECT(nearest_slots(o) == ((planes & 28) != 0) && nearest_entries(o, 5) == ((planes & 28) ? 5u : 0u));
        EXPECT(!throws([&] { check_nearest(&accel, D, nullptr, 5, 2.0, 4, &o); }));
        EXPECT(throws([&] { check_nearest(&accel, D, nullptr, 5, 2.0, 0, &o); }) == ((planes & 28) != 0));
    }
    // the sizes: checked_bytes refuses what wraps, n * k first, then the widest plane's bytes
    EXPECT(thrown([&] { (void)checked_bytes(SIZE_MAX / 8 + 1, 8, "n * k"); }) == "n * k does not fit the address space");
    EXPECT(thrown([&] { (void)checked_bytes(SIZE_MAX / 24 + 1, 24, "point"); }) == "point does not fit the address space");
    EXPECT(checked_bytes(SIZE_MAX / 24, 24, "point") == SIZE_MAX / 24 * 24);
    // alignment: points, radii, distance and point 8 bytes, count 4, id 16, touch any; NULL is not misaligned
    alignas(16) unsigned char mem[64];
    auto at = [&](size_t off) { return (void *)(mem + off); };
    EXPECT(!throws([&] { check_nearest_alignment((double *)at(8), (double *)at(24), lg_nearest_out{(uint8_t *)at(1), (uint32_t *)at(4), (double *)at(8), (double *)at(24), (uint32_t *)at(16)}); }));
    EXPECT(!throws([&] { check_nearest_alignment((double *)at(8), nullptr, none); }));
    EXPECT(thrown([&] { check_nearest_alignment((double *)at(4), nullptr, all); }) == "points is not 8-byte aligned");
    EXPECT(thrown([&] { check_nearest_alignment(D, (double *)at(4), all); }) == "radii is not 8-byte aligned");
    EXPECT(thrown([&] { check_nearest_alignment(D, nullptr, lg_nearest_out{nullptr, (uint32_t *)at(2), nullptr, nullptr, nullptr}); }) == "count is not 4-byte aligned");
    EXPECT(thrown([&] { check_nearest_alignment(D, nullptr, lg_nearest_out{nullptr, nullptr, (double *)at(4), nullptr, nullptr}); }) == "distance is not 8-byte aligned");
    EXPECT(thrown([&] { check_nearest_alignment(D, nullptr, lg_nearest_out{nullptr, nullptr, nullptr, (double *)at(12), nullptr}); }) == "point is not 8-byte aligned");
    EXPECT(thrown([&] { check_nearest_alignment(D, nullptr, lg_nearest_out{nullptr, nullptr, nullptr, nullptr, (uint32_t *)at(8)}); }) == "id is not 16-byte aligned");
    // the host form's staging, every subset of the planes, n up to a few tiles, k at its ends: a slot plane is k times a per-point one
    for (size_t n : {(size_t)1, (size_t)63, (size_t)65, (size_t)1025})
        for (uint32_t k : {1u, 3u, 8u})
            for (int planes = 1; planes < 32; ++planes) {
                lg_nearest_out o = subset(planes, ASKED);
                const size_t nk = check_nearest(&accel, D, nullptr, n, INF, k, &o);
                EXPECT(nk == ((planes & 28) ? n * k : 0));
                const StagedRound r = staged_round([&](auto &&f) { nearest_planes(o, n, nk, f); });
                EXPECT(r.plane_bytes.size() == 5);
                EXPECT(r.plane_bytes[0] == ((planes & 1) ? n : 0) && r.plane_bytes[1] == ((planes & 2) ? n * 4 : 0) && r.plane_bytes[2] == ((planes & 4) ? nk * 8 : 0) &&
                       r.plane_bytes[3] == ((planes & 8) ? nk * 24 : 0) && r.plane_bytes[4] == ((planes & 16) ? nk * 16 : 0));
            }
}

static void check_the_lds_rule() {
    // 256 lanes x (8 bytes a stack entry + 20 bytes a list entry); the limit is 160 KiB, met exactly at depth 60 with k = 8
    EXPECT(nearest_lds_bytes(1, 0) == 2048 && nearest_lds_bytes(0, 1) == 5120 && nearest_lds_bytes(32, 8) == 65536 + 40960);
    EXPECT(nearest_lds_bytes(60, 8) == NEAREST_LDS_LIMIT && NEAREST_LDS_LIMIT == 163840);
    EXPECT(!throws([&] { check_nearest_lds(60, 8); }));
    EXPECT(thrown([&] { check_nearest_lds(61, 8); }).find("nearest: a stack of 61 entries and lists of 8 need 165888 bytes") == 0);
    EXPECT(!throws([&] { check_nearest_lds(CLOSEST_MAX_DEPTH, 6); }) && throws([&] { check_nearest_lds(CLOSEST_MAX_DEPTH, 7); }));
    for (uint32_t depth = 1; depth <= CLOSEST_MAX_DEPTH; ++depth)
        for (uint32_t k = 0; k <= NEAREST_MAX_K; ++k)
            EXPECT(throws([&] { check_nearest_lds(depth, k); }) == ((size_t)256 * (8 * depth + 20 * k) > ((size_t)160 << 10)));
    EXPECT(!throws([&] { check_nearest_lds(CLOSEST_MAX_DEPTH, 0); })); // without a slot plane every scene the depth rule lets pass is answered
}

int main() {
    check_the_call();
    check_the_lds_rule();
    if (failures) { std::fprintf(stderr, "nearest_host_check: %d failures\n", failures); return 1; }
    std::printf("nearest_host_check: ok\n");
    return 0;
}
