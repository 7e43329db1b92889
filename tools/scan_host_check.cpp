// tools/scan_host_check.cpp -- the device-free host code of lg_range_scan* (lasgun_amd/csrc/scan_host.h: the lane rule, the two tile counts
// with their 32-bit limit, the planes' byte sizes, the NULL and alignment rules of lg_scan_out, the host form's staging) in a stand-alone
// program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_scan_host_sanitized.py does).  The counts
// go up to 2^64 - 1: an overflow in forming a tile count or a size is a UBSan report or a wrong value here, not a short buffer on a card.
// The launch is stubbed out: a "kernel" that fills the staged planes with bytes that name their place (host_check.h, staged_round); every caller's array is a heap
// block of exactly its size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/scan_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/scan_host.h"
#include "host_check.h"

using namespace lg;

static const double D[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

static bool refused(const void *accel, const double *origins, size_t n_poses, const double *beams, size_t n_beams, int lanes, const lg_scan_out *out) {
    return throws([&] { (void)check_scan(accel, origins, n_poses, beams, n_beams, lanes, out); });
}
static bool misaligned(const void *origins, const void *frames, const void *beams, const lg_scan_out &out) {
    return throws([&] { check_scan_alignment((const double *)origins, (const double *)frames, (const double *)beams, out); });
}
// the tile count of a shape in a form, -1 where it passes 2^32 - 1
static long long tiles(size_t n_poses, size_t n_beams, int form) {
    unsigned long long t = 0;
    return scan_tiles(n_poses, n_beams, form, &t) ? (long long)t : -1;
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of every output is looked at
static void run(size_t n_poses, size_t n_beams, int lanes, unsigned planes) {
    const size_t pairs = n_poses * n_beams;
    lg_scan_out out{planes & 1u ? (float *)ASKED : nullptr, planes & 2u ? (float *)ASKED : nullptr, planes & 4u ? (float *)ASKED : nullptr,
                    planes & 8u ? (uint32_t *)ASKED : nullptr, planes & 16u ? (uint32_t *)ASKED : nullptr, planes & 32u ? (float *)ASKED : nullptr};
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    const ScanShape shape = check_scan(&accel, D, n_poses, D, n_beams, lanes, &out);
    EXPECT(shape.pairs == pairs && shape.form == scan_lanes(n_poses, n_beams, lanes) && (long long)shape.tiles == tiles(n_poses, n_beams, shape.form));
    const StagedRound r = staged_round([&](auto &&f) { scan_planes(out, n_poses, pairs, f); });
    EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 4 * pairs : 0, planes & 2u ? 4 * 3 * pairs : 0, planes & 4u ? 4 * 3 * pairs : 0, planes & 8u ? 4 * 4 * pairs : 0,
                                                 planes & 16u ? 4 * n_poses : 0, planes & 32u ? 4 * n_poses : 0}));
    EXPECT(r.bytes == pairs * ((planes & 1u ? 4 : 0) + (planes & 2u ? 12 : 0) + (planes & 4u ? 12 : 0) + (planes & 8u ? 16 : 0)) + n_poses * ((planes & 16u ? 4 : 0) + (planes & 32u ? 4 : 0)));
}

int main() {
    int accel = 0;
    alignas(16) float f[8] = {0.0f};
    alignas(16) uint32_t u[8] = {0u};
    const lg_scan_out all{f, f, f, u, u, f}, none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t M = 0xFFFFFFFFull, TOP = ~(size_t)0;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    // ---- the lane rule: 1 and 2 are taken as given, 0 is pose lanes iff n_poses >= n_beams, anything else is -1
    const size_t counts[] = {0, 1, 7, 8, 63, 64, 65, 1024, M, M + 1, TOP - 1, TOP};
    for (size_t n : counts)
        for (size_t k : counts) {
            EXPECT(scan_lanes(n, k, 1) == 1 && scan_lanes(n, k, 2) == 2);
            EXPECT(scan_lanes(n, k, 0) == (n >= k ? 2 : 1));
            for (int bad : {-1, 3, 64, -2147483647 - 1, 2147483647}) EXPECT(scan_lanes(n, k, bad) == -1);
        }
    // ---- the tile counts: small shapes by hand
    EXPECT(tiles(1, 1, 1) == 1 && tiles(1, 64, 1) == 1 && tiles(1, 65, 1) == 2 && tiles(257, 1031, 1) == 257 * 17 && tiles(0, 5, 1) == 0 && tiles(5, 0, 1) == 0);
    EXPECT(tiles(1, 1, 2) == 1 && tiles(64, 8, 2) == 1 && tiles(65, 9, 2) == 4 && tiles(257, 1031, 2) == 5 * 129 && tiles(0, 5, 2) == 0 && tiles(5, 0, 2) == 0);
    // ... at their limit and one above, in both forms.  Beam lanes: n_poses * ceil(n_beams / 64)
    EXPECT(tiles(M, 1, 1) == (long long)M && tiles(M, 64, 1) == (long long)M && tiles(M + 1, 64, 1) == -1 && tiles(M, 65, 1) == -1);
    EXPECT(tiles(1, M, 1) == (1ll << 26) && tiles(63, M, 1) == 63ll << 26 && tiles(64, M, 1) == -1); // 64 * 2^26 = 2^32: one above the limit
    EXPECT(tiles(65535, 65537 * 64, 1) == 65535ll * 65537 && tiles(65536, 65536 * 64, 1) == -1 && tiles(65536, 65536 * 64 - 64, 1) == 65536ll * 65535); // 2^32 - 1 exactly
    EXPECT(tiles(TOP, 1, 1) == -1 && tiles(TOP, TOP, 1) == -1 && tiles(1, TOP, 1) == -1); // (2^58 tiles; n_beams > 2^32 - 1 is check_scan's own refusal besides)
    // Pose lanes: ceil(n_poses / 64) * ceil(n_beams / 8)
    EXPECT(tiles(64 * M, 8, 2) == (long long)M && tiles(64 * M + 1, 8, 2) == -1 && tiles(64 * M, 9, 2) == -1);
    EXPECT(tiles(64, M, 2) == (1ll << 29) && tiles(64 * 7, M, 2) == 7ll << 29 && tiles(64 * 8, M, 2) == -1 && tiles(64 * 7 + 1, M, 2) == -1);
    EXPECT(tiles(65535 * 64, 65537 * 8, 2) == 65535ll * 65537 && tiles(65536 * 64, 65536 * 8, 2) == -1 && tiles(65536 * 64 - 63, 65536 * 8 - 8, 2) == 65536ll * 65535);
    EXPECT(tiles(TOP, 1, 2) == -1 && tiles(TOP, TOP, 2) == -1 && tiles(TOP - 63, 1, 2) == -1);
    // ---- check_scan: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, D, 5, 0, &all));
    EXPECT(refused(nullptr, D, 3, D, 5, 0, &all));
    EXPECT(refused(&accel, D, 3, D, 5, 0, nullptr));
    EXPECT(refused(&accel, nullptr, 3, D, 5, 0, &all));
    EXPECT(refused(&accel, D, 3, nullptr, 5, 0, &all));
    EXPECT(refused(&accel, D, 3, D, 5, 0, &none));
    for (int bad : {-1, 3, 1 << 20}) EXPECT(refused(&accel, D, 3, D, 5, bad, &all));
    EXPECT(refused(&accel, D, 1, D, M + 1, 1, &all) && refused(&accel, D, 1, D, M + 1, 2, &all) && refused(&accel, D, 1, D, TOP, 0, &all)); // n_beams > 2^32 - 1
    EXPECT(!refused(&accel, D, 1, D, M, 1, &all) && !refused(&accel, D, 1, D, M, 2, &all));
    EXPECT(!refused(&accel, D, M, D, 64, 1, &all) && refused(&accel, D, M + 1, D, 64, 1, &all) && refused(&accel, D, M, D, 65, 1, &all));
    EXPECT(!refused(&accel, D, 64 * M, D, 8, 2, &all) && refused(&accel, D, 64 * M + 1, D, 8, 2, &all) && refused(&accel, D, 64 * M, D, 9, 2, &all));
    EXPECT(!refused(&accel, D, M + 1, D, 64, 2, &all) && !refused(&accel, D, M + 1, D, 64, 0, &all)); // the form decides: auto takes pose lanes here
    EXPECT(refused(&accel, D, 64 * 8, D, M, 0, &all) && refused(&accel, D, 64, D, M, 1, &all) && !refused(&accel, D, 63, D, M, 0, &all));
    EXPECT(refused(&accel, D, TOP, D, TOP, 0, &all) && refused(&accel, D, TOP, D, 1, 1, &all) && refused(&accel, D, TOP, D, 1, 2, &all));
    // what a checked call is
    {
        const ScanShape a = check_scan(&accel, D, 257, D, 1031, 0, &all), b = check_scan(&accel, D, 1031, D, 257, 0, &all), c = check_scan(&accel, D, 64 * M, D, 8, 2, &all);
        EXPECT(a.form == 1 && a.tiles == 257u * 17u && a.pairs == 257u * 1031u);
        EXPECT(b.form == 2 && b.tiles == 17u * 33u && b.pairs == 257u * 1031u);
        EXPECT(c.form == 2 && c.tiles == 0xFFFFFFFFu && c.pairs == 64 * M * 8);
    }
    // the sizes
    EXPECT(checked_bytes(0, 16, "x") == 0 && checked_bytes(TOP / 16, 16, "x") == TOP / 16 * 16 && checked_bytes(5, 0, "x") == 0);
    EXPECT(throws([&] { (void)checked_bytes(TOP / 16 + 1, 16, "x"); }));
    // a single NULL output in every position is accepted, a single non-NULL one too
    for (int k = 0; k < 6; ++k) {
        lg_scan_out one = none, but = all;
        float **fp[6] = {&one.range, &one.point, &one.normal, nullptr, nullptr, &one.nearest};
        float **bp[6] = {&but.range, &but.point, &but.normal, nullptr, nullptr, &but.nearest};
        if (fp[k]) { *fp[k] = f; *bp[k] = nullptr; }
        else if (k == 3) { one.id = u; but.id = nullptr; }
        else { one.hits = u; but.hits = nullptr; }
        EXPECT(!refused(&accel, D, 3, D, 5, 0, &one));
        EXPECT(!refused(&accel, D, 3, D, 5, 0, &but));
    }
    // ---- the alignment rule: the inputs 8, id 16, the float planes, hits and nearest 4; NULL is not misaligned
    const char *base = reinterpret_cast<const char *>(f);
    EXPECT(!misaligned(D, D, D, all) && !misaligned(D, nullptr, D, all) && !misaligned(D, D, D, none));
    EXPECT(misaligned(base + 4, D, D, all) && misaligned(D, base + 4, D, all) && misaligned(D, D, base + 4, all));
    for (int k = 0; k < 6; ++k)
        for (int off : {1, 2, 4, 8}) {
            lg_scan_out o = all;
            char *p = reinterpret_cast<char *>(k == 3 || k == 4 ? (void *)u : (void *)f) + off;
            if (k == 0) o.range = (float *)p; else if (k == 1) o.point = (float *)p; else if (k == 2) o.normal = (float *)p;
            else if (k == 3) o.id = (uint32_t *)p; else if (k == 4) o.hits = (uint32_t *)p; else o.nearest = (float *)p;
            EXPECT(misaligned(D, D, D, o) == (off % (k == 3 ? 16 : 4) != 0));
        }
    // ---- staging and placement: every subset of the outputs, shapes on both sides of the lane rule
    const size_t shapes[][2] = {{1, 1}, {1, 65}, {65, 9}, {9, 65}, {17, 130}, {64, 8}};
    for (const auto &s : shapes)
        for (unsigned planes = 1; planes < 64; ++planes)
            for (int lanes = 0; lanes < 3; ++lanes) run(s[0], s[1], lanes, planes);
    if (failures) { std::fprintf(stderr, "scan_host_check: %d failures\n", failures); return 1; }
    std::printf("scan_host_check: ok\n");
    return 0;
}
