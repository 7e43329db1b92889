// tools/gather_host_check.cpp -- the device-free host code of lg_radiance_gather* (lasgun_amd/csrc/gather_host.h: the lane rule, the two
// tile counts with their 32-bit limit, the four byte sizes, the NULL and alignment rules of lg_gather_out, the batch a parked call is cut
// into, the host form's staging) in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_gather_host_sanitized.py does).  The counts go up to 2^64 - 1: an overflow in forming a tile count, a size or a batch is a
// UBSan report or a wrong value here, not a short buffer on a card.  The launch is stubbed out: a "kernel" that fills the staged outputs
// batch by batch with bytes that name their place (host_check.h, staged_round); every caller's array is a heap block of exactly its size, so a copy past an end is
// an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/gather_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/gather_host.h"
#include "host_check.h"

using namespace lg;

static const double D[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

static bool refused(const void *accel, const double *origins, size_t n_poses, const double *dirs, size_t n_dirs, const double *weights, size_t n_weights, int lanes,
                    const lg_gather_out *out) {
    return throws([&] { (void)check_gather(accel, origins, n_poses, dirs, n_dirs, weights, n_weights, lanes, out); });
}
static bool misaligned(const void *origins, const void *frames, const void *dirs, const void *weights, const lg_gather_out &out) {
    return throws([&] { check_gather_alignment((const double *)origins, (const double *)frames, (const double *)dirs, (const double *)weights, out); });
}
// the tile count of a shape in a form, -1 where it passes 2^32 - 1
static long long tiles(size_t n_poses, size_t n_dirs, int form) {
    unsigned long long t = 0;
    return gather_tiles(n_poses, n_dirs, form, &t) ? (long long)t : -1;
}
// count * each * bytes, -1 where it does not fit size_t
static long long bytes(size_t count, size_t each, size_t b) {
    try {
        return (long long)(gather_bytes(count, each, b, "x") >> 4); // (>> 4: the top values stay positive in a long long)
    } catch (const std::exception &) {
        return -1;
    }
}

// one host-form call without a device: check, the batches as launch.cpp walks the poses, then stage, "launch" and place (staged_round)
static void run(size_t n_poses, size_t n_dirs, size_t n_weights, int lanes, unsigned planes, size_t park_bytes) {
    const size_t pairs = n_poses * n_dirs;
    lg_gather_out out{planes & 1u ? (double *)ASKED : nullptr, planes & 2u ? (double *)ASKED : nullptr};
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    const GatherShape shape = check_gather(&accel, D, n_poses, D, n_dirs, D, n_weights, lanes, &out);
    EXPECT(shape.pairs == pairs && shape.form == gather_lanes(n_poses, n_dirs, lanes) && (long long)shape.tiles == tiles(n_poses, n_dirs, shape.form));
    const size_t batch = out.radiance ? n_poses : gather_batch_poses(n_poses, n_dirs, shape.form, park_bytes);
    EXPECT(batch >= 1 && batch <= n_poses);
    EXPECT(out.radiance || batch == 1 || batch * n_dirs * 24 <= park_bytes);
    size_t covered = 0;
    for (size_t p0 = 0; p0 < n_poses; p0 += batch) { // a batch's tiles stay within the call's
        const size_t np = n_poses - p0 < batch ? n_poses - p0 : batch;
        EXPECT(tiles(np, n_dirs, shape.form) >= 0 && tiles(np, n_dirs, shape.form) <= (long long)shape.tiles);
        covered += np;
    }
    EXPECT(covered == n_poses);
    // the two outputs as query.cpp stages them: 3 doubles a ray, 3 doubles a pose and weight set
    const StagedRound r = staged_round([&](auto &&f) { f(out.radiance, pairs * 3, 8, "radiance"); f(out.sums, n_poses * n_weights * 3, 8, "sums"); });
    EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 24 * pairs : 0, planes & 2u ? 24 * n_poses * n_weights : 0}));
}

int main() {
    int accel = 0;
    alignas(16) double f[4] = {0.0};
    const lg_gather_out all{f, f}, none{nullptr, nullptr}, rad{f, nullptr}, sum{nullptr, f};
    const size_t M = 0xFFFFFFFFull, TOP = ~(size_t)0;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    // ---- the lane rule: 1 and 2 are taken as given, 0 is pose lanes iff n_poses >= n_dirs, anything else is -1
    const size_t counts[] = {0, 1, 7, 8, 63, 64, 65, 1024, M, M + 1, TOP - 1, TOP};
    for (size_t n : counts)
        for (size_t k : counts) {
            EXPECT(gather_lanes(n, k, 1) == 1 && gather_lanes(n, k, 2) == 2);
            EXPECT(gather_lanes(n, k, 0) == (n >= k ? 2 : 1));
            for (int bad : {-1, 3, 64, -2147483647 - 1, 2147483647}) EXPECT(gather_lanes(n, k, bad) == -1);
        }
    // ---- the tile counts: small shapes by hand
    EXPECT(tiles(1, 1, 1) == 1 && tiles(1, 64, 1) == 1 && tiles(1, 65, 1) == 2 && tiles(257, 1031, 1) == 257 * 17 && tiles(0, 5, 1) == 0 && tiles(5, 0, 1) == 0);
    EXPECT(tiles(1, 1, 2) == 1 && tiles(64, 8, 2) == 8 && tiles(65, 9, 2) == 18 && tiles(257, 1031, 2) == 5 * 1031 && tiles(0, 5, 2) == 0 && tiles(5, 0, 2) == 0);
    // ... at their limit and one above, in both forms.  Direction lanes: n_poses * ceil(n_dirs / 64)
    EXPECT(tiles(M, 1, 1) == (long long)M && tiles(M, 64, 1) == (long long)M && tiles(M + 1, 64, 1) == -1 && tiles(M, 65, 1) == -1);
    EXPECT(tiles(1, M, 1) == (1ll << 26) && tiles(63, M, 1) == 63ll << 26 && tiles(64, M, 1) == -1); // 64 * 2^26 = 2^32: one above the limit
    EXPECT(tiles(65535, 65537 * 64, 1) == 65535ll * 65537 && tiles(65536, 65536 * 64, 1) == -1 && tiles(65536, 65536 * 64 - 64, 1) == 65536ll * 65535); // 2^32 - 1 exactly
    EXPECT(tiles(TOP, 1, 1) == -1 && tiles(TOP, TOP, 1) == -1 && tiles(1, TOP, 1) == -1);
    // Pose lanes: ceil(n_poses / 64) * n_dirs
    EXPECT(tiles(64 * M, 1, 2) == (long long)M && tiles(64 * M + 1, 1, 2) == -1 && tiles(64 * M, 2, 2) == -1);
    EXPECT(tiles(64, M, 2) == (long long)M && tiles(1, M, 2) == (long long)M && tiles(65, M, 2) == -1 && tiles(64, M + 1, 2) == -1);
    EXPECT(tiles(65535 * 64, 65537, 2) == 65535ll * 65537 && tiles(65536 * 64, 65536, 2) == -1 && tiles(65536 * 64 - 63, 65535, 2) == 65536ll * 65535);
    EXPECT(tiles(TOP, 1, 2) == -1 && tiles(TOP, TOP, 2) == -1 && tiles(TOP - 63, 1, 2) == -1);
    // ---- the sizes: count * each * bytes at SIZE_MAX and one above
    EXPECT(bytes(0, 5, 24) == 0 && bytes(5, 0, 24) == 0 && bytes(3, 5, 24) == (360 >> 4));
    EXPECT(bytes(TOP / 24, 1, 24) == (long long)((TOP / 24 * 24) >> 4) && bytes(TOP / 24 + 1, 1, 24) == -1 && bytes(1, TOP / 24 + 1, 24) == -1);
    EXPECT(bytes(TOP / 8, 1, 8) == (long long)((TOP / 8 * 8) >> 4) && bytes(TOP / 8 + 1, 1, 8) == -1);
    EXPECT(bytes(TOP / 72, 9, 8) == (long long)((TOP / 72 * 72) >> 4) && bytes(TOP / 72 + 1, 9, 8) == -1);
    EXPECT(bytes(TOP, TOP, 1) == -1 && bytes(M + 1, M + 1, 1) == -1 && bytes(M + 1, M, 1) == (long long)(((M + 1) * M) >> 4) && bytes(TOP, 1, 1) == (long long)(TOP >> 4));
    // ---- check_gather: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, D, 5, D, 2, 0, &all));
    EXPECT(refused(nullptr, D, 3, D, 5, D, 2, 0, &all));
    EXPECT(refused(&accel, D, 3, D, 5, D, 2, 0, nullptr));
    EXPECT(refused(&accel, nullptr, 3, D, 5, D, 2, 0, &all));
    EXPECT(refused(&accel, D, 3, nullptr, 5, D, 2, 0, &all));
    EXPECT(refused(&accel, D, 3, D, 5, D, 2, 0, &none));
    EXPECT(refused(&accel, D, 3, D, 5, nullptr, 2, 0, &all) && refused(&accel, D, 3, D, 5, D, 0, 0, &all) && refused(&accel, D, 3, D, 5, nullptr, 2, 0, &sum));
    EXPECT(!refused(&accel, D, 3, D, 5, nullptr, 0, 0, &rad) && !refused(&accel, D, 3, D, 5, nullptr, TOP, 0, &rad)); // weights are ignored where sums is not asked for
    EXPECT(!refused(&accel, D, 3, D, 5, D, 2, 0, &sum) && !refused(&accel, D, 3, D, 5, D, 2, 0, &rad));
    for (int bad : {-1, 3, 1 << 20}) EXPECT(refused(&accel, D, 3, D, 5, D, 2, bad, &all));
    EXPECT(refused(&accel, D, 1, D, M + 1, D, 1, 1, &all) && refused(&accel, D, 1, D, M + 1, D, 1, 2, &all) && refused(&accel, D, 1, D, TOP, D, 1, 0, &all)); // n_dirs > 2^32 - 1
    EXPECT(!refused(&accel, D, 1, D, M, D, 1, 1, &all) && !refused(&accel, D, 1, D, M, D, 1, 2, &all));
    EXPECT(!refused(&accel, D, M, D, 64, D, 1, 1, &all) && refused(&accel, D, M + 1, D, 64, D, 1, 1, &all) && refused(&accel, D, M, D, 65, D, 1, 1, &all));
    EXPECT(!refused(&accel, D, 64 * M, D, 1, D, 1, 2, &all) && refused(&accel, D, 64 * M + 1, D, 1, D, 1, 2, &all) && refused(&accel, D, 64 * M, D, 2, D, 1, 2, &all));
    EXPECT(refused(&accel, D, M + 1, D, 63, D, 1, 1, &all) && !refused(&accel, D, M + 1, D, 63, D, 1, 2, &all) && !refused(&accel, D, M + 1, D, 63, D, 1, 0, &all)); // the form decides: auto takes pose lanes here
    EXPECT(refused(&accel, D, TOP, D, TOP, D, 1, 0, &all) && refused(&accel, D, TOP, D, 1, D, 1, 1, &all) && refused(&accel, D, TOP, D, 1, D, 1, 2, &all));
    // the four sizes, each as the one that does not fit (the tiles do): n_poses*n_dirs*24 cannot pass 2^32 tiles * 64 * 24; n_dirs*n_weights*8;
    // n_poses*n_weights*24; n_poses*72
    EXPECT(!refused(&accel, D, 1, D, M, D, TOP / 8 / M, 1, &sum) && refused(&accel, D, 1, D, M, D, TOP / 8 / M + 1, 1, &sum));
    EXPECT(!refused(&accel, D, 64 * M, D, 1, D, TOP / 24 / (64 * M), 2, &sum) && refused(&accel, D, 64 * M, D, 1, D, TOP / 24 / (64 * M) + 1, 2, &sum));
    EXPECT(!refused(&accel, D, 1, D, M, nullptr, TOP, 1, &rad)); // ... and neither is looked at without sums
    EXPECT(gather_bytes(64 * M, 9, 8, "frames") == 64 * M * 72 && gather_bytes(64 * M, 1, 24, "radiance") == 64 * M * 24);
    // what a checked call is
    {
        const GatherShape a = check_gather(&accel, D, 257, D, 1031, D, 9, 0, &all), b = check_gather(&accel, D, 1031, D, 257, D, 9, 0, &all),
                          c = check_gather(&accel, D, 64 * M, D, 1, D, 1, 2, &all);
        EXPECT(a.form == 1 && a.tiles == 257u * 17u && a.pairs == 257u * 1031u);
        EXPECT(b.form == 2 && b.tiles == 17u * 257u && b.pairs == 257u * 1031u);
        EXPECT(c.form == 2 && c.tiles == 0xFFFFFFFFu && c.pairs == 64 * M);
    }
    // ---- the alignment rule: every pointer 8; NULL is not misaligned; weights are looked at with sums alone
    const char *base = reinterpret_cast<const char *>(f);
    EXPECT(!misaligned(D, D, D, D, all) && !misaligned(D, nullptr, D, nullptr, rad) && !misaligned(D, D, D, D, none));
    for (int off : {1, 2, 4, 8, 12}) {
        const bool bad = off % 8 != 0;
        const lg_gather_out r{(double *)(base + off), f}, s{f, (double *)(base + off)};
        EXPECT(misaligned(base + off, D, D, D, all) == bad && misaligned(D, base + off, D, D, all) == bad && misaligned(D, D, base + off, D, all) == bad);
        EXPECT(misaligned(D, D, D, base + off, all) == bad && !misaligned(D, D, D, base + off, rad));
        EXPECT(misaligned(D, D, D, D, r) == bad && misaligned(D, D, D, D, s) == bad);
    }
    // ---- the cap and the batch: whole poses within the cap, never fewer than one, never more than the call has; pose lanes in blocks of 64
    EXPECT(gather_park_bytes(nullptr) == (size_t)1024 << 20 && gather_park_bytes("") == (size_t)1024 << 20 && gather_park_bytes("0") == (size_t)1024 << 20);
    EXPECT(gather_park_bytes("2") == (size_t)2 << 20 && gather_park_bytes("64") == (size_t)64 << 20 && gather_park_bytes("-3") == (size_t)1024 << 20);
    EXPECT(gather_park_bytes("2x") == (size_t)1024 << 20 && gather_park_bytes("abc") == (size_t)1024 << 20);
    EXPECT(gather_park_bytes("18446744073709551615") == (TOP >> 20) << 20 && gather_park_bytes("99999999999999999999999") == (TOP >> 20) << 20);
    const size_t MB = (size_t)1 << 20;
    EXPECT(gather_batch_poses(257, 1031, 1, 2 * MB) == 84 && gather_batch_poses(257, 1031, 2, 2 * MB) == 64 && gather_batch_poses(257, 1031, 2, MB) == 42);
    EXPECT(gather_batch_poses(257, 1031, 1, 1024 * MB) == 257 && gather_batch_poses(257, 1031, 2, 1024 * MB) == 257);
    EXPECT(gather_batch_poses(1000, 100, 2, 128 * 2400) == 128 && gather_batch_poses(1000, 100, 2, 129 * 2400) == 128 && gather_batch_poses(1000, 100, 1, 129 * 2400) == 129);
    // the cap below one pose: one pose a batch, in either form, up to the widest direction set
    EXPECT(gather_batch_poses(257, 1031, 1, 1031 * 24 - 1) == 1 && gather_batch_poses(257, 1031, 2, 1031 * 24 - 1) == 1 && gather_batch_poses(257, 1031, 1, 1031 * 24) == 1);
    EXPECT(gather_batch_poses(257, 1031, 1, 0) == 1 && gather_batch_poses(5, M, 1, MB) == 1 && gather_batch_poses(5, M, 2, MB) == 1 && gather_batch_poses(1, 1, 1, TOP) == 1);
    EXPECT(gather_batch_poses(64 * M, 1, 2, TOP) == 64 * M && gather_batch_poses(M, 64, 1, (TOP >> 20) << 20) == M);
    // ---- staging and placement: every subset of the outputs, shapes on both sides of the lane rule, caps from below one pose to the whole call
    const size_t shapes[][2] = {{1, 1}, {1, 65}, {65, 9}, {9, 65}, {17, 130}, {130, 17}, {64, 1}};
    for (const auto &s : shapes)
        for (unsigned planes = 1; planes < 4; ++planes)
            for (int lanes = 0; lanes < 3; ++lanes)
                for (size_t nw : {(size_t)1, (size_t)3, (size_t)9})
                    for (size_t cap : {(size_t)0, (size_t)23, s[1] * 24, s[1] * 24 * 3 + 5, s[1] * 24 * 64, s[1] * 24 * 70, 1024 * MB}) run(s[0], s[1], nw, lanes, planes, cap);
    if (failures) { std::fprintf(stderr, "gather_host_check: %d failures\n", failures); return 1; }
    std::printf("gather_host_check: ok\n");
    return 0;
}
