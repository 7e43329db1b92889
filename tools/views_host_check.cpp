// tools/views_host_check.cpp -- the device-free host code of lg_capture_views* (lasgun_amd/csrc/views_host.h: the work-tile count with its
// 32-bit limit, both byte sizes, what a valid view is and the uniform-samples rule, the NULL and alignment rules, lg_view -> DView) in a
// stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_views_host_sanitized.py does).  The
// counts go up to 2^64 - 1: an overflow in forming a tile count or a size is a UBSan report or a wrong value here, not a short buffer on a
// card.  Every table is a heap block of exactly its size, so a read past a table's end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/views_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/views_host.h"
#include "host_check.h"

using namespace lg;

// the work tiles of a call, -1 where they pass 2^32 - 1
static long long tiles(size_t n_views, uint32_t w, uint32_t h, unsigned long long S) {
    unsigned long long per = 0, work = 0;
    return view_tiles(n_views, w, h, S, &per, &work) ? (long long)work : -1;
}
// n_views * w * h * bytes, -1 where it does not fit size_t
static long long bytes(size_t n_views, uint32_t w, uint32_t h, size_t b) {
    try {
        return (long long)(view_bytes(n_views, w, h, b, "x") >> 4); // (>> 4: the top values stay positive in a long long)
    } catch (const std::exception &) {
        return -1;
    }
}
static lg_view view(uint32_t root, uint32_t reserved = 0) {
    lg_view v;
    std::memset(&v, 0, sizeof v);
    v.view[2] = 1.0; v.up[1] = 1.0; v.aux[0] = 1.0; v.image_plane_height = 0.5;
    v.samples_root = root; v.reserved = reserved;
    return v;
}
static std::string refusal(const void *accel, const lg_view *views, size_t n, uint32_t w, uint32_t h, const void *rgba, const void *rgb) {
    return thrown([&] { (void)check_views(accel, views, n, w, h, rgba, rgb); });
}
static bool misaligned(const void *rgba, const void *rgb) {
    return throws([&] { check_views_alignment(rgba, rgb); });
}

int main() {
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    alignas(16) unsigned char out[32] = {0};
    const size_t M = 0xFFFFFFFFull, TOP = ~(size_t)0;
    const uint32_t U = 0xFFFFFFFFu;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    // ---- the tile count: small shapes by hand
    EXPECT(tiles(1, 1, 1, 1) == 1 && tiles(2, 8, 8, 1) == 2 && tiles(2, 9, 8, 1) == 4 && tiles(3, 13, 11, 4) == 3 * 4 * 4 && tiles(130, 9, 9, 1) == 520);
    EXPECT(tiles(0, 8, 8, 1) == 0 && tiles(5, 0, 8, 1) == 0 && tiles(5, 8, 0, 1) == 0 && tiles(3, 128, 128, 9) == 3 * 256 * 9);
    // ... at 2^32 - 1 and one above: by the views, by the film, by the samples
    EXPECT(tiles(M, 8, 8, 1) == (long long)M && tiles(M + 1, 8, 8, 1) == -1 && tiles(M, 9, 8, 1) == -1 && tiles(M, 8, 8, 2) == -1);
    EXPECT(tiles(65535, 65537 * 8, 8, 1) == 65535ll * 65537 && tiles(65536, 65536 * 8, 8, 1) == -1 && tiles(65536, 65535 * 8, 1, 1) == 65536ll * 65535);
    EXPECT(tiles(3, 5 * 8, 17 * 8, 16843009) == (long long)M && tiles(3, 5 * 8, 17 * 8, 16843010) == -1); // 255 * 16843009 = 2^32 - 1
    EXPECT(tiles(1, 65535 * 8, 65537 * 8, 1) == (long long)M && tiles(1, 65536 * 8, 65536 * 8, 1) == -1 && tiles(4, 1u << 18, 1u << 18, 1) == -1);
    EXPECT(tiles(1, U, U, 1) == -1 && tiles(TOP, 1, 1, 1) == -1 && tiles(TOP, U, U, 65536) == -1 && tiles(1, 8, 8, M) == (long long)M && tiles(1, 8, 8, M + 1) == -1);
    // ---- the sizes: n_views * w * h * bytes at SIZE_MAX and one above
    EXPECT(bytes(0, 5, 5, 4) == 0 && bytes(5, 0, 5, 24) == 0 && bytes(3, 5, 2, 24) == (720 >> 4));
    EXPECT(bytes(TOP / 4, 1, 1, 4) == (long long)((TOP / 4 * 4) >> 4) && bytes(TOP / 4 + 1, 1, 1, 4) == -1);
    EXPECT(bytes(TOP / 24, 1, 1, 24) == (long long)((TOP / 24 * 24) >> 4) && bytes(TOP / 24 + 1, 1, 1, 24) == -1);
    EXPECT(bytes(TOP / 128, 1, 1, 128) == (long long)((TOP / 128 * 128) >> 4) && bytes(TOP / 128 + 1, 1, 1, 128) == -1);
    EXPECT(bytes(M + 1, U, U, 1) == -1 && bytes(M + 1, 65536, 65536, 1) == -1 && bytes(M, 65536, 65536, 1) == (long long)((M << 32) >> 4));
    EXPECT(bytes(M, 65536, 65536, 4) == -1 && bytes(TOP, U, U, 24) == -1 && bytes(1, U, U, 24) == -1 && bytes(1, U, U, 1) == (long long)(((size_t)U * U) >> 4));
    // ---- check_views: every error of the contract that needs no device
    {
        std::unique_ptr<lg_view[]> two(new lg_view[2]);
        two[0] = view(2); two[1] = view(2);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, out).empty());
        EXPECT(refusal(nullptr, two.get(), 2, 16, 16, out, out) == "accel is NULL" && refusal(&accel, nullptr, 2, 16, 16, out, out) == "views is NULL");
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, nullptr, nullptr).find("both NULL") != std::string::npos);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, nullptr).empty() && refusal(&accel, two.get(), 2, 16, 16, nullptr, out).empty());
        EXPECT(!refusal(&accel, two.get(), 2, 0, 16, out, out).empty() && !refusal(&accel, two.get(), 2, 16, 0, out, out).empty());
        for (uint32_t bad : {0u, 257u, U}) {
            two[1] = view(bad);
            EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, out).find("view 1: samples_root") == 0);
            two[1] = view(2); two[0] = view(bad);
            EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, out).find("view 0: samples_root") == 0);
            two[0] = view(2);
        }
        two[1] = view(2, 1);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, out) == "view 1: reserved must be 0");
        two[1] = view(3);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, out).find("differs from view 0's") != std::string::npos);
        two[0] = view(256); two[1] = view(256);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, out, out).empty() && refusal(&accel, two.get(), 2, 8 * 256, 8 * 128, out, out).find("32 bits") != std::string::npos);
        // a count no table can have is refused before the table is walked: the block holds two records
        two[0] = view(1); two[1] = view(1);
        EXPECT(refusal(&accel, two.get(), M + 1, 8, 8, out, out).find("32 bits") != std::string::npos && refusal(&accel, two.get(), TOP, 1, 1, out, out).find("32 bits") != std::string::npos);
    }
    // ... and what a checked call is
    {
        const size_t K = 130;
        std::unique_ptr<lg_view[]> many(new lg_view[K]);
        for (size_t v = 0; v < K; ++v) many[v] = view(3);
        const ViewShape s = check_views(&accel, many.get(), K, 45, 27, out, nullptr);
        EXPECT(s.samples_root == 3 && s.tiles_x == 6 && s.tiles_per_view == 24 && s.pixel_tiles == 130 * 24 && s.pixels == K * 45 * 27);
        EXPECT(tiles(K, 45, 27, 9) == 130 * 24 * 9);
        // the host form's staging (query.cpp: 4 bytes and 3 doubles a pixel), for every subset of the two films
        for (unsigned films = 1; films < 4; ++films) {
            uint8_t *rgba = films & 1u ? (uint8_t *)ASKED : nullptr;
            double *rgb = films & 2u ? (double *)ASKED : nullptr;
            const StagedRound r = staged_round([&](auto &&f) { f(rgba, s.pixels * 4, 4, "rgba"); f(rgb, s.pixels * 3, 8, "rgb"); });
            EXPECT(r.plane_bytes == (std::vector<size_t>{films & 1u ? 4 * s.pixels : 0, films & 2u ? 24 * s.pixels : 0}));
        }
        // lg_view -> DView: the fields as given, ss_distance = 1 / samples_root
        many[7].origin[1] = -0.0; many[7].aux[2] = 1e300; many[7].pixel_separation = 1.0;
        const std::vector<DView> d = to_dviews(many.get(), K);
        EXPECT(d.size() == K && d[7].origin.y == 0.0 && std::signbit(d[7].origin.y) && d[7].aux.z == 1e300 && d[7].pixel_separation == 1.0 && d[7].image_plane_height == 0.5);
        EXPECT(d[0].ss_root == 3 && d[0].ss_distance == 1.0 / 3.0 && d[0].pad == 0 && d[K - 1].view.z == 1.0 && d[K - 1].up.y == 1.0 && d[K - 1].aux.x == 1.0);
        EXPECT(to_dview(view(1)).ss_distance == 1.0 && to_dview(view(256)).ss_distance == 1.0 / 256.0);
    }
    // ---- the device form's alignment rule: rgba 4, rgb 8; a NULL output is not looked at
    EXPECT(!misaligned(out, out) && !misaligned(nullptr, out) && !misaligned(out, nullptr) && !misaligned(out + 4, out + 8) && !misaligned(out + 12, out + 16));
    for (int k = 1; k < 4; ++k) EXPECT(misaligned(out + k, out) && misaligned(out + k, nullptr));
    for (int k = 1; k < 8; ++k) EXPECT(misaligned(out, out + k) && misaligned(nullptr, out + k));
    if (failures) { std::fprintf(stderr, "views_host_check: %d failures\n", failures); return 1; }
    std::printf("views_host_check: ok\n");
    return 0;
}
