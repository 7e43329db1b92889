// tools/view_features_host_check.cpp -- the device-free host code of lg_capture_view_features* (lasgun_amd/csrc/view_features_host.h: the
// plane table, every NULL rule, the film's limits, the pixel-tile count with its 32-bit limit, each plane's byte size, the views' own rules
// and the uniform-samples rule, the alignment rule, the host form's staging through planes_host.h's HostStaging) in a stand-alone program, meant to be built with -fsanitize=address,undefined and run
// on the CPU (tests/test_view_features_host_sanitized.py does).  The counts go up to 2^64 - 1: an overflow in forming a tile count or a
// size is a UBSan report or a wrong value here, not a short buffer on a card.  Every table is a heap block of exactly its size, so a read
// past a table's end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/view_features_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/view_features_host.h"
#include "host_check.h"

using namespace lg;

static lg_view view(uint32_t root, uint32_t reserved = 0) {
    lg_view v;
    std::memset(&v, 0, sizeof v);
    v.view[2] = 1.0; v.up[1] = 1.0; v.aux[0] = 1.0; v.image_plane_height = 0.5;
    v.samples_root = root; v.reserved = reserved;
    return v;
}
alignas(16) static unsigned char mem[64] = {0};
enum { DEPTH = 1, NORMAL = 2, ALBEDO = 4, COVERAGE = 8, ID = 16, POINT = 32, ALL = 63 };
// the planes of `mask`, each at mem + shift
static lg_view_features planes(int mask, size_t shift = 0) {
    lg_view_features f;
    std::memset(&f, 0, sizeof f);
    if (mask & DEPTH) f.depth = reinterpret_cast<float *>(mem + shift);
    if (mask & NORMAL) f.normal = reinterpret_cast<float *>(mem + shift);
    if (mask & ALBEDO) f.albedo = reinterpret_cast<float *>(mem + shift);
    if (mask & COVERAGE) f.coverage = reinterpret_cast<float *>(mem + shift);
    if (mask & ID) f.id = reinterpret_cast<uint32_t *>(mem + shift);
    if (mask & POINT) f.point = reinterpret_cast<float *>(mem + shift);
    return f;
}
static const double *const TABLE = reinterpret_cast<const double *>(mem);
static std::string refusal(const void *accel, const lg_view *views, size_t n, uint32_t w, uint32_t h, const lg_view_features *out, const double *table = TABLE) {
    return thrown([&] { (void)check_view_features(accel, views, n, w, h, out, table); });
}
static bool has(const std::string &s, const char *word) { return s.find(word) != std::string::npos; }
static std::string misaligned(const lg_view_features &out, const double *table = TABLE) {
    return thrown([&] { check_view_features_alignment(out, table); });
}

int main() {
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    const size_t M = 0xFFFFFFFFull, TOP = ~(size_t)0;
    const uint32_t U = 0xFFFFFFFFu, EDGE = 0xFFFFFFF8u; // 2^32 - 8
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    std::unique_ptr<lg_view[]> two(new lg_view[2]);
    two[0] = view(1); two[1] = view(1);
    const lg_view_features all = planes(ALL), depth = planes(DEPTH), none = planes(0);
    // ---- the plane table: six planes in the struct's order, their elements a pixel and their alignment
    {
        std::string names;
        size_t per = 0, n = 0;
        view_feature_planes(all, [&](auto *p, size_t per_pixel, size_t align, const char *what) {
            names += what; names += ' '; per += per_pixel * sizeof *p; ++n;
            EXPECT(align == (std::string(what) == "id" ? 16u : 4u) && p != nullptr);
        });
        EXPECT(names == "depth normal albedo coverage id point " && n == 6 && per == 60); // at most 60 bytes a pixel
    }
    // ---- every NULL rule
    EXPECT(refusal(&accel, two.get(), 2, 16, 16, &all).empty());
    EXPECT(refusal(nullptr, two.get(), 2, 16, 16, &all) == "accel is NULL" && refusal(&accel, nullptr, 2, 16, 16, &all) == "views is NULL");
    EXPECT(refusal(&accel, two.get(), 2, 16, 16, nullptr) == "out is NULL" && has(refusal(&accel, two.get(), 2, 16, 16, &none), "every plane of out is NULL"));
    for (int bit = 1; bit <= POINT; bit <<= 1) { // each plane alone is a call; albedo alone needs its table
        const lg_view_features one = planes(bit);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, &one).empty());
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, &one, nullptr).empty() == (bit != ALBEDO));
    }
    EXPECT(has(refusal(&accel, two.get(), 2, 16, 16, &all, nullptr), "material_rgb is NULL"));
    // ---- the film: 0, and the 2^32 - 8 rule (one view of one row: a single tile row, no other limit in the way)
    EXPECT(has(refusal(&accel, two.get(), 2, 0, 16, &all), "empty film") && has(refusal(&accel, two.get(), 2, 16, 0, &all), "empty film"));
    EXPECT(refusal(&accel, two.get(), 1, EDGE, 1, &depth).empty() && refusal(&accel, two.get(), 1, 1, EDGE, &depth).empty());
    EXPECT(has(refusal(&accel, two.get(), 1, EDGE + 1u, 1, &depth), "2^32 - 8") && has(refusal(&accel, two.get(), 1, 1, EDGE + 1u, &depth), "2^32 - 8"));
    EXPECT(has(refusal(&accel, two.get(), 1, U, 1, &depth), "2^32 - 8") && has(refusal(&accel, two.get(), 1, 1, U, &depth), "2^32 - 8"));
    // ---- the tile count at 2^32 - 1 and one above: by the views, by the film.  The samples run in a loop and do not count.  A count no table
    // can have is refused before the table is walked: the block holds two records.
    EXPECT(refusal(&accel, two.get(), 1, 65535 * 8, 65537 * 8, &depth).empty() && has(refusal(&accel, two.get(), 1, 65536 * 8, 65536 * 8, &depth), "32 bits"));
    EXPECT(has(refusal(&accel, two.get(), M + 1, 8, 8, &depth), "32 bits") && has(refusal(&accel, two.get(), M + 1, 1, 1, &depth), "32 bits"));
    EXPECT(has(refusal(&accel, two.get(), M, 9, 8, &depth), "32 bits") && has(refusal(&accel, two.get(), TOP, 1, 1, &all), "32 bits"));
    EXPECT(has(refusal(&accel, two.get(), 65536, 65536 * 8, 8, &depth), "32 bits") && has(refusal(&accel, two.get(), 4, 1u << 18, 1u << 18, &all), "32 bits"));
    {
        unsigned long long per = 0, tiles = 0;
        EXPECT(view_tiles(M, 8, 8, 1, &per, &tiles) && tiles == M && !view_tiles(M + 1, 8, 8, 1, &per, &tiles));
        EXPECT(view_tiles(65535, 65537 * 8, 8, 1, &per, &tiles) && tiles == 65535ull * 65537 && view_tiles(130, 9, 9, 1, &per, &tiles) && per == 4 && tiles == 520);
        two[0] = view(256); two[1] = view(256); // S = 65536 a pixel: the same tiles
        const ViewShape s = check_view_features(&accel, two.get(), 2, 45, 27, &all, TABLE);
        EXPECT(s.samples_root == 256 && s.tiles_x == 6 && s.tiles_per_view == 24 && s.pixel_tiles == 48 && s.pixels == 2 * 45 * 27);
        two[0] = view(1); two[1] = view(1);
        // the host form's staging (query.cpp: the table's elements a pixel times the call's pixels), for every subset of the planes
        for (int mask = 1; mask <= ALL; ++mask) {
            lg_view_features out = planes(mask);
            const StagedRound r = staged_round([&](auto &&f) {
                view_feature_planes(out, [&](auto *&p, size_t per_pixel, size_t align, const char *what) { f(p, s.pixels * per_pixel, align, what); });
            });
            EXPECT(r.plane_bytes == (std::vector<size_t>{mask & DEPTH ? 4 * s.pixels : 0, mask & NORMAL ? 12 * s.pixels : 0, mask & ALBEDO ? 12 * s.pixels : 0,
                                                         mask & COVERAGE ? 4 * s.pixels : 0, mask & ID ? 16 * s.pixels : 0, mask & POINT ? 12 * s.pixels : 0}));
        }
    }
    // ---- each plane's byte size at SIZE_MAX and one above: n_views * w * h * 4, 12 and 16 (the tile count is out of the way at w = h = 1
    // only below 2^32 views, so the sizes are driven through view_bytes, the function check_view_features calls per plane)
    {
        auto bytes = [](size_t n, uint32_t w, uint32_t h, size_t b) -> long long {
            try { return (long long)(view_bytes(n, w, h, b, "x") >> 4); } catch (const std::exception &) { return -1; }
        };
        for (size_t b : {(size_t)4, (size_t)12, (size_t)16})
            EXPECT(bytes(TOP / b, 1, 1, b) == (long long)((TOP / b * b) >> 4) && bytes(TOP / b + 1, 1, 1, b) == -1);
        EXPECT(bytes(M, 65536, 65536, 1) == (long long)((M << 32) >> 4) && bytes(M, 65536, 65536, 4) == -1 && bytes(1, U, U, 16) == -1 && bytes(1, U, U, 4) == -1);
        // ... and through the check itself: 2^29 x 2^29 tiles pass 2^32 - 1 long before a size passes SIZE_MAX, so the tile rule answers first;
        // the largest film the tile rule admits has every plane's size far inside size_t
        EXPECT(refusal(&accel, two.get(), 1, 65535 * 8, 65537 * 8, &all).empty());
    }
    // ---- the views' own rules and the uniform-samples rule
    for (uint32_t bad : {0u, 257u, U}) {
        two[1] = view(bad);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, &all).find("view 1: samples_root") == 0);
        two[1] = view(1); two[0] = view(bad);
        EXPECT(refusal(&accel, two.get(), 2, 16, 16, &all).find("view 0: samples_root") == 0);
        two[0] = view(1);
    }
    two[1] = view(1, 1);
    EXPECT(refusal(&accel, two.get(), 2, 16, 16, &all) == "view 1: reserved must be 0");
    two[1] = view(3);
    EXPECT(has(refusal(&accel, two.get(), 2, 16, 16, &all), "differs from view 0's"));
    two[0] = view(3);
    EXPECT(refusal(&accel, two.get(), 2, 16, 16, &all).empty());
    // ---- the device form's alignment rule: id 16, the float planes 4, material_rgb 8 with albedo alone; a NULL plane is not looked at
    EXPECT(misaligned(all).empty() && misaligned(none, nullptr).empty() && misaligned(planes(ALL, 16)).empty() && misaligned(planes(ALL & ~ID, 4)).empty());
    for (size_t k = 1; k < 16; ++k) EXPECT(has(misaligned(planes(ID, k)), "id is not 16-byte aligned"));
    for (size_t k = 1; k < 4; ++k)
        for (int bit : {DEPTH, NORMAL, ALBEDO, COVERAGE, POINT}) EXPECT(has(misaligned(planes(bit, k)), "is not 4-byte aligned"));
    for (size_t k = 1; k < 8; ++k) {
        EXPECT(has(misaligned(planes(ALBEDO), reinterpret_cast<const double *>(mem + k)), "material_rgb is not 8-byte aligned"));
        EXPECT(misaligned(planes(ALL & ~ALBEDO), reinterpret_cast<const double *>(mem + k)).empty()); // ignored without albedo
    }
    if (failures) { std::fprintf(stderr, "view_features_host_check: %d failures\n", failures); return 1; }
    std::printf("view_features_host_check: ok\n");
    return 0;
}
