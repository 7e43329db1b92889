// tools/features_host_check.cpp -- the struct-handling host code of lg_capture_features* (lasgun_amd/csrc/features_host.h: argument
// validation, staging, compact-to-film placement) in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the
// CPU (tests/test_features_host_sanitized.py does).  The launch is stubbed out: a "kernel" that fills the compact planes with values that
// name their pixel.  Every film plane is a heap block of exactly width*height pixels, so a placement that reads or writes outside the
// rectangle's rows, or past a plane's end, is a sanitizer report; a wrong placement inside is caught by the values.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/features_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/features_host.h"
#include "host_check.h"

using namespace lg;

static bool refused(const void *accel, const lg_features *out, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const double *table) {
    return throws([&] { (void)check_features(accel, out, w, h, x0, y0, x1, y1, table); });
}

// the stubbed launch: pixel (x, y) of the rectangle, compact index i, gets values made of its film offset
static void stub_launch(const lg_features &st, uint32_t w, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    size_t i = 0;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t x = x0; x < x1; ++x, ++i) {
            const float v = (float)((size_t)y * w + x);
            if (st.depth) st.depth[i] = v;
            if (st.coverage) st.coverage[i] = v + 0.5f;
            for (size_t c = 0; c < 3; ++c) {
                if (st.normal) st.normal[3 * i + c] = v + 0.125f * (float)(c + 1);
                if (st.albedo) st.albedo[3 * i + c] = -(v + 0.125f * (float)(c + 1));
            }
            for (size_t c = 0; c < 4; ++c)
                if (st.id) st.id[4 * i + c] = (uint32_t)((size_t)y * w + x) * 4u + (uint32_t)c;
        }
}

// one host-form call without a device: check, stage, "launch", place; then every pixel of every plane is looked at
static void run(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, unsigned planes) {
    const size_t n = (size_t)w * h;
    const float F = -7.0f;
    const uint32_t U = 0xA5A5A5A5u;
    // exactly sized heap blocks (not vectors: no capacity slack for the sanitizer to forgive)
    std::unique_ptr<float[]> depth(planes & 1u ? new float[n] : nullptr), normal(planes & 2u ? new float[3 * n] : nullptr),
        albedo(planes & 4u ? new float[3 * n] : nullptr), coverage(planes & 8u ? new float[n] : nullptr);
    std::unique_ptr<uint32_t[]> id(planes & 16u ? new uint32_t[4 * n] : nullptr);
    for (size_t i = 0; i < n; ++i) {
        if (depth) depth[i] = F;
        if (coverage) coverage[i] = F;
        for (size_t c = 0; c < 3; ++c) { if (normal) normal[3 * i + c] = F; if (albedo) albedo[3 * i + c] = F; }
        for (size_t c = 0; c < 4; ++c) if (id) id[4 * i + c] = U;
    }
    const lg_features out{depth.get(), normal.get(), albedo.get(), coverage.get(), id.get()};
    const double table[3] = {0.25, 0.5, 0.75};
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    const size_t pixels = check_features(&accel, &out, w, h, x0, y0, x1, y1, table);
    EXPECT(pixels == (size_t)(x1 - x0) * (y1 - y0));
    if (pixels == 0) return;
    HostStaging staging;
    lg_features st = out; // ... where a plane asked for becomes its compact rows, held as query.cpp holds them: a buffer of exactly their size
    std::vector<const void *> compact;
    feature_planes(st, [&](auto *&p, size_t per_pixel, size_t, const char *) {
        if (p) p = staging.hold<std::remove_reference_t<decltype(*p)>>(pixels * per_pixel);
        compact.push_back(p);
    });
    EXPECT(compact.size() == 5);
    stub_launch(st, w, x0, y0, x1, y1);
    place_features(out, compact.data(), w, x0, y0, x1, y1);
    staging.place(); // (nothing was staged: the form places what it holds)
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            const bool in = x >= x0 && x < x1 && y >= y0 && y < y1;
            const float v = (float)i;
            if (depth) EXPECT(depth[i] == (in ? v : F));
            if (coverage) EXPECT(coverage[i] == (in ? v + 0.5f : F));
            for (size_t c = 0; c < 3; ++c) {
                if (normal) EXPECT(normal[3 * i + c] == (in ? v + 0.125f * (float)(c + 1) : F));
                if (albedo) EXPECT(albedo[3 * i + c] == (in ? -(v + 0.125f * (float)(c + 1)) : F));
            }
            for (size_t c = 0; c < 4; ++c)
                if (id) EXPECT(id[4 * i + c] == (in ? (uint32_t)i * 4u + (uint32_t)c : U));
        }
}

int main() {
    int accel = 0;
    float f = 0.0f;
    uint32_t u = 0u;
    const double table[3] = {0.0, 0.0, 0.0};
    const lg_features all{&f, &f, &f, &f, &u}, none{nullptr, nullptr, nullptr, nullptr, nullptr}, no_albedo{&f, &f, nullptr, &f, &u};
    // ---- argument validation: every error of the contract
    EXPECT(refused(nullptr, &all, 8, 8, 0, 0, 8, 8, table));
    EXPECT(refused(&accel, nullptr, 8, 8, 0, 0, 8, 8, table));
    EXPECT(refused(&accel, &none, 8, 8, 0, 0, 8, 8, table));
    EXPECT(refused(&accel, &all, 8, 8, 0, 0, 8, 8, nullptr));        // albedo without material_rgb
    EXPECT(!refused(&accel, &no_albedo, 8, 8, 0, 0, 8, 8, nullptr)); // ... which is ignored otherwise
    EXPECT(refused(&accel, &all, 8, 8, 0, 0, 9, 8, table));
    EXPECT(refused(&accel, &all, 8, 8, 0, 0, 8, 9, table));
    EXPECT(refused(&accel, &all, 8, 8, 5, 0, 4, 8, table));
    EXPECT(refused(&accel, &all, 8, 8, 0, 5, 8, 4, table));
    EXPECT(refused(&accel, &all, 0, 0, 0, 0, 1, 1, table));
    EXPECT(refused(&accel, &all, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, table)); // coordinates beyond 2^32 - 8
    EXPECT(refused(&accel, &all, 0xFFFFFFF8u, 0xFFFFFFF8u, 0, 0, 0xFFFFFFF8u, 0xFFFFFFF8u, table)); // 2^58 tiles
    EXPECT(!refused(&accel, &all, 0xFFFFFFF8u, 1, 0xFFFFFFF0u, 0, 0xFFFFFFF8u, 1, table));          // the last admissible column
    EXPECT(refused(&accel, &all, 8u << 16, 8u << 16, 0, 0, 8u << 16, 8u << 16, table));             // exactly 2^32 tiles
    EXPECT(!refused(&accel, &all, 8u << 16, 8u << 16, 0, 0, 8u << 16, (8u << 16) - 8u, table));      // 2^32 - 65536
    // a single NULL plane in every position is accepted, a single non-NULL plane in every position too
    for (int k = 0; k < 5; ++k) {
        lg_features one = none, but = all;
        float **fp[4] = {&one.depth, &one.normal, &one.albedo, &one.coverage};
        float **bp[4] = {&but.depth, &but.normal, &but.albedo, &but.coverage};
        if (k < 4) { *fp[k] = &f; *bp[k] = nullptr; } else { one.id = &u; but.id = nullptr; }
        EXPECT(!refused(&accel, &one, 8, 8, 0, 0, 8, 8, table));
        EXPECT(!refused(&accel, &but, 8, 8, 0, 0, 8, 8, table));
    }
    // empty rectangles: 0 pixels, not an error
    EXPECT(check_features(&accel, &all, 8, 8, 3, 3, 3, 7, table) == 0 && check_features(&accel, &all, 8, 8, 3, 3, 7, 3, table) == 0);
    EXPECT(check_features(&accel, &all, 0, 0, 0, 0, 0, 0, table) == 0 && check_features(&accel, &all, 8, 8, 8, 8, 8, 8, table) == 0);
    // ---- placement: every subset of the planes (a NULL plane in every position and combination) for every kind of rectangle
    const uint32_t W = 21, H = 13;
    const uint32_t rects[][4] = {{0, 0, W, H}, {3, 5, 20, 12}, {8, 8, 16, 13}, {0, 6, W, 7}, {10, 0, 11, H}, {20, 12, 21, 13}, {0, 0, 1, 1}, {4, 4, 4, 9}};
    for (const auto &r : rects)
        for (unsigned planes = 1; planes < 32; ++planes) run(W, H, r[0], r[1], r[2], r[3], planes);
    run(1, 1, 0, 0, 1, 1, 31);
    run(1, 64, 0, 7, 1, 60, 31);
    run(64, 1, 7, 0, 60, 1, 31);
    if (failures) { std::fprintf(stderr, "features_host_check: %d failures\n", failures); return 1; }
    std::printf("features_host_check: ok\n");
    return 0;
}
