// lasgun_amd/csrc/features_host.h -- the part of lg_capture_features* (query.cpp) that handles the caller's lg_features struct and touches no
// device: the one table of its planes (feature_planes), what both forms refuse before anything is allocated or enqueued, the host form's
// staging of the compact planes, and their placement at the film's offsets.  Kept free of HIP so that tools/features_host_check.cpp can run exactly this text under
// AddressSanitizer / UBSan on the CPU with the launch stubbed out.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lasgun_hip.h"

namespace lg {

static_assert(sizeof(lg_features) == 40 && offsetof(lg_features, depth) == 0 && offsetof(lg_features, normal) == 8 && offsetof(lg_features, albedo) == 16 &&
                  offsetof(lg_features, coverage) == 24 && offsetof(lg_features, id) == 32,
              "lg_features: five pointers, 40 bytes");

// The host form's compact planes (row-major pixels of the rectangle) on their way back: only the planes asked for have any size
struct FeatureStaging {
    std::vector<float> depth, normal, albedo, coverage;
    std::vector<uint32_t> id;
    FeatureStaging(const lg_features &out, size_t pixels);
};
// The five planes of lg_features (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, the
// plane's staging, its elements a pixel, its alignment in bytes, its name) in the struct's order.  The NULL rule, the staging's sizes,
// the host form's device buffers and copies, the device form's buffer checks and the placement all go through here.
template <class Out, class F> inline void feature_planes(Out &out, F &&f) {
    f(out.depth, &FeatureStaging::depth, 1, 4, "depth");
    f(out.normal, &FeatureStaging::normal, 3, 4, "normal");
    f(out.albedo, &FeatureStaging::albedo, 3, 4, "albedo");
    f(out.coverage, &FeatureStaging::coverage, 1, 4, "coverage");
    f(out.id, &FeatureStaging::id, 4, 16, "id");
}
inline FeatureStaging::FeatureStaging(const lg_features &out, size_t pixels) {
    feature_planes(out, [&](auto *p, auto plane, size_t per_pixel, size_t, const char *) { if (p) (this->*plane).resize(pixels * per_pixel); });
}

// The pixels of the rectangle, 0 for an empty one (a successful no-op); everything the contract calls an error is thrown here.  The
// rectangle's rule is lg_capture_rect's.
inline size_t check_features(const void *accel, const lg_features *out, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                             const double *material_rgb) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    bool any = false;
    feature_planes(*out, [&](auto *p, auto, size_t, size_t, const char *) { any = any || p; });
    if (!any) throw std::runtime_error("every plane of out is NULL: at least one output");
    if (out->albedo && !material_rgb) throw std::runtime_error("albedo is requested and material_rgb is NULL");
    if (x1 > w || y1 > h || x0 > x1 || y0 > y1) throw std::runtime_error("bad rectangle");
    // (a tile's pixel coordinates are 32-bit: the last tile of a row or column may reach 7 pixels beyond x1 / y1)
    if (x1 > 0xFFFFFFF8u || y1 > 0xFFFFFFF8u) throw std::runtime_error("rectangle beyond 2^32 - 8: the coordinates of a tile's pixels are 32-bit");
    const unsigned long long tiles = (unsigned long long)((x1 - x0 + 7u) / 8u) * ((y1 - y0 + 7u) / 8u);
    if (tiles > 0xFFFFFFFFull) throw std::runtime_error("too many pixels in one feature capture: 8 x 8 tiles are counted in 32 bits");
    return (size_t)(x1 - x0) * (y1 - y0);
}

// compact rows -> the film's rows: `n` elements a pixel; nothing outside the rectangle is read or written
template <class T>
inline void place_plane(T *film, const std::vector<T> &compact, size_t n, uint32_t w, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    if (!film) return;
    const size_t rw = x1 - x0;
    for (uint32_t y = y0; y < y1; ++y)
        std::memcpy(film + ((size_t)y * w + x0) * n, compact.data() + (size_t)(y - y0) * rw * n, rw * n * sizeof(T));
}
inline void place_features(const lg_features &out, const FeatureStaging &st, uint32_t w, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    feature_planes(out, [&](auto *p, auto plane, size_t per_pixel, size_t, const char *) { place_plane(p, st.*plane, per_pixel, w, x0, y0, x1, y1); });
}

} // namespace lg
