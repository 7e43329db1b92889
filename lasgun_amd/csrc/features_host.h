// lasgun_amd/csrc/features_host.h -- the part of lg_capture_features* (query.cpp) that handles the caller's lg_features struct and touches no
// device: the one table of its planes (feature_planes), what both forms refuse before anything is allocated or enqueued, and the placement
// of the host form's compact planes (held in planes_host.h's HostStaging) at the film's offsets.  Kept free of HIP so that
// tools/features_host_check.cpp can run exactly this text under AddressSanitizer / UBSan on the CPU with the launch stubbed out.
#pragma once
#include <type_traits>

#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_features) == 40 && offsetof(lg_features, depth) == 0 && offsetof(lg_features, normal) == 8 && offsetof(lg_features, albedo) == 16 &&
                  offsetof(lg_features, coverage) == 24 && offsetof(lg_features, id) == 32,
              "lg_features: five pointers, 40 bytes");

// The five planes of lg_features (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements a pixel, its alignment in bytes, its name) in the struct's order -- elements a pixel, since the two forms size a plane
// differently: the rectangle for the host form's compact planes, the film for the device form.  The NULL rule, the host form's compact
// planes, device buffers and copies, the device form's buffer checks and the placement all go through here.
template <class Out, class F> inline void feature_planes(Out &out, F &&f) {
    f(out.depth, 1, 4, "depth");
    f(out.normal, 3, 4, "normal");
    f(out.albedo, 3, 4, "albedo");
    f(out.coverage, 1, 4, "coverage");
    f(out.id, 4, 16, "id");
}

// The pixels of the rectangle, 0 for an empty one (a successful no-op); everything the contract calls an error is thrown here.  The
// rectangle's rule is lg_capture_rect's.
inline size_t check_features(const void *accel, const lg_features *out, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                             const double *material_rgb) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { feature_planes(*out, f); });
    if (out->albedo && !material_rgb) throw std::runtime_error("albedo is requested and material_rgb is NULL");
    if (x1 > w || y1 > h || x0 > x1 || y0 > y1) throw std::runtime_error("bad rectangle");
    // (a tile's pixel coordinates are 32-bit: the last tile of a row or column may reach 7 pixels beyond x1 / y1)
    if (x1 > 0xFFFFFFF8u || y1 > 0xFFFFFFF8u) throw std::runtime_error("rectangle beyond 2^32 - 8: the coordinates of a tile's pixels are 32-bit");
    const unsigned long long tiles = (unsigned long long)((x1 - x0 + 7u) / 8u) * ((y1 - y0 + 7u) / 8u);
    if (tiles > 0xFFFFFFFFull) throw std::runtime_error("too many pixels in one feature capture: 8 x 8 tiles are counted in 32 bits");
    return (size_t)(x1 - x0) * (y1 - y0);
}

// compact rows -> the film's rows: `n` elements a pixel; nothing outside the rectangle is read or written
template <class T> inline void place_plane(T *film, const T *compact, size_t n, uint32_t w, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    if (!film) return;
    const size_t rw = x1 - x0;
    for (uint32_t y = y0; y < y1; ++y)
        std::memcpy(film + ((size_t)y * w + x0) * n, compact + (size_t)(y - y0) * rw * n, rw * n * sizeof(T));
}
// ... of every plane asked for: compact[k] is the k-th plane's compact rows (the table's order; not looked at for a plane not asked for)
inline void place_features(const lg_features &out, const void *const *compact, uint32_t w, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    feature_planes(out, [&](auto *p, size_t per_pixel, size_t, const char *) {
        place_plane(p, static_cast<const std::remove_pointer_t<decltype(p)> *>(*compact++), per_pixel, w, x0, y0, x1, y1);
    });
}

} // namespace lg
