// lasgun_amd/csrc/view_features_host.h -- the part of lg_capture_view_features* (query.cpp) that touches no device: the one table of the
// planes of lg_view_features (view_feature_planes), what both forms refuse before anything is allocated or enqueued -- the NULL rules, the
// film's limits, the tile count with its 32-bit limit, every plane's byte size, the views' own rules --, and the device form's alignment
// rule.  The tile count, the sizes, what a valid view is and lg_view -> DView are views_host.h's, not restated.  Arithmetic on size_t that
// can overflow, so kept free of HIP: tools/view_features_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU,
// and both entry points call it.
#pragma once
#include "views_host.h"

namespace lg {

static_assert(sizeof(lg_view_features) == 48 && offsetof(lg_view_features, depth) == 0 && offsetof(lg_view_features, normal) == 8 && offsetof(lg_view_features, albedo) == 16 &&
                  offsetof(lg_view_features, coverage) == 24 && offsetof(lg_view_features, id) == 32 && offsetof(lg_view_features, point) == 40,
              "lg_view_features: six pointers, 48 bytes");

// The six planes of lg_view_features (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, the
// plane's elements a pixel, its alignment in bytes, its name) in the struct's order.  The NULL rule, the sizes, the host form's staging,
// the device form's buffer checks and the alignment rule all go through here.
template <class Out, class F> inline void view_feature_planes(Out &out, F &&f) {
    f(out.depth, 1, 4, "depth");
    f(out.normal, 3, 4, "normal");
    f(out.albedo, 3, 4, "albedo");
    f(out.coverage, 1, 4, "coverage");
    f(out.id, 4, 16, "id");
    f(out.point, 3, 4, "point");
}

// Everything the contract calls an error that needs no device and no scene; n_views is not 0 (an empty batch is answered before this).
// The samples of a pixel run in a loop in one lane, so a call's tiles are its PIXEL tiles (view_tiles with S = 1).  As in check_views,
// view 0 gives the call's samples_root, and the tile count and the sizes are checked BEFORE the other records are read.
inline ViewShape check_view_features(const void *accel, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, const lg_view_features *out, const double *material_rgb) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!views) throw std::runtime_error("views is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { view_feature_planes(*out, f); });
    if (out->albedo && !material_rgb) throw std::runtime_error("albedo is requested and material_rgb is NULL");
    if (w == 0 || h == 0) throw std::runtime_error("view features: an empty film (width or height is 0)");
    // (a tile's pixel coordinates are 32-bit: the last tile of a row or column may reach 7 pixels beyond the film's edge)
    if (w > 0xFFFFFFF8u || h > 0xFFFFFFF8u) throw std::runtime_error("film beyond 2^32 - 8: the coordinates of a tile's pixels are 32-bit");
    check_view(views[0], 0);
    const uint32_t root = views[0].samples_root;
    unsigned long long per_view = 0, tiles = 0;
    if (!view_tiles(n_views, w, h, 1, &per_view, &tiles))
        throw std::runtime_error("too many pixels in one view-feature capture: n_views * ceil(w/8) * ceil(h/8) pixel tiles are counted in 32 bits");
    view_feature_planes(*out, [&](auto *p, size_t per_pixel, size_t, const char *what) {
        if (p) (void)view_bytes(n_views, w, h, per_pixel * sizeof *p, (std::string("n_views * width * height elements of ") + what).c_str());
    });
    (void)view_bytes(n_views, 1, 1, sizeof(DView), "n_views * 128 bytes of view records");
    for (size_t v = 1; v < n_views; ++v) {
        check_view(views[v], v);
        if (views[v].samples_root != root)
            throw std::runtime_error("view " + std::to_string(v) + ": samples_root " + std::to_string(views[v].samples_root) + " differs from view 0's " + std::to_string(root) +
                                     ": the views of one call have the same samples_root");
    }
    const uint32_t tiles_x = w / 8u + (w % 8u ? 1u : 0u);
    return {root, tiles_x, (uint32_t)per_view, (uint32_t)tiles, n_views * ((size_t)w * h)};
}
// The device form's alignment rule: id 16 bytes (one store a pixel), the float planes 4, material_rgb 8 where albedo asks for it
inline void check_view_features_alignment(const lg_view_features &out, const double *material_rgb) {
    check_planes_alignment([&](auto &&f) { view_feature_planes(out, f); });
    if (out.albedo && (uintptr_t)material_rgb % 8) throw std::runtime_error("material_rgb is not 8-byte aligned");
}

} // namespace lg
