// lasgun_amd/csrc/views_host.h -- the part of lg_capture_views* (query.cpp) that touches no device: the work-tile count with its 32-bit
// limit, both byte sizes, what makes a view record valid and the uniform-samples rule, the NULL and alignment rules, and lg_view -> DView.
// Arithmetic on size_t that can overflow, so kept free of HIP: tools/views_host_check.cpp runs exactly this text under AddressSanitizer /
// UBSan on the CPU, and both entry points call it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lasgun_hip.h"
#include "dscene.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_view) == 120 && offsetof(lg_view, origin) == 0 && offsetof(lg_view, view) == 24 && offsetof(lg_view, up) == 48 && offsetof(lg_view, aux) == 72 &&
                  offsetof(lg_view, image_plane_height) == 96 && offsetof(lg_view, pixel_separation) == 104 && offsetof(lg_view, samples_root) == 112 &&
                  offsetof(lg_view, reserved) == 116,
              "lg_view: 120 bytes, no padding");
static_assert(sizeof(DView) == 128 && offsetof(DView, image_plane_height) == 96 && offsetof(DView, ss_distance) == 112 && offsetof(DView, ss_root) == 120,
              "DView: the layout k_views.hip reads (view_load)");

constexpr unsigned long long VIEW_MAX_TILES = 0xFFFFFFFFull; // work tiles are counted in 32 bits, as the other queries' are
constexpr uint32_t VIEW_MAX_SAMPLES_ROOT = 256u;

// The 8 x 8 tiles of one film, and the work tiles of a call: n_views * ceil(w / 8) * ceil(h / 8) * S.  false: more than 2^32 - 1 (no product
// is formed where it could overflow)
inline bool view_tiles(size_t n_views, uint32_t w, uint32_t h, unsigned long long S, unsigned long long *per_view, unsigned long long *work_tiles) {
    const unsigned long long tx = (unsigned long long)(w / 8u) + (w % 8u ? 1u : 0u), ty = (unsigned long long)(h / 8u) + (h % 8u ? 1u : 0u);
    *per_view = tx * ty; // (< 2^29 * 2^29: fits)
    *work_tiles = 0;
    if (n_views == 0 || *per_view == 0 || S == 0) return true;
    if (*per_view > VIEW_MAX_TILES) return false;
    if ((unsigned long long)n_views > VIEW_MAX_TILES / *per_view) return false;
    const unsigned long long pixel_tiles = (unsigned long long)n_views * *per_view;
    if (pixel_tiles > VIEW_MAX_TILES / S) return false;
    *work_tiles = pixel_tiles * S;
    return true;
}
// n_views * w * h * bytes as a size_t, refused where it does not fit the address space
inline size_t view_bytes(size_t n_views, uint32_t w, uint32_t h, size_t bytes, const char *what) {
    const size_t pixels = (size_t)w * h; // (< 2^64: two 32-bit factors)
    if (pixels && n_views > SIZE_MAX / pixels) throw std::runtime_error(std::string(what) + " does not fit the address space");
    const size_t n = n_views * pixels;
    if (bytes && n > SIZE_MAX / bytes) throw std::runtime_error(std::string(what) + " does not fit the address space");
    return n * bytes;
}

// One record's own rules (lg_view_rays* and every view of a batch): samples_root 1 .. 256, reserved 0; everything else is taken as given
inline void check_view(const lg_view &view, size_t index) {
    const uint32_t root = view.samples_root;
    if (root == 0 || root > VIEW_MAX_SAMPLES_ROOT) throw std::runtime_error("view " + std::to_string(index) + ": samples_root is " + std::to_string(root) + ", not 1 .. 256");
    if (view.reserved != 0) throw std::runtime_error("view " + std::to_string(index) + ": reserved must be 0");
}
// What a checked call is
struct ViewShape {
    uint32_t samples_root, tiles_x, tiles_per_view;
    uint32_t pixel_tiles;   // n_views * tiles_per_view
    size_t pixels;          // n_views * w * h
};
// Everything the contract calls an error that needs no device and no scene; n_views is not 0 (an empty batch is answered before this).
// View 0 gives the call's samples_root; the tile count and the sizes are checked BEFORE the other records are read, so that a count that
// cannot be a table's length is refused without walking it.  Non-finite fields of a view are accepted as they are.
inline ViewShape check_views(const void *accel, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, const void *rgba, const void *rgb) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!views) throw std::runtime_error("views is NULL");
    if (!rgba && !rgb) throw std::runtime_error("rgba and rgb are both NULL: at least one output");
    if (w == 0 || h == 0) throw std::runtime_error("views: an empty film (width or height is 0)");
    check_view(views[0], 0);
    const uint32_t root = views[0].samples_root;
    unsigned long long per_view = 0, work = 0;
    if (!view_tiles(n_views, w, h, (unsigned long long)root * root, &per_view, &work))
        throw std::runtime_error("too many pixels in one view batch: n_views * ceil(w/8) * ceil(h/8) * samples work tiles are counted in 32 bits");
    (void)view_bytes(n_views, w, h, 4, "n_views * width * height * 4 bytes of rgba");
    (void)view_bytes(n_views, w, h, 3 * sizeof(double), "n_views * width * height * 24 bytes of rgb");
    (void)view_bytes(n_views, 1, 1, sizeof(DView), "n_views * 128 bytes of view records");
    for (size_t v = 1; v < n_views; ++v) {
        check_view(views[v], v);
        if (views[v].samples_root != root)
            throw std::runtime_error("view " + std::to_string(v) + ": samples_root " + std::to_string(views[v].samples_root) + " differs from view 0's " + std::to_string(root) +
                                     ": the views of one call have the same samples_root");
    }
    const uint32_t tiles_x = w / 8u + (w % 8u ? 1u : 0u);
    return {root, tiles_x, (uint32_t)per_view, (uint32_t)(n_views * per_view), n_views * ((size_t)w * h)};
}
// The device form's alignment rule: rgba 4 bytes (one word a pixel), rgb 8
inline void check_views_alignment(const void *rgba, const void *rgb) {
    check_alignment(rgba, 4, "rgba");
    check_alignment(rgb, 8, "rgb");
}
// lg_view -> the record the kernels read: the fields as given, and Camera::set_supersampling's ss_distance = 1.0 / (double)samples_root
inline DView to_dview(const lg_view &v) {
    DView d;
    d.origin = V3{v.origin[0], v.origin[1], v.origin[2]}; d.view = V3{v.view[0], v.view[1], v.view[2]};
    d.up = V3{v.up[0], v.up[1], v.up[2]}; d.aux = V3{v.aux[0], v.aux[1], v.aux[2]};
    d.image_plane_height = v.image_plane_height; d.pixel_separation = v.pixel_separation;
    d.ss_distance = 1.0 / (double)v.samples_root;
    d.ss_root = v.samples_root; d.pad = 0u;
    return d;
}
inline std::vector<DView> to_dviews(const lg_view *views, size_t n_views) {
    std::vector<DView> d(n_views);
    for (size_t v = 0; v < n_views; ++v) d[v] = to_dview(views[v]);
    return d;
}

} // namespace lg
