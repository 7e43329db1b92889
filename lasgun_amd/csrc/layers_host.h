// lasgun_amd/csrc/layers_host.h -- the part of lg_hit_layers* (query.cpp) that touches no device: the limits, the product n * max_layers
// and the planes' byte sizes with their overflow checks, and the one table of lg_layers_out's planes (layer_planes) with what follows
// from it: the NULL and alignment rules, the host form's staging and its placement.  Arithmetic on size_t that can overflow, so kept free
// of HIP: tools/layers_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and both entry points call it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lasgun_hip.h"

namespace lg {

static_assert(sizeof(lg_layers_out) == 40 && offsetof(lg_layers_out, hits) == 0 && offsetof(lg_layers_out, along) == 8 && offsetof(lg_layers_out, id) == 16 &&
                  offsetof(lg_layers_out, count) == 24 && offsetof(lg_layers_out, inside) == 32,
              "lg_layers_out: five pointers, 40 bytes");
static_assert(sizeof(lg_hit) == 96, "lg_hit: 96 bytes, the widest element of a layer plane");

constexpr unsigned long long LAYERS_MAX_RAYS = 0xFFFFFFFFull * 64ull; // 64-ray tiles are counted in 32 bits, as lg_intersect's are

// count * bytes_each as a size_t, refused where it does not fit the address space
inline size_t layers_bytes(size_t count, size_t bytes_each, const char *what) {
    if (bytes_each && count > SIZE_MAX / bytes_each) throw std::runtime_error(std::string(what) + " does not fit the address space");
    return count * bytes_each;
}

// The host form's outputs on their way back: only what is asked for has any size.  An error on the way leaves the caller's arrays as they were.
struct LayersStaging {
    std::vector<lg_hit> hits;
    std::vector<double> along;
    std::vector<uint32_t> id, count;
    std::vector<double> inside;
    LayersStaging(const lg_layers_out &out, size_t n, size_t total);
};
// The five planes of lg_layers_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, the
// plane's staging, its elements, its alignment in bytes, its name) in the struct's order; total = n * max_layers.  The alignment and NULL
// rules, the staging's sizes, the host form's device buffers and copies, the device form's buffer checks and the placement all go through here.
template <class Out, class F> inline void layer_planes(Out &out, size_t n, size_t total, F &&f) {
    f(out.hits, &LayersStaging::hits, total, 16, "hits");
    f(out.along, &LayersStaging::along, total, 8, "along");
    f(out.id, &LayersStaging::id, total * 4, 16, "id");
    f(out.count, &LayersStaging::count, n, 4, "count");
    f(out.inside, &LayersStaging::inside, n, 8, "inside");
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  Returns
// n * max_layers, the elements of a layer plane: no count or size of layer_planes wraps.  (The sorted order's own limit on n depends on
// the accel's setting: query.cpp, check_sorted_count.)
inline size_t check_layers(const void *accel, const double *rays, size_t n, uint32_t max_layers, const lg_layers_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    bool any = false;
    layer_planes(*out, 0, 0, [&](auto *p, auto, size_t, size_t, const char *) { any = any || p; });
    if (!any) throw std::runtime_error("every plane of out is NULL: at least one output");
    if (max_layers == 0) throw std::runtime_error("max_layers is 0: at least one layer");
    if ((unsigned long long)n > LAYERS_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    if (n > SIZE_MAX / max_layers) throw std::runtime_error("n * max_layers does not fit the address space");
    const size_t total = n * (size_t)max_layers;
    (void)layers_bytes(n, 6 * sizeof(double), "rays");
    (void)layers_bytes(total, sizeof(lg_hit), "a plane of n * max_layers elements"); // 96 bytes an element, the widest (hits)
    return total;
}
inline LayersStaging::LayersStaging(const lg_layers_out &out, size_t n, size_t total) {
    layer_planes(out, n, total, [&](auto *p, auto plane, size_t count, size_t, const char *) { if (p) (this->*plane).resize(count); });
}
inline void place_layers(const lg_layers_out &out, const LayersStaging &st) {
    layer_planes(out, 0, 0, [&](auto *p, auto plane, size_t, size_t, const char *) {
        if (p && !(st.*plane).empty()) std::memcpy(p, (st.*plane).data(), (st.*plane).size() * sizeof *p);
    });
}
// The device form's alignment rule: rays 8 bytes, the planes theirs (hits and id 16, along and inside 8, count 4); NULL is not misaligned
inline void check_layers_alignment(const double *rays, const lg_layers_out &out) {
    const auto aligned = [](const void *p, size_t align, const char *what) {
        if (p && (uintptr_t)p % align) throw std::runtime_error(std::string(what) + " is not " + std::to_string(align) + "-byte aligned");
    };
    aligned(rays, 8, "rays");
    layer_planes(out, 0, 0, [&](auto *p, auto, size_t, size_t align, const char *what) { aligned(p, align, what); });
}

} // namespace lg
