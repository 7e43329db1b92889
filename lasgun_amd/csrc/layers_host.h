// lasgun_amd/csrc/layers_host.h -- the part of lg_hit_layers* (query.cpp) that touches no device: the limits, the product n * max_layers
// and the planes' byte sizes with their overflow checks, and the one table of lg_layers_out's planes (layer_planes) with what follows
// from it: the NULL and alignment rules (the size and alignment rules themselves and the host form's staging are planes_host.h's).
// Arithmetic on size_t that can overflow, so kept free of HIP: tools/layers_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and both entry points call it.
#pragma once
#include "../../include/lasgun_hip.h"
#include "planes_host.h"

namespace lg {

static_assert(sizeof(lg_layers_out) == 40 && offsetof(lg_layers_out, hits) == 0 && offsetof(lg_layers_out, along) == 8 && offsetof(lg_layers_out, id) == 16 &&
                  offsetof(lg_layers_out, count) == 24 && offsetof(lg_layers_out, inside) == 32,
              "lg_layers_out: five pointers, 40 bytes");
static_assert(sizeof(lg_hit) == 96, "lg_hit: 96 bytes, the widest element of a layer plane");

// The five planes of lg_layers_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order; total = n * max_layers.  The alignment and NULL rules, the host
// form's staging, device buffers and copies and the device form's buffer checks all go through here.
template <class Out, class F> inline void layer_planes(Out &out, size_t n, size_t total, F &&f) {
    f(out.hits, total, 16, "hits");
    f(out.along, total, 8, "along");
    f(out.id, total * 4, 16, "id");
    f(out.count, n, 4, "count");
    f(out.inside, n, 8, "inside");
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  Returns
// n * max_layers, the elements of a layer plane: no count or size of layer_planes wraps.  (The sorted order's own limit on n depends on
// the accel's setting: query.cpp, check_sorted_count.)
inline size_t check_layers(const void *accel, const double *rays, size_t n, uint32_t max_layers, const lg_layers_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    require_any_plane([&](auto &&f) { layer_planes(*out, 0, 0, f); });
    if (max_layers == 0) throw std::runtime_error("max_layers is 0: at least one layer");
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    if (n > SIZE_MAX / max_layers) throw std::runtime_error("n * max_layers does not fit the address space");
    const size_t total = n * (size_t)max_layers;
    (void)checked_bytes(n, 6 * sizeof(double), "rays");
    (void)checked_bytes(total, sizeof(lg_hit), "a plane of n * max_layers elements"); // 96 bytes an element, the widest (hits)
    return total;
}
// The device form's alignment rule: rays 8 bytes, the planes theirs (hits and id 16, along and inside 8, count 4); NULL is not misaligned
inline void check_layers_alignment(const double *rays, const lg_layers_out &out) {
    check_alignment(rays, 8, "rays");
    check_planes_alignment([&](auto &&f) { layer_planes(out, 0, 0, f); });
}

} // namespace lg
