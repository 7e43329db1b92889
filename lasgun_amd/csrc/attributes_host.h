// lasgun_amd/csrc/attributes_host.h -- the part of lg_hit_attributes* (query.cpp) that touches no device: the limits, the planes' byte sizes
// with their overflow checks, the one table of lg_attr_out's planes (attr_planes) with what follows from it -- the NULL and alignment rules
// (the size and alignment rules themselves and the host forms' staging are planes_host.h's) --, and the counts table a record of the _of form is checked against: its layout, its builder
// and the check itself (attr_record_ok: ONE function for the host and for attr_of_kernel, k_attributes.hip).  Arithmetic on size_t that can
// overflow and an index check that guards every dereference of the _of form, so kept free of HIP: tools/attributes_host_check.cpp runs
// exactly this text under AddressSanitizer / UBSan on the CPU, and the entry points call it.
#pragma once
#include "../../include/lasgun_hip.h"
#include "planes_host.h"

#if defined(__HIPCC__)
#define LG_ATTR_HD __host__ __device__ __forceinline__
#else
#define LG_ATTR_HD inline
#endif

namespace lg {

static_assert(sizeof(lg_attr_out) == 56 && offsetof(lg_attr_out, hits) == 0 && offsetof(lg_attr_out, flags) == 8 && offsetof(lg_attr_out, bary) == 16 &&
                  offsetof(lg_attr_out, uv) == 24 && offsetof(lg_attr_out, local) == 32 && offsetof(lg_attr_out, frame) == 40 && offsetof(lg_attr_out, dp) == 48,
              "lg_attr_out: seven pointers, 56 bytes");
static_assert(sizeof(lg_hit) == 96, "lg_hit: 96 bytes, the widest row of a plane");
constexpr uint32_t ATTR_HIT = 1u, ATTR_NO_HIT = 2u, ATTR_BAD_RECORD = 4u; // the flag words k_attributes.hip writes
static_assert(ATTR_HIT == LG_ATTR_HIT && ATTR_NO_HIT == LG_ATTR_NO_HIT && ATTR_BAD_RECORD == LG_ATTR_BAD_RECORD, "the flag words k_attributes.hip writes");

// ---- the counts table: what a record may name.  Words: [0] accels, [1] spheres, [2] boxes, [3] 0; then two words per accel -- the face
// count of the mesh it is (0 for a group) and that mesh's first triangle in the triangle tables --; then per sphere the accel it sits in;
// then per box likewise.
constexpr size_t ATTR_COUNTS_HEAD = 4;
inline std::vector<uint32_t> attr_counts_build(const std::vector<uint32_t> &faces, const std::vector<uint32_t> &tri_base, const std::vector<uint32_t> &sphere_accel,
                                               const std::vector<uint32_t> &cuboid_accel) {
    if (faces.size() != tri_base.size()) throw std::runtime_error("attr_counts_build: one face count and one first triangle per accel");
    if (faces.size() > 0xFFFFFFFFull || sphere_accel.size() > 0xFFFFFFFFull || cuboid_accel.size() > 0xFFFFFFFFull) throw std::runtime_error("attr_counts_build: counts are 32-bit");
    std::vector<uint32_t> t;
    t.reserve(ATTR_COUNTS_HEAD + 2 * faces.size() + sphere_accel.size() + cuboid_accel.size());
    t.push_back((uint32_t)faces.size()); t.push_back((uint32_t)sphere_accel.size()); t.push_back((uint32_t)cuboid_accel.size()); t.push_back(0u);
    for (size_t a = 0; a < faces.size(); ++a) { t.push_back(faces[a]); t.push_back(tri_base[a]); }
    t.insert(t.end(), sphere_accel.begin(), sphere_accel.end());
    t.insert(t.end(), cuboid_accel.begin(), cuboid_accel.end());
    return t;
}
// Does (kind, prim, instance) -- lg_hit's numbering, kind 1 sphere, 2 box, 3 triangle -- name a primitive of the accel `counts` was built
// for?  Reads `counts` only at indices its own header vouches for.  (kind 0, a miss, names nothing and is answered before this.)
LG_ATTR_HD bool attr_record_ok(const uint32_t *counts, uint32_t kind, uint32_t prim, uint32_t instance) {
    const uint32_t accels = counts[0], spheres = counts[1], cuboids = counts[2];
    if (kind < 1u || kind > 3u || instance >= accels) return false;
    if (kind == 3u) return prim < counts[ATTR_COUNTS_HEAD + 2ull * instance];
    const unsigned long long owners = ATTR_COUNTS_HEAD + 2ull * accels;
    if (kind == 1u) return prim < spheres && counts[owners + prim] == instance;
    return prim < cuboids && counts[owners + spheres + prim] == instance;
}
// a triangle's index in the triangle tables, for a record attr_record_ok has passed
LG_ATTR_HD uint32_t attr_triangle_index(const uint32_t *counts, uint32_t prim, uint32_t instance) { return counts[ATTR_COUNTS_HEAD + 2ull * instance + 1ull] + prim; }

// The seven planes of lg_attr_out (or of a copy that f may edit), each written down here and nowhere else: f(the struct's pointer, its
// elements, its alignment in bytes, its name) in the struct's order.  The alignment and NULL rules, the host forms' staging, device
// buffers and copies and the device forms' buffer checks all go through here.
template <class Out, class F> inline void attr_planes(Out &out, size_t n, F &&f) {
    f(out.hits, n, 16, "hits");
    f(out.flags, n, 4, "flags");
    f(out.bary, n * 3, 8, "bary");
    f(out.uv, n * 2, 8, "uv");
    f(out.local, n * 3, 8, "local");
    f(out.frame, n * 6, 8, "frame");
    f(out.dp, n * 6, 8, "dp");
}

// Everything the contract calls an error that needs no device, thrown here; n is not 0 (an empty set is answered before this).  After it no
// count or size of attr_planes wraps.  of_form: lg_hit_attributes_of* -- `records` is its hits argument (not looked at otherwise), and
// out->hits has to be NULL.  (The sorted order's own limit on n depends on the accel's setting: query.cpp, check_sorted_count.)
inline void check_attributes(const void *accel, const double *rays, const lg_hit *records, bool of_form, size_t n, const lg_attr_out *out) {
    if (!accel) throw std::runtime_error("accel is NULL");
    if (!rays) throw std::runtime_error("rays is NULL");
    if (of_form && !records) throw std::runtime_error("hits is NULL");
    if (!out) throw std::runtime_error("out is NULL");
    if (of_form && out->hits) throw std::runtime_error("out->hits is not NULL: the _of form reads records and writes none");
    require_any_plane([&](auto &&f) { attr_planes(*out, 0, f); });
    if ((unsigned long long)n > QUERY_MAX_RAYS) throw std::runtime_error("too many rays in one query");
    (void)checked_bytes(n, 6 * sizeof(double), "rays");
    (void)checked_bytes(n, sizeof(lg_hit), "a plane of n rows"); // 96 bytes a row, the widest (hits)
}
// The device forms' alignment rule: rays 8 bytes, the records 16, the planes theirs (hits 16; flags 4; the double planes 8); NULL is not misaligned
inline void check_attributes_alignment(const double *rays, const lg_hit *records, const lg_attr_out &out) {
    check_alignment(rays, 8, "rays");
    check_alignment(records, 16, "hits");
    check_planes_alignment([&](auto &&f) { attr_planes(out, 0, f); });
}

} // namespace lg
