// tools/attributes_host_check.cpp -- the device-free host code of lg_hit_attributes* / lg_hit_attributes_of* (lasgun_amd/csrc/attributes_host.h:
// the limits and the planes' byte sizes with their overflow checks, the NULL and alignment rules of lg_attr_out and of the _of form's
// records, the host forms' staging, the counts table and attr_record_ok) in a stand-alone program, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_attributes_host_sanitized.py does).  The counts go up to 2^64 - 1: an
// overflow in forming a size is a UBSan report or a wrong value here, not a short buffer on a card.  The launch is stubbed out: a "kernel"
// that fills the staged planes with bytes that name their place (host_check.h, staged_round); every caller's array is a heap block of exactly its size, so a copy
// past an end is an ASan report.  attr_record_ok is the function attr_of_kernel calls before it reads anything through a record: here it
// runs over an exhaustive small grid of records against a table that is a heap block of exactly its size, and is compared with a
// brute-force statement of the contract.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/attributes_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/attributes_host.h"
#include "host_check.h"

using namespace lg;

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};

static bool refused(const void *accel, const double *rays, const lg_hit *records, bool of_form, size_t n, const lg_attr_out *out) {
    return throws([&] { check_attributes(accel, rays, records, of_form, n, out); });
}
static bool misaligned(const void *rays, const void *records, const lg_attr_out &out) {
    return throws([&] { check_attributes_alignment((const double *)rays, (const lg_hit *)records, out); });
}
// lg_attr_out with the planes of a 7-bit mask named from `all`
static lg_attr_out subset(const lg_attr_out &all, unsigned planes) {
    return lg_attr_out{planes & 1u ? all.hits : nullptr, planes & 2u ? all.flags : nullptr, planes & 4u ? all.bary : nullptr, planes & 8u ? all.uv : nullptr,
                       planes & 16u ? all.local : nullptr, planes & 32u ? all.frame : nullptr, planes & 64u ? all.dp : nullptr};
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of every output is looked at
static void run(size_t n, unsigned planes) {
    const lg_attr_out all{(lg_hit *)ASKED, (uint32_t *)ASKED, (double *)ASKED, (double *)ASKED, (double *)ASKED, (double *)ASKED, (double *)ASKED};
    lg_attr_out out = subset(all, planes);
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    check_attributes(&accel, D, nullptr, false, n, &out);
    const StagedRound r = staged_round([&](auto &&f) { attr_planes(out, n, f); });
    EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 96 * n : 0, planes & 2u ? 4 * n : 0, planes & 4u ? 8 * 3 * n : 0, planes & 8u ? 8 * 2 * n : 0, planes & 16u ? 8 * 3 * n : 0,
                                                 planes & 32u ? 8 * 6 * n : 0, planes & 64u ? 8 * 6 * n : 0}));
    const size_t want_bytes = n * ((planes & 1u ? 96 : 0) + (planes & 2u ? 4 : 0) + (planes & 4u ? 24 : 0) + (planes & 8u ? 16 : 0) + (planes & 16u ? 24 : 0) + (planes & 32u ? 48 : 0) + (planes & 64u ? 48 : 0));
    EXPECT(r.bytes == want_bytes);
}

// attr_record_ok over every record of a small grid, for one scene description, against the contract said in plain loops
static void records(const std::vector<uint32_t> &faces, const std::vector<uint32_t> &tri_base, const std::vector<uint32_t> &sphere_accel, const std::vector<uint32_t> &cuboid_accel) {
    const std::vector<uint32_t> table = attr_counts_build(faces, tri_base, sphere_accel, cuboid_accel);
    EXPECT(table.size() == ATTR_COUNTS_HEAD + 2 * faces.size() + sphere_accel.size() + cuboid_accel.size());
    std::unique_ptr<uint32_t[]> heap(new uint32_t[table.size()]); // exactly its size: a read past the end is an ASan report
    std::memcpy(heap.get(), table.data(), table.size() * sizeof(uint32_t));
    const uint32_t edge[] = {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 0x3FFFFFFFu, 0x40000000u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const uint32_t kinds[] = {1u, 2u, 3u, 4u, 5u, 7u, 8u, 255u, 0x80000001u, 0xFFFFFFFFu};
    for (uint32_t kind : kinds)
        for (uint32_t prim : edge)
            for (uint32_t inst : edge) {
                bool want = false;
                if (kind == 1u) want = prim < sphere_accel.size() && inst < faces.size() && sphere_accel[prim] == inst;
                else if (kind == 2u) want = prim < cuboid_accel.size() && inst < faces.size() && cuboid_accel[prim] == inst;
                else if (kind == 3u) want = inst < faces.size() && prim < faces[inst];
                const bool got = attr_record_ok(heap.get(), kind, prim, inst);
                EXPECT(got == want);
                if (got && kind == 3u) EXPECT(attr_triangle_index(heap.get(), prim, inst) == tri_base[inst] + prim);
            }
}

int main() {
    int accel = 0;
    alignas(16) lg_hit h[2];
    alignas(16) double d[8] = {0.0};
    alignas(16) uint32_t u[8] = {0u};
    std::memset(h, 0, sizeof h);
    const lg_attr_out all{h, u, d, d, d, d, d}, none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const lg_attr_out no_hits = subset(all, 0x7Eu);
    const size_t TOP = ~(size_t)0, EDGE = TOP / 96; // the most lg_hit records an address space holds
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(QUERY_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    // ---- check_attributes: every error of the contract that needs no device, both forms
    EXPECT(!refused(&accel, D, nullptr, false, 3, &all));
    EXPECT(refused(nullptr, D, nullptr, false, 3, &all));
    EXPECT(refused(&accel, nullptr, nullptr, false, 3, &all));
    EXPECT(refused(&accel, D, nullptr, false, 3, nullptr));
    EXPECT(refused(&accel, D, nullptr, false, 3, &none));
    EXPECT(!refused(&accel, D, h, true, 2, &no_hits));
    EXPECT(refused(&accel, D, nullptr, true, 2, &no_hits)); // the _of form without records
    EXPECT(refused(&accel, D, h, true, 2, &all));           // ... with out->hits
    EXPECT(refused(nullptr, D, h, true, 2, &no_hits) && refused(&accel, nullptr, h, true, 2, &no_hits) && refused(&accel, D, h, true, 2, nullptr));
    EXPECT(refused(&accel, D, h, true, 2, &none));
    // the ray limit: (2^32 - 1) * 64 and one above; the address space: SIZE_MAX / 96 rows and one above
    EXPECT(!refused(&accel, D, nullptr, false, QUERY_MAX_RAYS, &all) && refused(&accel, D, nullptr, false, QUERY_MAX_RAYS + 1, &all) && refused(&accel, D, nullptr, false, TOP, &all));
    EXPECT(!refused(&accel, D, h, true, QUERY_MAX_RAYS, &no_hits) && refused(&accel, D, h, true, QUERY_MAX_RAYS + 1, &no_hits));
    EXPECT(QUERY_MAX_RAYS <= EDGE); // (so the ray limit is the one that binds; the sizes are checked all the same)
    EXPECT(checked_bytes(0, 96, "x") == 0 && checked_bytes(EDGE, 96, "x") == EDGE * 96 && checked_bytes(5, 0, "x") == 0);
    EXPECT(throws([&] { (void)checked_bytes(EDGE + 1, 96, "x"); }));
    // ---- the NULL rule: every combination of the seven planes; only all NULL is refused; the _of form refuses every one with hits
    for (unsigned planes = 0; planes < 128; ++planes) {
        const lg_attr_out o = subset(all, planes);
        EXPECT(refused(&accel, D, nullptr, false, 3, &o) == (planes == 0));
        EXPECT(refused(&accel, D, h, true, 2, &o) == (planes == 0 || (planes & 1u)));
        EXPECT(refused(nullptr, D, nullptr, false, 3, &o) && refused(&accel, nullptr, nullptr, false, 3, &o));
    }
    // ---- the alignment rule: rays 8; records and hits 16; flags 4; the double planes 8; NULL is not misaligned
    const char *base = reinterpret_cast<const char *>(d);
    EXPECT(!misaligned(D, nullptr, all) && !misaligned(D, h, none) && !misaligned(nullptr, nullptr, all));
    for (int off : {1, 2, 4}) EXPECT(misaligned(base + off, nullptr, all));
    EXPECT(!misaligned(base + 8, nullptr, all));
    for (int off : {1, 2, 4, 8}) EXPECT(misaligned(D, reinterpret_cast<const char *>(h) + off, no_hits));
    EXPECT(!misaligned(D, reinterpret_cast<const char *>(h) + 16, no_hits));
    const size_t want_align[7] = {16, 4, 8, 8, 8, 8, 8};
    for (int k = 0; k < 7; ++k)
        for (int off : {1, 2, 4, 8, 16}) {
            lg_attr_out o = all;
            char *moved = (k == 0 ? reinterpret_cast<char *>(h) : k == 1 ? reinterpret_cast<char *>(u) : reinterpret_cast<char *>(d)) + off;
            if (k == 0) o.hits = reinterpret_cast<lg_hit *>(moved);
            else if (k == 1) o.flags = reinterpret_cast<uint32_t *>(moved);
            else (k == 2 ? o.bary : k == 3 ? o.uv : k == 4 ? o.local : k == 5 ? o.frame : o.dp) = reinterpret_cast<double *>(moved);
            EXPECT(misaligned(D, nullptr, o) == ((size_t)off % want_align[k] != 0));
        }
    // ---- staging and placement: every subset of the planes, shapes with partial tiles
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)129})
        for (unsigned planes = 1; planes < 128; ++planes) run(n, planes);
    // ---- the counts table and the record check, exhaustively over a small grid
    records({}, {}, {}, {});                                               // nothing at all: every record is refused
    records({0}, {0}, {}, {});                                             // an empty root
    records({0}, {0}, {0, 0, 0}, {0});                                     // a root of spheres and a box
    records({0, 5}, {0, 0}, {}, {});                                       // a mesh under the root
    records({0, 0, 4, 0, 4, 7}, {0, 0, 3, 0, 3, 9}, {0, 1, 1, 3, 0}, {3, 3, 1}); // groups, two instances of one mesh, another mesh
    records({0, 0x3FFFFFFFu}, {0, 1}, {0, 0xFFFFFFFFu}, {0xFFFFFFFFu});     // the largest face count; primitives that sit nowhere
    {
        bool thrown = false;
        try { (void)attr_counts_build({0, 1}, {0}, {}, {}); } catch (const std::exception &) { thrown = true; }
        EXPECT(thrown);
    }
    if (failures) { std::fprintf(stderr, "attributes_host_check: %d failures\n", failures); return 1; }
    std::printf("attributes_host_check: ok\n");
    return 0;
}
