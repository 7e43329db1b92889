// tools/paths_host_check.cpp -- the device-free host code of lg_trace_paths* (lasgun_amd/csrc/paths_host.h: the limits, the product
// n * max_bounces and the planes' byte sizes with their overflow checks, the rule table's validation, the NULL and alignment rules of
// lg_paths_out, the host form's staging) in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_paths_host_sanitized.py does).  The counts go up to 2^64 - 1: an overflow in forming a product or a size is a UBSan report
// or a wrong value here, not a short buffer on a card.  The launch is stubbed out: a "kernel" that fills the staged planes with values that
// name their element; every caller's array is a heap block of exactly its size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/paths_host_check.cpp -o check && ./check
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../lasgun_amd/csrc/paths_host.h"

using namespace lg;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
static const lg_path_rule RULES[3] = {{LG_PATH_REFRACT, 0u, 1.5, 1.0}, {LG_PATH_REFLECT, 0u, 1.0, 0.5}, {LG_PATH_ABSORB, 0u, 1.0, 1.0}};

static bool refused(const void *accel, const double *rays, size_t n, uint32_t max_bounces, const lg_paths_out *out, const lg_path_rule *rules = RULES, size_t n_rules = 3,
                    size_t materials = 3, int normal = 0) {
    try {
        (void)check_paths(accel, rays, n, max_bounces, rules, n_rules, materials, normal, out);
    } catch (const std::exception &e) {
        return e.what()[0] != 0;
    }
    return false;
}
static size_t checked(const void *accel, size_t n, uint32_t max_bounces, const lg_paths_out *out) { return check_paths(accel, D, n, max_bounces, RULES, 3, 3, 0, out); }
static bool misaligned(const void *rays, const void *start_medium, const lg_paths_out &out) {
    try {
        check_paths_alignment((const double *)rays, (const uint32_t *)start_medium, out);
    } catch (const std::exception &e) {
        return e.what()[0] != 0;
    }
    return false;
}
// lg_paths_out with the planes of a 9-bit mask named from `all`, in the struct's order
static lg_paths_out subset(const lg_paths_out &all, unsigned planes) {
    return lg_paths_out{planes & 1u ? all.hits : nullptr,   planes & 2u ? all.point : nullptr, planes & 4u ? all.id : nullptr,
                        planes & 8u ? all.along : nullptr,  planes & 16u ? all.count : nullptr, planes & 32u ? all.end : nullptr,
                        planes & 64u ? all.gain : nullptr,  planes & 128u ? all.last : nullptr, planes & 256u ? all.medium : nullptr};
}

// one host-form call without a device: check, stage, "launch", place; then every element of every output is looked at
static void run(size_t n, uint32_t max_bounces, unsigned planes) {
    const size_t total = n * max_bounces;
    std::unique_ptr<lg_hit[]> hits(planes & 1u ? new lg_hit[total] : nullptr);
    std::unique_ptr<double[]> point(planes & 2u ? new double[3 * total] : nullptr), along(planes & 8u ? new double[total] : nullptr),
        gain(planes & 64u ? new double[n] : nullptr), last(planes & 128u ? new double[6 * n] : nullptr);
    std::unique_ptr<uint32_t[]> id(planes & 4u ? new uint32_t[4 * total] : nullptr), count(planes & 16u ? new uint32_t[n] : nullptr),
        end(planes & 32u ? new uint32_t[n] : nullptr), medium(planes & 256u ? new uint32_t[n] : nullptr);
    const lg_paths_out out{hits.get(), point.get(), id.get(), along.get(), count.get(), end.get(), gain.get(), last.get(), medium.get()};
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    EXPECT(checked(&accel, n, max_bounces, &out) == total);
    PathsStaging st(out, n, total);
    EXPECT(st.hits.size() == (out.hits ? total : 0) && st.point.size() == (out.point ? 3 * total : 0) && st.id.size() == (out.id ? 4 * total : 0) &&
           st.along.size() == (out.along ? total : 0) && st.count.size() == (out.count ? n : 0) && st.end.size() == (out.end ? n : 0) &&
           st.gain.size() == (out.gain ? n : 0) && st.last.size() == (out.last ? 6 * n : 0) && st.medium.size() == (out.medium ? n : 0));
    // what the host form allocates on the device and copies back: the table's counts in the plane's own elements
    size_t staged_bytes = 0, want_bytes = 0;
    path_planes(out, n, total, [&](auto *p, auto plane, size_t elems, size_t, const char *) { if (p) { staged_bytes += (st.*plane).size() * sizeof *p; want_bytes += elems * sizeof *p; } });
    EXPECT(staged_bytes == want_bytes);
    EXPECT(want_bytes == (out.hits ? 96 * total : 0) + (out.point ? 24 * total : 0) + (out.id ? 16 * total : 0) + (out.along ? 8 * total : 0) + (out.count ? 4 * n : 0) +
                             (out.end ? 4 * n : 0) + (out.gain ? 8 * n : 0) + (out.last ? 48 * n : 0) + (out.medium ? 4 * n : 0));
    for (size_t e = 0; e < total; ++e) { // the stubbed launch
        if (out.hits) {
            lg_hit h;
            std::memset(&h, 0, sizeof h);
            h.t = (double)e + 0.25; h.prim = (uint32_t)e; h.material = -(int32_t)e;
            st.hits[e] = h;
        }
        for (size_t c = 0; c < 3; ++c)
            if (out.point) st.point[3 * e + c] = (double)(3 * e + c) + 0.75;
        for (size_t c = 0; c < 4; ++c)
            if (out.id) st.id[4 * e + c] = (uint32_t)(4 * e + c);
        if (out.along) st.along[e] = (double)e + 0.5;
    }
    for (size_t i = 0; i < n; ++i) {
        if (out.count) st.count[i] = (uint32_t)(i + 7);
        if (out.end) st.end[i] = (uint32_t)(i + 11);
        if (out.gain) st.gain[i] = (double)i + 0.125;
        for (size_t c = 0; c < 6; ++c)
            if (out.last) st.last[6 * i + c] = (double)(6 * i + c) + 0.375;
        if (out.medium) st.medium[i] = (uint32_t)(i + 13);
    }
    place_paths(out, st);
    for (size_t e = 0; e < total; ++e) {
        if (hits) EXPECT(hits[e].t == (double)e + 0.25 && hits[e].prim == (uint32_t)e && hits[e].material == -(int32_t)e);
        for (size_t c = 0; c < 3; ++c)
            if (point) EXPECT(point[3 * e + c] == (double)(3 * e + c) + 0.75);
        for (size_t c = 0; c < 4; ++c)
            if (id) EXPECT(id[4 * e + c] == (uint32_t)(4 * e + c));
        if (along) EXPECT(along[e] == (double)e + 0.5);
    }
    for (size_t i = 0; i < n; ++i) {
        if (count) EXPECT(count[i] == (uint32_t)(i + 7));
        if (end) EXPECT(end[i] == (uint32_t)(i + 11));
        if (gain) EXPECT(gain[i] == (double)i + 0.125);
        for (size_t c = 0; c < 6; ++c)
            if (last) EXPECT(last[6 * i + c] == (double)(6 * i + c) + 0.375);
        if (medium) EXPECT(medium[i] == (uint32_t)(i + 13));
    }
}

int main() {
    int accel = 0;
    alignas(16) lg_hit h[2];
    alignas(16) double d[8] = {0.0};
    alignas(16) uint32_t u[8] = {0u};
    std::memset(h, 0, sizeof h);
    const lg_paths_out all{h, d, u, d, u, u, d, d, u}, none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t TOP = ~(size_t)0, EDGE = TOP / 96; // the most lg_hit records an address space holds
    const uint32_t KMAX = 0xFFFFFFFFu;
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(PATHS_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    // ---- check_paths: every error of the contract that needs no device
    EXPECT(!refused(&accel, D, 3, 5, &all) && checked(&accel, 3, 5, &all) == 15);
    EXPECT(refused(nullptr, D, 3, 5, &all));
    EXPECT(refused(&accel, nullptr, 3, 5, &all));
    EXPECT(refused(&accel, D, 3, 5, nullptr));
    EXPECT(refused(&accel, D, 3, 5, &none));
    // max_bounces of 0, 1 and 2^32 - 1
    EXPECT(refused(&accel, D, 1, 0, &all) && refused(&accel, D, PATHS_MAX_RAYS, 0, &all));
    EXPECT(!refused(&accel, D, 1, 1, &all) && checked(&accel, 1, 1, &all) == 1);
    EXPECT(!refused(&accel, D, 1, KMAX, &all) && checked(&accel, 1, KMAX, &all) == KMAX);
    EXPECT(!refused(&accel, D, 65, KMAX, &all) && checked(&accel, 65, KMAX, &all) == 65ull * KMAX);
    // the ray limit: (2^32 - 1) * 64 and one above
    EXPECT(!refused(&accel, D, PATHS_MAX_RAYS, 1, &all) && checked(&accel, PATHS_MAX_RAYS, 1, &all) == PATHS_MAX_RAYS);
    EXPECT(refused(&accel, D, PATHS_MAX_RAYS + 1, 1, &all) && refused(&accel, D, TOP, 1, &all) && refused(&accel, D, TOP, KMAX, &all));
    // n * max_bounces just under, at and over SIZE_MAX / 96: the hits plane's bytes fit or do not, whichever planes are asked for
    const uint32_t KS[] = {(uint32_t)1 << 20, 1000003u, KMAX};
    for (uint32_t k : KS) {
        const size_t under = EDGE / k; // under * k <= EDGE < (under + 1) * k
        EXPECT(under <= PATHS_MAX_RAYS && under * k <= EDGE && EDGE - under * k < k);
        EXPECT(!refused(&accel, D, under, k, &all) && checked(&accel, under, k, &all) == under * k);
        EXPECT(refused(&accel, D, under + 1, k, &all));
        const lg_paths_out only_count = subset(all, 16u); // the limit does not depend on the planes asked for
        EXPECT(!refused(&accel, D, under, k, &only_count) && refused(&accel, D, under + 1, k, &only_count));
        // no count of the plane table wraps at the edge: the widest in elements (id, 4 a vertex) and in bytes (hits)
        size_t most = 0;
        path_planes(all, under, under * k, [&](auto *p, auto, size_t elems, size_t, const char *) { EXPECT(elems <= TOP / sizeof *p); most = elems > most ? elems : most; });
        EXPECT(most == 4 * under * k || most == 6 * under);
    }
    // the product itself: n * max_bounces beyond 2^64 is refused before it is formed
    EXPECT(refused(&accel, D, PATHS_MAX_RAYS, KMAX, &all) && refused(&accel, D, (size_t)1 << 33, (uint32_t)1 << 31, &all));
    // the sizes
    EXPECT(paths_bytes(0, 96, "x") == 0 && paths_bytes(EDGE, 96, "x") == EDGE * 96 && paths_bytes(5, 0, "x") == 0);
    {
        bool thrown = false;
        try { (void)paths_bytes(EDGE + 1, 96, "x"); } catch (const std::exception &) { thrown = true; }
        EXPECT(thrown);
    }
    // ---- the rules: NULL, a count that is not the accel's, an unknown action, reserved set; normal outside {0, 1}
    EXPECT(refused(&accel, D, 3, 5, &all, nullptr, 3, 3));
    EXPECT(refused(&accel, D, 3, 5, &all, RULES, 2, 3) && refused(&accel, D, 3, 5, &all, RULES, 3, 2) && refused(&accel, D, 3, 5, &all, RULES, 0, 3));
    EXPECT(!refused(&accel, D, 3, 5, &all, RULES, 0, 0)); // (a scene without materials: an empty table, nothing read)
    EXPECT(!refused(&accel, D, 3, 5, &all, RULES, 2, 2) && !refused(&accel, D, 3, 5, &all, RULES, 1, 1));
    for (size_t m = 0; m < 3; ++m) {
        std::unique_ptr<lg_path_rule[]> r(new lg_path_rule[3]); // (a heap block of exactly the table's size: a read past it is a report)
        for (uint32_t action = 0; action < 8; ++action) {
            std::memcpy(r.get(), RULES, sizeof RULES);
            r[m].action = action;
            EXPECT(refused(&accel, D, 3, 5, &all, r.get(), 3, 3) == (action > LG_PATH_REFRACT));
        }
        std::memcpy(r.get(), RULES, sizeof RULES);
        r[m].action = KMAX;
        EXPECT(refused(&accel, D, 3, 5, &all, r.get(), 3, 3));
        std::memcpy(r.get(), RULES, sizeof RULES);
        r[m].reserved = 1u;
        EXPECT(refused(&accel, D, 3, 5, &all, r.get(), 3, 3));
        r[m].reserved = 0u;
        r[m].ior = 0.0; r[m].gain = -1.0; // (any f64 is a value, not an error)
        EXPECT(!refused(&accel, D, 3, 5, &all, r.get(), 3, 3));
    }
    for (int normal : {-1, 2, 3, 1 << 30}) EXPECT(refused(&accel, D, 3, 5, &all, RULES, 3, 3, normal));
    EXPECT(!refused(&accel, D, 3, 5, &all, RULES, 3, 3, 1));
    // ---- the NULL rule: every combination of the nine planes; only all NULL is refused
    for (unsigned planes = 0; planes < 512; ++planes) {
        const lg_paths_out o = subset(all, planes);
        EXPECT(refused(&accel, D, 3, 5, &o) == (planes == 0));
        EXPECT(refused(nullptr, D, 3, 5, &o) && refused(&accel, nullptr, 3, 5, &o) && refused(&accel, D, 3, 0, &o));
    }
    // ---- the alignment rule: rays 8; start_medium 4; hits and id 16; point, along, gain and last 8; count, end and medium 4; NULL is not misaligned
    const char *base = reinterpret_cast<const char *>(d);
    EXPECT(!misaligned(D, u, all) && !misaligned(D, nullptr, none) && !misaligned(nullptr, nullptr, all));
    for (int off : {1, 2, 4}) EXPECT(misaligned(base + off, nullptr, all));
    EXPECT(!misaligned(base + 8, nullptr, all));
    for (int off : {1, 2, 3}) EXPECT(misaligned(D, reinterpret_cast<const char *>(u) + off, all));
    EXPECT(!misaligned(D, reinterpret_cast<const char *>(u) + 4, all));
    const size_t want_align[9] = {16, 8, 16, 8, 4, 4, 8, 8, 4};
    for (int k = 0; k < 9; ++k)
        for (int off : {1, 2, 4, 8, 16}) {
            lg_paths_out o = all;
            char *hp = reinterpret_cast<char *>(h) + off, *dp = reinterpret_cast<char *>(d) + off, *up = reinterpret_cast<char *>(u) + off;
            if (k == 0) o.hits = reinterpret_cast<lg_hit *>(hp);
            else if (k == 1) o.point = reinterpret_cast<double *>(dp);
            else if (k == 2) o.id = reinterpret_cast<uint32_t *>(up);
            else if (k == 3) o.along = reinterpret_cast<double *>(dp);
            else if (k == 4) o.count = reinterpret_cast<uint32_t *>(up);
            else if (k == 5) o.end = reinterpret_cast<uint32_t *>(up);
            else if (k == 6) o.gain = reinterpret_cast<double *>(dp);
            else if (k == 7) o.last = reinterpret_cast<double *>(dp);
            else o.medium = reinterpret_cast<uint32_t *>(up);
            EXPECT(misaligned(D, nullptr, o) == ((size_t)off % want_align[k] != 0));
        }
    // ---- staging and placement: every subset of the planes, shapes with partial tiles and more than one vertex
    const size_t shapes[][2] = {{1, 1}, {1, 8}, {63, 2}, {64, 3}, {65, 1}, {129, 8}};
    for (const auto &s : shapes)
        for (unsigned planes = 1; planes < 512; ++planes) run(s[0], (uint32_t)s[1], planes);
    if (failures) { std::fprintf(stderr, "paths_host_check: %d failures\n", failures); return 1; }
    std::printf("paths_host_check: ok\n");
    return 0;
}
