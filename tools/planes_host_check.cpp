// tools/planes_host_check.cpp -- what the queries' host code shares (lasgun_amd/csrc/planes_host.h: the one overflow-checked size, the one
// alignment rule, the two rules over a plane table, and HostStaging, the host-memory half of query.cpp's RoundTrip) in a stand-alone
// program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_planes_host_sanitized.py does).  Every
// target of a placement is a heap block of exactly its size, so a copy past an end is an ASan report; a staging buffer that outlives
// its HostStaging is a leak report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/planes_host_check.cpp -o check && ./check
#include "host_check.h"

using namespace lg;

struct Wide { unsigned char b[96]; }; // as wide as lg_hit, the widest element of a plane
static_assert(sizeof(Wide) == 96 && sizeof(float) == 4 && sizeof(double) == 8, "the element sizes below");

// hold and stage of n elements of T; a block of exactly n elements is the target
template <class T> static void elements(size_t n) {
    std::unique_ptr<unsigned char[]> target(new unsigned char[n * sizeof(T)]);
    for (size_t i = 0; i < n * sizeof(T); ++i) target[i] = 0xEE;
    bool zeroed = true, kept = true, placed = true, prefill = true;
    {
        HostStaging st;
        unsigned char *held = reinterpret_cast<unsigned char *>(st.hold<T>(n));
        unsigned char *staged = reinterpret_cast<unsigned char *>(st.stage(reinterpret_cast<T *>(target.get()), n));
        EXPECT(n == 0 || (held && staged && held != staged));
        for (size_t i = 0; i < n * sizeof(T); ++i) { zeroed = zeroed && held[i] == 0 && staged[i] == 0; held[i] = 0x11; staged[i] = (unsigned char)(i * 5 + 1); }
        for (size_t i = 0; i < n * sizeof(T); ++i) prefill = prefill && target[i] == 0xEE; // nothing arrives before place()
        st.place();
        for (size_t i = 0; i < n * sizeof(T); ++i) { placed = placed && target[i] == (unsigned char)(i * 5 + 1); kept = kept && held[i] == 0x11; } // a held buffer is the form's to place
    }
    EXPECT(zeroed && prefill && placed && kept);
    { // the error path: destroyed without place(), the target stays as it was
        for (size_t i = 0; i < n * sizeof(T); ++i) target[i] = 0xEE;
        HostStaging st;
        unsigned char *staged = reinterpret_cast<unsigned char *>(st.stage(reinterpret_cast<T *>(target.get()), n));
        for (size_t i = 0; i < n * sizeof(T); ++i) staged[i] = 0x22;
    }
    prefill = true;
    for (size_t i = 0; i < n * sizeof(T); ++i) prefill = prefill && target[i] == 0xEE;
    EXPECT(prefill);
}

int main() {
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    static_assert(QUERY_MAX_RAYS == 0xFFFFFFFFull * 64ull, "64-ray tiles counted in 32 bits");
    // ---- HostStaging
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)129}) { elements<unsigned char>(n); elements<float>(n); elements<double>(n); elements<Wide>(n); }
    { HostStaging st; st.place(); } // nothing staged: nothing to do
    { // a NULL host is not staged and not placed
        HostStaging st;
        EXPECT(st.stage((double *)nullptr, 7) == nullptr && st.stage((Wide *)nullptr, 0) == nullptr);
        st.place();
    }
    { // two planes staged in order are placed in order: both aim at one block, and the later one's bytes are what stays where they overlap
        std::unique_ptr<uint32_t[]> target(new uint32_t[4]);
        HostStaging st;
        uint32_t *first = st.stage(target.get(), 4), *second = st.stage(target.get(), 2);
        for (int i = 0; i < 4; ++i) first[i] = 100u + i;
        for (int i = 0; i < 2; ++i) second[i] = 200u + i;
        st.place();
        EXPECT(target[0] == 200u && target[1] == 201u && target[2] == 102u && target[3] == 103u);
        st.place(); // (const: what was recorded is still there)
        EXPECT(target[0] == 200u && target[3] == 103u);
    }
    // ---- checked_bytes
    const size_t EDGE = SIZE_MAX / 96;
    EXPECT(checked_bytes(0, 96, "x") == 0 && checked_bytes(EDGE, 96, "x") == EDGE * 96 && checked_bytes(5, 0, "x") == 0 && checked_bytes(SIZE_MAX, 0, "x") == 0);
    EXPECT(checked_bytes(SIZE_MAX, 1, "x") == SIZE_MAX && checked_bytes(1, SIZE_MAX, "x") == SIZE_MAX);
    EXPECT(throws([&] { (void)checked_bytes(EDGE + 1, 96, "x"); }) && throws([&] { (void)checked_bytes(SIZE_MAX, 2, "x"); }));
    EXPECT(thrown([&] { (void)checked_bytes(EDGE + 1, 96, "a plane of n rows"); }) == "a plane of n rows does not fit the address space");
    // ---- check_alignment: NULL is not misaligned
    alignas(16) static unsigned char raw[64];
    for (size_t align : {(size_t)4, (size_t)8, (size_t)16}) {
        EXPECT(!throws([&] { check_alignment(nullptr, align, "p"); }) && !throws([&] { check_alignment(raw, align, "p"); }));
        for (size_t off : {(size_t)1, (size_t)2, (size_t)4, (size_t)8, (size_t)16}) EXPECT(throws([&] { check_alignment(raw + off, align, "p"); }) == (off % align != 0));
    }
    EXPECT(thrown([&] { check_alignment(raw + 4, 16, "id"); }) == "id is not 16-byte aligned");
    // ---- the two rules over a table
    struct Out { Wide *hits; double *along; uint32_t *count; };
    const auto table_of = [](const Out &out) {
        return [&out](auto &&f) { f(out.hits, 3, 16, "hits"); f(out.along, 3, 8, "along"); f(out.count, 1, 4, "count"); };
    };
    const Out none{nullptr, nullptr, nullptr}, fine{(Wide *)raw, (double *)(raw + 8), (uint32_t *)(raw + 4)};
    EXPECT(thrown([&] { require_any_plane(table_of(none)); }) == "every plane of out is NULL: at least one output");
    for (unsigned planes = 1; planes < 8; ++planes) {
        const Out o{planes & 1u ? fine.hits : nullptr, planes & 2u ? fine.along : nullptr, planes & 4u ? fine.count : nullptr};
        EXPECT(!throws([&] { require_any_plane(table_of(o)); }) && !throws([&] { check_planes_alignment(table_of(o)); }));
    }
    EXPECT(!throws([&] { check_planes_alignment(table_of(none)); }));
    { Out o = fine; o.hits = (Wide *)(raw + 8); EXPECT(thrown([&] { check_planes_alignment(table_of(o)); }) == "hits is not 16-byte aligned"); }
    { Out o = fine; o.along = (double *)(raw + 4); EXPECT(thrown([&] { check_planes_alignment(table_of(o)); }) == "along is not 8-byte aligned"); }
    { Out o = fine; o.count = (uint32_t *)(raw + 2); o.hits = (Wide *)(raw + 1); EXPECT(thrown([&] { check_planes_alignment(table_of(o)); }) == "hits is not 16-byte aligned"); } // the table's order
    // ---- staged_round (host_check.h), as the queries' programs use it: the bytes of each plane, nothing for one not asked for
    for (unsigned planes = 0; planes < 8; ++planes) {
        Out o{planes & 1u ? fine.hits : nullptr, planes & 2u ? fine.along : nullptr, planes & 4u ? fine.count : nullptr};
        const StagedRound r = staged_round([&](auto &&f) { f(o.hits, 3, 16, "hits"); f(o.along, 3, 8, "along"); f(o.count, 1, 4, "count"); });
        EXPECT(r.plane_bytes == (std::vector<size_t>{planes & 1u ? 288u : 0u, planes & 2u ? 24u : 0u, planes & 4u ? 4u : 0u}));
        EXPECT(r.bytes == (planes & 1u ? 288u : 0u) + (planes & 2u ? 24u : 0u) + (planes & 4u ? 4u : 0u));
    }
    if (failures) { std::fprintf(stderr, "planes_host_check: %d failures\n", failures); return 1; }
    std::printf("planes_host_check: ok\n");
    return 0;
}
