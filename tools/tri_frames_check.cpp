// tools/tri_frames_check.cpp -- the device-free part of the frame table of flat triangles (lasgun_amd/csrc/tri_frames_host.h: which accels
// get records, where they start, how large the table is, the build kernel's list) in a stand-alone program with its own main, meant to be
// built with -fsanitize=address,undefined and run on the CPU (tests/test_tri_frames_gate.py does).  One accel passes; every refusing
// condition alone flips it, with its own reason; the caps hold at their last admitted value and refuse at the next; the list is written
// into a heap block of exactly `records` entries and the table's indices into one of exactly tri_frames_bytes(records) bytes, so a write
// or an index beyond either is the sanitizer's to report; plans that do not add up are refused before anything is written.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/tri_frames_check.cpp -o check && ./check
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../lasgun_amd/csrc/tri_frames_host.h"

using namespace lg;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// a wall of the Cornell box: an instance of a two-triangle mesh without normals and without uv
static TriFramesAccel wall() { return TriFramesAccel{AF_MESH, 0u, 2u}; }

// plan, list and table of `accels`, each in a heap block of exactly its stated size: every record touched through the table's own indexing
static uint32_t run(const std::vector<TriFramesAccel> &accels, size_t n_tris, std::vector<uint32_t> &base) {
    base.assign(accels.size(), 0x12345678u);
    const uint32_t records = tri_frames_plan(accels.data(), accels.size(), n_tris, base.data());
    CHECK(records <= TRI_FRAMES_MAX_RECORDS);
    CHECK(tri_frames_plan_ok(accels.data(), accels.size(), n_tris, base.data(), records));
    std::unique_ptr<DTriFrameJob[]> jobs(new DTriFrameJob[records]); // exactly `records` entries
    CHECK(tri_frames_jobs(accels.data(), accels.size(), n_tris, base.data(), records, jobs.get()));
    std::unique_ptr<unsigned char[]> table(new unsigned char[tri_frames_bytes(records)]); // exactly the stated size
    std::memset(table.get(), 0, tri_frames_bytes(records));
    size_t seen = 0;
    for (size_t a = 0; a < accels.size(); ++a) {
        if (base[a] == NO_HIT) continue;
        CHECK(tri_frames_accel_gate(accels[a], n_tris) == TRI_FRAMES_OK);
        for (uint32_t k = 0; k < accels[a].faces; ++k) {
            const uint32_t idx = accels[a].tri_base + k;              // a hit's triangle index
            const size_t r = (size_t)base[a] + (idx - accels[a].tri_base); // the reader's expression (shade.h, shade_frame_tri)
            CHECK(r < records);
            CHECK(jobs[r].accel == (uint32_t)a && jobs[r].tri == idx);
            CHECK((size_t)jobs[r].tri < n_tris);
            DTriFrame f;
            std::memcpy(&f, table.get() + r * TRI_FRAME_BYTES, sizeof f); // the whole record lies inside the block
            CHECK(f.pad == 0u);
            table[r * TRI_FRAME_BYTES + TRI_FRAME_BYTES - 1] = 1u;        // ... to its last byte; and no record is visited twice
            ++seen;
        }
    }
    CHECK(seen == records);
    for (uint32_t r = 0; r < records; ++r) CHECK(table[(size_t)r * TRI_FRAME_BYTES + TRI_FRAME_BYTES - 1] == 1u);
    return records;
}

int main() {
    const size_t N = 1u << 20; // triangles in the tables
    // ---- one accel: every refusing condition alone
    CHECK(tri_frames_accel_gate(wall(), N) == TRI_FRAMES_OK);
    { TriFramesAccel A = wall(); A.flags = 0u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_NOT_MESH); }
    { TriFramesAccel A = wall(); A.flags |= AF_HAS_N; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_HAS_NORMALS); }
    { TriFramesAccel A = wall(); A.flags |= AF_HAS_UV | AF_SWAP_BACKFACE | AF_IDENTITY; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_OK); } // (uv, a backface swap, an identity: all in the record)
    { TriFramesAccel A = wall(); A.faces = 0u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_EMPTY); }
    { TriFramesAccel A = wall(); A.faces = TRI_FRAMES_MAX_INSTANCE; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_OK); }
    { TriFramesAccel A = wall(); A.faces = TRI_FRAMES_MAX_INSTANCE + 1u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_INSTANCE_CAP); }
    { TriFramesAccel A = wall(); A.faces = ~0u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_INSTANCE_CAP); }
    { TriFramesAccel A = wall(); A.tri_base = (uint32_t)N - 2u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_OK); }
    { TriFramesAccel A = wall(); A.tri_base = (uint32_t)N - 1u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_MALFORMED); }
    { TriFramesAccel A = wall(); A.tri_base = (uint32_t)N; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_MALFORMED); }
    { TriFramesAccel A = wall(); A.tri_base = ~0u; CHECK(tri_frames_accel_gate(A, N) == TRI_FRAMES_MALFORMED); } // (no 32-bit wrap)
    { TriFramesAccel A = wall(); CHECK(tri_frames_accel_gate(A, 0u) == TRI_FRAMES_MALFORMED); }
    // every combination of the four conditions: only the one asking passes
    int passed = 0;
    for (unsigned bits = 0; bits < 16u; ++bits) {
        TriFramesAccel A = wall();
        if (bits & 1u) A.flags &= ~(uint32_t)AF_MESH;
        if (bits & 2u) A.flags |= AF_HAS_N;
        if (bits & 4u) A.faces = TRI_FRAMES_MAX_INSTANCE + 1u;
        if (bits & 8u) A.tri_base = (uint32_t)N - 1u;
        CHECK((tri_frames_accel_gate(A, N) == TRI_FRAMES_OK) == (bits == 0u));
        passed += tri_frames_accel_gate(A, N) == TRI_FRAMES_OK ? 1 : 0;
    }
    CHECK(passed == 1);

    std::vector<uint32_t> base;
    // ---- the headline: a root group, five walls that are instances of one mesh, nothing else with triangles
    {
        std::vector<TriFramesAccel> s{{0u, 0u, 0u}};
        for (int i = 0; i < 5; ++i) s.push_back(wall());
        CHECK(run(s, 2u, base) == 10u);
        CHECK(base[0] == NO_HIT);
        for (uint32_t i = 0; i < 5u; ++i) CHECK(base[1 + i] == 2u * i);
    }
    // ---- refused accels between admitted ones leave no gap
    {
        std::vector<TriFramesAccel> s{wall(), {AF_MESH | AF_HAS_N, 2u, 7u}, {AF_MESH, 9u, TRI_FRAMES_MAX_INSTANCE + 1u}, {AF_MESH | AF_HAS_UV, 2000u, 3u}, {0u, 0u, 0u}};
        CHECK(run(s, N, base) == 5u);
        CHECK(base[0] == 0u && base[1] == NO_HIT && base[2] == NO_HIT && base[3] == 2u && base[4] == NO_HIT);
    }
    // ---- the accel's cap: 4,096 records are a table, 4,097 are none at all
    {
        std::vector<TriFramesAccel> s(4, TriFramesAccel{AF_MESH, 0u, TRI_FRAMES_MAX_INSTANCE});
        CHECK(run(s, N, base) == TRI_FRAMES_MAX_RECORDS);
        s.push_back(TriFramesAccel{AF_MESH, 5u, 1u});
        CHECK(run(s, N, base) == 0u);
        for (uint32_t b : base) CHECK(b == NO_HIT);
        s.back().flags |= AF_HAS_N; // (the one too many does not count once it is refused for itself)
        CHECK(run(s, N, base) == TRI_FRAMES_MAX_RECORDS);
    }
    // ---- many instances far beyond the cap: the running total neither wraps nor keeps a base
    {
        std::vector<TriFramesAccel> s(5000000, TriFramesAccel{AF_MESH, 0u, TRI_FRAMES_MAX_INSTANCE}); // 5.12e9 records asked for
        CHECK(run(s, N, base) == 0u);
    }
    // ---- nothing at all
    {
        std::vector<TriFramesAccel> s;
        CHECK(run(s, 0u, base) == 0u);
    }
    // ---- plans that do not add up are refused, and the list is not touched
    {
        std::vector<TriFramesAccel> s{wall(), wall()};
        const uint32_t records = run(s, N, base);
        CHECK(records == 4u);
        std::unique_ptr<DTriFrameJob[]> jobs(new DTriFrameJob[records]);
        for (uint32_t r = 0; r < records; ++r) jobs[r] = DTriFrameJob{77u, 77u};
        auto refused = [&](std::vector<TriFramesAccel> t, std::vector<uint32_t> b, uint32_t n, size_t n_tris) {
            CHECK(!tri_frames_plan_ok(t.data(), t.size(), n_tris, b.data(), n));
            CHECK(!tri_frames_jobs(t.data(), t.size(), n_tris, b.data(), n, jobs.get()));
            for (uint32_t r = 0; r < records; ++r) CHECK(jobs[r].accel == 77u && jobs[r].tri == 77u);
        };
        refused(s, {0u, 2u}, 3u, N);                 // a table one record short
        refused(s, {0u, 2u}, 5u, N);                 // ... one too long
        refused(s, {0u, 3u}, 4u, N);                 // a gap
        refused(s, {0u, 1u}, 4u, N);                 // an overlap
        refused(s, {2u, 0u}, 4u, N);                 // out of order
        refused(s, {1u, 3u}, 4u, N);                 // not from record 0
        refused(s, {0u, 2u}, 4u, 1u);                // triangles the tables do not hold
        refused(s, {0u, 0xFFFFFFF0u}, 4u, N);        // a base near 2^32
        { std::vector<TriFramesAccel> t = s; t[1].faces = 3u; refused(t, {0u, 2u}, 4u, N); }               // a block past the end
        { std::vector<TriFramesAccel> t = s; t[1].flags |= AF_HAS_N; refused(t, {0u, 2u}, 4u, N); }        // a base for an accel its own gate refuses
        { std::vector<TriFramesAccel> t = s; t[1].faces = TRI_FRAMES_MAX_INSTANCE + 1u; refused(t, {0u, 2u}, 1027u, N); }
        refused(s, {0u, 2u}, TRI_FRAMES_MAX_RECORDS + 1u, N); // beyond the cap
    }
    // ---- the launch's part: each condition alone
    CHECK(tri_frames_launch_gate(true, true, 10u));
    CHECK(!tri_frames_launch_gate(false, true, 10u));
    CHECK(!tri_frames_launch_gate(true, false, 10u));
    CHECK(!tri_frames_launch_gate(true, true, 0u));
    CHECK(tri_frames_launch_gate(true, true, TRI_FRAMES_MAX_RECORDS));
    CHECK(!tri_frames_launch_gate(true, true, TRI_FRAMES_MAX_RECORDS + 1u));

    if (failures) { std::fprintf(stderr, "tri_frames_check: %d failures\n", failures); return 1; }
    std::printf("tri_frames_check: ok\n");
    return 0;
}
