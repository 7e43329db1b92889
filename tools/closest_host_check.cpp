// tools/closest_host_check.cpp -- the device-free host code of lg_closest_points* (lasgun_amd/csrc/closest_host.h: the plane table, every
// check and every refusal in its order, the alignment rule, the host form's staging for every subset of the planes, the sphere gate, the
// shrink bound and the stack depth over scenes built here) compiled alone for the CPU, with its own main: nothing of HIP, nothing loaded
// into python.  tests/test_closest_host_sanitized.py builds it under AddressSanitizer and UBSan.
//
// usage: closest_host_check               the self-checks; prints "closest_host_check: ok"
//        closest_host_check IN OUT        IN: chains, each a count d (1 .. 8) then d x 24 doubles (an accel's m, then its minv, column-major
//                                         3 x 4 as Affine holds them), root first; OUT: per chain d doubles: shrink of every accel of it
#include <cmath>
#include <cstdio>
#include <limits>

#include "../lasgun_amd/csrc/closest_host.h"
#include "host_check.h"

using namespace lg;

static const double INF = std::numeric_limits<double>::infinity(), QNAN = std::numeric_limits<double>::quiet_NaN();

static Affine affine_identity() {
    Affine a{};
    for (int c = 0; c < 3; ++c) a.c[c][c] = 1.0;
    return a;
}
static Affine affine_scale(double x, double y, double z) {
    Affine a{};
    a.c[0][0] = x; a.c[1][1] = y; a.c[2][2] = z;
    return a;
}
static Affine affine_rot_z(double deg, double tx) {
    Affine a = affine_identity();
    const double r = deg * 3.14159265358979323846 / 180.0;
    a.c[0][0] = std::cos(r); a.c[0][1] = std::sin(r); a.c[1][0] = -std::sin(r); a.c[1][1] = std::cos(r);
    a.c[3][0] = tx;
    return a;
}

// A scene under construction: accels with their chains, trees, leaf slots
struct Built {
    std::vector<DAccel> accels;
    std::vector<DNode> nodes;
    std::vector<uint32_t> primref;
    std::vector<DLeafRec> soup;
    ClosestScene view() const { return ClosestScene{accels.data(), accels.size(), nodes.data(), nodes.size(), primref.data(), primref.size(), soup.data(), soup.size()}; }
    uint32_t accel(int32_t parent, const Affine &m, const Affine &minv) {
        DAccel a{};
        a.m = m; a.minv = minv; a.parent = parent; a.material = -1;
        const uint32_t id = (uint32_t)accels.size();
        if (parent < 0) { a.nchain = 1; a.chain[0] = id; }
        else {
            const DAccel &p = accels[(size_t)parent];
            a.nchain = p.nchain + 1;
            for (uint32_t i = 0; i < p.nchain; ++i) a.chain[i] = p.chain[i];
            a.chain[p.nchain] = id;
        }
        a.node_base = (uint32_t)nodes.size(); a.prim_base = (uint32_t)primref.size();
        accels.push_back(a);
        return id;
    }
    static DNode box(uint32_t link, uint32_t meta) {
        DNode n{};
        for (int k = 0; k < 3; ++k) { n.bmin[k] = -1.0; n.bmax[k] = 1.0; }
        n.link = link; n.meta = meta; n.parent = NO_HIT;
        return n;
    }
    // a slot: a sphere of radius 0.5 at the origin, a unit box, a triangle, or a nested accel
    uint32_t slot(uint32_t kind, uint32_t idx) {
        DLeafRec r{};
        if (kind == PK_SPHERE) { const double d[4] = {0.0, 0.0, 0.0, 0.5}; std::memcpy(r.w, d, sizeof d); }
        else if (kind == PK_CUBOID) { const double d[6] = {-1.0, -1.0, -1.0, 1.0, 1.0, 1.0}; std::memcpy(r.w, d, sizeof d); }
        else if (kind == PK_TRIANGLE) { const float f[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}; std::memcpy(r.w, f, sizeof f); }
        primref.push_back((kind << 30) | idx);
        soup.push_back(r);
        return (uint32_t)primref.size() - 1u;
    }
    // the tree of the accel made last: `interiors` interior nodes in a left-deep comb, every leaf holding one primitive of `kind`
    void comb(uint32_t interiors, uint32_t kind) {
        const uint32_t base = accels.back().prim_base;
        for (uint32_t i = 0; i < interiors; ++i) nodes.push_back(box(interiors + 1u + i, 0u));
        for (uint32_t i = 0; i <= interiors; ++i) nodes.push_back(box(slot(kind, 0u) - base, NODE_LEAF | 1u));
    }
};

static void check_the_call() {
    int accel = 0;
    const double D[3] = {0, 0, 0};
    double d = 0;
    uint32_t id[4] = {0, 0, 0, 0};
    lg_closest_out all{&d, &d, id}, none{nullptr, nullptr, nullptr};
    EXPECT(!throws([&] { check_closest(&accel, D, 1, INF, &all); }));
    EXPECT(!throws([&] { check_closest(&accel, D, 1, 0.0, &all); }));
    // every refusal, in its order: each call has every LATER fault too, and names the first
    EXPECT(thrown([&] { check_closest(nullptr, nullptr, (size_t)-1, -1.0, nullptr); }) == "accel is NULL");
    EXPECT(thrown([&] { check_closest(&accel, nullptr, (size_t)-1, -1.0, nullptr); }) == "points is NULL");
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)-1, -1.0, nullptr); }) == "out is NULL");
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)-1, -1.0, &none); }).find("every plane of out is NULL") == 0);
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)-1, -1.0, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)-1, QNAN, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)-1, -INF, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)-1, INF, &all); }) == "too many points in one query");
    EXPECT(thrown([&] { check_closest(&accel, D, (size_t)(QUERY_MAX_RAYS + 1), 1.0, &all); }) == "too many points in one query");
    EXPECT(!throws([&] { check_closest(&accel, D, (size_t)QUERY_MAX_RAYS, 1.0, &all); }));
    for (int planes = 1; planes < 8; ++planes) { // each plane alone is enough
        lg_closest_out o{(planes & 1) ? &d : nullptr, (planes & 2) ? &d : nullptr, (planes & 4) ? id : nullptr};
        EXPECT(!throws([&] { check_closest(&accel, D, 5, 2.0, &o); }));
    }
    // alignment: points, distance and point 8 bytes, id 16; NULL is not misaligned
    alignas(16) unsigned char mem[64];
    auto at = [&](size_t off) { return (void *)(mem + off); };
    EXPECT(!throws([&] { check_closest_alignment((double *)at(8), lg_closest_out{(double *)at(8), (double *)at(24), (uint32_t *)at(16)}); }));
    EXPECT(!throws([&] { check_closest_alignment((double *)at(8), none); }));
    EXPECT(thrown([&] { check_closest_alignment((double *)at(4), all); }) == "points is not 8-byte aligned");
    EXPECT(thrown([&] { check_closest_alignment(D, lg_closest_out{(double *)at(4), nullptr, nullptr}); }) == "distance is not 8-byte aligned");
    EXPECT(thrown([&] { check_closest_alignment(D, lg_closest_out{nullptr, (double *)at(12), nullptr}); }) == "point is not 8-byte aligned");
    EXPECT(thrown([&] { check_closest_alignment(D, lg_closest_out{nullptr, nullptr, (uint32_t *)at(8)}); }) == "id is not 16-byte aligned");
    // the host form's staging, every subset of the planes, n up to a few tiles
    for (size_t n : {(size_t)1, (size_t)63, (size_t)65, (size_t)4097})
        for (int planes = 1; planes < 8; ++planes) {
            lg_closest_out o{(planes & 1) ? (double *)ASKED : nullptr, (planes & 2) ? (double *)ASKED : nullptr, (planes & 4) ? (uint32_t *)ASKED : nullptr};
            const StagedRound r = staged_round([&](auto &&f) { closest_planes(o, n, f); });
            EXPECT(r.plane_bytes.size() == 3);
            EXPECT(r.plane_bytes[0] == ((planes & 1) ? n * 8 : 0) && r.plane_bytes[1] == ((planes & 2) ? n * 24 : 0) && r.plane_bytes[2] == ((planes & 4) ? n * 16 : 0));
        }
}

static void check_the_tables() {
    const Affine I = affine_identity();
    {   // one accel, one leaf, one sphere: nothing is ever pushed
        Built b;
        b.accel(-1, I, I);
        b.comb(0, PK_SPHERE);
        const ClosestTables t = closest_tables(b.view());
        EXPECT(t.depth == 1u && t.refused == -1 && t.accel.size() == 1);
        EXPECT(t.accel[0].shrink > 0.999 && t.accel[0].shrink <= 1.0 && t.accel[0].delta >= 0.0 && t.accel[0].omega > 0.0 && t.qmax > 0.0);
    }
    for (uint32_t k : {1u, 2u, 7u, 40u, 70u}) { // a comb of k interior nodes: one pushed sibling a level
        Built b;
        b.accel(-1, I, I);
        b.comb(k, PK_TRIANGLE);
        EXPECT(closest_tables(b.view()).depth == k + 1u);
        EXPECT((closest_tables(b.view()).depth > CLOSEST_MAX_DEPTH) == (k + 1u > CLOSEST_MAX_DEPTH));
    }
    {   // a root leaf with two nested accels, each a comb of 3: both pushed, the first walked with nothing of the leaf below it
        Built b;
        b.accel(-1, I, I);
        b.nodes.push_back(Built::box(0u, NODE_LEAF | 2u));
        b.slot(PK_ACCEL, 1u);
        b.slot(PK_ACCEL, 2u);
        for (int c = 0; c < 2; ++c) { b.accel(0, I, I); b.comb(3, PK_CUBOID); }
        const ClosestTables t = closest_tables(b.view());
        EXPECT(t.depth >= 3u + 2u && t.depth <= 3u + 2u + 2u); // (the rule is allowed one entry of slack a level, never less than the walk needs)
    }
    {   // the gate: a sphere under a uniform scale and a rotation passes, under (1.2, 0.8, 1.0) it is refused by instance; boxes and meshes pass
        Built b;
        b.accel(-1, affine_rot_z(30.0, 0.5), affine_rot_z(-30.0, 0.0));
        b.nodes.push_back(Built::box(0u, NODE_LEAF | 3u));
        b.slot(PK_ACCEL, 1u); b.slot(PK_ACCEL, 2u); b.slot(PK_ACCEL, 3u);
        b.accel(0, affine_scale(1.2, 1.2, 1.2), affine_scale(1 / 1.2, 1 / 1.2, 1 / 1.2)); b.comb(1, PK_SPHERE);
        b.accel(0, affine_scale(1.2, 0.8, 1.0), affine_scale(1 / 1.2, 1 / 0.8, 1.0)); b.comb(1, PK_CUBOID);
        b.accel(0, affine_scale(1.2, 0.8, 1.0), affine_scale(1 / 1.2, 1 / 0.8, 1.0)); b.comb(1, PK_TRIANGLE);
        double shrink[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
        EXPECT(closest_gate(b.view(), shrink, 8) == -1);
        EXPECT(shrink[0] > 0.99 && shrink[0] <= 1.0 && shrink[1] > 1.19 && shrink[1] <= 1.2 && shrink[2] > 0.4 && shrink[2] <= 0.8 && shrink[4] == -1);
        EXPECT(closest_gate(b.view(), shrink, 2) == -1 && closest_gate(b.view(), nullptr, 0) == -1);
        b.slot(PK_SPHERE, 0u); // ... and a sphere in accel 3
        b.nodes.back() = Built::box((uint32_t)b.primref.size() - 1u - b.accels[3].prim_base, NODE_LEAF | 1u);
        EXPECT(closest_gate(b.view(), nullptr, 0) == 3);
        b.accels[2].m = affine_scale(0.0, 1.0, 1.0); // a singular chain proves nothing
        EXPECT(closest_tables(b.view()).accel[2].shrink == 0.0);
    }
    {   // a triangle without altitude (collinear, distinct vertices): the walk never prunes
        Built b;
        b.accel(-1, I, I);
        b.comb(0, PK_TRIANGLE);
        const float f[9] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 2.f, 2.f, 2.f};
        std::memcpy(b.soup[0].w, f, sizeof f);
        EXPECT(closest_tables(b.view()).qmax == -1.0);
        const float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 2.f, 2.f, 2.f}; // a repeated vertex is harmless
        std::memcpy(b.soup[0].w, g, sizeof g);
        EXPECT(closest_tables(b.view()).qmax > 0.0);
    }
    {   // a sphere below the magnitude range: the walk never prunes (squares of such distances underflow)
        Built b;
        b.accel(-1, I, I);
        b.comb(1, PK_SPHERE);
        EXPECT(closest_tables(b.view()).qmax > 0.0);
        const double tiny[4] = {0.0, 0.0, 0.0, 0x1p-101};
        std::memcpy(b.soup[0].w, tiny, sizeof tiny);
        EXPECT(closest_tables(b.view()).qmax == -1.0);
        b.accels[0].m = affine_scale(0x1p-60, 0x1p-60, 0x1p-60); // ... and one taken below it by its chain
        b.accels[0].minv = affine_scale(0x1p60, 0x1p60, 0x1p60);
        const double small[4] = {0.0, 0.0, 0.0, 0x1p-50};
        std::memcpy(b.soup[0].w, small, sizeof small);
        std::memcpy(b.soup[1].w, small, sizeof small);
        EXPECT(closest_tables(b.view()).qmax == -1.0);
    }
    {   // tables that name something out of range are refused, nothing is read beyond them
        Built b;
        b.accel(-1, I, I);
        b.comb(2, PK_SPHERE);
        Built c = b; c.nodes[0].link = 99u;
        EXPECT(throws([&] { closest_tables(c.view()); }));
        c = b; c.nodes[2].link = 7u;
        EXPECT(throws([&] { closest_tables(c.view()); }));
        c = b; c.nodes[0].link = 0u; // a tree that does not end
        EXPECT(throws([&] { closest_tables(c.view()); }));
        c = b; c.accels[0].nchain = 9u;
        EXPECT(throws([&] { closest_tables(c.view()); }));
        c = b; c.primref[0] = (PK_ACCEL << 30) | 5u;
        EXPECT(throws([&] { closest_tables(c.view()); }));
        c = b; c.soup.pop_back();
        EXPECT(throws([&] { closest_tables(c.view()); }));
    }
}

static int chains(const char *in_path, const char *out_path) {
    std::FILE *in = std::fopen(in_path, "rb");
    if (!in) { std::fprintf(stderr, "closest_host_check: cannot read %s\n", in_path); return 2; }
    std::vector<double> out;
    double d;
    size_t count = 0;
    while (std::fread(&d, sizeof d, 1, in) == 1) {
        const int depth = (int)d;
        if (depth < 1 || depth > MAX_CHAIN) { std::fprintf(stderr, "closest_host_check: a chain of %d accels\n", depth); return 2; }
        Built b;
        for (int k = 0; k < depth; ++k) {
            double m[24];
            if (std::fread(m, sizeof m, 1, in) != 1) { std::fprintf(stderr, "closest_host_check: a short chain\n"); return 2; }
            Affine a, ai;
            std::memcpy(a.c, m, 12 * sizeof(double));
            std::memcpy(ai.c, m + 12, 12 * sizeof(double));
            b.accel(k - 1, a, ai);
            if (k + 1 < depth) { b.nodes.push_back(Built::box(0u, NODE_LEAF | 1u)); b.slot(PK_ACCEL, (uint32_t)k + 1u); }
            else b.comb(0, PK_CUBOID);
        }
        std::vector<double> shrink((size_t)depth, -1.0);
        (void)closest_gate(b.view(), shrink.data(), depth);
        out.insert(out.end(), shrink.begin(), shrink.end());
        ++count;
    }
    std::fclose(in);
    std::FILE *f = std::fopen(out_path, "wb");
    if (!f || (!out.empty() && std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) || std::fclose(f) != 0) {
        std::fprintf(stderr, "closest_host_check: cannot write %s\n", out_path);
        return 2;
    }
    std::printf("closest_host_check: ok, %zu chains\n", count);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3) return chains(argv[1], argv[2]);
    check_the_call();
    check_the_tables();
    if (failures) { std::fprintf(stderr, "closest_host_check: %d failures\n", failures); return 1; }
    std::printf("closest_host_check: ok\n");
    return 0;
}
