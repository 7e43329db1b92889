// tools/packet_gate_check.cpp -- the device-free gate of the packet walk (lasgun_amd/csrc/packet_host.h: which scene graphs the packet form
// may take, how deep its stack gets) in a stand-alone program with its own main, meant to be built with -fsanitize=address,undefined and
// run on the CPU (tests/test_packet_walk_predicate.py does).  It builds small scene-graph tables by hand -- a root tree over spheres, a mesh
// straight in the root, a group of spheres, a group with its lone mesh -- checks that the gate admits them, then breaks ONE condition at
// a time and checks that exactly that refusal comes back; random trees pin packet_stack_need to a recursive restatement.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/packet_gate_check.cpp -o check && ./check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../lasgun_amd/csrc/packet_host.h"

using namespace lg;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Tables {
    std::vector<DAccel> accels;
    std::vector<DNode> nodes;
    std::vector<uint32_t> primref;
    uint32_t stack_depth = 8;
    PacketRefusal gate() const { return packet_scene_gate(accels.data(), accels.size(), nodes.data(), nodes.size(), primref.data(), primref.size(), stack_depth); }
};

static DNode leaf(uint32_t first, uint32_t count) { DNode n{}; n.link = first; n.meta = NODE_LEAF | count; n.parent = NO_HIT; return n; }
static DNode interior(uint32_t second, uint32_t axis) { DNode n{}; n.link = second; n.meta = axis; n.parent = NO_HIT; return n; }
static DAccel accel(uint32_t node_base, uint32_t prim_base, int32_t parent, uint32_t flags) {
    DAccel a{};
    a.node_base = node_base; a.prim_base = prim_base; a.parent = parent; a.flags = flags; a.lone = NO_HIT;
    return a;
}
static uint32_t ref(uint32_t kind, uint32_t idx) { return kind << 30 | idx; }

// accel 0: the root, three nodes (an interior node over two leaves): leaf A = {sphere, accel 1, accel 2}, leaf B = {cuboid, accel 3}
// accel 1: a mesh straight in the root, one leaf of two triangles;  accel 2: a group, one leaf {sphere, cuboid}
// accel 3: a group whose one slot is accel 4, its lone mesh (one leaf of two triangles)
static Tables good() {
    Tables t;
    t.nodes = {interior(2, 0), leaf(0, 3), leaf(3, 2), /* 3: accel 1 */ leaf(0, 2), /* 4: accel 2 */ leaf(0, 2), /* 5: accel 3 */ leaf(0, 1), /* 6: accel 4 */ leaf(0, 2)};
    t.primref = {ref(PK_SPHERE, 0), ref(PK_ACCEL, 1), ref(PK_ACCEL, 2), ref(PK_CUBOID, 0), ref(PK_ACCEL, 3),
                 /* 5 */ ref(PK_TRIANGLE, 0), ref(PK_TRIANGLE, 1), /* 7 */ ref(PK_SPHERE, 1), ref(PK_CUBOID, 1), /* 9 */ ref(PK_ACCEL, 4),
                 /* 10 */ ref(PK_TRIANGLE, 2), ref(PK_TRIANGLE, 3)};
    t.accels = {accel(0, 0, -1, 0), accel(3, 5, 0, AF_MESH | AF_IDENTITY), accel(4, 7, 0, 0), accel(5, 9, 0, 0), accel(6, 10, 3, AF_MESH | AF_IDENTITY)};
    t.accels[3].lone = 4;
    return t;
}

static int need_restated(const std::vector<DNode> &n, size_t i) { // the longest chain of interior nodes from node i
    if (n[i].meta & NODE_LEAF) return 0;
    const int a = need_restated(n, i + 1), b = need_restated(n, n[i].link);
    return 1 + (a > b ? a : b);
}
// a random tree in the flattened layout: first child behind its parent, second child at `link`
static void grow(std::vector<DNode> &n, std::mt19937 &rng, int depth) {
    const size_t me = n.size();
    if (depth >= 40 || n.size() > 4000 || rng() % 100 >= 48) { n.push_back(leaf(0, 1)); return; } // (just subcritical: mostly small trees, some deep ones)
    n.push_back(interior(0, rng() % 3));
    grow(n, rng, depth + 1);
    n[me].link = (uint32_t)n.size();
    grow(n, rng, depth + 1);
}

int main() {
    CHECK(packet_launch_gate(true, true, true) == PACKET_OK);
    CHECK(packet_launch_gate(false, true, true) == PACKET_NO_PAIRS);
    CHECK(packet_launch_gate(true, false, true) == PACKET_NOT_LEVEL0);
    CHECK(packet_launch_gate(true, true, false) == PACKET_SWITCH_OFF);

    CHECK(good().gate() == PACKET_OK);
    { Tables t = good(); t.accels[0].flags |= AF_MESH; CHECK(t.gate() == PACKET_ROOT_MESH); }
    { Tables t = good(); t.stack_depth = 0; CHECK(t.gate() == PACKET_STACK); }
    { Tables t = good(); t.stack_depth = 1; CHECK(t.gate() == PACKET_OK); }
    for (size_t a = 1; a < 5; ++a) { // any nested tree with an interior node at its root
        Tables t = good();
        t.nodes[t.accels[a].node_base] = interior(t.accels[a].node_base + 1u, 1);
        CHECK(t.gate() == PACKET_NESTED_TREE);
    }
    { Tables t = good(); t.accels[2].parent = 3; CHECK(t.gate() == PACKET_NESTED_DEEP); }                 // a group inside a group
    { Tables t = good(); t.accels[3].lone = NO_HIT; CHECK(t.gate() != PACKET_OK); }                        // a mesh inside a group that is not its lone mesh
    { Tables t = good(); t.accels[4].flags &= ~(uint32_t)AF_MESH; CHECK(t.gate() == PACKET_NESTED_DEEP); } // ... whose "lone mesh" is a group
    { Tables t = good(); t.primref[8] = ref(PK_ACCEL, 1); CHECK(t.gate() == PACKET_NESTED_SLOT); }         // a group's leaf holds another accel
    { Tables t = good(); t.primref[8] = ref(PK_TRIANGLE, 0); CHECK(t.gate() == PACKET_NESTED_SLOT); }      // ... or a triangle
    { Tables t = good(); t.nodes[5] = leaf(0, 2); CHECK(t.gate() == PACKET_NESTED_SLOT); }                 // a lone group with a second slot
    { Tables t = good(); t.primref[9] = ref(PK_ACCEL, 1); CHECK(t.gate() == PACKET_NESTED_SLOT); }         // ... whose slot is another accel
    { Tables t = good(); t.accels[1].lone = 4; CHECK(t.gate() == PACKET_NESTED_SLOT); }                    // a mesh with a lone mesh
    // tables that do not describe a scene graph: refused, never read outside
    { Tables t = good(); t.accels[2].node_base = 99; CHECK(t.gate() == PACKET_MALFORMED); }
    { Tables t = good(); t.accels[2].parent = 17; CHECK(t.gate() == PACKET_MALFORMED); }
    { Tables t = good(); t.accels[2].prim_base = 11; CHECK(t.gate() == PACKET_MALFORMED); }
    { Tables t = good(); t.nodes[0].link = 1; CHECK(t.gate() == PACKET_MALFORMED); }
    { Tables t = good(); t.nodes[0].link = 77; CHECK(t.gate() == PACKET_MALFORMED); }
    { Tables t; CHECK(t.gate() == PACKET_MALFORMED); }

    std::mt19937 rng(20240521u);
    for (int k = 0; k < 2000; ++k) {
        std::vector<DNode> n;
        grow(n, rng, 0);
        const int want = need_restated(n, 0);
        CHECK(packet_stack_need(n.data(), n.size()) == want);
        Tables t;
        t.nodes = n; t.accels = {accel(0, 0, -1, 0)}; t.primref = {ref(PK_SPHERE, 0)};
        t.stack_depth = (uint32_t)want;
        CHECK(t.gate() == PACKET_OK);
        if (want > 0) { t.stack_depth = (uint32_t)want - 1u; CHECK(t.gate() == PACKET_STACK); }
    }
    CHECK(packet_stack_need(nullptr, 0) == -1);

    if (failures) { std::fprintf(stderr, "packet_gate_check: %d failures\n", failures); return 1; }
    std::printf("packet_gate_check: ok\n");
    return 0;
}
