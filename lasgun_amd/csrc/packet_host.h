// lasgun_amd/csrc/packet_host.h -- the gate of the packet form of the plain exact walk (packet.h), the part that touches no
// device: which scene graphs the packet walk may take, and how deep its per-wave stack gets.  Index arithmetic over caller-supplied
// tables, kept free of HIP: tools/packet_gate_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, launch.cpp calls it.
//
// The packet walk keeps ONE cursor and ONE stack per wave for the root accel's tree and handles a nested accel in place, without a stack:
// that is only a walk of the nested accel when its tree is a single root record.  The shapes it takes (packet.h, packet_nested):
//   a mesh accel entered from the root whose node 0 is a leaf;
//   a group entered from the root whose node 0 is a leaf of spheres and cuboids;
//   a group entered from the root whose node 0 is a leaf of ONE slot, its lone mesh (DAccel::lone), whose node 0 is a leaf.
// Anything else -- a nested tree with interior nodes, a group inside a group, a mesh that is the root -- keeps the per-lane walk.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dscene.h"

namespace lg {

enum PacketRefusal : int {
    PACKET_OK = 0,
    PACKET_NO_PAIRS = 1,      // the launch would not take the pair form (wf_takes_pairs)
    PACKET_NOT_LEVEL0 = 2,    // not the level-0 closest launch of the level-by-level pipeline for the scene's own camera
    PACKET_SWITCH_OFF = 3,    // lg_accel_set_packet_walk(0) / LASGUN_PACKET_WALK=0
    PACKET_MALFORMED = 4,     // tables that do not describe a scene graph (an index outside its table)
    PACKET_ROOT_MESH = 5,     // the root accel is a mesh
    PACKET_NESTED_TREE = 6,   // a nested accel whose node 0 is an interior node
    PACKET_NESTED_DEEP = 7,   // a nested accel that is entered from another nested accel (and is not that one's lone mesh)
    PACKET_NESTED_SLOT = 8,   // a nested group's leaf holds an accel that is not its lone mesh, or a triangle
    PACKET_STACK = 9,         // the root tree is deeper than the wave's stack
};

// the launch's own conditions
inline PacketRefusal packet_launch_gate(bool takes_pairs, bool level0_of_pipeline, bool switched_on) {
    if (!takes_pairs) return PACKET_NO_PAIRS;
    if (!level0_of_pipeline) return PACKET_NOT_LEVEL0;
    if (!switched_on) return PACKET_SWITCH_OFF;
    return PACKET_OK;
}

// The deepest the packet's stack gets over the tree nodes[0 .. n) (first child of interior node i = i + 1, second = nodes[i].link): one far
// child can be pending per interior node of the current path, so the longest chain of interior nodes from node 0.  -1: a malformed tree.
inline int packet_stack_need(const DNode *nodes, size_t n) {
    if (n == 0) return -1;
    // (children lie behind their parent: one pass in index order sees every node after its parent)
    int worst = 0;
    // depth[i] = interior nodes above node i; kept in the caller-free way: a small explicit stack of (node, depth)
    struct Item { size_t node; int depth; };
    Item todo[130];
    int top = 0;
    todo[top++] = Item{0, 0};
    size_t visited = 0;
    while (top > 0) {
        const Item it = todo[--top];
        if (it.node >= n || ++visited > n) return -1;
        if (nodes[it.node].meta & NODE_LEAF) continue;
        const int below = it.depth + 1;
        if (below > worst) worst = below;
        if (below > 64 || top + 2 > 130) return -1; // (the reference panics beyond 64 per level, bvh.rs:497)
        const size_t c0 = it.node + 1, c1 = nodes[it.node].link;
        if (c1 <= c0) return -1;
        todo[top++] = Item{c1, below};
        todo[top++] = Item{c0, below};
    }
    return worst;
}

// The scene graph's part of the gate.  accels[0 .. n_accels), nodes[0 .. n_nodes) (an accel's tree starts at its node_base), primref[0 ..
// n_prims) (an accel's leaves index it from its prim_base), stack_depth = the entries a wave's slice of the LDS stacks holds.
inline PacketRefusal packet_scene_gate(const DAccel *accels, size_t n_accels, const DNode *nodes, size_t n_nodes, const uint32_t *primref,
                                       size_t n_prims, uint32_t stack_depth) {
    if (n_accels == 0 || n_nodes == 0) return PACKET_MALFORMED;
    if (accels[0].node_base >= n_nodes) return PACKET_MALFORMED;
    if (accels[0].flags & AF_MESH) return PACKET_ROOT_MESH;
    // the root tree ends where the next accel's tree begins
    size_t root_end = n_nodes;
    for (size_t a = 1; a < n_accels; ++a)
        if (accels[a].node_base > accels[0].node_base && accels[a].node_base < root_end) root_end = accels[a].node_base;
    const int need = packet_stack_need(nodes + accels[0].node_base, root_end - accels[0].node_base);
    if (need < 0) return PACKET_MALFORMED;
    if ((uint32_t)need > stack_depth) return PACKET_STACK;
    for (size_t a = 1; a < n_accels; ++a) {
        const DAccel &A = accels[a];
        if (A.node_base >= n_nodes || A.parent < 0 || (size_t)A.parent >= n_accels) return PACKET_MALFORMED;
        const DNode &root = nodes[A.node_base];
        if (!(root.meta & NODE_LEAF)) return PACKET_NESTED_TREE;
        if (A.parent != 0) { // only as the lone mesh of a group that is entered from the root
            const DAccel &G = accels[(size_t)A.parent];
            if (G.parent != 0 || G.lone != (uint32_t)a || !(A.flags & AF_MESH)) return PACKET_NESTED_DEEP;
        }
        if (A.flags & AF_MESH) {
            if (A.lone != NO_HIT) return PACKET_NESTED_SLOT; // (a mesh has no lone mesh of its own)
            continue;
        }
        const size_t first = (size_t)A.prim_base + root.link, count = root.meta & 0xFFFFu;
        if (first > n_prims || count > n_prims - first) return PACKET_MALFORMED;
        if (A.lone != NO_HIT) {
            if (A.lone >= n_accels || count != 1 || primref[first] != ((uint32_t)PK_ACCEL << 30 | A.lone)) return PACKET_NESTED_SLOT;
            continue;
        }
        for (size_t s = first; s < first + count; ++s) {
            const uint32_t kind = primref[s] >> 30;
            if (kind != PK_SPHERE && kind != PK_CUBOID) return PACKET_NESTED_SLOT;
        }
    }
    return PACKET_OK;
}

} // namespace lg
