// tools/level_door_host_check.cpp -- the host part of the walk's level door (lasgun_amd/csrc/host.cpp, level_door_records: every accel's
// door record and lone-mesh mark) in a stand-alone program, meant to be built together with host.cpp under -fsanitize=address,undefined and
// run on the CPU (tests/test_level_door_predicate.py does).  It flattens scenes that hold every case of the two rules and looks at every
// accel's record again from the tables: the door's axis is the thinnest of the node-0 box, its coefficients are that row of minv, and a group
// is marked lone exactly when it holds one identity mesh accel under the same 48 bytes of box.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/level_door_host_check.cpp lasgun_amd/csrc/host.cpp -o check && ./check
#include <cstdio>
#include <cstring>
#include <memory>

#include "../lasgun_amd/csrc/host.h"

using namespace lg;

static int failures = 0;
static bool quiet = false; // (while a record is stale on purpose)
#define EXPECT(c) do { if (!(c)) { if (!quiet) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const char PLANE[] = "o plane\nv -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0 1\n\nf 1 2 3\nf 1 3 4\n";

static uint32_t add_plane(Scene &s) {
    std::unique_ptr<Obj> obj(new Obj());
    parse_obj_text(PLANE, sizeof PLANE - 1, *obj);
    s.meshes.push_back(std::move(obj));
    return (uint32_t)s.meshes.size() - 1u;
}
static SceneNode mesh_node(uint32_t mesh) {
    SceneNode n; n.kind = SceneNode::MESH; n.obj = mesh; n.mat = material_default(); n.has_mat = true;
    return n;
}
static SceneNode sphere_node(double x, double y, double z, double r) {
    SceneNode n; n.kind = SceneNode::SPHERE; n.a[0] = x; n.a[1] = y; n.a[2] = z; n.b[0] = r; n.mat = material_default(); n.has_mat = true;
    return n;
}
static void add_group(Aggregate &to, std::unique_ptr<Aggregate> g) {
    SceneNode n; n.kind = SceneNode::GROUP; n.mat = material_default(); n.group = std::move(g);
    to.contents.push_back(std::move(n));
}
// one wall of the Cornell shell: scale, optional rotation, translation, one plane mesh
static std::unique_ptr<Aggregate> wall(uint32_t plane, int rot_axis, double tx, double ty, double tz) {
    std::unique_ptr<Aggregate> g(new Aggregate());
    transform_concat_self(g->transform, transform_scale(2.0, 1.0, 2.0));
    if (rot_axis == 0) transform_concat_self(g->transform, transform_rotate_x(90.0));
    if (rot_axis == 2) transform_concat_self(g->transform, transform_rotate_z(90.0));
    const double d[3] = {tx, ty, tz};
    transform_concat_self(g->transform, transform_translate(d));
    g->contents.push_back(mesh_node(plane));
    return g;
}

// every accel's record, restated from the finished tables; returns the number of groups marked lone
static int check_records(const FlatScene &f) {
    int lone = 0;
    for (size_t i = 0; i < f.accels.size(); ++i) {
        const DAccel &A = f.accels[i];
        const DNode &n0 = f.nodes[A.node_base];
        const double e[3] = {n0.bmax[0] - n0.bmin[0], n0.bmax[1] - n0.bmin[1], n0.bmax[2] - n0.bmin[2]};
        int k = -1;
        for (int a = 0; a < 3; ++a)
            if (std::memcmp(&A.door[4], &n0.bmin[a], 8) == 0 && std::memcmp(&A.door[5], &n0.bmax[a], 8) == 0 &&
                std::memcmp(&A.door[0], &A.minv.c[0][a], 8) == 0 && std::memcmp(&A.door[1], &A.minv.c[1][a], 8) == 0 &&
                std::memcmp(&A.door[2], &A.minv.c[2][a], 8) == 0 && std::memcmp(&A.door[3], &A.minv.c[3][a], 8) == 0 && k < 0 &&
                !(e[(a + 1) % 3] < e[a]) && !(e[(a + 2) % 3] < e[a]))
                k = a;
        EXPECT(k >= 0); // the record is one axis's row and planes, and no other axis is thinner
        // the lone rule, stated independently of how host.cpp walks the tables
        bool want = false;
        uint32_t m = NO_HIT;
        if (!(A.flags & AF_MESH) && (n0.meta & NODE_LEAF) && (n0.meta & 0xFFFFu) == 1u) {
            const uint32_t ref = f.primref[A.prim_base + n0.link];
            if ((ref >> 30) == PK_ACCEL) {
                m = ref & PRIM_INDEX_MASK;
                const DAccel &M = f.accels[m];
                const DNode &m0 = f.nodes[M.node_base];
                want = (M.flags & AF_MESH) && (M.flags & AF_IDENTITY) && (uint32_t)M.parent == (uint32_t)i;
                for (int a = 0; a < 3; ++a)
                    want = want && std::memcmp(&n0.bmin[a], &m0.bmin[a], 8) == 0 && std::memcmp(&n0.bmax[a], &m0.bmax[a], 8) == 0;
            }
        }
        EXPECT(A.lone == (want ? m : NO_HIT));
        if (A.lone != NO_HIT) { ++lone; EXPECT(A.lone < f.accels.size() && A.lone != i); }
    }
    return lone;
}

int main() {
    {   // the five walls (each a lone mesh in a transformed group), a sphere beside them in the root
        Scene s;
        const uint32_t plane = add_plane(s);
        add_group(*s.root, wall(plane, -1, 0.0, -2.0, 0.0));
        add_group(*s.root, wall(plane, -1, 0.0, 2.0, 0.0));
        add_group(*s.root, wall(plane, 2, -2.0, 0.0, 0.0));
        add_group(*s.root, wall(plane, 2, 2.0, 0.0, 0.0));
        add_group(*s.root, wall(plane, 0, 0.0, 0.0, -2.0));
        s.root->contents.push_back(sphere_node(1.0, -1.25, 0.0, 1.0));
        FlatScene f;
        flatten_scene(s, f);
        EXPECT(f.accels.size() == 11);
        const int lone = check_records(f);
        EXPECT(lone == 5);
        std::printf("walls: %d of 5 groups lone\n", lone);
        EXPECT(f.accels[0].lone == NO_HIT);
        for (const DAccel &A : f.accels)
            if (A.flags & AF_MESH) { EXPECT(A.lone == NO_HIT); EXPECT(A.door[4] == 0.0 && A.door[5] == 0.0); } // the plane: thinnest on y
    }
    {   // a group with a mesh and a sphere (not lone); group -> group -> mesh (the inner one lone, the outer one not: its slot is a group);
        // an identity group with a lone mesh; a mesh straight in the root (the root holds more than it)
        Scene s;
        const uint32_t plane = add_plane(s);
        std::unique_ptr<Aggregate> both(new Aggregate());
        transform_concat_self(both->transform, transform_rotate_y(30.0));
        both->contents.push_back(mesh_node(plane));
        both->contents.push_back(sphere_node(0.0, 0.5, 0.0, 0.25));
        add_group(*s.root, std::move(both));
        std::unique_ptr<Aggregate> outer(new Aggregate());
        transform_concat_self(outer->transform, transform_scale(1.0, 3.0, 0.5));
        add_group(*outer, wall(plane, 2, 0.5, 0.0, 0.0));
        add_group(*s.root, std::move(outer));
        std::unique_ptr<Aggregate> idg(new Aggregate());
        idg->contents.push_back(mesh_node(plane));
        add_group(*s.root, std::move(idg));
        s.root->contents.push_back(mesh_node(plane));
        FlatScene f;
        flatten_scene(s, f);
        const int lone = check_records(f);
        EXPECT(lone == 2);
        // accels in pre-order: 0 root, 1 `both`, 2 its mesh, 3 outer, 4 inner, 5 its mesh, 6 the identity group, 7 its mesh, 8 the root's mesh
        EXPECT(f.accels.size() == 9);
        if (f.accels.size() == 9) {
            EXPECT(f.accels[1].lone == NO_HIT && f.accels[3].lone == NO_HIT && f.accels[4].lone == 5u && f.accels[6].lone == 7u && f.accels[0].lone == NO_HIT);
            EXPECT((f.accels[6].flags & AF_IDENTITY) != 0u);
        }
        // a record made stale on purpose is found by the restatement (the check checks)
        f.accels[4].lone = NO_HIT;
        const int before = failures;
        quiet = true;
        check_records(f);
        quiet = false;
        const bool found = failures == before + 1;
        failures = before;
        EXPECT(found);
        level_door_records(f); // ... and made again from the tables
        EXPECT(check_records(f) == 2);
    }
    {   // a root that is itself one lone mesh: the root is marked like any group, and the walk never "enters" it
        Scene s;
        const uint32_t plane = add_plane(s);
        s.root->contents.push_back(mesh_node(plane));
        FlatScene f;
        flatten_scene(s, f);
        EXPECT(check_records(f) == 1 && f.accels.size() == 2 && f.accels[0].lone == 1u);
    }
    if (failures) { std::fprintf(stderr, "level_door_host_check: %d failures\n", failures); return 1; }
    std::printf("level_door_host_check: ok\n");
    return 0;
}
