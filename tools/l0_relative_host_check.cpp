// tools/l0_relative_host_check.cpp -- the host part of the level-0 closest pass's origin-relative form (lasgun_amd/csrc/host.cpp,
// l0_relative_camera / l0_relative_origins: the gate and every accel's local origin) in a stand-alone program, meant to be built together
// with host.cpp under -fsanitize=address,undefined and run on the CPU (tests/test_l0_relative_predicate.py does).  It flattens the scenes of
// tools/level_door_host_check.cpp -- the five walls and a sphere; groups in groups, a mesh beside a sphere, identity groups, a mesh in the
// root -- and restates every accel's origin from the tables: the parent's origin through the accel's own inverse transform, by xf_point.
// It prints the walls' table (hexadecimal floats, one accel per line) for the test to read.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/l0_relative_host_check.cpp lasgun_amd/csrc/host.cpp -o check && ./check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../lasgun_amd/csrc/host.h"

using namespace lg;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

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

static bool same_bits(const V3 &a, const V3 &b) { return std::memcmp(&a, &b, sizeof a) == 0; }
// every accel's origin again, from its PARENT's (not along the chain, as host.cpp walks): local[i] = xf_point(minv[i], local[parent])
static void check_table(const FlatScene &f, const V3 &origin, const std::vector<V3> &local) {
    EXPECT(local.size() == f.accels.size());
    for (size_t i = 0; i < f.accels.size() && i < local.size(); ++i) {
        const DAccel &A = f.accels[i];
        const V3 from = A.parent < 0 ? origin : local[(size_t)A.parent];
        EXPECT(A.parent < (int32_t)i);
        EXPECT(same_bits(local[i], xf_point(A.minv, from)));
        if (A.flags & AF_IDENTITY) EXPECT(same_bits(local[i], from)); // the kept ray of an identity accel: the same origin
    }
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const V3 up{0.0, 1.0, 0.0}, aux{1.0, 0.0, 0.0};
    {   // the camera's part of the gate
        EXPECT(l0_relative_camera(V3{0.25, 0.5, 6.0}, up, aux, 0.0));
        EXPECT(l0_relative_camera(V3{0.0, 0.5, 6.0}, up, aux, -0.0)); // +0 is clean; a pixel separation of -0 still makes zeros
        EXPECT(!l0_relative_camera(V3{0.25, 0.5, 6.0}, up, aux, 1.0)); // orthographic
        EXPECT(!l0_relative_camera(V3{-0.0, 0.5, 6.0}, up, aux, 0.0));
        EXPECT(!l0_relative_camera(V3{0.25, -0.0, 6.0}, up, aux, 0.0));
        EXPECT(!l0_relative_camera(V3{0.25, 0.5, -0.0}, up, aux, 0.0));
        EXPECT(!l0_relative_camera(V3{inf, 0.5, 6.0}, up, aux, 0.0));
        EXPECT(!l0_relative_camera(V3{0.25, nan, 6.0}, up, aux, 0.0));
        EXPECT(!l0_relative_camera(V3{0.25, 0.5, 6.0}, V3{0.0, nan, 0.0}, aux, 0.0));
        EXPECT(!l0_relative_camera(V3{0.25, 0.5, 6.0}, up, V3{inf, 0.0, 0.0}, 0.0));
        EXPECT(!l0_relative_camera(V3{0.25, 0.5, 6.0}, up, aux, nan));
    }
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
        const V3 origin{0.25, 0.5, 6.0};
        std::vector<V3> local;
        EXPECT(l0_relative_origins(f, origin, local));
        check_table(f, origin, local);
        for (size_t i = 0; i < local.size(); ++i) std::printf("walls accel %zu %a %a %a\n", i, local[i].x, local[i].y, local[i].z);
        // an origin that is not plain: refused, whatever the scene
        EXPECT(!l0_relative_origins(f, V3{-0.0, 0.5, 6.0}, local));
        EXPECT(!l0_relative_origins(f, V3{0.25, inf, 6.0}, local));
        EXPECT(!l0_relative_origins(f, V3{0.25, 0.5, nan}, local));
        EXPECT(local.size() == f.accels.size()); // (sized even when refused)
        EXPECT(l0_relative_origins(f, V3{1e6, -3e5, 2.5e6}, local));
        check_table(f, V3{1e6, -3e5, 2.5e6}, local);
    }
    {   // groups in groups, a mesh beside a sphere, an identity group with a mesh, a mesh straight in the root
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
        EXPECT(f.accels.size() == 9);
        for (const V3 &origin : {V3{0.3, 0.4, 5.0}, V3{0.0, 0.0, 5.0}, V3{-7.5, 1.25, 2.0}}) {
            std::vector<V3> local;
            EXPECT(l0_relative_origins(f, origin, local));
            check_table(f, origin, local);
        }
        // a chain that does not end at its own accel is refused, not walked
        FlatScene g = f;
        g.accels[4].chain[g.accels[4].nchain - 1u] = 3u;
        std::vector<V3> local;
        EXPECT(!l0_relative_origins(g, V3{0.3, 0.4, 5.0}, local));
    }
    if (failures) { std::fprintf(stderr, "l0_relative_host_check: %d failures\n", failures); return 1; }
    std::printf("l0_relative_host_check: ok\n");
    return 0;
}
