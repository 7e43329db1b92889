"""Scenes at the scene graph's limits (test_limit_scenes_host.py, test_gpu_scene_limits.py): eight levels of nesting
(MAX_CHAIN, dscene.h) and one more, 64 and 65 accels (the line at which the accel records leave LDS, accel.cpp), and per-lane stacks deep
enough that the 256-lane kernels need more than 64 KiB of dynamic LDS.  Built through any of the three bindings (the product's, the oracle's,
pyref.Api), deterministically: what a search found is committed as constants, and the search itself as a function that a device-free test
re-runs.  add_group moves the aggregate it is given, so every builder makes the innermost level first."""
import math

import numpy as np

import level_door_scenes as D
from lasgun_amd import scenes as S

W, H = 64, 48  # the films of the limit tests
MAX_LEVELS = 8  # MAX_CHAIN (lasgun_amd/csrc/dscene.h): accels on the path root .. self


# ---- eight levels, shallow trees ------------------------------------------------------------------------------------------------------
def _turn(g, level):
    """The transform of the group at `level` (the root is level 1): no two alike, one exact identity, one swap_backface group."""
    k = level % 6
    if k == 2:
        g.scale(1.15, 0.9, 1.05); g.rotate_y(20.0); g.translate([0.1, -0.05, 0.05])
    elif k == 3:
        pass  # exactly the identity: the walk's AF_IDENTITY shortcut, deep in a chain
    elif k == 4:
        g.rotate_x(-15.0); g.swap_backface()
    elif k == 5:
        g.translate([-0.12, 0.08, 0.1])
    elif k == 0:
        g.rotate_z(25.0); g.scale(0.95, 1.1, 0.9)
    else:
        g.rotate(12.0, [0.6, 0.0, 0.8]); g.translate([0.05, 0.05, -0.05])


def _chain(api, levels):
    """root (level 1) -> groups at levels 2 .. levels - 1 -> a lone mesh at level `levels`: the last group holds one untransformed mesh and
    nothing else; every other level holds one or two primitives beside its group, and the group at levels - 2 a second branch of the same
    depth (_side_branch).  Accels in scene-graph order: the chain 0 .. levels - 2, the mesh levels - 1, the side branch levels, levels + 1."""
    scene = D._base(api, recursion=2)
    scene.camera.look_at([0.2, 0.3, 3.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    plastic, matte, glass = D._mats(api)
    mirror = api.Material.mirror([0.6, 0.6, 0.6])
    torus = scene.parse_obj(S.torus_obj(6, 4, R=0.8, r=0.3, normals=False))
    inner = api.Aggregate.new()
    _turn(inner, levels - 1)
    inner.add_obj_of(torus, plastic)  # the lone mesh: level `levels`
    for level in range(levels - 2, 1, -1):
        g = api.Aggregate.new()
        _turn(g, level)
        a = 0.9 * level
        g.add_sphere([0.9 * math.cos(a), 0.9 * math.sin(a), 0.35 * math.cos(2.0 * a)], 0.22, glass if level == 4 else (matte if level & 1 else plastic))
        if level == 3:
            g.add_cube([-0.9 * math.cos(a) - 0.15, -0.9 * math.sin(a) - 0.15, -0.3], 0.3, matte if level == 3 else plastic)
        g.add_group(inner)
        if level == levels - 2:
            g.add_group(_side_branch(api, level, plastic, matte))
        inner = g
    scene.root.add_sphere([-1.15, 0.9, 0.1], 0.3, mirror)
    scene.root.add_cube([0.85, -1.3, -0.2], 0.4, matte)
    scene.root.add_group(inner)
    return scene


def _side_branch(api, level, plastic, matte):
    """Beside the lone mesh's group: a group at level + 1 that holds primitives AND a transformed group at level + 2 with primitives of its
    own -- a walk that comes back from the last level goes on in a level whose ray it has to derive again through the whole chain."""
    last = api.Aggregate.new()
    last.rotate_y(35.0); last.scale(0.8, 1.2, 0.9); last.translate([0.1, -0.3, 0.2]); last.swap_backface()
    last.add_sphere([0.0, 0.0, 0.0], 0.3, plastic); last.add_cube([-0.45, 0.1, -0.2], 0.3, matte)
    g = api.Aggregate.new()
    g.rotate_z(-20.0); g.scale(1.1, 0.9, 1.0); g.translate([0.0, 0.1, 0.35])
    g.add_sphere([-0.7, 0.55, 0.0], 0.25, matte); g.add_cube([0.45, -0.7, -0.1], 0.32, plastic); g.add_sphere([0.6, 0.5, 0.3], 0.2, plastic)
    g.add_group(last)
    return g


def chain8_shallow(api):
    """Eight levels, a few primitives a level, the mesh alone in a level-7 group and a group of primitives at level 8 beside it: ten accels,
    small stacks, the LDS-resident form fits."""
    return _chain(api, MAX_LEVELS)


def chain9(api):
    """The same with one more level: the oracle renders it, the product refuses it."""
    return _chain(api, MAX_LEVELS + 1)


# ---- 64 and 65 accels -----------------------------------------------------------------------------------------------------------------
def _many_accels(api, accels):
    """Exactly `accels` accels, the root included: small transformed groups on a 9-wide grid, each holding a sphere or a cube, four holding a
    mesh instance (group + mesh: two accels each), two nested two deep; a floor and a second light, so that some points lie in shadow."""
    scene = D._base(api, recursion=1)
    scene.camera.look_at([0.3, 1.2, 6.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    scene.add_point_light([-2.5, 1.5, 3.0], [0.5, 0.5, 0.4], [1.0, 0.0, 0.0])
    plastic, matte, glass = D._mats(api)
    torus = scene.parse_obj(S.torus_obj(6, 4, R=0.16, r=0.06, normals=False))
    left, slot = accels - 1, 0
    cells = [30, 41] + [c for c in range(72) if c not in (30, 41)]  # the two nested groups near the middle of the grid

    def place(g):
        nonlocal slot
        x, y = cells[slot] % 9, cells[slot] // 9
        g.rotate_z(13.0 * slot); g.scale(1.0 + 0.03 * (slot % 5), 1.0, 0.8 + 0.05 * (slot % 4))
        g.translate([0.5 * (x - 4) + 0.07 * (y & 1), 0.5 * (y - 3.5), 0.25 * ((slot * 7) % 5 - 2)])
        slot += 1

    for k in range(2):  # group -> group -> sphere and cube: two accels each
        g2 = api.Aggregate.new(); g2.rotate_x(30.0 + 20.0 * k); g2.translate([0.05, 0.0, 0.02])
        g2.add_sphere([0.0, 0.0, 0.0], 0.2, plastic); g2.add_cube([0.05, 0.05, -0.1], 0.22, matte)
        g1 = api.Aggregate.new(); place(g1); g1.add_sphere([-0.12, 0.1, 0.0], 0.08, matte); g1.add_group(g2)
        scene.root.add_group(g1)
        left -= 2
    for k in range(4):  # a mesh instance in a group: two accels each
        g = api.Aggregate.new(); place(g); g.rotate_x(60.0 + 25.0 * k); g.add_obj_of(torus, plastic if k & 1 else matte)
        if k >= 2:
            g.add_sphere([0.0, 0.0, 0.0], 0.07, matte)  # (not lone)
        scene.root.add_group(g)
        left -= 2
    while left > 0:
        g = api.Aggregate.new(); place(g)
        if slot % 3:
            g.add_sphere([0.0, 0.0, 0.0], 0.17, glass if slot == 20 else (plastic if slot & 1 else matte))
        else:
            g.add_cube([-0.13, -0.13, -0.13], 0.26, matte if slot & 1 else plastic)
        scene.root.add_group(g)
        left -= 1
    scene.root.add_sphere([0.0, -0.2, 0.0], 0.3, plastic)  # at the centre of the bounds, among the groups
    scene.root.add_box([-3.0, -2.3, -1.5], [3.0, -2.2, 1.5], matte)  # the floor the grid throws shadows on
    return scene


def accels64(api):
    """64 accels: the accel records of the 256-lane forms are still in LDS (accel.cpp: accels <= 64)."""
    return _many_accels(api, 64)


def accels65(api):
    """65 accels: the 256-lane forms read the DAccel table in global memory (arec == nullptr in walk.h)."""
    return _many_accels(api, 65)


# ---- deep stacks: eight levels, found by a seeded search ------------------------------------------------------------------------------
DEEP_SPHERES = 128  # spheres a level
DEEP_CANDIDATES = 24  # seeds tried per level
# per level, innermost first: the seed the search kept (test_limit_scenes_host.py runs the search again and compares)
DEEP_A_BASE, DEEP_A_SEEDS, DEEP_A_MAX_STACK = 200000, (200004, 201012, 202022, 203000, 204016, 205003, 206011, 207000), 66
DEEP_C_BASE, DEEP_C_SEEDS, DEEP_C_MAX_STACK = 0, (1, 1000, 2001, 3002, 4001, 5015, 6000, 7003), 64


def deep_scene(api, seeds, spheres=DEEP_SPHERES):
    """len(seeds) levels of `spheres` random spheres each, seeds[0] the innermost level's, seeds[-1] the root's; every group turned and moved
    a little, one glass sphere at the root."""
    scene = D._base(api, recursion=1)
    scene.camera.look_at([0.3, 0.4, 6.5], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    plastic, matte, glass = D._mats(api)
    inner = None
    for idx, seed in enumerate(seeds):
        root = idx == len(seeds) - 1
        agg = scene.root if root else api.Aggregate.new()
        rng = np.random.default_rng(seed)
        if not root:
            agg.rotate_y(float(rng.uniform(-30.0, 30.0))); agg.translate([float(v) for v in rng.uniform(-0.3, 0.3, 3)])
        for k in range(spheres):
            c, r = [float(v) for v in rng.uniform(-2.0, 2.0, 3)], float(rng.uniform(0.02, 0.15))
            agg.add_sphere(c, r, glass if root and k == 0 else (plastic if k & 1 else matte))
        if inner is not None:
            agg.add_group(inner)
        inner = agg
    return scene


def deep_search(api, levels=MAX_LEVELS, base=0, candidates=DEEP_CANDIDATES, spheres=DEEP_SPHERES):
    """Greedy, inside out: per level the seed among base + 1000 * level + [0, candidates) whose scene so far has the largest max_stack (the
    first of equals).  (seeds, max_stack); device-free, about two seconds."""
    seeds, best = [], 0
    for level in range(levels):
        tried = [(api.host_build_dump(deep_scene(api, seeds + [base + 1000 * level + c], spheres))[2]["max_stack"], -c) for c in range(candidates)]
        best, c = max(tried)
        seeds.append(base + 1000 * level - c)
    return tuple(seeds), best


def deep_a(api):
    """The deepest stacks a constructible scene reached: max_stack >= 65, more than 64 KiB of dynamic LDS in the 256-lane forms."""
    return deep_scene(api, DEEP_A_SEEDS)


def deep_c(api):
    """Shallower than deep_a and still above 64 KiB: the second accel of the limit-is-monotone test."""
    return deep_scene(api, DEEP_C_SEEDS)


def lds_bytes_256(max_stack):
    """Dynamic LDS of a 256-lane traversal launch without the accel records: (max_stack + 2 guard entries) words a lane (accel.cpp)."""
    return (max_stack + 2) * 256 * 4


SCENES = {"chain8_shallow": chain8_shallow, "accels64": accels64, "accels65": accels65, "deep_a": deep_a, "deep_c": deep_c}
