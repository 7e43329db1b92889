"""The scenes and points of the closest-point tests (tests/test_closest_witness.py on the CPU, tests/test_gpu_closest_points.py on the
device), numpy, tests/pyref.py and the brute force (tests/closest_ref.py) only.  Every builder runs on pyref.Api and on the library alike.
4097 points a scene, made without a device: uniform in 1.5 x the scene's bounds, surface points (the brute force's own closest points of
the first of those: distance 0 up to rounding), exact vertices, box corners and edge midpoints, sphere centres, the tie constructions (a
mesh vertex pushed away from its mesh's centroid: every face around it answers with that vertex, the same bits), points at 1e6 and
non-finite points."""
import functools

import numpy as np

import closest_ref as R
import limit_scenes as L
import pyref
from lasgun_amd import scenes as S

N_POINTS = 4097
INF, NAN = float("inf"), float("nan")

TETRA_OBJ = """o tetra
v 0 0 0
v 1 0 0
v 0 1 0
v 0 0 1
f 1 3 2
f 1 2 4
f 1 4 3
f 2 3 4
"""


def own_scene(api):
    """Three spheres (one in a rotated, uniformly scaled group), three boxes (one under rotation plus non-uniform scale), a tetrahedron
    instanced twice (once under rotation plus non-uniform scale), three levels of groups below the root.  No sphere sits under a
    non-uniform scale: the gate admits the scene."""
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.5, 1.0, 7.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    scene.add_point_light([0.0, 5.0, 5.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0])
    M = api.Material
    red, green, blue = M.matte([0.8, 0.2, 0.2], 0.0), M.plastic([0.2, 0.8, 0.2], [0.5, 0.5, 0.5], 0.3), M.matte([0.2, 0.2, 0.8], 10.0)
    tetra = scene.parse_obj(TETRA_OBJ)
    root = scene.root
    root.add_sphere([-1.5, 0.5, 0.0], 0.5, red)
    root.add_sphere([2.0, -1.0, 0.5], 0.75, green)
    root.add_box([-0.5, -2.0, -0.5], [0.5, -1.5, 0.5], blue)
    root.add_obj_of(tetra, red)
    inner = api.Aggregate.new()  # level 3 below the root's level 1: rotation plus non-uniform scale; no sphere
    inner.scale(1.2, 0.8, 1.0)
    inner.rotate(40.0, [0.6, 0.0, 0.8])
    inner.translate([0.25, 0.5, -0.25])
    inner.add_box([-0.5, -0.25, -0.25], [0.5, 0.25, 0.25], green)
    inner.add_obj_of(tetra, blue)
    deepest = api.Aggregate.new()  # level 4: a box alone, translated
    deepest.translate([0.0, 1.0, 0.0])
    deepest.add_cube([-0.25, -0.25, -0.25], 0.5, red)
    inner.add_group(deepest)
    middle = api.Aggregate.new()  # level 2: rotated, uniformly scaled; holds a sphere
    middle.scale(1.2, 1.2, 1.2)
    middle.rotate_y(30.0)
    middle.rotate_z(-20.0)
    middle.translate([0.5, 1.5, -1.0])
    middle.add_sphere([0.0, 0.0, 0.0], 0.4, blue)
    middle.add_group(inner)
    root.add_group(middle)
    return scene


def torus_scene(api):
    """A 24 x 16 torus (fat leaves) in a translated group, plus 40 spheres at the root (a sphere tree of several nodes)."""
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 1.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    scene.add_point_light([0.0, 5.0, 5.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0])
    M = api.Material
    mesh = scene.parse_obj(S.torus_obj(24, 16, normals=True))
    g = api.Aggregate.new()
    g.rotate_x(35.0)
    g.translate([0.1, -0.2, 0.0])
    g.add_obj_of(mesh, M.matte([0.7, 0.7, 0.7], 0.0))
    scene.root.add_group(g)
    for i in range(40):
        scene.root.add_sphere([-1.6 + 0.08 * i, -1.7 + 0.02 * (i % 7), 1.2 - 0.05 * i], 0.06 + 0.002 * (i % 5), M.matte([0.6, 0.6, 0.6], 0.0))
    return scene


SCENES = {"own": own_scene, "cornell": lambda api: S.cornell_scene(api, "plastic"), "torus": torus_scene}
MESH_SCENES = ("own", "cornell", "torus")  # every one of them holds a mesh
LIMIT_SCENES = dict(L.SCENES)  # the depth-8 scenes: each matches the brute force or is refused exactly where the gate says


def builder(name):
    return SCENES[name] if name in SCENES else LIMIT_SCENES[name]


# ---- the gate, restated from the chains alone (the header's rule) ------------------------------------------------------------------------
def linear_part(chain):
    """L: the 3 x 3 part of the composed local -> world transform (root's outermost), rows x columns."""
    total = np.eye(3)
    for m, _, _ in chain:
        total = total @ np.array([[m[c][r] for c in range(3)] for r in range(3)], dtype=np.float64)
    return total


def gate(cat):
    """-1, or the first accel that holds a sphere under a chain whose L^T L is not within 2^-40 (relative) of a multiple of the identity."""
    holders = sorted({inst for _, _, inst in cat.spheres})
    for inst in holders:
        lin = linear_part(cat.accels[inst]["chain"])
        s = lin.T @ lin
        s2 = np.trace(s) / 3.0
        if not (s2 > 0.0 and np.abs(s - s2 * np.eye(3)).max() <= 2.0 ** -40 * s2):
            return inst
    return -1


# ---- the points ---------------------------------------------------------------------------------------------------------------------------
def world_bounds(b):
    pts = [b.tri.reshape(-1, 3), b.box.reshape(-1, 3)]
    if len(b.cw):
        r = np.sqrt(R.dot(b.pw - b.cw, b.pw - b.cw))[:, None]
        pts += [b.cw - r, b.cw + r]
    allp = np.concatenate(pts)
    allp = allp[np.isfinite(allp).all(axis=1)]
    return allp.min(axis=0), allp.max(axis=0)


def tie_points(b):
    """For every mesh instance, some of its vertices pushed away from the instance's centroid by 0.5 and by 2 edge lengths."""
    out = []
    if not len(b.tri):
        return np.zeros((0, 3))
    inst = b.ids[len(b.cw) + len(b.box):, 0]
    for i in np.unique(inst):
        tri = b.tri[inst == i]
        verts = np.unique(tri.reshape(-1, 3), axis=0)
        cen = verts.mean(axis=0)
        edge = np.sqrt(((tri[:, 1] - tri[:, 0]) ** 2).sum(axis=1)).mean()
        pick = verts[:: max(1, len(verts) // 12)][:12]
        d = pick - cen
        d /= np.sqrt((d * d).sum(axis=1))[:, None]
        out += [pick + d * (0.5 * edge), pick + d * (2.0 * edge)]
    return np.concatenate(out)


def make_points(b, seed):
    rng = np.random.default_rng(seed)
    lo, hi = world_bounds(b)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    uniform = lambda m: mid + (rng.uniform(-1.5, 1.5, (m, 3)) * half)  # noqa: E731
    fixed = []
    fixed.append(b.closest(uniform(400))["point"])                           # on a surface, up to rounding
    if len(b.tri):
        t = b.tri[rng.permutation(len(b.tri))[:120]]
        fixed += [t[:, 0], t[:, 1], (t[:, 0] + t[:, 1]) / 2.0, (t[:, 1] + t[:, 2]) / 2.0, (t[:, 0] + t[:, 1] + t[:, 2]) / 3.0]
    if len(b.box):
        c = b.box
        fixed += [c.reshape(-1, 3), (c[:, 0] + c[:, 7]) / 2.0, (c[:, 0] + c[:, 1]) / 2.0, (c[:, 0] + c[:, 6]) / 2.0, (c[:, 1] + c[:, 7]) / 2.0,
                  (c[:, 0] + c[:, 3]) / 2.0, (c[:, 4] + c[:, 7]) / 2.0, (c[:, 0] + c[:, 5]) / 2.0, (c[:, 2] + c[:, 7]) / 2.0]  # corners, the centre, face centres
    if len(b.cw):
        s = rng.permutation(len(b.cw))[:64]
        fixed += [b.cw[s], b.cw[s] + (b.pw[s] - b.cw[s]) * 0.5, b.pw[s]]       # centres, inside, on the surface (the pole)
    fixed.append(tie_points(b))
    far = rng.normal(0.0, 1.0, (64, 3))
    fixed.append(far / np.sqrt((far * far).sum(axis=1))[:, None] * 1e6)
    bad = uniform(8)
    bad[np.arange(8), [0, 1, 2, 0, 1, 2, 0, 1]] = [NAN, INF, -INF, INF, NAN, NAN, -INF, -INF]
    bad[7, 2] = NAN
    fixed.append(bad)
    fixed = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 3) for f in fixed])[:N_POINTS - 256]
    pts = np.concatenate([fixed, uniform(N_POINTS - len(fixed))])
    assert pts.shape == (N_POINTS, 3)
    return np.ascontiguousarray(pts[rng.permutation(N_POINTS)])


@functools.lru_cache(maxsize=None)
def case(name):
    """(pyref scene, brute force, points, the brute force's answer at radius +INF) of a scene, once."""
    pscene = builder(name)(pyref.Api)
    b = R.Brute(pscene)
    pts = make_points(b, 1000 + sorted(list(SCENES) + list(LIMIT_SCENES)).index(name))
    return pscene, b, pts, b.closest(pts)


def radii(want):
    """The four radii of the GPU test: +INF, 0, the median distance of the hits, 2^-20."""
    d = want["distance"]
    return (INF, 0.0, float(np.median(d[np.isfinite(d)])), 2.0 ** -20)
