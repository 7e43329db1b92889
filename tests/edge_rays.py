"""Deterministic edge-case rays for the ray queries (numpy only).

edge_rays(...) returns (rays, family): an (n, 6) float64 array (origin, direction) and an (n,) array of family names.  The rays come in
64-ray tiles built on purpose, because which form of the walk's node step a wave takes depends on all 64 of its lanes: a tile whose lanes
are all "plain" (finite origin, finite non-zero direction with a finite non-zero 1/d) and share one sign triple of 1/d takes that sign
triple's step, any other tile the generic slab test.  The generator asserts those construction properties itself.

  F1  uniform tiles: per sign triple, whole tiles of plain rays aimed through the scene's bounds (hits and misses)
  F2  one poisoned lane: an F1 tile whose lane 0, 1, 31, 32, 62 or 63 carries a component that is not plain for the node step
      or not for the identity shortcut (ray_plain) (+-0, +-5e-324, +-inf, NaN in
      the direction; -0, +-inf, NaN in the origin) or a plain but extreme one (|d| >= 2^1022: 1/d is subnormal)
  F3  signed-zero twins: pairs of rays that differ only in +0.0 / -0.0 components
  F4  slab planes: origins exactly on a face plane of a box and of the scene's bounds with a +-0 direction component on that axis (the
      0 * inf of the slab test); rays exactly through box edges and corners
  F5  triangles (mesh_grid_obj's grid): rays exactly through shared edges and vertices, rays in the mesh plane, rays from the surface
  F6  magnitudes: d scaled by 2^k far beyond the render's range, origins at |o| ~ 2^99, 2^101 and 1e300
  F7  finite-then-NaN: huge directions, for which a sphere's quadratic overflows to t = NaN after a box has been accepted at t < 1
"""
import numpy as np

TILE = 64
POISON_LANES = (0, 1, 31, 32, 62, 63)
INF, NAN = float("inf"), float("nan")
# direction component poisons, origin component poisons, plain-but-extreme direction components
DIR_POISON = (0.0, -0.0, 5e-324, -5e-324, INF, -INF, NAN)
ORG_POISON = (-0.0, INF, -INF, NAN)
DIR_EXTREME = (2.0 ** 1022, -(2.0 ** 1022), 2.0 ** 1023)
MAG_EXPONENTS = (-1074, -101, -100, -99, 0, 99, 100, 101, 510, 511, 512, 1000, 1023)
MESH_N, MESH_STEP = 48, 0.25  # mesh_grid_obj: 48 x 48 quads, 2 triangles each (4608 faces), vertices on a 0.25 lattice


def is_plain(ray):
    """What the walk's node step calls plain (walk.h neg_mask_x): finite origin, and every 1/d finite and non-zero."""
    o, d = ray[:3], ray[3:]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dinv = 1.0 / d
    return bool(np.all(np.isfinite(o)) and np.all(np.isfinite(dinv)) and np.all(dinv != 0.0))


def f64_plain_ray(ray):
    """What the identity shortcut calls plain (walk.h ray_plain): no component NaN, infinite or -0.0."""
    return bool(np.all(np.isfinite(ray)) and not np.any((ray == 0.0) & np.signbit(ray)))


def sign_triple(ray):
    """dir_is_neg of bvh.rs:463 packed as x | y << 1 | z << 2 (the sign of 1/d: -0.0 counts as negative)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dinv = 1.0 / ray[3:]
    return int(dinv[0] < 0) | int(dinv[1] < 0) << 1 | int(dinv[2] < 0) << 2


def mesh_grid_obj(n=MESH_N, step=MESH_STEP):
    """OBJ text of an n x n grid of unit quads in the plane z = 0 (x, y in [0, n*step]), each split along its (i, j) -> (i+1, j+1)
    diagonal: every vertex and every edge midpoint is exact in f32 and f64."""
    lines = ["o grid"]
    for j in range(n + 1):
        for i in range(n + 1):
            lines.append("v %r %r 0.0" % (i * step, j * step))
    idx = lambda i, j: j * (n + 1) + i + 1  # noqa: E731
    for j in range(n):
        for i in range(n):
            lines.append("f %d %d %d" % (idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            lines.append("f %d %d %d" % (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return "\n".join(lines) + "\n"


def _tile_f1(rng, lo, hi, k):
    """One tile of plain rays of sign triple k through the box [lo, hi] widened by half its size (so that some miss)."""
    size = hi - lo
    sgn = np.array([-1.0 if k >> a & 1 else 1.0 for a in range(3)])
    rays = np.empty((TILE, 6))
    for lane in range(TILE):
        target = lo - 0.25 * size + rng.uniform(0.0, 1.5, 3) * size
        d = sgn * rng.uniform(0.05, 1.0, 3) * np.max(size)
        o = target - d * rng.uniform(0.5, 2.0)  # t of the target in [0.5, 2]: t < 1 and t >= 1 both occur
        rays[lane] = np.concatenate([o, d])
        assert is_plain(rays[lane]) and sign_triple(rays[lane]) == k
    return rays


def _poisons():
    for a in range(3):
        for v in DIR_POISON:
            yield "d", a, v
        for v in ORG_POISON:
            yield "o", a, v
        for v in DIR_EXTREME:
            yield "x", a, v


class _Out:
    def __init__(self):
        self.rays, self.fam = [], []

    def add(self, family, rays):
        rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
        self.rays.append(rays)
        self.fam += [family] * rays.shape[0]

    def result(self):
        return np.concatenate(self.rays), np.array(self.fam)


def edge_rays(lo, hi, boxes=(), mesh=False, huge=False, seed=0, f1_tiles=2):
    """(rays, family) for a scene whose world bounds are [lo, hi] and whose boxes (min, max) are `boxes`; mesh=True adds F5 (the scene
    holds mesh_grid_obj at the identity), huge=True adds F7 (the scene of f7_scene)."""
    with np.errstate(over="ignore"):  # (F6 scales directions to overflow on purpose)
        return _edge_rays(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), boxes, mesh, huge, seed, f1_tiles)


def _edge_rays(lo, hi, boxes, mesh, huge, seed, f1_tiles):
    rng = np.random.default_rng(seed)
    out = _Out()
    centre, size = 0.5 * (lo + hi), hi - lo
    # ---- F1: uniform tiles, every sign triple
    f1 = {k: [_tile_f1(rng, lo, hi, k) for _ in range(f1_tiles)] for k in range(8)}
    for k in range(8):
        for t in f1[k]:
            out.add("F1", t)
    # ---- F2: one poisoned lane per copy of an F1 tile (every poison, every poisoned lane position, every sign triple)
    for p, (where, axis, value) in enumerate(_poisons()):
        k, lane = p % 8, POISON_LANES[p % len(POISON_LANES)]
        tile = f1[k][0].copy()
        tile[lane, (3 if where in "dx" else 0) + axis] = value
        both = is_plain(tile[lane]) and f64_plain_ray(tile[lane])
        assert both == (where == "x"), (where, axis, value)
        assert all(is_plain(r) and sign_triple(r) == k for i, r in enumerate(tile) if i != lane)
        out.add("F2", tile)
    # ---- F3: signed-zero twins (axis-parallel and in-plane rays, zeros in the origin and the direction)
    twins = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for s in (1.0, -1.0):
            for off in (0.0, 0.3):
                o = centre.copy()
                o[a] = centre[a] - s * 2.0 * size[a]
                o[b] = 0.0
                o[c] = off * size[c]
                d = np.zeros(3)
                d[a] = s * size[a]
                d[c] = 0.0 if off == 0.0 else -0.1 * size[c]
                for away in (1.0, -1.0):  # towards the scene, and away from it (misses)
                    for zb in (0.0, -0.0):
                        for zd in (0.0, -0.0):
                            oo, dd = o.copy(), d * away
                            oo[b] = zb
                            dd[b] = zd
                            twins.append(np.concatenate([oo, dd]))
    twins = np.array(twins)
    assert np.array_equal(np.abs(twins[0::4]), np.abs(twins[3::4]))  # (twins differ in the sign of zeros only)
    out.add("F3", twins)
    # ---- F4: origins on face planes of the boxes and of the bounds, with a +-0 component on that axis; edges and corners
    f4 = []
    for bmin, bmax in list(boxes) + [(lo, hi)]:
        bmin, bmax = np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
        bc = 0.5 * (bmin + bmax)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for plane in (bmin[a], bmax[a]):
                for zero in (0.0, -0.0):
                    for inside in (True, False):
                        o = bc.copy()
                        o[a] = plane
                        if not inside:
                            o[b] = bmax[b] + (bmax[b] - bmin[b])
                        d = np.zeros(3)
                        d[a] = zero
                        d[b], d[c] = (-1.0 if not inside else 0.5), 0.25
                        f4.append(np.concatenate([o, d]))
        for cx in (0, 1):  # through every corner, exactly: o = corner + 2 * e, d = -e (e dyadic)
            for cy in (0, 1):
                for cz in (0, 1):
                    corner = np.array([(bmin, bmax)[cx][0], (bmin, bmax)[cy][1], (bmin, bmax)[cz][2]])
                    e = np.array([1.0 if cx else -1.0, 0.5 if cy else -0.5, 0.25 if cz else -0.25])
                    f4.append(np.concatenate([corner + 2.0 * e, -e]))
                    e2 = e.copy()
                    e2[0] = 0.0  # along the edge's plane: through the edge at x = corner's x
                    f4.append(np.concatenate([corner + 2.0 * e2, -e2]))
    out.add("F4", f4)
    # ---- F5: the grid mesh (z = 0, vertices on a MESH_STEP lattice)
    if mesh:
        f5 = []
        ext = MESH_N * MESH_STEP
        for _ in range(64):
            i, j = rng.integers(1, MESH_N, 2)
            v = np.array([i * MESH_STEP, j * MESH_STEP, 0.0])
            for target in (v, v + [0.5 * MESH_STEP, 0.0, 0.0], v + [0.0, 0.5 * MESH_STEP, 0.0], v + [0.5 * MESH_STEP, 0.5 * MESH_STEP, 0.0]):
                e = np.array([rng.choice([-0.5, 0.0, 0.25]), rng.choice([-0.25, 0.0, 0.5]), rng.choice([1.0, -1.0])])
                f5.append(np.concatenate([target + 4.0 * e, -e]))  # through a vertex / an edge midpoint / a diagonal's midpoint
            f5.append(np.concatenate([v, [0.0, 0.0, 1.0]]))     # from the surface, away
            f5.append(np.concatenate([v, [0.0, 0.0, -1.0]]))    # from the surface, through
            f5.append(np.concatenate([v + [0.1, 0.05, 0.0], [0.3, -0.2, 1.0]]))
            f5.append(np.concatenate([v + [0.1, 0.05, 0.0], [0.3, -0.2, -1.0]]))
            for zd in (0.0, -0.0):                                # in the plane
                f5.append(np.concatenate([v - [1.0, 0.0, 0.0], [1.0, 0.5, zd]]))
                f5.append(np.concatenate([[-1.0, j * MESH_STEP, 0.0], [ext, 0.0, zd]]))
        out.add("F5", f5)
    # ---- F6: magnitudes
    f6 = []
    base_d = np.array([0.3, -0.2, -1.0]) * np.max(size)
    base_o = centre - 2.0 * base_d
    for k in MAG_EXPONENTS:
        f6.append(np.concatenate([base_o, base_d * 2.0 ** k]))
        f6.append(np.concatenate([base_o, np.array([0.0, 0.0, -1.0]) * 2.0 ** k]))
    for m in (2.0 ** 99, 2.0 ** 101, 1e300):
        for u in (np.array([1.0, 0.0, 0.0]), np.array([0.6, -0.48, 0.64]), np.array([0.0, 0.0, 1.0])):
            o = centre + u * m
            for scale in (1.0, 2.0 ** -60, 2.0 ** 40):
                f6.append(np.concatenate([o, -u * m * scale]))
    out.add("F6", f6)
    # ---- F7: finite-then-NaN candidates
    if huge:
        f7 = []
        for e in (154, 155, 160, 170, 200, 300):
            for o, u in (((0.0, 0.0, 10.0), (0.0, 0.0, -1.0)), ((0.0, 0.1, 10.0), (0.0, 0.0, -1.0)), ((0.3, 0.2, 8.0), (-0.03, -0.02, -1.0)),
                         ((0.0, 0.0, -10.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 2.5), (0.0, 0.0, -1.0))):
                f7.append(np.concatenate([o, np.array(u) * 10.0 ** e]))
        out.add("F7", f7)
    return out.result()


def f7_scene(api, with_sphere=True):
    """A box at z in [2, 3] and, unless with_sphere is False, a unit sphere at the origin: o = (0, 0, 10), d = (0, 0, -1e160) is
    accepted by the box at t = 7e-160, then by the sphere at t = NaN (its quadratic overflows), which wins."""
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 0.0, 10.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    M = api.Material
    scene.root.add_box([-0.5, -0.5, 2.0], [0.5, 0.5, 3.0], M.matte([0.8, 0.2, 0.2], 0.0))
    if with_sphere:
        scene.root.add_sphere([0.0, 0.0, 0.0], 1.0, M.plastic([0.2, 0.3, 0.9], [0.5, 0.5, 0.5], 0.2))
    return scene


F7_BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 3.0))
F7_BOXES = (((-0.5, -0.5, 2.0), (0.5, 0.5, 3.0)),)


def f3_scene(api):
    """Signed zeros through the transform shortcut: spheres and a box at an exact-identity root, in a nested exact-identity group, in a
    group translated by zero (its builder's products turn the translation's -0.0 back into +0.0: an exact identity again) and in a group
    rotated by 360 degrees (cos is exactly 1, sin is not 0: walked through its transform)."""
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 0.0, 10.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    M = api.Material
    scene.root.add_sphere([0.0, 0.0, 0.0], 0.75, M.matte([0.8, 0.8, 0.8], 0.0))
    scene.root.add_box([1.0, -0.5, -0.5], [2.0, 0.5, 0.5], M.matte([0.2, 0.8, 0.2], 10.0))
    ident = api.Aggregate.new()
    ident.add_sphere([-1.5, 0.0, 0.0], 0.5, M.plastic([0.9, 0.3, 0.2], [0.5, 0.5, 0.5], 0.3))
    ident.add_box([-0.5, 1.0, -0.5], [0.5, 2.0, 0.5], M.matte([0.2, 0.2, 0.8], 0.0))
    scene.root.add_group(ident)
    zero = api.Aggregate.new()
    zero.translate([0.0, 0.0, 0.0])
    zero.add_sphere([0.0, -1.5, 0.0], 0.5, M.metal([0.2, 0.9, 1.1], [3.9, 2.4, 2.2], 0.1, 0.2))
    zero.add_box([-0.5, -0.5, 1.0], [0.5, 0.5, 2.0], M.matte([0.9, 0.9, 0.1], 0.0))
    scene.root.add_group(zero)
    turn = api.Aggregate.new()
    turn.rotate_z(360.0)
    turn.add_sphere([1.5, 1.5, 0.0], 0.4, M.matte([0.5, 0.9, 0.9], 5.0))
    turn.add_box([-2.0, -2.0, -0.5], [-1.0, -1.0, 0.5], M.matte([0.9, 0.5, 0.9], 0.0))
    scene.root.add_group(turn)
    return scene


F3_BOUNDS = ((-2.0, -2.0, -1.0), (2.0, 2.0, 2.0))
F3_BOXES = (((1.0, -0.5, -0.5), (2.0, 0.5, 0.5)), ((-0.5, 1.0, -0.5), (0.5, 2.0, 0.5)), ((-0.5, -0.5, 1.0), (0.5, 0.5, 2.0)),
            ((-2.0, -2.0, -0.5), (-1.0, -1.0, 0.5)))


def grid_scene(api):
    """mesh_grid_obj at the identity (4608 triangles, enough for the pruned walk to be the default) with a box and a sphere above it."""
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([6.0, 6.0, 20.0], [6.0, 6.0, 0.0], [0.0, 1.0, 0.0])
    M = api.Material
    scene.root.add_obj_of(scene.parse_obj(mesh_grid_obj()), M.plastic([0.6, 0.6, 0.6], [0.5, 0.5, 0.5], 0.2))
    scene.root.add_box([2.0, 2.0, 0.5], [3.0, 3.0, 1.5], M.matte([0.8, 0.3, 0.3], 0.0))
    scene.root.add_sphere([8.0, 8.0, 1.0], 0.75, M.matte([0.3, 0.3, 0.8], 0.0))
    return scene


GRID_BOUNDS = ((0.0, 0.0, -0.5), (MESH_N * MESH_STEP, MESH_N * MESH_STEP, 1.75))
GRID_BOXES = (((2.0, 2.0, 0.5), (3.0, 3.0, 1.5)),)


def scene_geometry(witness, pscene):
    """(lo, hi, boxes) for edge_rays from a query_witness.Witness and its pyref scene: the root accel's world bounds and the root's own
    boxes (world space when the root's transform is the identity, as in every scene the tests use; elsewhere only aim is lost)."""
    lo, hi = witness.root.bound()
    boxes = [(node[1], node[2]) for node in pscene.root.contents if node[0] == "cuboid"]
    return lo, hi, boxes
