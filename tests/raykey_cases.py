"""Ray sets that pin the coherence key (tests/raykey_ref.py restates it), shared by the host check (tests/test_raykey_host.py) and the
device check (tests/test_gpu_query_key.py) -- numpy only.  Every set is deterministic; key_ray_set(lo, hi) is about 2 * 10^5 rays.

No ray here has an infinite x or y direction component together with dz < 0 (raykey_ref: the one input whose key hangs on the sign of
a generated NaN)."""
import numpy as np

import raykey_ref as R

INF, NAN = float("inf"), float("nan")
# the degenerate rows of tests/test_gpu_ray_query_order.py, test_the_key_separates_directions_and_origins
ODD_ROWS = ((0.0,) * 6, (NAN,) * 6, (INF, -INF, NAN, 0.0, 0.0, 0.0), (1e300, -1e300, 0.0, INF, -INF, 1.0), (0.0, 0.0, 0.0, 5e-324, 0.0, 0.0))
MAGNITUDES = (5e-324, 1e-300, 1e300)
SCALES = (1e-200, 3.0, 1e200)  # d and c * d share a key while |d|_1 stays finite
ORIGIN_MASKS = (0x249, 0x492, 0x924)  # bits 31..20 shifted down: where the cell index of x, y, z lives


def rotated_root_scene(api):
    """A few spheres and a box under a root that carries a non-uniform scale and two rotations: the world bounds of its box are those of
    the 8 transformed corners, not of the transformed (lo, hi) pair."""
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 0.0, 12.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    M = api.Material
    root = scene.root
    root.scale(1.5, 0.6, 2.25)
    root.rotate_z(30.0)
    root.rotate_x(-20.0)
    root.translate([0.25, -0.5, 0.125])
    root.add_box([-1.0, -2.0, -0.5], [2.0, 1.0, 1.5], M.matte([0.8, 0.3, 0.3], 0.0))
    for i in range(24):
        root.add_sphere([-1.5 + 0.15 * i, 1.25 - 0.1 * i, -1.0 + 0.11 * i], 0.2 + 0.01 * (i % 5), M.plastic([0.3, 0.5, 0.8], [0.5, 0.5, 0.5], 0.3))
    return scene


def _with(origins, dirs):
    origins, dirs = np.asarray(origins, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    n = max(len(origins), len(dirs))
    return np.concatenate([np.broadcast_to(origins, (n, 3)), np.broadcast_to(dirs, (n, 3))], axis=1)


def special_directions():
    """Every triple over (+0, -0, +-1, 0.3, -0.7): the six axes, the eight diagonals, every direction with one or two components +-0.0
    (both signs of zero in z among them) and the zero directions of every sign pattern."""
    v = np.array([0.0, -0.0, 1.0, -1.0, 0.3, -0.7])
    g = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)
    assert len(g) == 216
    return g


def fold_directions(rng, n=1500):
    """dz = +0, -0 and one ulp either side of zero (the unfold is taken for dz < 0.0 alone), dx and dy anywhere, also on the axes."""
    xy = rng.normal(0.0, 1.0, (n, 2))
    xy[: n // 10, 0] = 0.0
    xy[n // 10: n // 5, 1] = -0.0
    return np.concatenate([np.concatenate([xy, np.full((n, 1), z)], axis=1) for z in (0.0, -0.0, 5e-324, -5e-324)])


def border_directions():
    """Directions whose octahedral coordinate is exactly a cell border k / 1024, k = 0 .. 1024, and one ulp of the component either side.
    p = k / 512 - 1 is exact, and with the other two components (1 - |p|) * t and (1 - |p|) * (1 - t), t dyadic, |d|_1 is exactly 1: the
    division returns p itself.  Both axes of the map, both hemispheres (on the lower one the border is that of the unfolded coordinate),
    and the same directions times 3 (where |d|_1 and the division round)."""
    k = np.arange(R.DIR_CELLS + 1, dtype=np.float64)
    p = k / (R.DIR_CELLS / 2) - 1.0
    rest = 1.0 - np.abs(p)
    out = []
    for t in (0.25, 1.0):
        for sz in (1.0, -1.0):
            for so in (1.0, -1.0):
                q, z = so * rest * t, sz * rest * (1.0 - t)
                assert np.array_equal((np.abs(p) + np.abs(q)) + np.abs(z), np.ones_like(p))
                for a in (p, np.nextafter(p, -INF), np.nextafter(p, INF)):
                    out.append(np.stack([a, q, z], axis=1))
                    out.append(np.stack([q, a, z], axis=1))
    d = np.concatenate(out)
    return np.concatenate([d, 3.0 * d])


def magnitude_directions(rng, n=400):
    """Small-integer directions times 5e-324, 1e-300 and 1e300 (exact, and |d|_1 finite), and times 1e308 where |d|_1 overflows to
    infinity with every component finite."""
    base = rng.integers(-8, 9, (n, 3)).astype(np.float64)
    base[:8] = [(sx, sy, sz) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    out = [base * m for m in MAGNITUDES]
    big = rng.uniform(-1.7, 1.7, (n, 3)) * 1e308
    big[:8] = base[:8] * 1e308
    with np.errstate(over="ignore"):
        l1 = (np.abs(big[:, 0]) + np.abs(big[:, 1])) + np.abs(big[:, 2])
    big = big[np.isinf(l1)]
    assert np.isfinite(big).all() and len(big) > n // 2
    return np.concatenate(out + [big])


def border_origins(rng, lo, hi, per=24):
    """Origins exactly on every cell border lo + k * (hi - lo) / 16 of every axis, k = 0 .. 16, and one ulp either side; the other two
    coordinates anywhere in the bounds."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    out = []
    for a in range(3):
        for k in range(R.ORIGIN_CELLS + 1):
            b = lo[a] + k * (hi[a] - lo[a]) / R.ORIGIN_CELLS
            for v in (b, np.nextafter(b, -INF), np.nextafter(b, INF)):
                o = rng.uniform(lo, hi, (per, 3))
                o[:, a] = v
                out.append(o)
    return np.concatenate(out)


def key_ray_set(lo, hi, seed=0, n_uniform=80000):
    """The rays the key is demanded bit for bit on, for a scene whose world bounds are [lo, hi]."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    rng = np.random.default_rng(seed)
    centre, size = 0.5 * (lo + hi), hi - lo
    inside = lambda n: rng.uniform(lo, hi, (n, 3))  # noqa: E731
    sets = []
    # origins uniform over 3 x the bounds, normal directions
    sets.append(_with(rng.uniform(centre - 1.5 * size, centre + 1.5 * size, (n_uniform, 3)), rng.normal(0.0, 1.0, (n_uniform, 3))))
    # origins on the cell borders, directions normal and special
    bo = border_origins(rng, lo, hi)
    sp = special_directions()
    sets.append(_with(bo, rng.normal(0.0, 1.0, (len(bo), 3))))
    sets.append(_with(bo, sp[np.arange(len(bo)) % len(sp)]))
    # the special, fold, border and extreme directions from origins in the bounds, and from the bounds' corners and centre
    for d in (sp, fold_directions(rng), border_directions(), magnitude_directions(rng)):
        sets.append(_with(inside(len(d)), d))
    for o in (lo, hi, centre):
        sets.append(_with(o[None, :], sp))
    # NaN, infinities, the zero direction
    sets.append(np.tile(np.array(ODD_ROWS), (30, 1)))
    rays = np.ascontiguousarray(np.concatenate(sets))
    d = rays[:, 3:]
    assert not ((np.isinf(d[:, 0]) | np.isinf(d[:, 1])) & (d[:, 2] < 0.0)).any()
    return rays


def check_reach(rays, bounds):
    """The set is not vacuous (by the restatement alone): every origin cell index on every axis, the first and last direction cell on
    both axes, both hemispheres, at least 5 * 10^4 distinct keys."""
    oc, dc = R.origin_cells(rays, bounds), R.direction_cells(rays)
    for a in range(3):
        assert set(oc[:, a].tolist()) == set(range(R.ORIGIN_CELLS)), (a, sorted(set(oc[:, a].tolist())))
    for a in range(2):
        assert {0, R.DIR_CELLS - 1} <= set(dc[:, a].tolist()), a
    lower = R.octahedral(rays)[2]
    assert lower.sum() > len(rays) // 10 and (~lower).sum() > len(rays) // 10
    distinct = len(np.unique(R.ray_key(rays, bounds)))
    assert distinct >= 50000, distinct


def check_layout(keyfn, lo, hi, seed=0, n=4096):
    """What the documented layout promises, asked of keyfn(rays) -> uint32 keys without going through the restatement:
      one cell along x, y or z at a fixed direction changes bits of that axis's mask in bits 31..20 alone (and changes some);
      another direction leaves bits 31..20 alone;
      d and c * d share a key (|d|_1 finite);
      the +z and -z hemispheres of one (x, y) differ."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    rng = np.random.default_rng(seed)
    cell = (hi - lo) / R.ORIGIN_CELLS
    d = rng.normal(0.0, 1.0, (n, 3))
    for a in range(3):
        c0 = rng.integers(0, R.ORIGIN_CELLS, (n, 3))
        c0[:, a] = rng.integers(0, R.ORIGIN_CELLS - 1, n)
        c1 = c0.copy()
        c1[:, a] += 1
        k0, k1 = keyfn(_with(lo + (c0 + 0.5) * cell, d)), keyfn(_with(lo + (c1 + 0.5) * cell, d))
        x = (k0 ^ k1).astype(np.uint32)
        assert (x != 0).all(), a
        assert (x & np.uint32(0xFFFFF) == 0).all(), a
        assert ((x >> np.uint32(20)) & np.uint32(~ORIGIN_MASKS[a] & 0xFFF) == 0).all(), a
        # ... and the cell index is read in binary: cell i and cell i + 1 differ in exactly the bits that i and i + 1 differ in
        want = R.spread(c0[:, a].astype(np.uint32) ^ c1[:, a].astype(np.uint32), R.ORIGIN_BITS, 3) << np.uint32(a)
        assert np.array_equal(x >> np.uint32(20), want), a
    o = rng.uniform(lo, hi, (n, 3))
    k0, k1 = keyfn(_with(o, d)), keyfn(_with(o, rng.normal(0.0, 1.0, (n, 3))))
    assert np.array_equal(k0 >> np.uint32(20), k1 >> np.uint32(20))
    assert len(np.unique(k0 & np.uint32(0xFFFFF))) > n // 2  # (and the direction is in the low bits)
    for c in SCALES:
        assert np.array_equal(keyfn(_with(o, c * d)), k0), c
    z = np.abs(d[:, 2]) + 0.1 * (np.abs(d[:, 0]) + np.abs(d[:, 1]))  # (|dz| at least a tenth of the rest: far from the fold)
    up, down = keyfn(_with(o, np.stack([d[:, 0], d[:, 1], z], axis=1))), keyfn(_with(o, np.stack([d[:, 0], d[:, 1], -z], axis=1)))
    assert (up != down).all()
    assert np.array_equal(up >> np.uint32(20), down >> np.uint32(20))
