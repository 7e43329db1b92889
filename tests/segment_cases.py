"""The segments of the segment-proximity tests (tests/test_segments_witness.py on the CPU, tests/test_gpu_closest_segments.py on the device)
on the scenes of tests/closest_cases.py: numpy, tests/pyref.py and the brute force (tests/segment_ref.py over tests/closest_ref.py) only.
4097 segments a scene, made without a device: short, medium and long random segments (the long ones at least the bounds' diagonal),
segments through triangles' interiors, segments parallel to a triangle's edge, degenerate segments (closest_cases' own points), the tie
construction (a segment that starts at a mesh vertex pushed away from its mesh and leads farther away: every face around the vertex answers
with that vertex, the same bits), segments inside, through and beside spheres, segments wholly inside boxes, endpoints at 1e6 and
non-finite segments."""
import functools

import numpy as np

import closest_cases as C
import segment_ref as SR

N_SEGMENTS = C.N_POINTS
INF, NAN = float("inf"), float("nan")
SCENES = C.SCENES


def unit(v):
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def make_segments(name, b, pts, seed):
    rng = np.random.default_rng(seed)
    lo, hi = C.world_bounds(b)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    uniform = lambda m: mid + (rng.uniform(-1.5, 1.5, (m, 3)) * half)  # noqa: E731
    direction = lambda m: unit(rng.normal(0.0, 1.0, (m, 3)))  # noqa: E731
    seg = lambda p0, p1: np.concatenate([np.asarray(p0, dtype=np.float64).reshape(-1, 3), np.asarray(p1, dtype=np.float64).reshape(-1, 3)], axis=1)  # noqa: E731
    parts = {}
    p0 = uniform(500)
    parts["medium"] = seg(p0, uniform(500))
    d = direction(300)
    off = mid + rng.uniform(-0.4, 0.4, (300, 3)) * half
    reach = rng.uniform(0.55, 1.5, (300, 1)) * diag
    parts["long"] = seg(off - d * reach, off + d * reach)
    if len(b.tri):
        t = b.tri[rng.integers(0, len(b.tri), 500)]
        w = rng.dirichlet([2.0, 2.0, 2.0], 500)
        inner = (t * w[:, :, None]).sum(axis=1)
        n = unit(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) + 1e-300)
        d = unit(n * rng.choice([-1.0, 1.0], (500, 1)) + rng.normal(0.0, 0.4, (500, 3)))
        edge = np.sqrt(((t[:, 1] - t[:, 0]) ** 2).sum(axis=1))[:, None]
        parts["through"] = seg(inner - d * edge * rng.uniform(0.1, 0.5, (500, 1)), inner + d * edge * rng.uniform(0.1, 0.5, (500, 1)))
        t = b.tri[rng.integers(0, len(b.tri), 200)]
        e = rng.integers(0, 3, 200)
        a, c = t[np.arange(200), e], t[np.arange(200), (e + 1) % 3]
        p0 = a + (c - a) * rng.uniform(-0.5, 0.5, (200, 1)) + direction(200) * np.sqrt(((c - a) ** 2).sum(axis=1))[:, None] * rng.uniform(0.05, 0.6, (200, 1))
        parts["parallel"] = seg(p0, p0 + (c - a) * rng.choice([-2.0, -0.5, 0.25, 1.0], (200, 1)))
        inst = b.ids[len(b.cw) + len(b.box):, 0]
        t0, t1 = [], []
        for i in np.unique(inst):  # closest_cases.tie_points' construction, led farther away
            tri = b.tri[inst == i]
            verts = np.unique(tri.reshape(-1, 3), axis=0)
            edge = np.sqrt(((tri[:, 1] - tri[:, 0]) ** 2).sum(axis=1)).mean()
            pick = verts[:: max(1, len(verts) // 12)][:12]
            away = unit(pick - verts.mean(axis=0))
            for push in (0.5, 2.0):
                t0.append(pick + away * (push * edge))
                t1.append(pick + away * (push * edge) + away * (0.1 * diag))
        parts["ties"] = seg(np.concatenate(t0), np.concatenate(t1))
    parts["degenerate"] = seg(pts[:200], pts[:200])
    if len(b.cw):
        s = rng.integers(0, len(b.cw), 360)
        cw, rad = b.cw[s], np.sqrt(((b.pw[s] - b.cw[s]) ** 2).sum(axis=1))[:, None]
        kind = np.arange(360) % 3
        r0 = np.where(kind == 0, rng.uniform(0.0, 0.8, 360), np.where(kind == 1, rng.uniform(0.0, 0.8, 360), rng.uniform(1.05, 1.6, 360)))[:, None]
        r1 = np.where(kind == 0, rng.uniform(0.0, 0.8, 360), np.where(kind == 1, rng.uniform(1.2, 2.5, 360), rng.uniform(1.05, 1.6, 360)))[:, None]
        d0 = direction(360)
        d1 = np.where((kind == 2)[:, None], unit(d0 + rng.normal(0.0, 0.3, (360, 3))), direction(360))
        parts["spheres"] = seg(cw + d0 * rad * r0, cw + d1 * rad * r1)
    if len(b.box):
        k = rng.integers(0, len(b.box), 240)
        w0, w1 = rng.dirichlet([1.0] * 8, 240), rng.dirichlet([1.0] * 8, 240)
        parts["inside a box"] = seg((b.box[k] * w0[:, :, None]).sum(axis=1), (b.box[k] * w1[:, :, None]).sum(axis=1))
    far = direction(64) * 1e6
    parts["far"] = seg(far, np.where((np.arange(64) % 2 == 0)[:, None], far + direction(64) * 0.5 * diag, uniform(64)))
    bad = seg(uniform(8), uniform(8))
    bad[np.arange(8), [0, 1, 2, 3, 4, 5, 0, 4]] = [NAN, INF, -INF, INF, NAN, NAN, -INF, -INF]
    parts["non-finite"] = bad
    fixed = np.concatenate(list(parts.values()))
    assert len(fixed) <= N_SEGMENTS - 1000, len(fixed)
    p0 = uniform(N_SEGMENTS - len(fixed))
    short = seg(p0, p0 + direction(len(p0)) * diag * rng.uniform(0.005, 0.15, (len(p0), 1)))
    segs = np.concatenate([fixed, short])
    assert segs.shape == (N_SEGMENTS, 6)
    return np.ascontiguousarray(segs[rng.permutation(N_SEGMENTS)]), diag


@functools.lru_cache(maxsize=None)
def case(name):
    """(pyref scene, brute force, segments, the brute force's answer at radius +INF, the bounds' diagonal) of a scene, once."""
    pscene, b, pts, _ = C.case(name)
    segs, diag = make_segments(name, b, pts, 3000 + sorted(list(C.SCENES) + list(C.LIMIT_SCENES)).index(name))
    return pscene, b, segs, SR.closest_segments(b, segs, [INF])[0], diag


def mixed_radii(name, seed):
    """A radius per segment: a seeded mix of +INF, 0, -0.0, the median, 2^-20, NaN, -1 and random values between 0 and twice the median."""
    _, _, segs, want, _ = case(name)
    med = C.radii(want)[2]
    rng = np.random.default_rng(seed)
    fixed = np.array([INF, 0.0, -0.0, med, 2.0 ** -20, NAN, -1.0])
    pick = rng.integers(0, len(fixed) + 3, len(segs))
    return np.where(pick < len(fixed), fixed[np.minimum(pick, len(fixed) - 1)], rng.uniform(0.0, 2.0 * med, len(segs)))


@functools.lru_cache(maxsize=None)
def references(name):
    """The brute force's answers under closest_cases.radii's four shared radii and under mixed_radii(name, 30): five dicts, the candidates
    formed once."""
    _, b, segs, want, _ = case(name)
    return SR.closest_segments(b, segs, list(C.radii(want)) + [mixed_radii(name, 30)])


def lengths(segs):
    with np.errstate(invalid="ignore"):
        return np.sqrt(((segs[:, 3:] - segs[:, :3]) ** 2).sum(axis=1))
