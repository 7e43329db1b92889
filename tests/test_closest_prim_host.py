"""The per-primitive arithmetic of lg_closest_points* on the CPU: lasgun_amd/csrc/closest_prim.h compiled into a stand-alone program
(tools/closest_prim_check.cpp, its own main, nothing loaded into python) with -ffp-contract=off under AddressSanitizer and UBSan, against
the numpy restatement (tests/closest_ref.py, which tests/test_gpu_closest_points.py holds the kernel to) word for word on more than 10^5
seeded (point, primitive) cases: all seven triangle regions, needles and zero-area triangles, repeated vertices, magnitudes from 1e-150 to
1e150, NaN and +-inf, sphere centres, points inside boxes, and groups of candidates with exact ties for the winner's rule.  With this green,
a mismatch on the GPU is the device build's, not the restatement's.  Three seeded faults, built into the check program alone with
-DLG_CLOSEST_FAULT, must each fail the same comparison: a `<` for a `<=` in a region test, a fused product, a swapped tie.

An independent check in exact rational arithmetic (fractions.Fraction) on the same f64 inputs: the stated algorithm run exactly gives the true
squared distance; EVERY returned point -- slivers and far points included -- has barycentrics in [0, 1] within a tolerance worked out for
its row (64 u M / h, plus 16 u (D / h)^2 in the interior region: at most 5.9e-12 on the well-shaped family; for a point above the interior of
a sliver of altitude 1e-7 x its edge the derived tolerance exceeds 1 and says nothing -- measured over all 300 ill-conditioned rows the
barycentrics leave [0, 1] by at most 1.6e-9); the worst relative error of d2 on the well-shaped family (smallest altitude >= 1e-3 x the
longest edge, the point within 100 edge lengths) is recorded below and bounded at 4 x:

    WELL_SHAPED_WORST = 1.2e-14   (measured: see test_the_rational_check_bounds_the_well_shaped_family; slivers' d2 is printed, not
                                   bounded: 1.1e-2 at worst, above a sliver's interior)"""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import closest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined,float-cast-overflow",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
WELL_SHAPED_WORST = 1.2e-14  # the worst relative error of d2 measured on the well-shaped family (DESIGN.md section 3.7 quotes it)
GROUP = 4                    # consecutive records offered to one winner


def random_triangles(rng, m, scale=1.0):
    a = rng.uniform(-2.0, 2.0, (m, 3))
    return a * scale, (a + rng.normal(0.0, 1.0, (m, 3))) * scale, (a + rng.normal(0.0, 1.0, (m, 3))) * scale


def around(rng, a, b, c):
    """Points spread over all seven regions: a barycentric combination well beyond the triangle, lifted off its plane."""
    m = len(a)
    u, v = rng.uniform(-1.0, 2.0, (m, 1)), rng.uniform(-1.0, 2.0, (m, 1))
    n = np.cross(b - a, c - a)
    return a + (b - a) * u + (c - a) * v + n * rng.normal(0.0, 0.5, (m, 1))


def case_set():
    """(records (m, 32), the rows of each family)."""
    rng = np.random.default_rng(28)
    fam, rows = {}, []

    def add(name, kind, q, geom):
        m = len(q)
        rec = np.zeros((m, 32))
        rec[:, 0] = kind
        rec[:, 1:4] = q
        g = np.asarray(geom, dtype=np.float64).reshape(m, -1)
        rec[:, 4:4 + g.shape[1]] = g
        fam[name] = (sum(len(x) for x in rows), m)
        rows.append(rec)

    tri = lambda a, b, c: np.concatenate([a, b, c], axis=1)  # noqa: E731
    a, b, c = random_triangles(rng, 40000)
    add("regions", 3, around(rng, a, b, c), tri(a, b, c))
    # needles (c nearly on ab) and zero-area triangles (c exactly a + (b - a) / 2, or beyond b)
    a, b, _ = random_triangles(rng, 9000)
    t = rng.uniform(-0.5, 1.5, (9000, 1))
    c = a + (b - a) * t + rng.normal(0.0, 1.0, (9000, 3)) * rng.choice([0.0, 1e-300, 1e-17, 1e-12, 1e-8, 1e-4], (9000, 1))
    c[:1500] = (a[:1500] + b[:1500]) / 2.0
    add("needles", 3, around(rng, a, b, a + rng.normal(0.0, 1.0, (9000, 3))), tri(a, b, c))
    # repeated vertices: a == b, b == c, a == c, all three
    a, b, c = random_triangles(rng, 8000)
    which = np.arange(8000) % 4
    b = np.where((which == 0)[:, None] | (which == 3)[:, None], a, b)
    c = np.where((which == 1)[:, None], b, np.where((which == 2)[:, None] | (which == 3)[:, None], a, c))
    add("repeated", 3, a + rng.normal(0.0, 1.0, (8000, 3)), tri(a, b, c))
    # magnitudes 1e-150 .. 1e150
    scale = 10.0 ** rng.uniform(-150.0, 150.0, (12000, 1))
    scale[:4] = [[1e-150], [1e150], [1e-160], [1e154]]
    a, b, c = random_triangles(rng, 12000)
    add("scaled", 3, around(rng, a, b, c) * scale, tri(a * scale, b * scale, c * scale))
    # NaN and +-inf anywhere
    a, b, c = random_triangles(rng, 6000)
    add("poison", 3, around(rng, a, b, c), tri(a, b, c))
    lo = fam["poison"][0]
    rows[-1][np.arange(6000), rng.integers(1, 13, 6000)] = rng.choice([NAN, INF, -INF, 0.0, -0.0, 1e308, -1e308], 6000)
    assert lo == sum(len(x) for x in rows[:-1])
    # spheres: general, the centre itself (l == 0), inside, and poisoned
    cw = rng.uniform(-3.0, 3.0, (12000, 3))
    pw = cw + rng.normal(0.0, 1.0, (12000, 3))
    q = cw + rng.normal(0.0, 1.0, (12000, 3)) * rng.choice([0.0, 1e-200, 0.3, 1.0, 5.0, 1e6], (12000, 1))
    q[:64, 0] = rng.choice([NAN, INF, -INF], 64)
    add("spheres", 1, q, np.concatenate([cw, pw], axis=1))
    # boxes: the unit box's corners under a random affine map; points inside, outside, on corners; one flat box in four
    unit = np.array([[k & 1, (k >> 1) & 1, (k >> 2) & 1] for k in range(8)], dtype=np.float64)
    m = 9000
    lin = rng.normal(0.0, 1.0, (m, 3, 3))
    lin[::4, :, 2] = 0.0  # flat: the corners coincide in pairs
    org = rng.uniform(-2.0, 2.0, (m, 1, 3))
    corners = org + np.einsum("kj,mij->mki", unit, lin)
    q = org[:, 0] + np.einsum("mj,mij->mi", rng.uniform(-0.5, 1.5, (m, 3)), lin)
    q[:500] = corners[:500, 3]
    add("boxes", 2, q, corners.reshape(m, 24))
    # ties: a group's records 0 and 2 (and 1 and 3) are the same primitive under different keys, larger key first and smaller key first
    a, b, c = random_triangles(rng, 2000)
    q = around(rng, a, b, c)
    rep = lambda x: np.repeat(x, 4, axis=0)  # noqa: E731
    add("ties", 3, rep(q), tri(rep(a), rep(b), rep(c)))
    rec = np.ascontiguousarray(np.concatenate(rows))
    m = len(rec)
    group = np.arange(m) // GROUP
    rec[:, 28] = group
    rec[:, 29] = rng.integers(0, 5, m)           # instance
    rec[:, 30] = rng.integers(0, 1000, m)        # prim
    rec[:, 31] = np.repeat(rng.choice([INF, 0.0, 0.5, 4.0, 100.0], m // GROUP + 1), GROUP)[:m]  # r2, one a group
    lo, n = fam["ties"]
    assert lo % GROUP == 0
    rec[lo:lo + n, 29] = np.tile([3, 1, 1, 3], n // 4)  # the same d2 four times over: the smallest (instance, kind, prim) must win from either side
    rec[lo:lo + n, 30] = np.tile([7, 9, 9, 2], n // 4)
    rec[lo:lo + n, 31] = INF
    return rec, fam


def restated(rec):
    """What the program must write: (m, 9)."""
    kind, q, g = rec[:, 0].astype(np.int64), rec[:, 1:4], rec[:, 4:28]
    m = len(rec)
    x, d2 = np.zeros((m, 3)), np.zeros(m)
    t = kind == 3
    x[t], d2[t], _ = R.closest_triangle(q[t], g[t, 0:3], g[t, 3:6], g[t, 6:9])
    s = kind == 1
    x[s], d2[s] = R.closest_sphere(q[s], g[s, 0:3], g[s, 3:6])
    b = kind == 2
    x[b], d2[b], _ = R.closest_box(q[b], g[b].reshape(-1, 8, 3))
    key = (rec[:, 29].astype(np.uint64) << np.uint64(34)) | (kind.astype(np.uint64) << np.uint64(32)) | rec[:, 30].astype(np.uint64)
    out = np.zeros((m, 9))
    out[:, 0:3], out[:, 3] = x, d2
    best_d2, best_key, best_x = INF, -1.0, np.zeros(3)
    for i in range(m):  # the winner's rule, record by record as the program offers them
        if i % GROUP == 0:
            best_d2, best_key, best_x = INF, -1.0, np.zeros(3)
        d, k = d2[i], float(key[i])
        if d <= rec[i, 31] and d < INF and (d < best_d2 or (d == best_d2 and (best_key < 0 or k < best_key))):
            best_d2, best_key, best_x = d, k, x[i]
        out[i, 4], out[i, 5], out[i, 6:9] = best_d2, best_key, best_x
    return out


def build(cxx, exe, fault=0):
    subprocess.check_call([cxx] + FLAGS + (["-DLG_CLOSEST_FAULT=%d" % fault] if fault else []) + [os.path.join(ROOT, "tools", "closest_prim_check.cpp"), "-o", exe])


def run(exe, tmp, rec):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    rec.tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "closest_prim_check: ok, %d cases" % len(rec) in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    out = np.fromfile(dst, dtype=np.float64).reshape(-1, 9)
    assert len(out) == len(rec)
    return out


def differences(out, want):
    """Rows where the program and the restatement differ in any word; a NaN is SOME NaN."""
    nan = np.isnan(want)
    bad = (np.isnan(out) != nan).any(axis=1)
    g, w = np.where(nan, 0.0, out), np.where(nan, 0.0, want)
    bad |= (np.ascontiguousarray(g).view(np.uint64) != np.ascontiguousarray(w).view(np.uint64)).any(axis=1)
    return np.nonzero(bad)[0]


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    tmp = str(tmp_path_factory.mktemp("closest_prim"))
    exe = os.path.join(tmp, "closest_prim_check")
    build(cxx, exe)
    rec, fam = case_set()
    return cxx, tmp, exe, rec, fam, restated(rec)


def test_the_case_set_reaches_every_class(bench):
    _, _, _, rec, fam, want = bench
    assert len(rec) >= 100000
    rows = lambda name: slice(fam[name][0], fam[name][0] + fam[name][1])  # noqa: E731
    r = rec[rows("regions")]
    _, region = R.closest_on_triangle(r[:, 1:4], r[:, 4:7], r[:, 7:10], r[:, 10:13])
    assert all((region == k).sum() >= 1000 for k in range(1, 8)), np.bincount(region, minlength=8)
    assert np.isnan(want[rows("repeated"), 3]).any() and not np.isnan(want[rows("repeated"), 3]).all(), "a repeated vertex: a vertex, an edge point or NaN"
    assert np.isnan(want[rows("poison"), 3]).sum() >= 1000
    s = rec[rows("spheres")]
    assert ((s[:, 1:4] == s[:, 4:7]).all(axis=1)).sum() >= 500, "the sphere's centre itself"
    assert np.isfinite(want[rows("scaled"), 3]).mean() > 0.3 and not np.isfinite(want[rows("scaled"), 3]).all(), "magnitudes that overflow d2 and magnitudes that do not"
    bx = want[rows("boxes")]
    assert (bx[:, 3] == 0.0).sum() >= 100 and (bx[:, 3] > 0.0).sum() >= 1000 and np.isfinite(bx[:, 3]).all()
    t = want[rows("ties")].reshape(-1, GROUP, 9)
    k = lambda i, p: float((i << 34) | (3 << 32) | p)  # noqa: E731
    assert (t[:, -1, 5] == k(1, 9)).all() and (t[:, 0, 5] == k(3, 7)).all() and (t[:, 3, 3] == t[:, 0, 3]).all(), "four equal d2: the smallest key wins from either side"
    assert (want[:, 5] < 0).sum() >= 1000 and (want[:, 5] >= 0).sum() >= 50000, "radii that exclude and radii that admit"


def test_header_and_restatement_agree_word_for_word(bench):
    _, tmp, exe, rec, fam, want = bench
    bad = differences(run(exe, tmp, rec), want)
    where = [n for n in fam if len(bad) and fam[n][0] <= bad[0] < fam[n][0] + fam[n][1]]
    assert len(bad) == 0, (len(bad), int(bad[0]), where, rec[bad[0]].tolist())


@pytest.mark.parametrize("fault", [1, 2, 3])
def test_a_seeded_fault_fails_the_comparison(bench, fault):
    """1: `d4 < d3` for `d4 <= d3` in step 2; 2: vc formed with a fused multiply-add; 3: an exact tie given to the LARGER key."""
    cxx, tmp, _, rec, _, want = bench
    tree = os.path.join(tmp, "fault%d" % fault)
    os.makedirs(tree)
    exe = os.path.join(tree, "closest_prim_check")
    build(cxx, exe, fault)
    assert len(differences(run(exe, tree, rec), want)) >= 10, fault


# ---- the independent check: the stated algorithm in exact rational arithmetic ------------------------------------------------------------
def exact_d2(q, a, b, c):
    """(d2, v, w) of the header's algorithm run on Fractions: the true squared distance and the closest point's barycentrics (x = a + v ab + w ac)."""
    F = lambda p: [Fraction(float(t)) for t in p]  # noqa: E731
    q, a, b, c = F(q), F(a), F(b), F(c)
    sub = lambda u, v: [u[i] - v[i] for i in range(3)]  # noqa: E731
    dt = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]  # noqa: E731
    ab, ac, ap = sub(b, a), sub(c, a), sub(q, a)
    d1, d2 = dt(ab, ap), dt(ac, ap)
    bp = sub(q, b)
    d3, d4 = dt(ab, bp), dt(ac, bp)
    cp = sub(q, c)
    d5, d6 = dt(ab, cp), dt(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    if d1 <= 0 and d2 <= 0:
        v, w = Fraction(0), Fraction(0)
    elif d3 >= 0 and d4 <= d3:
        v, w = Fraction(1), Fraction(0)
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        v, w = d1 / (d1 - d3), Fraction(0)
    elif d6 >= 0 and d5 <= d6:
        v, w = Fraction(0), Fraction(1)
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        v, w = Fraction(0), d2 / (d2 - d6)
    elif va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v = 1 - w
    else:
        den = 1 / (va + vb + vc)
        v, w = vb * den, vc * den
    x = [a[i] + ab[i] * v + ac[i] * w for i in range(3)]
    e = sub(q, x)
    return dt(e, e), v, w


def barycentrics_of(x, a, b, c):
    """The exact least-squares barycentrics (v, w) of a returned point x (floats) in the plane of (a, b, c)."""
    F = lambda p: [Fraction(float(t)) for t in p]  # noqa: E731
    x, a, b, c = F(x), F(a), F(b), F(c)
    ab, ac, ax = [b[i] - a[i] for i in range(3)], [c[i] - a[i] for i in range(3)], [x[i] - a[i] for i in range(3)]
    dt = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]  # noqa: E731
    g11, g12, g22, r1, r2 = dt(ab, ab), dt(ab, ac), dt(ac, ac), dt(ab, ax), dt(ac, ax)
    det = g11 * g22 - g12 * g12
    return (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det


def test_the_rational_check_bounds_the_well_shaped_family():
    """Every row -- slivers and far points included -- is held to barycentrics in [0, 1] within a tolerance worked out for that row
    (DESIGN.md section 3.7), u = 2^-53: the returned point is off the triangle by at most a few u of the largest coordinate M, which the
    smallest altitude h turns into 64 u M / h of a barycentric; in the interior region (7) the barycentrics themselves come from
    differences of products of size (E D)^2 that stand for (E h)^2, D the distance from a to the point: 16 u (D / h)^2 more.  The relative
    error of d2 is bounded on the well-shaped family alone; for the rest it is printed."""
    rng = np.random.default_rng(2828)
    m = 1500
    a, b, c = random_triangles(rng, m)
    q = around(rng, a, b, c) + rng.normal(0.0, 1.0, (m, 3)) * rng.choice([0.0, 1.0, 30.0], (m, 1))
    # slivers: c pulled towards the line ab; a tenth of them with the point above the sliver's own interior (region 7 of a sliver)
    sl = np.arange(m) % 5 == 0
    c[sl] = a[sl] + (b[sl] - a[sl]) * rng.uniform(0.1, 0.9, (sl.sum(), 1)) + (c[sl] - a[sl]) * 1e-7
    above = np.arange(m) % 50 == 0
    n = np.cross(b - a, c - a)
    q[above] = (a + (b - a) * 0.3 + (c - a) * 0.3 + n / np.sqrt((n * n).sum(axis=1))[:, None] * rng.uniform(0.01, 1.0, (m, 1)))[above]
    x, d2, region = R.closest_triangle(q, a, b, c)
    edges = np.sqrt(np.maximum(((b - a) ** 2).sum(axis=1), np.maximum(((c - a) ** 2).sum(axis=1), ((c - b) ** 2).sum(axis=1))))
    h = np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1)) / edges  # the smallest altitude
    dist = np.sqrt(((q - a) ** 2).sum(axis=1))
    well = (h >= 1e-3 * edges) & (dist <= 100.0 * edges)
    big = np.maximum(np.maximum(np.abs(a).max(axis=1), np.abs(b).max(axis=1)), np.maximum(np.abs(c).max(axis=1), np.abs(q).max(axis=1)))
    u = 2.0 ** -53
    tol = 64.0 * u * big / h + np.where(region == 7, 16.0 * u * (dist / h) ** 2, 0.0)
    worst, excess = {True: 0.0, False: 0.0}, {True: 0.0, False: 0.0}
    for i in range(m):
        exact, _, _ = exact_d2(q[i], a[i], b[i], c[i])
        v, w = barycentrics_of(x[i], a[i], b[i], c[i])
        t = Fraction(float(tol[i]))
        assert -t <= v and -t <= w and v + w <= 1 + t, (i, float(v), float(w), int(region[i]), float(tol[i]), bool(well[i]))
        excess[bool(well[i])] = max(excess[bool(well[i])], float(max(-v, -w, v + w - 1, 0)))
        if exact > 0:
            rel = abs(float((Fraction(float(d2[i])) - exact) / exact))
            worst[bool(well[i])] = max(worst[bool(well[i])], rel)
    print("closest point on a triangle, relative error of d2 against exact arithmetic: well-shaped %.3e (%d cases), slivers and far points %.3e (%d cases)"
          % (worst[True], int(well.sum()), worst[False], int((~well).sum())))
    print("barycentrics outside [0, 1] by at most: well-shaped %.3e (largest tolerance %.3e), slivers and far points %.3e (largest tolerance %.3e; region 7 of a sliver: %d cases)"
          % (excess[True], tol[well].max(), excess[False], tol[~well].max(), int((sl & (region == 7)).sum())))
    assert well.sum() >= 800 and (sl & (region == 7)).sum() >= 10
    assert tol[well].max() <= 1e-9, "the well-shaped family is held to [0, 1] within 1e-9 at the least"
    assert worst[True] <= 4.0 * WELL_SHAPED_WORST, worst
