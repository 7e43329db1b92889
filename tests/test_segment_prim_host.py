"""The per-primitive arithmetic of lg_closest_segments* on the CPU: lasgun_amd/csrc/segment_prim.h compiled into a stand-alone program
(tools/segment_prim_check.cpp, its own main, nothing loaded into python) with -ffp-contract=off under AddressSanitizer and UBSan -- built
exactly as tests/test_closest_prim_host.py builds its program --, against the numpy restatement (tests/segment_ref.py, which
tests/test_gpu_closest_segments.py holds the kernel to) word for word on more than 10^5 seeded (segment, primitive) cases: every one of the
six triangle sub-candidates as the winner, lattice coordinates (exact zeros, exact ties, parallel and collinear segments), segments parallel
to an edge, degenerate segments, needles and repeated vertices, magnitudes from 1e-150 to 1e150, NaN and +-inf, the three sphere cases,
segments inside, outside and through boxes, and groups of candidates with exact ties for the winner's rule.  Three seeded faults, built
into the check program alone with -DLG_SEGMENT_FAULT, must each fail the same comparison: a `<` for a `<=` in the parameter clamp, a fused
product in the segment-segment denominator, a swapped tie between sub-candidates.

An independent check, so that the restatement is not its own judge: the header's steps in exact rational arithmetic (fractions.Fraction;
square roots to 2^-200) on the same f64 inputs, for the triangle candidate and the sphere's two non-crossing cases, on well-shaped triangles
(smallest altitude >= 1e-3 x the longest edge) and segments within 100 edge lengths -- the shape class of tests/test_closest_prim_host.py.
The worst relative error of d2 measured there is recorded below and bounded at twice that; "d2 == 0 iff the exact segment meets the exact
primitive" holds on every case whose exact distance exceeds 2^-30 of the input magnitude or is zero by construction.
For the sphere the check runs in ONE direction only: its cases are built never to meet the surface (the non-crossing cases), and it asserts
that none is classified as crossing; that a true crossing gives d2 == 0 is the word-for-word test's and the GPU test's, not this one's.

    TRIANGLE_WORST = 6.1e-14, SPHERE_WORST = 1.4e-15   (measured: see test_the_rational_check_bounds_the_well_shaped_family)"""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import closest_ref as R
import segment_ref as SR
from test_closest_prim_host import FLAGS, around, differences, random_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
TRIANGLE_WORST = 6.1e-14  # the worst relative error of d2 measured on the well-shaped family (DESIGN.md section 3.7 quotes both)
SPHERE_WORST = 1.4e-15
GROUP = 4
W = 36


def segments_around(rng, a, b, c, spread=1.0):
    return around(rng, a, b, c), around(rng, a, b, c) + rng.normal(0.0, spread, a.shape)


def case_set():
    """(records (m, 36), the rows of each family)."""
    rng = np.random.default_rng(30)
    fam, rows = {}, []

    def add(name, kind, p0, p1, geom):
        m = len(p0)
        rec = np.zeros((m, W))
        rec[:, 0] = kind
        rec[:, 1:4], rec[:, 4:7] = p0, p1
        g = np.asarray(geom, dtype=np.float64).reshape(m, -1)
        rec[:, 7:7 + g.shape[1]] = g
        fam[name] = (sum(len(x) for x in rows), m)
        rows.append(rec)

    tri = lambda a, b, c: np.concatenate([a, b, c], axis=1)  # noqa: E731
    a, b, c = random_triangles(rng, 30000)
    p0, p1 = segments_around(rng, a, b, c)
    add("general", 3, p0, p1, tri(a, b, c))
    # lattice coordinates: exact zeros and ties, parallel, collinear and touching configurations
    lat = lambda m: rng.integers(-2, 3, (m, 3)).astype(np.float64)  # noqa: E731
    add("lattice", 3, lat(16000), lat(16000), tri(lat(16000), lat(16000), lat(16000)))
    # parallel to an edge: p1 - p0 an exact multiple of b - a (binary fractions keep it exact often, not always)
    a, b, c = random_triangles(rng, 8000)
    p0 = around(rng, a, b, c)
    add("parallel", 3, p0, p0 + (b - a) * rng.choice([-2.0, -0.5, 0.25, 1.0, 3.0], (8000, 1)), tri(a, b, c))
    # degenerate segments
    a, b, c = random_triangles(rng, 6000)
    p0 = around(rng, a, b, c)
    add("degenerate", 3, p0, p0.copy(), tri(a, b, c))
    # needles, zero-area triangles and repeated vertices
    a, b, _ = random_triangles(rng, 8000)
    t = rng.uniform(-0.5, 1.5, (8000, 1))
    c = a + (b - a) * t + rng.normal(0.0, 1.0, (8000, 3)) * rng.choice([0.0, 1e-300, 1e-17, 1e-12, 1e-8, 1e-4], (8000, 1))
    c[:1000] = (a[:1000] + b[:1000]) / 2.0
    which = np.arange(8000) % 8
    b = np.where((which == 5)[:, None] | (which == 7)[:, None], a, b)
    c = np.where((which == 6)[:, None] | (which == 7)[:, None], a, c)
    p0, p1 = segments_around(rng, a, b, a + rng.normal(0.0, 1.0, (8000, 3)))
    add("needles", 3, p0, p1, tri(a, b, c))
    # magnitudes 1e-150 .. 1e150
    scale = 10.0 ** rng.uniform(-150.0, 150.0, (8000, 1))
    scale[:4] = [[1e-150], [1e150], [1e-160], [1e154]]
    a, b, c = random_triangles(rng, 8000)
    p0, p1 = segments_around(rng, a, b, c)
    add("scaled", 3, p0 * scale, p1 * scale, tri(a * scale, b * scale, c * scale))
    # NaN and +-inf anywhere
    a, b, c = random_triangles(rng, 5000)
    p0, p1 = segments_around(rng, a, b, c)
    add("poison", 3, p0, p1, tri(a, b, c))
    rows[-1][np.arange(5000), rng.integers(1, 16, 5000)] = rng.choice([NAN, INF, -INF, 0.0, -0.0, 1e308, -1e308], 5000)
    # spheres: outside, inside, crossing, through the centre, degenerate, lattice
    m = 14000
    cw = rng.uniform(-3.0, 3.0, (m, 3))
    pw = cw + rng.normal(0.0, 1.0, (m, 3))
    rad = np.sqrt(((pw - cw) ** 2).sum(axis=1))[:, None]
    unit = lambda: (lambda v: v / np.sqrt((v * v).sum(axis=1))[:, None])(rng.normal(0.0, 1.0, (m, 3)))  # noqa: E731
    p0 = cw + unit() * rad * rng.choice([0.0, 0.2, 0.9, 1.0, 1.1, 3.0], (m, 1))
    p1 = cw + unit() * rad * rng.choice([0.0, 0.2, 0.9, 1.0, 1.1, 3.0], (m, 1))
    p1[:1000] = p0[:1000]
    p0[1000:3000], p1[1000:3000], cw[1000:3000], pw[1000:3000] = lat(2000), lat(2000), lat(2000), lat(2000)
    p0[3000:3064, 0] = rng.choice([NAN, INF, -INF], 64)
    add("spheres", 1, p0, p1, np.concatenate([cw, pw], axis=1))
    # boxes: the unit box under a random affine map; segments inside, outside, through; one flat box in four
    unit8 = np.array([[k & 1, (k >> 1) & 1, (k >> 2) & 1] for k in range(8)], dtype=np.float64)
    m = 4000
    lin = rng.normal(0.0, 1.0, (m, 3, 3))
    lin[::4, :, 2] = 0.0
    org = rng.uniform(-2.0, 2.0, (m, 1, 3))
    corners = org + np.einsum("kj,mij->mki", unit8, lin)
    inside = lambda lo, hi: org[:, 0] + np.einsum("mj,mij->mi", rng.uniform(lo, hi, (m, 3)), lin)  # noqa: E731
    p0, p1 = inside(-0.5, 1.5), inside(-0.5, 1.5)
    p0[:1200], p1[:1200] = inside(0.1, 0.9)[:1200], inside(0.1, 0.9)[:1200]
    p1[1200:1400] = p0[1200:1400]
    p0[1400:1600] = corners[1400:1600, 3]
    add("boxes", 2, p0, p1, corners.reshape(m, 24))
    # ties: a group's four records are the same primitive and segment under different keys
    a, b, c = random_triangles(rng, 1500)
    p0, p1 = segments_around(rng, a, b, c)
    rep = lambda x: np.repeat(x, 4, axis=0)  # noqa: E731
    add("ties", 3, rep(p0), rep(p1), tri(rep(a), rep(b), rep(c)))
    pad = (-sum(len(x) for x in rows[:-1])) % GROUP
    assert pad == 0, "the tie groups start on a group boundary"
    rec = np.ascontiguousarray(np.concatenate(rows))
    m = len(rec)
    rec[:, 31] = np.arange(m) // GROUP
    rec[:, 32] = rng.integers(0, 5, m)
    rec[:, 33] = rng.integers(0, 1000, m)
    rec[:, 34] = np.repeat(rng.choice([INF, 0.0, 0.5, 4.0, 100.0], m // GROUP + 1), GROUP)[:m]
    lo, n = fam["ties"]
    rec[lo:lo + n, 32] = np.tile([3, 1, 1, 3], n // 4)
    rec[lo:lo + n, 33] = np.tile([7, 9, 9, 2], n // 4)
    rec[lo:lo + n, 34] = INF
    return rec, fam


def restated(rec):
    """What the program must write: (m, 12)."""
    kind, p0, p1, g = rec[:, 0].astype(np.int64), rec[:, 1:4], rec[:, 4:7], rec[:, 7:31]
    m = len(rec)
    x, s, d2, which = np.zeros((m, 3)), np.zeros(m), np.zeros(m), np.zeros(m)
    t = kind == 3
    x[t], s[t], d2[t], which[t] = SR.seg_triangle(p0[t], p1[t], g[t, 0:3], g[t, 3:6], g[t, 6:9])
    sp = kind == 1
    x[sp], s[sp], d2[sp], _ = SR.seg_sphere(p0[sp], p1[sp], g[sp, 0:3], g[sp, 3:6])
    b = kind == 2
    x[b], s[b], d2[b], _ = SR.seg_box(p0[b], p1[b], g[b].reshape(-1, 8, 3))
    key = (rec[:, 32].astype(np.uint64) << np.uint64(34)) | (kind.astype(np.uint64) << np.uint64(32)) | rec[:, 33].astype(np.uint64)
    out = np.zeros((m, 12))
    out[:, 0:3], out[:, 3], out[:, 4], out[:, 5] = x, s, d2, which
    best = (INF, -1.0, 0.0, np.zeros(3))
    for i in range(m):  # the winner's rule, record by record as the program offers them
        if i % GROUP == 0:
            best = (INF, -1.0, 0.0, np.zeros(3))
        d, k = d2[i], float(key[i])
        if d <= rec[i, 34] and d < INF and (d < best[0] or (d == best[0] and (best[1] < 0 or k < best[1]))):
            best = (d, k, s[i], x[i])
        out[i, 6], out[i, 7], out[i, 8], out[i, 9:12] = best
    return out


def build(cxx, exe, fault=0):
    subprocess.check_call([cxx] + FLAGS + (["-DLG_SEGMENT_FAULT=%d" % fault] if fault else []) + [os.path.join(ROOT, "tools", "segment_prim_check.cpp"), "-o", exe])


def run(exe, tmp, rec):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    rec.tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "segment_prim_check: ok, %d cases" % len(rec) in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    out = np.fromfile(dst, dtype=np.float64).reshape(-1, 12)
    assert len(out) == len(rec)
    return out


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    tmp = str(tmp_path_factory.mktemp("segment_prim"))
    exe = os.path.join(tmp, "segment_prim_check")
    build(cxx, exe)
    rec, fam = case_set()
    return cxx, tmp, exe, rec, fam, restated(rec)


def test_the_case_set_reaches_every_class(bench):
    _, _, _, rec, fam, want = bench
    assert len(rec) >= 100000
    rows = lambda name: slice(fam[name][0], fam[name][0] + fam[name][1])  # noqa: E731
    which = want[rows("general"), 5].astype(int)
    print("general triangles, winners by sub-candidate 1 .. 6:", np.bincount(which, minlength=7)[1:].tolist())
    assert all((which == k).sum() >= 300 for k in range(1, 7)), np.bincount(which, minlength=7)
    lat = want[rows("lattice")]
    assert (lat[:, 4] == 0.0).sum() >= 1000 and (lat[:, 4] > 0.0).sum() >= 1000, "lattice: touching configurations beside separated ones"
    assert (want[rows("degenerate"), 5] == 0).all() and (want[rows("degenerate"), 3] == 0.0).all()
    poison = ~np.isfinite(rec[rows("poison"), 1:16]).all(axis=1)
    assert poison.sum() >= 1500 and np.isfinite(want[rows("poison"), 4]).all(), "ONE poisoned word: a NaN sub-candidate never replaces anything, and one that involves neither the word is left"
    assert np.isfinite(want[rows("scaled"), 4]).mean() > 0.3 and not np.isfinite(want[rows("scaled"), 4]).all()
    s = rec[rows("spheres")]
    case = SR.seg_sphere(s[:, 1:4], s[:, 4:7], s[:, 7:10], s[:, 10:13])[3]
    print("spheres by case (point, outside, inside, crossing, fallback):", [int((case == k).sum()) for k in range(10, 15)])
    assert all((case == k).sum() >= 500 for k in (SR.SPHERE_POINT, SR.SPHERE_OUTSIDE, SR.SPHERE_INSIDE, SR.SPHERE_CROSSING))
    bx = want[rows("boxes")]
    assert (bx[:, 4] == 0.0).sum() >= 300 and (bx[:, 4] > 0.0).sum() >= 1000
    t = want[rows("ties")].reshape(-1, GROUP, 12)
    k = lambda i, p: float((i << 34) | (3 << 32) | p)  # noqa: E731
    assert (t[:, -1, 7] == k(1, 9)).all() and (t[:, 0, 7] == k(3, 7)).all(), "four equal d2: the smallest key wins from either side"
    assert np.signbit(want[:, 3]).sum() == 0 and np.signbit(want[:, 8]).sum() == 0, "a parameter is never -0.0"
    ok = ~np.isnan(want[:, 3])
    assert (want[ok, 3] >= 0.0).all() and (want[ok, 3] <= 1.0).all()


def test_header_and_restatement_agree_word_for_word(bench):
    _, tmp, exe, rec, fam, want = bench
    bad = differences(run(exe, tmp, rec), want)
    where = [n for n in fam if len(bad) and fam[n][0] <= bad[0] < fam[n][0] + fam[n][1]]
    assert len(bad) == 0, (len(bad), int(bad[0]), where, rec[bad[0]].tolist())


@pytest.mark.parametrize("fault", [1, 2, 3])
def test_a_seeded_fault_fails_the_comparison(bench, fault):
    """1: `x < 0` for `x <= 0` in seg_clamp01 (a -0.0 parameter escapes); 2: the segment-segment denominator formed with a fused
    multiply-add; 3: a tie between two sub-candidates given to the LATER one."""
    cxx, tmp, _, rec, _, want = bench
    tree = os.path.join(tmp, "fault%d" % fault)
    os.makedirs(tree)
    exe = os.path.join(tree, "segment_prim_check")
    build(cxx, exe, fault)
    assert len(differences(run(exe, tree, rec), want)) >= 10, fault


# ---- the independent check: the header's steps in exact rational arithmetic -----------------------------------------------------------------
def F(p):
    return [Fraction(float(t)) for t in p]


def fsub(u, v):
    return [u[i] - v[i] for i in range(3)]


def fdot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def fcross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def fclamp(x):
    return min(max(x, Fraction(0)), Fraction(1))


def fsqrt(x):
    """sqrt of a non-negative Fraction, within 2^-200 relative."""
    if x == 0:
        return Fraction(0)
    shift = 400 + 2 * max(0, x.denominator.bit_length() - x.numerator.bit_length())
    return Fraction(math.isqrt((x.numerator << shift) // x.denominator), 1 << (shift // 2))


def exact_point_triangle(q, a, b, c):
    from test_closest_prim_host import exact_d2
    return exact_d2([float(t) for t in q], [float(t) for t in a], [float(t) for t in b], [float(t) for t in c])[0]


def exact_edge(p0, p1, e0, e1):
    d1, d2, r = fsub(p1, p0), fsub(e1, e0), fsub(p0, e0)
    a, e, f = fdot(d1, d1), fdot(d2, d2), fdot(d2, r)
    assert a > 0 and e > 0, "the well-shaped family: neither the segment nor an edge is a point (the header's a <= 0 and e <= 0 branches are the word-for-word test's)"
    c, b = fdot(d1, r), fdot(d1, d2)
    denom = a * e - b * b
    s = fclamp((b * f - c * e) / denom) if denom != 0 else Fraction(0)
    t = (b * s + f) / e
    if t < 0:
        t, s = Fraction(0), fclamp(-c / a)
    elif t > 1:
        t, s = Fraction(1), fclamp((b - c) / a)
    w = [p0[i] + d1[i] * s - e0[i] - d2[i] * t for i in range(3)]
    return fdot(w, w)


def exact_triangle(p0, p1, a, b, c):
    """The exact squared distance of segment and triangle: the header's six sub-candidates in exact arithmetic."""
    p0, p1, a, b, c = F(p0), F(p1), F(a), F(b), F(c)
    ab, ac, qp = fsub(b, a), fsub(c, a), fsub(p0, p1)
    n = fcross(ab, ac)
    d, ap = fdot(qp, n), fsub(p0, a)
    t, e = fdot(ap, n), fcross(qp, ap)
    v, w = fdot(ac, e), -fdot(ab, e)
    if d < 0:
        d, t, v, w = -d, -t, -v, -w
    if d > 0 and 0 <= t <= d and v >= 0 and w >= 0 and v + w <= d:
        return Fraction(0)
    return min(exact_point_triangle(p0, a, b, c), exact_point_triangle(p1, a, b, c), exact_edge(p0, p1, a, b), exact_edge(p0, p1, b, c), exact_edge(p0, p1, c, a))


def exact_sphere(p0, p1, cw, pw):
    """(the exact distance, squared, of the segment to the sphere's surface; does the exact segment meet it)."""
    p0, p1, cw, pw = F(p0), F(p1), F(cw), F(pw)
    rw2 = fdot(fsub(pw, cw), fsub(pw, cw))
    u, v0, v1 = fsub(p1, p0), fsub(p0, cw), fsub(p1, cw)
    s = fclamp(fdot(fsub(cw, p0), u) / fdot(u, u))
    vm = [v0[i] + u[i] * s for i in range(3)]
    lmin2, lmax2 = fdot(vm, vm), max(fdot(v0, v0), fdot(v1, v1))
    if lmin2 > rw2:
        d = fsqrt(lmin2) - fsqrt(rw2)
        return d * d, False
    if lmax2 < rw2:
        d = fsqrt(rw2) - fsqrt(lmax2)
        return d * d, False
    return Fraction(0), True


def test_the_rational_check_bounds_the_well_shaped_family():
    rng = np.random.default_rng(3030)
    m = 1200
    a, b, c = random_triangles(rng, m)
    p0 = around(rng, a, b, c) + rng.normal(0.0, 1.0, (m, 3)) * rng.choice([0.0, 1.0, 30.0], (m, 1))
    p1 = p0 + rng.normal(0.0, 1.0, (m, 3)) * rng.choice([0.3, 1.0, 5.0], (m, 1))
    # zero by construction: the segment through an interior point of the triangle, both ends well off the plane
    zero = np.arange(m) % 6 == 0
    inner = a + (b - a) * 0.3 + (c - a) * 0.3
    nrm = np.cross(b - a, c - a)
    p0[zero], p1[zero] = (inner + nrm)[zero], (inner - nrm * 0.5)[zero]
    edges = np.sqrt(np.maximum(((b - a) ** 2).sum(axis=1), np.maximum(((c - a) ** 2).sum(axis=1), ((c - b) ** 2).sum(axis=1))))
    h = np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1)) / edges
    far = np.maximum(np.sqrt(((p0 - a) ** 2).sum(axis=1)), np.sqrt(((p1 - a) ** 2).sum(axis=1)))
    well = (h >= 1e-3 * edges) & (far <= 100.0 * edges)
    big = np.max(np.abs(np.concatenate([a, b, c, p0, p1], axis=1)), axis=1)
    _, _, d2, _ = SR.seg_triangle(p0, p1, a, b, c)
    worst = 0.0
    for i in np.nonzero(well)[0]:
        exact = exact_triangle(p0[i], p1[i], a[i], b[i], c[i])
        if zero[i]:
            assert d2[i] == 0.0, (i, "pierced by construction")  # (inner is rounded: the exact segment crosses well inside all the same)
            assert exact == 0
            continue
        if exact == 0 or exact > Fraction(float(big[i])) ** 2 * Fraction(1, 1 << 60):
            assert (d2[i] == 0.0) == (exact == 0), (i, d2[i], float(exact))
        if exact > 0 and d2[i] > 0.0:
            worst = max(worst, abs(float((Fraction(float(d2[i])) - exact) / exact)))
    print("segment against a triangle, relative error of d2 against exact arithmetic on the well-shaped family: %.3e (%d cases)" % (worst, int(well.sum())))
    assert well.sum() >= 800
    assert worst <= 2.0 * TRIANGLE_WORST, worst
    # the sphere's non-crossing cases
    cw = rng.uniform(-3.0, 3.0, (m, 3))
    pw = cw + rng.normal(0.0, 1.0, (m, 3))
    rad = np.sqrt(((pw - cw) ** 2).sum(axis=1))[:, None]
    unit = lambda: (lambda v: v / np.sqrt((v * v).sum(axis=1))[:, None])(rng.normal(0.0, 1.0, (m, 3)))  # noqa: E731
    inside = (np.arange(m) % 2 == 0)[:, None]
    p0 = cw + unit() * rad * np.where(inside, rng.uniform(0.0, 0.7, (m, 1)), rng.uniform(1.5, 30.0, (m, 1)))
    p1 = np.where(inside, cw + unit() * rad * rng.uniform(0.0, 0.7, (m, 1)), p0 + unit() * rad * rng.uniform(0.1, 0.4, (m, 1)))
    _, _, d2, case = SR.seg_sphere(p0, p1, cw, pw)
    worst_s, counted = 0.0, 0
    for i in range(m):
        exact, meets = exact_sphere(p0[i], p1[i], cw[i], pw[i])
        assert not meets and case[i] in (SR.SPHERE_OUTSIDE, SR.SPHERE_INSIDE) and d2[i] > 0.0, (i, int(case[i]))
        worst_s = max(worst_s, abs(float((Fraction(float(d2[i])) - exact) / exact)))
        counted += 1
    print("segment against a sphere (not crossing), relative error of d2 against exact arithmetic: %.3e (%d cases)" % (worst_s, counted))
    assert worst_s <= 2.0 * SPHERE_WORST, worst_s
