"""The next ray of a ray path on the CPU: lasgun_amd/csrc/bounce.h compiled into a stand-alone program (tools/bounce_check.cpp, its own
main, nothing loaded into python) with -ffp-contract=off under AddressSanitizer and UBSan, against the numpy restatement
(tests/bounce_ref.py, which tests/test_gpu_ray_paths.py holds the kernel to) word for word on ~10^5 vertices: each action x both normals x
both media, grazing incidence (ci = 0 and 1 +- 1 ulp), the critical angle +- a few ulps for ior 1.5 and 1/1.5, s = +-0.0, un-normalised
directions from 5e-324 to 1e300, NaN and infinite components (those compared as "degenerate or not", finite results bit for bit).
With this green, a mismatch on the GPU is the device build's, not the restatement's.  Three seeded faults in a scratch copy of the header
must each fail the same comparison: the mirror taken with the unflipped s, the offset's sign swapped, eta inverted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounce_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined,float-cast-overflow",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def unit(v):
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def records(action, normal, medium, ior, d, p, ng, ns):
    m = len(d)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (m,))  # noqa: E731
    return np.ascontiguousarray(np.concatenate([np.stack([full(action), full(normal), full(medium), full(ior)], axis=1), d, p, ng, ns], axis=1))


def nudged(x, steps):
    for _ in range(abs(steps)):
        x = np.nextafter(x, INF if steps > 0 else -INF)
    return x


def vertex_set():
    """(m, 16) records, and the rows of each family."""
    rng = np.random.default_rng(21)
    fam, rows = {}, []

    def add(name, r):
        fam[name] = (sum(len(x) for x in rows), len(r))
        rows.append(r)

    def frame(m):
        ng = unit(rng.normal(0.0, 1.0, (m, 3)))
        ns = unit(ng + 0.2 * rng.normal(0.0, 1.0, (m, 3)))
        return rng.uniform(-50.0, 50.0, (m, 3)), ng, ns

    # each action x both normals x both media, plain directions of any length near 1, ior of glass, water, diamond and their inverses
    for action in (B.REFLECT, B.PASS, B.REFRACT):
        for normal in (0, 1):
            for medium in (0, 1):
                m = 6000
                p, ng, ns = frame(m)
                ior = rng.choice([1.5, 1.0 / 1.5, 1.33, 2.4, 1.0, 1.0003], m)
                add("plain-%d-%d-%d" % (action, normal, medium), records(action, normal, medium, ior, rng.normal(0.0, 1.0, (m, 3)), p, ng, ns))
    # grazing incidence: ci = 0 (d in the surface) and ci = 1 +- 1 ulp (d along -N, nudged), N an axis and a general normal
    m = 2000
    p, ng, ns = frame(m)
    ng[: m // 2] = (0.0, 0.0, 1.0)
    t = unit(np.cross(ng, rng.normal(0.0, 1.0, (m, 3))))
    for action in (B.REFLECT, B.REFRACT):
        for medium in (0, 1):
            add("graze0-%d-%d" % (action, medium), records(action, 0, medium, 1.5, t, p, ng, ns))
            for k in (-1, 0, 1):
                d = -ng.copy()
                d[:, 2] = nudged(d[:, 2], k)
                add("graze1-%d-%d-%d" % (action, medium, k), records(action, 0, medium, 1.5, d, p, ng, ns))
    # the critical angle +- a few ulps: leaving glass (medium 1, ior 1.5) and the same eta from outside (medium 0, ior 1 / 1.5)
    N = np.array([[0.0, 0.0, 1.0]])
    for medium, ior in ((1, 1.5), (0, 1.0 / 1.5)):
        sin_c = 1.0 / 1.5
        ds = []
        for k in range(-40, 41):
            sx = nudged(np.float64(sin_c), k)
            ds.append((sx, 0.0, -np.sqrt(1.0 - sx * sx)))
            ds.append((sx * 3.0, 0.0, -np.sqrt(1.0 - sx * sx) * 3.0))
        d = np.array(ds)
        m = len(d)
        add("critical-%d" % medium, records(B.REFRACT, 0, medium, ior, d, np.zeros((m, 3)), np.repeat(N, m, axis=0), np.repeat(N, m, axis=0)))
    # s = +-0.0: a direction in the surface (+0.0) and a zero normal under a negative direction (-0.0: every product is -0.0)
    zs = [((1.0, 0.0, 0.0), (0.0, 0.0, 1.0)), ((-1.0, -1.0, -1.0), (0.0, 0.0, 0.0)), ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ((-1.0, 0.0, -0.0), (0.0, 0.0, 1.0))]
    for action in (B.REFLECT, B.PASS, B.REFRACT):
        d, n = np.array([z[0] for z in zs]), np.array([z[1] for z in zs])
        add("zero-s-%d" % action, records(action, 0, 0, 1.5, d, np.ones((len(zs), 3)), n, n))
    # un-normalised directions, 5e-324 .. 1e300
    m = 8000
    p, ng, ns = frame(m)
    scale = 10.0 ** rng.uniform(-324.0, 300.0, m)
    scale[:8] = (5e-324, 1e-323, 2.3e-308, 1e-162, 1e-154, 1e154, 1e200, 1e300)
    d = unit(rng.normal(0.0, 1.0, (m, 3))) * scale[:, None]
    for action in (B.REFLECT, B.REFRACT):
        add("scaled-%d" % action, records(action, 1, rng.integers(0, 2, m), 1.5, d, p, ng, ns))
    # NaN and infinite components anywhere
    m = 6000
    p, ng, ns = frame(m)
    r = records(rng.choice([B.REFLECT, B.PASS, B.REFRACT], m), rng.integers(0, 2, m), rng.integers(0, 2, m), 1.5, rng.normal(0.0, 1.0, (m, 3)), p, ng, ns)
    r[np.arange(m), rng.integers(3, 16, m)] = rng.choice([NAN, INF, -INF, 0.0, -0.0, 1e300, -1e300], m)
    add("poison", r)
    return np.ascontiguousarray(np.concatenate(rows)), fam


def restated(rec):
    action, normal, medium, ior = rec[:, 0].astype(np.uint32), rec[:, 1] != 0.0, rec[:, 2].astype(np.uint32), rec[:, 3]
    d, p, ng, ns = rec[:, 4:7], rec[:, 7:10], rec[:, 10:13], rec[:, 13:16]
    o2, d2, m2, did = B.bounce(action, ior, d, p, ng, np.where(normal[:, None], ns, ng), medium)
    return o2, d2, m2, B.finite(o2, d2), did


def build(cxx, src, exe):
    subprocess.check_call([cxx] + FLAGS + [src, "-o", exe])


def run(exe, tmp, rec):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    rec.tofile(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and "bounce_check: ok, %d vertices" % len(rec) in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    out = np.fromfile(dst, dtype=np.float64).reshape(-1, 8)
    assert len(out) == len(rec)
    return out


def differences(out, want):
    """Rows where the program and the restatement differ: the finite flag, the medium, and -- where finite -- any word of (o', d')."""
    o2, d2, m2, fin, _ = want
    bad = (out[:, 7] != 0.0) != fin
    bad |= out[:, 6].astype(np.uint32) != m2
    w_got = np.ascontiguousarray(out[:, :6]).view(np.uint64)
    w_want = np.ascontiguousarray(np.concatenate([o2, d2], axis=1)).view(np.uint64)
    bad |= fin & (w_got != w_want).any(axis=1)
    return np.nonzero(bad)[0]


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    tmp = str(tmp_path_factory.mktemp("bounce"))
    exe = os.path.join(tmp, "bounce_check")
    build(cxx, os.path.join(ROOT, "tools", "bounce_check.cpp"), exe)
    rec, fam = vertex_set()
    return cxx, tmp, exe, rec, fam, restated(rec)


def test_the_vertex_set_reaches_every_branch(bench):
    _, _, _, rec, fam, (o2, d2, m2, fin, did) = bench
    assert 90000 <= len(rec) <= 130000
    rows = lambda name: slice(fam[name][0], fam[name][0] + fam[name][1])  # noqa: E731
    for medium in (0, 1):
        c = did[rows("critical-%d" % medium)]
        assert (c == B.DID_TIR).sum() >= 20 and (c == B.DID_REFRACT).sum() >= 20, ("both sides of the critical angle", medium)
    for k in (B.DID_REFLECT, B.DID_PASS, B.DID_REFRACT, B.DID_TIR):
        assert (did == k).sum() >= 1000, k
    assert (~fin).sum() >= 1000 and fin[rows("poison")].any() and not fin[rows("poison")].all()
    assert not fin[rows("scaled-3")].all() and fin[rows("scaled-3")].mean() > 0.3
    s = B.dot(rec[:, 4:7], rec[:, 10:13])[rows("zero-s-1")]
    assert (s == 0.0).all() and np.signbit(s).any() and not np.signbit(s).all(), "s = +0.0 and s = -0.0"
    plain = np.concatenate([np.arange(*np.array(fam[n]).cumsum()) for n in fam if n.startswith("plain-3")])
    flipped = B.dot(rec[plain, 4:7], rec[plain, 10:13]) > 0.0
    assert 0.3 < flipped.mean() < 0.7, "the normal is flipped for about half of the plain vertices"


def test_a_mirror_and_a_glass_slab_by_hand():
    """The restatement against numbers worked out by hand: 45 degrees onto a mirror; straight into glass; 30 degrees out of ior 2 (sin 90)."""
    z, up = np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])
    o2, d2, m2, did = B.bounce([B.REFLECT], np.array([1.0]), np.array([[1.0, 0.0, -1.0]]), z, up, up, [0])
    assert d2.tolist() == [[1.0, 0.0, 1.0]] and o2.tolist() == [[0.0, 0.0, 2.0 ** -36]] and m2.tolist() == [0] and did.tolist() == [B.DID_REFLECT]
    o2, d2, m2, did = B.bounce([B.REFRACT], np.array([1.5]), np.array([[0.0, 0.0, -2.0]]), z, up, up, [0])
    assert d2.tolist() == [[0.0, 0.0, -2.0]] and o2.tolist() == [[0.0, 0.0, -2.0 ** -36]] and m2.tolist() == [1] and did.tolist() == [B.DID_REFRACT]
    # from inside (medium 1), the normal given facing along d: flipped; sin(30) * 2 = 1: total internal reflection, no toggle
    o2, d2, m2, did = B.bounce([B.REFRACT], np.array([2.0]), np.array([[0.5, 0.0, np.sqrt(0.75)]]), z, -up, up, [1])
    assert did.tolist() in ([B.DID_TIR], [B.DID_REFRACT])  # (sin2 = 4 * (1 - 0.75) is 1.0 up to an ulp)
    o2, d2, m2, did = B.bounce([B.REFRACT], np.array([2.0]), np.array([[0.6, 0.0, 0.8]]), z, -up, up, [1])
    assert did.tolist() == [B.DID_TIR] and m2.tolist() == [1] and d2.tolist() == [[0.6, 0.0, -0.8]] and o2.tolist() == [[0.0, 0.0, -2.0 ** -36]]
    o2, d2, m2, did = B.bounce([B.PASS], np.array([2.0]), np.array([[0.6, 0.0, 0.8]]), z, -up, -up, [1])
    assert did.tolist() == [B.DID_PASS] and m2.tolist() == [0] and d2.tolist() == [[0.6, 0.0, 0.8]] and o2.tolist() == [[0.0, 0.0, 2.0 ** -36]]


def test_header_and_restatement_agree_word_for_word(bench):
    _, tmp, exe, rec, fam, want = bench
    bad = differences(run(exe, tmp, rec), want)
    where = [n for n in fam if len(bad) and fam[n][0] <= bad[0] < fam[n][0] + fam[n][1]]
    assert len(bad) == 0, (len(bad), int(bad[0]), where, rec[bad[0]].tolist())


FAULTS = {
    "the mirror with the unflipped s": ("        s = -s;\n", ""),
    "the offset's sign swapped": ("back = V3{p.x + step.x, p.y + step.y, p.z + step.z}, through = V3{p.x - step.x, p.y - step.y, p.z - step.z}",
                                  "back = V3{p.x - step.x, p.y - step.y, p.z - step.z}, through = V3{p.x + step.x, p.y + step.y, p.z + step.z}"),
    "eta inverted": ("(medium & 1u) ? ior : 1.0 / ior", "(medium & 1u) ? 1.0 / ior : ior"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_seeded_fault_fails_the_comparison(bench, fault):
    cxx, tmp, _, rec, _, want = bench
    tree = os.path.join(tmp, "fault%d" % sorted(FAULTS).index(fault))
    os.makedirs(os.path.join(tree, "tools"))
    os.makedirs(os.path.join(tree, "lasgun_amd", "csrc"))
    shutil.copy(os.path.join(ROOT, "tools", "bounce_check.cpp"), os.path.join(tree, "tools"))
    shutil.copy(os.path.join(ROOT, "lasgun_amd", "csrc", "vecmath.h"), os.path.join(tree, "lasgun_amd", "csrc"))
    text = open(os.path.join(ROOT, "lasgun_amd", "csrc", "bounce.h")).read()
    old, new = FAULTS[fault]
    assert text.count(old) == 1, (fault, "the line the fault is seeded in")
    with open(os.path.join(tree, "lasgun_amd", "csrc", "bounce.h"), "w") as f:
        f.write(text.replace(old, new))
    exe = os.path.join(tree, "bounce_check")
    build(cxx, os.path.join(tree, "tools", "bounce_check.cpp"), exe)
    assert len(differences(run(exe, tree, rec), want)) >= 100, fault
