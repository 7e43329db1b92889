"""Direction sets (include/lasgun_hip.h: lg_open_directions, lg_open_directions_device): which of K shared directions are open above each
of N points, the rays made in the kernel, the answer bit-packed and counted.

The reference is restated here: above(i, k) in numpy with the header's operation order, s = (n.x*d.x + n.y*d.y) + n.z*d.z, s > 0.0 (every
pair without normals); occ from lg_occluded on the explicit rays (points[i], dirs[k]) of the ABOVE pairs only; open = above & ~occ, packed
with packbits(bitorder="little").  No mismatching bit or count is tolerated anywhere.

  1  bit for bit against the restatement in every traversal form, bits and both counts, for shapes with partial blocks of 64 points and
     partial bytes of 8 directions on either side, on both and on none, one point, one direction, more tiles than a workgroup has waves, and
     (LDS form) more tiles than twice the grid's waves: the tile claim's other path;
  2  the same against the CPU oracle's occlusion answer on the above pairs;
  3  normals=None: every pair is walked, bits = ~lg_occluded on all pairs, above = n_dirs, and the answer differs from the one with normals;
  4  the horizon's edges against the numpy rule: exact zeros, exact cancellation, -0.0, a subnormal s, zero / NaN / infinite normals, zero
     and NaN directions, NaN and infinite point coordinates;
  5  stride and padding: row_bytes = ceil(K / 8) and + 3 over 0xA5: used bytes exact, padding bits 0, the bytes behind untouched;
  6  counts: written not accumulated (garbage prefill), the same call twice, counts only, bits only, one count only, open = row popcounts;
  7  the device form on a stream that is not the default one: the host form's bytes;
  8  errors refused before any launch with every output at its prefill; empty sets a no-op.
No vacuous comparison: three classes of pairs -- below the horizon, above and blocked, open -- each hold at least 10 % of every full
matrix and occur in every smaller case, asserted on the reference's answer before anything is compared; a 1 x 1 case is run once per class.
Points: the first hits of a coarse camera grid (lg_camera_rays + lg_intersect) pushed out along ng by the shading offset, normals ng;
directions: a Fibonacci lattice of length 0.5 * |hi - lo| of the hits' bounds."""
import numpy as np
import pytest

import lasgun_amd as la
from oracle_lib import oracle
from test_gpu_visibility import SCENES, set_form, reset, spread

pytestmark = pytest.mark.gpu

G = la.api
ERR = 2.220446049250313e-16 * 65536.0  # the shading offset, 2^-36 (integrate.rs:40)
FULL = 1031                            # points and directions per scene: 17 blocks of 64 points x 129 bytes of 8 directions
GRID = (48, 36)                        # the coarse camera grid the points are first hits of
SHAPES = [(63, 7), (64, 8), (65, 9), (1, 64), (63, 1), (65, 1), (129, 1), (17, 130), (257, 1031), (FULL, FULL)]
BELOW, BLOCKED, OPEN = 0, 1, 2


def horizon(nrm, dirs):
    """above(i, k), the header's rule in numpy f64: three products, two sums in the stated order, nothing fused."""
    n, d = nrm[:, None, :], dirs[None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
        return s > 0.0


def restate(occluded, pts, nrm, dirs):
    """(above, open) of the contract, (n, k) bool each; `occluded`: rays -> bool, asked about the above pairs only."""
    n, k = len(pts), len(dirs)
    above = np.ones((n, k), dtype=bool) if nrm is None else horizon(nrm, dirs)
    i, j = np.nonzero(above)
    rays = np.ascontiguousarray(np.concatenate([pts[i], dirs[j]], axis=1))  # origin and direction as given: no arithmetic
    occ = np.zeros((n, k), dtype=bool)
    if len(rays):
        occ[i, j] = occluded(rays)
    return above, above & ~occ


def classes(above, opened):
    return np.where(opened, OPEN, np.where(above, BLOCKED, BELOW))


def pack(opened):
    return np.packbits(opened, axis=1, bitorder="little")


def not_vacuous(cls, ctx, share=0.0):
    for c in (BELOW, BLOCKED, OPEN):
        f = float(np.mean(cls == c))
        assert f > 0.0 and f >= share, ("the comparison would be vacuous: share of class", c, f, ctx)


def balanced(cls_rows):
    """The index of the row of `cls_rows` whose rarest class is most frequent."""
    return int(np.argmax(np.min([np.mean(cls_rows == c, axis=1) for c in (BELOW, BLOCKED, OPEN)], axis=0)))


def choose(cls, n, m):
    """Rows and columns of the full matrix for an n x m case: spread evenly; a single row or column is the one of the full matrix in which
    all three classes are best represented (a choice of INPUTS, made on the reference's answer)."""
    rows, cols = spread(FULL, n), spread(FULL, m)
    if n == 1:
        rows = np.array([balanced(cls[:, cols])])
    if m == 1:
        cols = np.array([balanced(cls[rows].T)])
    return rows, cols


def compare(ctx, got, above, opened):
    bits, nopen, nabove = got
    n, k = above.shape
    assert bits.shape == (n, (k + 7) // 8) and bits.dtype == np.uint8 and nopen.dtype == np.uint32 and nabove.dtype == np.uint32, ctx
    want = pack(opened)
    assert np.array_equal(bits, want), (ctx, int(np.unpackbits(bits ^ want).sum()), "bits differ")
    assert np.array_equal(nopen, opened.sum(axis=1)), (ctx, "open")
    assert np.array_equal(nabove, above.sum(axis=1)), (ctx, "above")


_setup = {}


def setup(name):
    """(accel, points, normals, dirs) of a scene, built once."""
    if name not in _setup:
        accel = G.Accel.from_scene(SCENES[name](G))
        assert G.camera_samples(accel) == 1
        rays = G.camera_rays(accel, *GRID)
        odd = ~(np.isfinite(rays).all(axis=1) & (rays[:, 3:] != 0.0).any(axis=1))  # (a zero or NaN ray "hits" with a NaN point in every scene)
        assert not odd.any(), (name, "camera rays that are not finite or have no direction", int(odd.sum()), len(rays), np.flatnonzero(odd)[:8], rays[odd][:3])
        hits = G.intersect(accel, rays)
        hit = hits[hits["kind"] != 0]
        assert len(hit) >= FULL, len(hit)
        odd = ~(np.isfinite(hit["p"]).all(axis=1) & np.isfinite(hit["ng"]).all(axis=1) & np.isfinite(hit["t"]))
        assert not odd.any(), (name, "hits that are not finite", int(odd.sum()), len(hit), np.flatnonzero(odd)[:8], hit[odd][:3])
        sel = hit[spread(len(hit), FULL)]
        pts = np.ascontiguousarray(sel["p"] + sel["ng"] * ERR)
        nrm = np.ascontiguousarray(sel["ng"])
        lo, hi = hit["p"].min(axis=0), hit["p"].max(axis=0)
        reach = 0.5 * float(np.linalg.norm(hi - lo))
        assert np.isfinite(reach) and reach > 0.0, (name, lo, hi)
        _setup[name] = (accel, pts, nrm, la.sphere_directions(FULL, reach))
    return _setup[name]


_full = {}


def full_reference(name, form, accel):
    """(above, open) of the scene's full matrix by lg_occluded in the accel's current form; computed once per (scene, form), never changed."""
    if (name, form) not in _full:
        _, pts, nrm, dirs = setup(name)
        above, opened = restate(lambda r: G.occluded(accel, r), pts, nrm, dirs)
        above.setflags(write=False)
        opened.setflags(write=False)
        _full[name, form] = (above, opened)
    return _full[name, form]


# ---- 1: bit for bit against the restatement, every form -------------------------------------------------------------------------------
FORMS = [("cornell_glass", "lds"), ("instanced", "reference"), ("instanced", "prune"), ("cornell_glass", "reference"), ("mesh_glass", "fast")]


@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_bits_and_counts_equal_the_restatement(name, form):
    accel, pts, nrm, dirs = setup(name)
    set_form(accel, form)
    try:
        above, opened = full_reference(name, form, accel)
        cls = classes(above, opened)
        not_vacuous(cls, (name, form), share=0.10)
        for n, m in SHAPES:
            rows, cols = choose(cls, n, m)
            p, nn, d = np.ascontiguousarray(pts[rows]), np.ascontiguousarray(nrm[rows]), np.ascontiguousarray(dirs[cols])
            a, o = restate(lambda r: G.occluded(accel, r), p, nn, d)
            assert np.array_equal(a, above[np.ix_(rows, cols)]) and np.array_equal(o, opened[np.ix_(rows, cols)]), (name, form, n, m, "not a function of the ray")
            not_vacuous(classes(a, o), (name, form, n, m))
            compare((name, form, n, m), G.open_directions(accel, p, d, nn, counts=True), a, o)
        # 1 x 1: one pair, so once per class
        for c in (BELOW, BLOCKED, OPEN):
            at = np.argwhere(cls == c)
            i, k = at[len(at) // 2]
            p, nn, d = pts[i:i + 1].copy(), nrm[i:i + 1].copy(), dirs[k:k + 1].copy()
            a, o = restate(lambda r: G.occluded(accel, r), p, nn, d)
            assert int(classes(a, o)[0, 0]) == c
            bits, nopen, nabove = accel.open_directions(p, d, nn, counts=True)
            assert bits.shape == (1, 1) and (int(bits[0, 0]), int(nopen[0]), int(nabove[0])) == (int(c == OPEN), int(c == OPEN), int(c != BELOW)), (name, form, c)
    finally:
        reset(accel)


def test_more_tiles_than_twice_the_grids_waves():
    """LDS form: one 1024-lane workgroup per CU, 16 waves each; 17 blocks of points x ceil(K / 8) bytes of directions > 2 x 16 x CUs."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = 16 * cus + 4  # 17 * ceil(k / 8) = 34 cus + 17 tiles; 4100 directions on 256 CUs
    assert 17 * ((k + 7) // 8) > 2 * 16 * cus
    accel, pts, nrm, dirs = setup("cornell_glass")
    d = la.sphere_directions(k, float(np.linalg.norm(dirs[0])))
    set_form(accel, "lds")
    try:
        above, opened = restate(lambda r: G.occluded(accel, r), pts, nrm, d)
        not_vacuous(classes(above, opened), k, share=0.10)
        compare(("lds", FULL, k), G.open_directions(accel, pts, d, nrm, counts=True), above, opened)
    finally:
        reset(accel)


# ---- 2: against the CPU oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_glass", "instanced"])
def test_bits_and_counts_equal_the_cpu_oracles_answer(name):
    accel, pts, nrm, dirs = setup(name)
    o = oracle()
    oaccel = o.Accel(SCENES[name](o))
    p, nn = np.ascontiguousarray(pts[spread(FULL, 257)]), np.ascontiguousarray(nrm[spread(FULL, 257)])
    above, opened = restate(lambda r: o.occluded(oaccel, r, 16), p, nn, dirs)
    not_vacuous(classes(above, opened), name, share=0.10)
    compare((name, "oracle"), G.open_directions(accel, p, dirs, nn, counts=True), above, opened)


# ---- 3: no normals ---------------------------------------------------------------------------------------------------------------------
def test_without_normals_every_pair_is_walked():
    accel, pts, nrm, dirs = setup("instanced")
    n, m = 130, 257
    p, nn, d = np.ascontiguousarray(pts[spread(FULL, n)]), np.ascontiguousarray(nrm[spread(FULL, n)]), np.ascontiguousarray(dirs[spread(FULL, m)])
    rays = np.concatenate([np.repeat(p, m, axis=0), np.tile(d, (n, 1))], axis=1)
    occ = G.occluded(accel, rays).reshape(n, m)
    assert 0.10 <= occ.mean() <= 0.90
    bits, nopen, nabove = G.open_directions(accel, p, d, None, counts=True)
    assert np.array_equal(bits, pack(~occ)) and np.array_equal(nopen, (~occ).sum(axis=1))
    assert (nabove == m).all()
    above, opened = restate(lambda r: G.occluded(accel, r), p, nn, d)
    not_vacuous(classes(above, opened), "with normals")
    with_normals = G.open_directions(accel, p, d, nn, counts=True)
    compare("with normals", with_normals, above, opened)
    assert not np.array_equal(with_normals[0], bits) and not np.array_equal(with_normals[2], nabove), "the horizon mask is live"
    assert (opened <= ~occ).all(), "what is open above the horizon is open without one"


# ---- 4: the horizon's edges ------------------------------------------------------------------------------------------------------------
def test_the_horizons_edges_follow_the_numpy_rule():
    accel, pts, nrm, dirs = setup("cornell_glass")
    inf, nan, tiny = np.inf, np.nan, 5e-324
    normals = np.array([[0.0, 1.0, 0.0],      # 0: exactly perpendicular to dirs[0], exact zeros
                        [1.0, 1.0, 0.0],      # 1: exact cancellation with dirs[1]
                        [-0.0, -0.0, -0.0],   # 2: s = -0.0 with dirs[2]
                        [tiny, 0.0, 0.0],     # 3: the smallest subnormal: above dirs[0]
                        [0.0, 0.0, 0.0],      # 4: a zero normal
                        [nan, 1.0, 0.0],      # 5: a NaN normal
                        [inf, 0.0, 0.0],      # 6: an infinite component meeting a zero in dirs[3]: NaN s
                        [1.0, 0.0, 0.0],      # 7, 8: for the NaN and the infinite point coordinate
                        [1.0, 0.0, 0.0]])
    # The carrier point and the four scene-length directions are chosen on lg_occluded's answer (a choice of INPUTS): one point from which,
    # of the lattice's directions with d.x > 0, one is blocked and one open, and likewise of those with d.x < 0
    cand = spread(FULL, 129)
    xpos, xneg = np.flatnonzero(tiny * dirs[:, 0] > 0.0), np.flatnonzero(tiny * dirs[:, 0] < 0.0)  # (d.x that the subnormal normal does not round away)

    def occluded_from(cols):
        rays = np.concatenate([np.repeat(pts[cand], len(cols), axis=0), np.tile(dirs[cols], (len(cand), 1))], axis=1)
        return G.occluded(accel, rays).reshape(len(cand), len(cols))
    opos, oneg = occluded_from(xpos), occluded_from(xneg)
    mixed = opos.any(axis=1) & ~opos.all(axis=1) & oneg.any(axis=1) & ~oneg.all(axis=1)
    assert mixed.any()
    c = int(np.flatnonzero(mixed)[0])
    d = np.array([[1.0, 0.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0],
                  [0.0, 0.0, 0.0],            # 4: a zero direction
                  [nan, 0.0, 1.0],            # 5: a NaN direction
                  dirs[xpos[np.argmax(opos[c])]], dirs[xpos[np.argmin(opos[c])]],    # 6, 7: d.x > 0, blocked and open from the carrier
                  dirs[xneg[np.argmax(oneg[c])]], dirs[xneg[np.argmin(oneg[c])]]])   # 8, 9: d.x < 0, blocked and open from the carrier
    p = np.ascontiguousarray(np.tile(pts[cand[c]], (len(normals), 1)))
    p[7, 1] = nan
    p[8, 0] = inf
    a = horizon(normals, d)
    with np.errstate(invalid="ignore"):
        s2 = (normals[2, 0] * d[2, 0] + normals[2, 1] * d[2, 1]) + normals[2, 2] * d[2, 2]
    assert s2 == 0.0 and np.signbit(s2)
    assert not a[0, 0] and not a[1, 1] and not a[2, 2], "perpendicular, cancelled and -0.0 are not above"
    assert a[3, 0] and a[3, 6] and a[3, 7] and not a[3, 8] and not a[3, 9] and not a[3, 3], "the smallest subnormal times a positive d.x is above"
    assert not a[4].any() and not a[5].any(), "a zero and a NaN normal are above nothing"
    assert not a[6, 3] and a[6, 0] and a[6, 6] and not a[6, 8], "inf * 0 is NaN: not above; inf * 1 is"
    assert not a[:, 4].any() and not a[:, 5].any(), "a zero and a NaN direction are above no horizon"
    assert a[7, 6] and a[8, 6], "the horizon does not look at the point"
    for nn in (normals, None):
        above, opened = restate(lambda r: G.occluded(accel, r), p, nn, d)
        cls = classes(above, opened)
        if nn is not None:
            assert np.array_equal(above, a)
            not_vacuous(cls, "edges")
            assert cls[3, 6] == BLOCKED and cls[3, 7] == OPEN and cls[6, 6] == BLOCKED and cls[6, 7] == OPEN, "walked pairs of either verdict"
        else:
            assert (cls[:7, 6:] == BLOCKED).any() and (cls[:7, 6:] == OPEN).any(), "without normals nothing is below: both verdicts among the walked pairs"
        compare(("edges", nn is not None), G.open_directions(accel, p, d, nn, counts=True), above, opened)
    # without normals the zero and the NaN direction are whatever lg_occluded answers: walked, and counted above
    assert (G.open_directions(accel, p, d, None, counts="only")[1] == len(d)).all()


# ---- 5: stride and padding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(17, 130), (65, 7), (64, 64)])
def test_stride_and_padding(n, m):
    accel, pts, nrm, dirs = setup("cornell_glass")
    rows, cols = spread(FULL, n), spread(FULL, m)
    p, nn, d = np.ascontiguousarray(pts[rows]), np.ascontiguousarray(nrm[rows]), np.ascontiguousarray(dirs[cols])
    used = (m + 7) // 8
    above, opened = restate(lambda r: G.occluded(accel, r), p, nn, d)
    not_vacuous(classes(above, opened), (n, m))
    want = pack(opened)
    for stride in (used, used + 3):
        buf = np.full((n, stride), 0xA5, dtype=np.uint8)
        G.open_directions(accel, p, d, nn, row_bytes=stride, into=(buf, None, None))
        assert np.array_equal(buf[:, :used], want), (n, m, stride)
        if m % 8:
            assert not (buf[:, used - 1] >> (m % 8)).any(), "padding bits of the last used byte are 0"
        assert (buf[:, used:] == 0xA5).all(), "bytes behind the used part of a row are never touched"


# ---- 6: counts -------------------------------------------------------------------------------------------------------------------------
def test_counts_are_written_not_accumulated():
    accel, pts, nrm, dirs = setup("instanced")
    n, m = 130, 257
    rows, cols = spread(FULL, n), spread(FULL, m)
    p, nn, d = np.ascontiguousarray(pts[rows]), np.ascontiguousarray(nrm[rows]), np.ascontiguousarray(dirs[cols])
    above, opened = restate(lambda r: G.occluded(accel, r), p, nn, d)
    not_vacuous(classes(above, opened), "counts")
    co, ca = opened.sum(axis=1).astype(np.uint32), above.sum(axis=1).astype(np.uint32)
    assert len(np.unique(co)) > 8
    bits, nopen, nabove = G.open_directions(accel, p, d, nn, counts=True)
    compare("counts", (bits, nopen, nabove), above, opened)
    assert np.array_equal(nopen, np.unpackbits(bits, axis=1).sum(axis=1))
    rng = np.random.default_rng(5)
    g1, g2 = (rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    for _ in range(2):  # the same call twice: the same counts
        b1, b2 = g1.copy(), g2.copy()
        got = G.open_directions(accel, p, d, nn, into=(None, b1, b2))  # counts only: bits = NULL
        assert got[0] is b1 and got[1] is b2
        assert np.array_equal(b1, co) and np.array_equal(b2, ca)
    only = G.open_directions(accel, p, d, nn, counts="only")
    assert len(only) == 2 and only[0].dtype == np.uint32 and np.array_equal(only[0], co) and np.array_equal(only[1], ca)
    alone = G.open_directions(accel, p, d, nn)  # bits only: both counts NULL
    assert np.array_equal(alone, bits)
    b1, b2 = g1.copy(), g2.copy()
    assert G.open_directions(accel, p, d, nn, into=(None, b1, None)) is b1 and np.array_equal(b1, co)  # one count only
    assert G.open_directions(accel, p, d, nn, into=(None, None, b2)) is b2 and np.array_equal(b2, ca)
    ao = G.ambient_occlusion(accel, p, nn, k=64, radius=float(np.linalg.norm(d[0])))
    assert ao.dtype == np.float64 and ao.shape == (n,) and (ao >= 0.0).all() and (ao <= 1.0).all() and 0.0 < ao.mean() < 1.0


# ---- 7: device form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel, pts, nrm, dirs = setup(name)
    set_form(accel, form)
    n, m = 257, FULL
    rows = spread(FULL, n)
    p, nn = np.ascontiguousarray(pts[rows]), np.ascontiguousarray(nrm[rows])
    try:
        device_form(torch, accel, p, nn, dirs, n, m)
    finally:
        reset(accel)


def device_form(torch, accel, p, nn, d, n, m):
    used = (m + 7) // 8
    above, opened = restate(lambda r: G.occluded(accel, r), p, nn, d)
    not_vacuous(classes(above, opened), ("device form", n, m), share=0.10)
    hbits, hopen, habove = G.open_directions(accel, p, d, nn, counts=True)
    compare(("host form", n, m), (hbits, hopen, habove), above, opened)
    dp, dn, dd = torch.from_numpy(p).cuda(), torch.from_numpy(nn).cuda(), torch.from_numpy(d).cuda()
    stream = torch.cuda.Stream()
    for stride in (used, used + 3):
        dbits = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
        dopen = torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        dabove = torch.full((n,), 0x7FFFFFFE, dtype=torch.int32, device="cuda")
        oopen = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        oabove = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            assert s != 0
            G.open_directions_device(accel, n, dp.data_ptr(), dn.data_ptr(), m, dd.data_ptr(), dbits.data_ptr(), stride, dopen.data_ptr(), dabove.data_ptr(), stream=s)
            G.open_directions_device(accel, n, dp.data_ptr(), dn.data_ptr(), m, dd.data_ptr(), None, stride, oopen.data_ptr(), oabove.data_ptr(), stream=s)
        stream.synchronize()
        got = dbits.cpu().numpy()
        assert np.ascontiguousarray(got[:, :used]).tobytes() == hbits.tobytes(), stride
        assert (got[:, used:] == 0xA5).all()
        for dev, host in ((dopen, hopen), (oopen, hopen), (dabove, habove), (oabove, habove)):
            assert dev.cpu().numpy().view(np.uint32).tobytes() == host.tobytes()


# ---- 8: errors and empty sets ----------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_empty_sets_are_a_no_op():
    torch = pytest.importorskip("torch")
    accel, pts, nrm, dirs = setup("cornell_glass")
    n, m = 70, 20
    p, nn, d = np.ascontiguousarray(pts[:n + 1]), np.ascontiguousarray(nrm[:n + 1]), np.ascontiguousarray(dirs[:m])
    used = (m + 7) // 8
    dp, dn, dd = torch.from_numpy(p).cuda(), torch.from_numpy(nn).cuda(), torch.from_numpy(d).cuda()
    dbits = torch.full((n, used), 0xA5, dtype=torch.uint8, device="cuda")
    dopen = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dabove = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hbits = np.full((n, used), 0xA5, dtype=np.uint8)
    hopen, habove = np.full(n, 0x5A5A5A5A, dtype=np.uint32), np.full(n, 0x5A5A5A5A, dtype=np.uint32)
    torch.cuda.synchronize()
    P, N, D, B, O, A = dp.data_ptr(), dn.data_ptr(), dd.data_ptr(), dbits.data_ptr(), dopen.data_ptr(), dabove.data_ptr()

    def V(*args):
        G.open_directions_device(accel, *args, stream=0)

    bad = [lambda: V(n, p.ctypes.data, N, m, D, B, used, O, A),          # host pointers
           lambda: V(n, P, nn.ctypes.data, m, D, B, used, O, A),
           lambda: V(n, P, N, m, d.ctypes.data, B, used, O, A),
           lambda: V(n, P, N, m, D, hbits.ctypes.data, used, O, A),
           lambda: V(n, P, N, m, D, B, used, hopen.ctypes.data, A),
           lambda: V(n, P, N, m, D, B, used, O, habove.ctypes.data),
           lambda: V(n, P + 4, N, m, D, B, used, O, A),                  # misaligned
           lambda: V(n, P, N + 4, m, D, B, used, O, A),
           lambda: V(n, P, N, m, D + 4, B, used, O, A),
           lambda: V(n, P, N, m, D, B, used, O + 2, A),
           lambda: V(n, P, N, m, D, B, used, O, A + 2),
           lambda: V(n, P, N, m, D, None, used, None, None),             # all outputs NULL
           lambda: V(n, P, N, m, D, B, used - 1, O, A),                  # row_bytes too small
           lambda: V(n, None, N, m, D, B, used, O, A),                   # NULL tables with non-zero counts
           lambda: V(n, P, N, m, None, B, used, O, A),
           lambda: V(n, P, N, 1 << 32, D, None, 1 << 29, O, A),          # n_dirs > 2^32 - 1
           lambda: V(1 << 36, P, N, 1 << 30, D, None, 1 << 27, O, A),    # 2^66 pairs: 2^57 tiles
           lambda: V(1 << 40, P, None, 8, D, None, 1, O, A),             # 2^34 tiles of one byte
           lambda: V(1 << 20, P, N, 8, D, B, 1 << 60, O, A),             # rows that do not fit the address space
           lambda: V(1 << 24, P, None, m, D, None, used, O, None)]       # 384 MiB of points: the buffer ends long before
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    hp, hn, hd = p.ctypes.data, nn.ctypes.data, d.ctypes.data
    host = [(accel.h, hp, hn, n, hd, m, None, used, None, None),
            (accel.h, hp, hn, n, hd, m, hbits.ctypes.data, used - 1, hopen.ctypes.data, habove.ctypes.data),
            (accel.h, None, hn, n, hd, m, hbits.ctypes.data, used, hopen.ctypes.data, habove.ctypes.data),
            (accel.h, hp, hn, n, None, m, hbits.ctypes.data, used, hopen.ctypes.data, habove.ctypes.data),
            (None, hp, hn, n, hd, m, hbits.ctypes.data, used, hopen.ctypes.data, habove.ctypes.data),
            (accel.h, hp, hn, n, hd, 1 << 32, None, 1 << 29, hopen.ctypes.data, habove.ctypes.data),
            (accel.h, hp, hn, 1 << 36, hd, 1 << 30, None, 1 << 27, hopen.ctypes.data, habove.ctypes.data),
            (accel.h, hp, hn, 1 << 20, hd, 8, hbits.ctypes.data, 1 << 60, hopen.ctypes.data, habove.ctypes.data)]
    for k, args in enumerate(host):
        assert G.call("open_directions", *args) != 0 and G.last_error(), k
    # empty sets: success, nothing written (whatever the pointers)
    for np_, nd in ((0, m), (n, 0), (0, 0)):
        V(np_, P, N, nd, D, B, used, O, A)
        assert G.call("open_directions", accel.h, hp, hn, np_, hd, nd, hbits.ctypes.data, used, hopen.ctypes.data, habove.ctypes.data) == 0
    assert G.call("open_directions", accel.h, None, None, 0, None, 0, None, 0, None, None) == 0
    assert G.open_directions(accel, np.zeros((0, 3)), d).shape == (0, used) and G.open_directions(accel, p, np.zeros((0, 3))).shape == (n + 1, 0)
    torch.cuda.synchronize()
    assert (dbits.cpu().numpy() == 0xA5).all() and (dopen.cpu().numpy() == 0x5A5A5A5A).all() and (dabove.cpu().numpy() == 0x5A5A5A5A).all()
    assert (hbits == 0xA5).all() and (hopen == 0x5A5A5A5A).all() and (habove == 0x5A5A5A5A).all()
    # and the call still works afterwards
    V(n, P, N, m, D, B, used, O, A)
    torch.cuda.synchronize()
    wb, wo, wa = G.open_directions(accel, p[:n], d, nn[:n], counts=True)
    assert dbits.cpu().numpy().tobytes() == wb.tobytes()
    assert dopen.cpu().numpy().view(np.uint32).tobytes() == wo.tobytes() and dabove.cpu().numpy().view(np.uint32).tobytes() == wa.tobytes()
