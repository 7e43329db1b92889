"""Visibility matrices (include/lasgun_hip.h: lg_visibility, lg_visibility_device): occlusion between two point sets, the segments made in
the kernel, the answer bit-packed.

  1  bit for bit against lg_occluded on the explicit segments (from[i], to[j] - from[i]) -- the subtraction done in numpy f64, the bytes
     packed with packbits(bitorder="little") -- in every traversal form, for matrix shapes with partial 8 x 8 blocks on either side, on
     both sides and on none, one row, one column, more blocks than a workgroup has waves, and more blocks than twice the grid's waves (the
     tile claim's other path);
  2  the same matrices against the CPU oracle's occlusion answer (orc_occluded);
  3  no vacuous comparison: in every scene and point set at least 10 % of the segments are occluded and at least 10 % visible, asserted on
     lg_occluded's / the oracle's answer before anything is compared.  (A 1 x 1 matrix is one segment: it is run twice, on an occluded
     segment and on a visible one.)  No mismatching bit is tolerated anywhere;
  4  stride and padding: row_bytes = ceil(n_to / 8) and + 3 over 0xA5: used bytes exact, padding bits 0, the bytes behind untouched;
  5  blocked = the row popcounts, written not accumulated (garbage prefill), counts only, bits only, the same call twice;
  6  a zero direction (a from point that is a to point), a NaN and an infinite coordinate: whatever lg_occluded answers;
  7  the device form on a stream that is not the default one: the host form's bytes;
  8  errors refused before any launch with every output at its prefill; empty point sets a no-op.
from points: the first hits of a coarse camera grid (lg_camera_rays + lg_intersect) pushed out along ng by the shading offset; to points: a
Fibonacci lattice on a sphere around the bounds of what the camera sees, then the scene's lights."""
import numpy as np
import pytest

import pyref

import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_radiance_query import FORM_SCENES

pytestmark = pytest.mark.gpu

G = la.api
ERR = 2.220446049250313e-16 * 65536.0  # the shading offset (integrate.rs:40)
FULL = 1031                            # from and to points per scene: 129 x 129 blocks, more than twice the waves of any grid
GRID = (48, 36)                        # the coarse camera grid the from points are first hits of
RADIUS = 1.0                           # the to points' sphere, in half-diagonals of the bounds
SCENES = {"cornell_glass": FORM_SCENES[0][1],                 # a sphere, a cube and the shell's five planes: resident in LDS
          "instanced": lambda api: S.instanced_scene(api),    # one mesh three times in scaled, rotated groups nested two deep; two lights
          "mesh_glass": FORM_SCENES[1][1]}                    # the torus in a scaled, rotated group: the scene the fast mode is run on
SHAPES = [(7, 9), (8, 8), (9, 7), (5, 13), (64, 1), (1, 64), (17, 130), (257, 1031), (FULL, FULL)]


def set_form(accel, form):
    G.set_mode(accel, False)
    G.set_prune(accel, form == "prune")
    fits = G.set_lds_scene(accel, form == "lds")
    if form == "lds":
        assert fits, "the scene is meant to sit in LDS"
    if form == "fast":
        G.set_mode(accel, True)  # (raises where the fast mode refuses the scene: the case is about a scene it admits)


def reset(accel):
    """The accel's own defaults again (the accels are shared by the tests of this file)."""
    set_form(accel, "reference")
    G.set_prune(accel, None)
    G.set_lds_scene(accel, True)


def sphere_points(centre, radius, n):
    """A Fibonacci lattice: n points spread evenly over the sphere."""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return centre + radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def point_sets(hits, lights):
    """(from, to), FULL points each, from the closest hits of the camera grid's rays and the scene's light positions."""
    hit = hits[hits["kind"] != 0]
    assert len(hit) >= FULL, len(hit)
    sel = hit[np.linspace(0, len(hit) - 1, FULL).round().astype(np.int64)]
    frm = np.ascontiguousarray(sel["p"] + sel["ng"] * ERR)
    lo, hi = hit["p"].min(axis=0), hit["p"].max(axis=0)
    lights = np.array(lights, dtype=np.float64).reshape(-1, 3)
    to = np.concatenate([sphere_points(0.5 * (lo + hi), RADIUS * 0.5 * float(np.linalg.norm(hi - lo)), FULL - len(lights)), lights])
    return frm, np.ascontiguousarray(to)


def segments(frm, to):
    """The explicit rays of the matrix, row-major: origin from[i], direction to[j] - from[i] (numpy f64: three separate subtractions)."""
    o = np.repeat(frm, len(to), axis=0)
    return np.concatenate([o, np.tile(to, (len(frm), 1)) - o], axis=1)


def pack(occ, n, m):
    return np.packbits(np.asarray(occ, dtype=bool).reshape(n, m), axis=1, bitorder="little")


def spread(total, n):
    return np.linspace(0, total - 1, n).round().astype(np.int64)


def mixed(fraction):
    """The index whose occluded fraction is nearest one half."""
    return int(np.argmin(np.abs(fraction - 0.5)))


def choose(full, n, m):
    """Rows and columns of the full matrix for an n x m case: spread evenly (the last column is a light); a single row or column is the
    most mixed one of the full matrix (a choice of INPUTS, made on the reference's answer)."""
    rows = np.array([mixed(full.mean(axis=1))]) if n == 1 else spread(FULL, n)
    cols = np.array([mixed(full[rows].mean(axis=0))]) if m == 1 else spread(FULL, m)
    if n == 1 and m > 1:
        rows = np.array([mixed(full[:, cols].mean(axis=1))])
    return rows, cols


def not_vacuous(occ, ctx):
    f = float(np.mean(occ))
    assert 0.10 <= f <= 0.90, ("the comparison would be vacuous: occluded fraction", f, ctx)


_setup = {}


def setup(name):
    """(accel, from, to) of a scene, built once."""
    if name not in _setup:
        accel = G.Accel.from_scene(SCENES[name](G))
        assert G.camera_samples(accel) == 1
        hits = G.intersect(accel, G.camera_rays(accel, *GRID))
        frm, to = point_sets(hits, [l[0] for l in SCENES[name](pyref.Api).lights])
        _setup[name] = (accel, frm, to)
    return _setup[name]


# ---- 1 and 3: bit for bit against lg_occluded, every form ----------------------------------------------------------------------------
FORMS = [("cornell_glass", "lds"), ("instanced", "reference"), ("instanced", "prune"), ("cornell_glass", "reference"), ("mesh_glass", "fast")]


@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_bits_equal_lg_occluded_on_the_explicit_segments(name, form):
    accel, frm, to = setup(name)
    set_form(accel, form)
    try:
        full = G.occluded(accel, segments(frm, to)).reshape(FULL, FULL)
        not_vacuous(full, (name, form))
        for n, m in SHAPES:
            rows, cols = choose(full, n, m)
            f, t = np.ascontiguousarray(frm[rows]), np.ascontiguousarray(to[cols])
            occ = G.occluded(accel, segments(f, t))
            assert np.array_equal(occ.reshape(n, m), full[np.ix_(rows, cols)]), (name, form, n, m, "lg_occluded is not a function of the ray")
            not_vacuous(occ, (name, form, n, m))
            bits, blocked = G.visibility(accel, f, t, counts=True)
            assert bits.shape == (n, (m + 7) // 8) and bits.dtype == np.uint8 and blocked.dtype == np.uint32
            want = pack(occ, n, m)
            assert np.array_equal(bits, want), (name, form, n, m, int((np.unpackbits(bits ^ want)).sum()), "bits differ")
            assert np.array_equal(blocked, occ.reshape(n, m).sum(axis=1)), (name, form, n, m)
        # 1 x 1: one segment, so once occluded and once visible
        for verdict in (True, False):
            i, j = np.argwhere(full == verdict)[len(np.argwhere(full == verdict)) // 2]
            f, t = frm[i:i + 1].copy(), to[j:j + 1].copy()
            assert bool(G.occluded(accel, segments(f, t))[0]) == verdict
            bits = accel.visibility(f, t)
            assert bits.shape == (1, 1) and int(bits[0, 0]) == int(verdict), (name, form, verdict, bits)
    finally:
        reset(accel)


# ---- 2 and 3: against the CPU oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_glass", "instanced"])
def test_bits_equal_the_cpu_oracles_occlusion(name):
    accel, frm, to = setup(name)
    o = oracle()
    oaccel = o.Accel(SCENES[name](o))
    n, m = 257, FULL
    f = np.ascontiguousarray(frm[spread(FULL, n)])
    occ = o.occluded(oaccel, segments(f, to), 16)
    not_vacuous(occ, name)
    bits, blocked = G.visibility(accel, f, to, counts=True)
    want = pack(occ, n, m)
    assert np.array_equal(bits, want), (name, int(np.unpackbits(bits ^ want).sum()), "bits differ from the oracle's")
    assert np.array_equal(blocked, occ.reshape(n, m).sum(axis=1))


# ---- 4: stride and padding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(17, 130), (9, 7), (8, 64)])
def test_stride_and_padding(n, m):
    accel, frm, to = setup("cornell_glass")
    f, t = np.ascontiguousarray(frm[spread(FULL, n)]), np.ascontiguousarray(to[spread(FULL, m)])
    used = (m + 7) // 8
    want = pack(G.occluded(accel, segments(f, t)), n, m)
    assert want.any()
    for stride in (used, used + 3):
        buf = np.full((n, stride), 0xA5, dtype=np.uint8)
        G.visibility(accel, f, t, row_bytes=stride, into=(buf, None))
        assert np.array_equal(buf[:, :used], want), (n, m, stride)
        if m % 8:
            assert not (buf[:, used - 1] >> (m % 8)).any(), "padding bits of the last used byte are 0"
        assert (buf[:, used:] == 0xA5).all(), "bytes behind the used part of a row are never touched"


# ---- 5: blocked ------------------------------------------------------------------------------------------------------------------------
def test_blocked_is_written_not_accumulated():
    accel, frm, to = setup("instanced")
    n, m = 130, 257
    f, t = np.ascontiguousarray(frm[spread(FULL, n)]), np.ascontiguousarray(to[spread(FULL, m)])
    occ = G.occluded(accel, segments(f, t)).reshape(n, m)
    counts = occ.sum(axis=1).astype(np.uint32)
    assert len(np.unique(counts)) > 8
    bits, blocked = G.visibility(accel, f, t, counts=True)
    assert np.array_equal(blocked, counts) and np.array_equal(blocked, np.unpackbits(bits, axis=1).sum(axis=1))
    garbage = np.random.default_rng(5).integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for _ in range(2):  # the same call twice: the same counts
        buf = garbage.copy()
        assert G.visibility(accel, f, t, into=(None, buf)) is buf  # counts only: bits = NULL
        assert np.array_equal(buf, counts)
    only = G.visibility(accel, f, t, counts="only")
    assert only.dtype == np.uint32 and np.array_equal(only, counts)
    alone = G.visibility(accel, f, t)  # bits only: blocked = NULL
    assert np.array_equal(alone, bits)


# ---- 6: edge inputs --------------------------------------------------------------------------------------------------------------------
def test_zero_directions_and_non_finite_coordinates():
    accel, frm, to = setup("cornell_glass")
    f, t = frm[spread(FULL, 19)].copy(), to[spread(FULL, 21)].copy()
    t[3] = f[5]                 # a zero direction
    t[8] = f[5]
    f[7, 1] = np.nan
    t[11, 2] = np.nan
    f[9, 0] = np.inf
    t[13, 1] = -np.inf
    t[14] = [np.inf, np.inf, np.nan]
    with np.errstate(invalid="ignore"):
        segs = segments(f, t)
    assert (segs[5 * 21 + 3, 3:] == 0.0).all() and np.isnan(segs[7 * 21:8 * 21, 1]).all() and np.isnan(segs[9 * 21 + 14, 3])  # (inf - inf)
    occ = G.occluded(accel, segs)
    bits, blocked = G.visibility(accel, f, t, counts=True)
    assert np.array_equal(bits, pack(occ, 19, 21))
    assert np.array_equal(blocked, occ.reshape(19, 21).sum(axis=1))
    assert occ.any() and not occ.all()


# ---- 7: device form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel, frm, to = setup(name)
    set_form(accel, form)
    n, m = 257, 1031
    f = np.ascontiguousarray(frm[spread(FULL, n)])
    try:
        device_form(torch, accel, f, to, n, m)
    finally:
        reset(accel)


def device_form(torch, accel, f, to, n, m):
    used = (m + 7) // 8
    host_bits, host_blocked = G.visibility(accel, f, to, counts=True)
    assert host_bits.any()
    df, dt = torch.from_numpy(f).cuda(), torch.from_numpy(to).cuda()
    stream = torch.cuda.Stream()
    for stride in (used, used + 3):
        dbits = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
        dblocked = torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        donly = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            G.visibility_device(accel, n, df.data_ptr(), m, dt.data_ptr(), dbits.data_ptr(), stride, dblocked.data_ptr(), stream=s)
            G.visibility_device(accel, n, df.data_ptr(), m, dt.data_ptr(), None, stride, donly.data_ptr(), stream=s)
        stream.synchronize()
        got = dbits.cpu().numpy()
        assert np.ascontiguousarray(got[:, :used]).tobytes() == host_bits.tobytes(), stride
        assert (got[:, used:] == 0xA5).all()
        assert dblocked.cpu().numpy().view(np.uint32).tobytes() == host_blocked.tobytes()
        assert donly.cpu().numpy().view(np.uint32).tobytes() == host_blocked.tobytes()


# ---- 8: errors and empty sets ------------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_empty_sets_are_a_no_op():
    torch = pytest.importorskip("torch")
    accel, frm, to = setup("cornell_glass")
    n, m = 20, 70
    f, t = np.ascontiguousarray(frm[:n + 1]), np.ascontiguousarray(to[:m])
    used = (m + 7) // 8
    df, dt = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    dbits = torch.full((n, used), 0xA5, dtype=torch.uint8, device="cuda")
    dblocked = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hbits = np.full((n, used), 0xA5, dtype=np.uint8)
    hblocked = np.full(n, 0x5A5A5A5A, dtype=np.uint32)
    torch.cuda.synchronize()
    V = G.visibility_device
    bad = [lambda: V(accel, n, f.ctypes.data, m, dt.data_ptr(), dbits.data_ptr(), used, dblocked.data_ptr(), stream=0),      # host pointers
           lambda: V(accel, n, df.data_ptr(), m, t.ctypes.data, dbits.data_ptr(), used, dblocked.data_ptr(), stream=0),
           lambda: V(accel, n, df.data_ptr(), m, dt.data_ptr(), hbits.ctypes.data, used, dblocked.data_ptr(), stream=0),
           lambda: V(accel, n, df.data_ptr(), m, dt.data_ptr(), dbits.data_ptr(), used, hblocked.ctypes.data, stream=0),
           lambda: V(accel, n, df.data_ptr() + 4, m, dt.data_ptr(), dbits.data_ptr(), used, dblocked.data_ptr(), stream=0),  # misaligned
           lambda: V(accel, n, df.data_ptr(), m, dt.data_ptr() + 4, dbits.data_ptr(), used, dblocked.data_ptr(), stream=0),
           lambda: V(accel, n, df.data_ptr(), m, dt.data_ptr(), dbits.data_ptr(), used, dblocked.data_ptr() + 2, stream=0),
           lambda: V(accel, n, df.data_ptr(), m, dt.data_ptr(), None, used, None, stream=0),                                 # both outputs NULL
           lambda: V(accel, n, df.data_ptr(), m, dt.data_ptr(), dbits.data_ptr(), used - 1, dblocked.data_ptr(), stream=0),  # row_bytes too small
           lambda: V(accel, n, None, m, dt.data_ptr(), dbits.data_ptr(), used, dblocked.data_ptr(), stream=0),
           lambda: V(accel, n, df.data_ptr(), m, None, dbits.data_ptr(), used, dblocked.data_ptr(), stream=0),
           lambda: V(accel, 1 << 36, df.data_ptr(), 1 << 36, dt.data_ptr(), None, 1 << 33, dblocked.data_ptr(), stream=0)]   # 2^66 segments
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    host = [(accel.h, f.ctypes.data, n, t.ctypes.data, m, None, used, None),
            (accel.h, f.ctypes.data, n, t.ctypes.data, m, hbits.ctypes.data, used - 1, hblocked.ctypes.data),
            (accel.h, None, n, t.ctypes.data, m, hbits.ctypes.data, used, hblocked.ctypes.data),
            (accel.h, f.ctypes.data, n, None, m, hbits.ctypes.data, used, hblocked.ctypes.data),
            (None, f.ctypes.data, n, t.ctypes.data, m, hbits.ctypes.data, used, hblocked.ctypes.data)]
    for k, args in enumerate(host):
        assert G.call("visibility", *args) != 0 and G.last_error(), k
    # empty point sets: success, nothing written (whatever the pointers)
    for nf, nt in ((0, m), (n, 0), (0, 0)):
        V(accel, nf, df.data_ptr(), nt, dt.data_ptr(), dbits.data_ptr(), used, dblocked.data_ptr(), stream=0)
        assert G.call("visibility", accel.h, f.ctypes.data, nf, t.ctypes.data, nt, hbits.ctypes.data, used, hblocked.ctypes.data) == 0
    assert G.call("visibility", accel.h, None, 0, None, 0, None, 0, None) == 0
    assert G.visibility(accel, np.zeros((0, 3)), t).shape == (0, used) and G.visibility(accel, f, np.zeros((0, 3))).shape == (n + 1, 0)
    torch.cuda.synchronize()
    assert (dbits.cpu().numpy() == 0xA5).all() and (dblocked.cpu().numpy() == 0x5A5A5A5A).all()
    assert (hbits == 0xA5).all() and (hblocked == 0x5A5A5A5A).all()
    # and the call still works afterwards
    V(accel, n, df.data_ptr(), m, dt.data_ptr(), dbits.data_ptr(), used, dblocked.data_ptr(), stream=0)
    torch.cuda.synchronize()
    want = G.visibility(accel, f[:n], t)
    assert dbits.cpu().numpy().tobytes() == want.tobytes()
