"""Range scans (include/lasgun_hip.h: lg_range_scan, lg_range_scan_device, lg_range_scan_lanes): the first hits along K shared beams from N
sensor poses, the rays made in the kernel, the answer as planes and two per-pose reductions.

The reference is restated here in numpy and NOTHING is tolerated: every plane and both reductions are compared bit for bit, floats as
uint32 views, NaNs included.  The explicit rays are built with the header's expression -- d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z,
three products and two sums, nothing fused -- or are the given bits when frames is None; they go through lg_intersect; then
range = t.astype(float32), point and normal = p and ng as float32, id = the four id words, hits = the count of kind != 0 and nearest = the
uint32 minimum of the hits' range patterns with initial value 0x7F800000.

  1  every traversal form, both lane forms and lanes=0 (4: identical bytes, and lg_range_scan_lanes names the form), all six outputs, for
     shapes with partial tiles on either side in either form, and (LDS form) more tiles than twice the grid's waves per lane form: the
     tile claim's other path;
  2  the same shapes, both lane forms, in the accel's default form against the CPU oracle's intersect (t, kind, prim, instance as the
     ray-query tests map them), three scenes;
  3  frames against the numpy expression: random rotations, a non-uniform scale with a shear, the identity frame on beams with -0.0, +-inf
     and NaN components (the rays differ from the NULL-frames rays exactly where the contract says), frames of NaNs, zero frames;
  5  outputs: every single plane alone and a few subsets, the same call twice, a pose with no hit (hits == 0, nearest == +inf).  The host
     form names only the buffers asked for to the library and stages its outputs, so "unrequested buffers untouched" and "over garbage"
     hold there by construction; they are really put to the test in 6 and 7;
  6  the device form on a stream that is not the default one: the host form's bytes, every output over a 0x25A5A5A5 prefill, the same
     call twice into the same buffers (hits and nearest written, not accumulated), and a subset of the outputs with the device buffers
     that were not asked for untouched;
  7  every error of the contract refused with every output at its prefill; empty sets a no-op.
No vacuous comparison: hits and misses are each at least 15 % of every full matrix (10 % with frames) and every smaller case holds at
least one of each, asserted on the reference's answer before anything is compared; the 1 x 1 case is run once for a hit and once for a miss.
Inputs, a function of the scene alone: with the camera's eye, view, up, aux, L = |view| and f = the Fibonacci lattice on the unit sphere,
pose i = eye + a_i view + 0.25 L (f_i.x aux + f_i.y up + f_i.z view / L), a = linspace(0, 1, 257), f = fib(257); the beams are fib(1031)."""
import ctypes

import numpy as np
import pytest

import pyref

import lasgun_amd as la
from lasgun_amd import _capi
from oracle_lib import oracle
from test_gpu_visibility import SCENES, FORMS, set_form, reset, spread, sphere_points

pytestmark = pytest.mark.gpu

G = la.api
NP, NB = 257, 1031                     # poses and beams per scene
INF_BITS = 0x7F800000
PLANES = la.SCAN_PLANES
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (63, 7), (64, 8), (65, 9), (129, 1), (17, 130), (NP, NB)]
BEAM, POSE = 1, 2


def fib(n):
    return sphere_points(np.zeros(3), 1.0, n)


def scan_inputs(name):
    """(poses, beams) of a scene: a function of the scene's camera alone."""
    cam = SCENES[name](pyref.Api).camera
    eye, view, up, aux = (np.array(v, dtype=np.float64) for v in (cam.origin, cam.view, cam.up, cam.aux))
    L = float(np.linalg.norm(view))
    f, a = fib(NP), np.linspace(0.0, 1.0, NP)
    poses = eye + a[:, None] * view + 0.25 * L * (f[:, 0:1] * aux + f[:, 1:2] * up + f[:, 2:3] * (view / L))
    return np.ascontiguousarray(poses), np.ascontiguousarray(fib(NB))


def explicit_rays(origins, frames, beams):
    """The n * k rays of a scan, pose-major: the header's expression in numpy f64 -- three products, two sums in the stated order, nothing
    fused -- or the beams' own bits without frames."""
    n, k = len(origins), len(beams)
    o = np.repeat(origins, k, axis=0)
    if frames is None:
        d = np.tile(beams, (n, 1))
    else:
        M, b = np.asarray(frames, dtype=np.float64).reshape(n, 1, 9), beams[None, :, :]
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.stack([(M[..., 3 * c] * b[..., 0] + M[..., 3 * c + 1] * b[..., 1]) + M[..., 3 * c + 2] * b[..., 2] for c in range(3)], axis=-1).reshape(n * k, 3)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


def restate(hits, n, k):
    """The six outputs of the contract from the lg_hit records of the n * k explicit rays."""
    with np.errstate(invalid="ignore", over="ignore"):
        rng = hits["t"].astype(np.float32).reshape(n, k)
        point = hits["p"].astype(np.float32).reshape(n, k, 3)
        normal = hits["ng"].astype(np.float32).reshape(n, k, 3)
    ident = np.stack([hits["kind"], hits["prim"], hits["instance"], hits["material"].view(np.uint32)], axis=1).astype(np.uint32).reshape(n, k, 4)
    hit = (hits["kind"] != 0).reshape(n, k)
    nearest = np.where(hit, rng.view(np.uint32), np.uint32(INF_BITS)).min(axis=1, initial=np.uint32(INF_BITS)).astype(np.uint32).view(np.float32)
    out = {"range": rng, "point": point, "normal": normal, "id": ident, "hits": hit.sum(axis=1).astype(np.uint32), "nearest": nearest}
    for v in out.values():
        v.setflags(write=False)
    return out


def sub(want, rows, cols):
    """The outputs of the rows x cols part of a matrix: the planes selected, the reductions taken again."""
    out = {p: np.ascontiguousarray(want[p][np.ix_(rows, cols)]) for p in ("range", "point", "normal", "id")}
    hit = out["id"][..., 0] != 0
    out["hits"] = hit.sum(axis=1).astype(np.uint32)
    out["nearest"] = np.where(hit, out["range"].view(np.uint32), np.uint32(INF_BITS)).min(axis=1, initial=np.uint32(INF_BITS)).astype(np.uint32).view(np.float32)
    return out


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare(ctx, got, want, planes=PLANES):
    assert set(got) == set(planes), (ctx, sorted(got))
    for p in planes:
        g, w = got[p], want[p]
        assert g.shape == w.shape and g.dtype == w.dtype, (ctx, p, g.shape, w.shape, g.dtype, w.dtype)
        diff = words(g) != words(w)
        assert not diff.any(), (ctx, p, int(diff.sum()), "words differ; first at", np.argwhere(diff)[0].tolist(), g[tuple(np.argwhere(diff)[0][:g.ndim])],
                                w[tuple(np.argwhere(diff)[0][:w.ndim])])


def not_vacuous(want, ctx, share=0.0):
    hit = want["id"][..., 0] != 0
    f = float(hit.mean())
    assert 0.0 < f < 1.0 and share <= f <= 1.0 - share, ("the comparison would be vacuous: hit share", f, ctx)


def mixed(share):
    """The index whose hit share is nearest one half."""
    return int(np.argmin(np.abs(share - 0.5)))


def choose(hit, n, m):
    """Rows and columns of the full matrix for an n x m case: spread evenly; a single row or column is the most mixed one of the full
    matrix (a choice of INPUTS, made on the reference's answer)."""
    rows, cols = spread(NP, n), spread(NB, m)
    if n == 1:
        rows = np.array([mixed(hit[:, cols].mean(axis=1))])
    if m == 1:
        cols = np.array([mixed(hit[rows].mean(axis=0))])
    return rows, cols


_setup = {}


def setup(name):
    """(accel, poses, beams) of a scene, built once."""
    if name not in _setup:
        poses, beams = scan_inputs(name)
        _setup[name] = (G.Accel.from_scene(SCENES[name](G)), poses, beams)
    return _setup[name]


_full = {}


def full_reference(name, form, accel):
    """The six outputs of the scene's full matrix by lg_intersect in the accel's current form; computed once per (scene, form), never changed."""
    if (name, form) not in _full:
        _, poses, beams = setup(name)
        _full[name, form] = restate(G.intersect(accel, explicit_rays(poses, None, beams)), NP, NB)
    return _full[name, form]


def scan(accel, o, b, frames=None, planes=PLANES, lanes=0):
    return G.range_scan(accel, o, b, frames, planes, lanes)


# ---- 1 and 4: bit for bit against the restatement, every form, both lane forms and auto -----------------------------------------------
@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_planes_and_reductions_equal_the_restatement(name, form):
    accel, poses, beams = setup(name)
    set_form(accel, form)
    try:
        full = full_reference(name, form, accel)
        not_vacuous(full, (name, form), share=0.15)
        hit = full["id"][..., 0] != 0
        for n, m in SHAPES:
            if (n, m) == (1, 1):
                continue
            rows, cols = choose(hit, n, m)
            o, b = np.ascontiguousarray(poses[rows]), np.ascontiguousarray(beams[cols])
            want = sub(full, rows, cols)
            if (n, m) != (NP, NB):
                again = restate(G.intersect(accel, explicit_rays(o, None, b)), n, m)
                compare((name, form, n, m, "not a function of the ray"), again, want)
            not_vacuous(want, (name, form, n, m))
            for lanes in (BEAM, POSE, 0):
                compare((name, form, n, m, lanes), scan(accel, o, b, lanes=lanes), want)
            assert G.range_scan_lanes(n, m) == (POSE if n >= m else BEAM) == G.call("range_scan_lanes", n, m, 0)
        # 1 x 1: one ray, so once for a hit and once for a miss
        for cls in (True, False):
            at = np.argwhere(hit == cls)
            i, k = at[len(at) // 2]
            o, b = poses[i:i + 1].copy(), beams[k:k + 1].copy()
            want = restate(G.intersect(accel, explicit_rays(o, None, b)), 1, 1)
            assert bool(want["id"][0, 0, 0] != 0) == cls and int(want["hits"][0]) == int(cls)
            assert np.isinf(want["range"][0, 0]) == (not cls) and np.isinf(want["nearest"][0]) == (not cls)
            for lanes in (BEAM, POSE, 0):
                compare((name, form, "1 x 1", cls, lanes), accel.range_scan(o, b, None, PLANES, lanes), want)
    finally:
        reset(accel)


@pytest.mark.parametrize("lanes", [BEAM, POSE], ids=["beam-lanes", "pose-lanes"])
def test_more_tiles_than_twice_the_grids_waves(lanes):
    """LDS form: one 1024-lane workgroup per CU, 16 waves each.  Beam lanes: 257 poses x ceil(K / 64) tiles; pose lanes: 5 blocks of 64
    poses x ceil(K / 8) tiles; K is the least lattice that passes 2 x 16 x CUs tiles."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per, blocks = (64, NP) if lanes == BEAM else (8, (NP + 63) // 64)
    k = per * (2 * 16 * cus // blocks) + 1
    assert blocks * ((k + per - 1) // per) > 2 * 16 * cus
    accel, poses, _ = setup("cornell_glass")
    beams = np.ascontiguousarray(fib(k))
    set_form(accel, "lds")
    try:
        want = restate(G.intersect(accel, explicit_rays(poses, None, beams)), NP, k)
        not_vacuous(want, ("lds", lanes, k), share=0.15)
        compare(("lds", lanes, NP, k), scan(accel, poses, beams, lanes=lanes), want)
    finally:
        reset(accel)


# ---- 2: against the CPU oracle ---------------------------------------------------------------------------------------------------------
def against_oracle(ctx, got, want):
    compare(ctx, {p: got[p] for p in ("range", "hits", "nearest")}, want, ("range", "hits", "nearest"))
    assert np.array_equal(got["id"][..., :3], want["id"][..., :3]), (ctx, "kind, prim, instance")
    assert np.array_equal(got["id"][..., 3] == 0xFFFFFFFF, want["id"][..., 0] == 0), (ctx, "a material exactly where there is a hit")


@pytest.mark.parametrize("name", ["cornell_glass", "instanced", "mesh_glass"])
def test_range_ids_and_reductions_equal_the_cpu_oracles_answer(name):
    """The full matrix and every smaller shape of case 1, both lane forms, in the accel's own default form."""
    accel, poses, beams = setup(name)
    o = oracle()
    oaccel = o.Accel(SCENES[name](o))
    o.set_trig_mode(True)
    try:
        ohits, _ = o.intersect(oaccel, explicit_rays(poses, None, beams), 16)
    finally:
        o.set_trig_mode(False)
    want = restate(ohits, NP, NB)
    not_vacuous(want, (name, "oracle"), share=0.15)
    hit = want["id"][..., 0] != 0
    for n, m in SHAPES:
        cases = [choose(hit, n, m)] if (n, m) != (1, 1) else [tuple(np.array([v]) for v in np.argwhere(hit == cls)[(hit == cls).sum() // 2]) for cls in (True, False)]
        for rows, cols in cases:
            part = sub(want, rows, cols)
            if (n, m) != (1, 1):
                not_vacuous(part, (name, "oracle", n, m))
            for lanes in (BEAM, POSE):
                against_oracle((name, "oracle", n, m, lanes), scan(accel, np.ascontiguousarray(poses[rows]), np.ascontiguousarray(beams[cols]), lanes=lanes), part)


# ---- 3: frames -------------------------------------------------------------------------------------------------------------------------
def rotations(n, seed):
    q = np.linalg.qr(np.random.default_rng(seed).normal(size=(n, 3, 3)))[0]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    assert np.allclose(np.linalg.det(q), 1.0) and np.abs(q @ q.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    return np.ascontiguousarray(q.reshape(n, 9))


def frame_case(accel, ctx, o, frames, b, share=0.10):
    n, m = len(o), len(b)
    want = restate(G.intersect(accel, explicit_rays(o, frames, b)), n, m)
    not_vacuous(want, ctx, share=share)
    for lanes in (BEAM, POSE):
        compare(ctx + (lanes,), scan(accel, o, b, frames, lanes=lanes), want)
    return want


@pytest.mark.parametrize("name,form", [("instanced", "reference"), ("cornell_glass", "lds"), ("mesh_glass", "fast")])
def test_frames_follow_the_numpy_expression(name, form):
    accel, poses, beams = setup(name)
    n, m = 65, 130
    o, b = np.ascontiguousarray(poses[spread(NP, n)]), np.ascontiguousarray(beams[spread(NB, m)])
    rot = rotations(n, 11)
    set_form(accel, form)
    try:
        plain = restate(G.intersect(accel, explicit_rays(o, None, b)), n, m)
        turned = frame_case(accel, (name, form, "rotations"), o, rot, b)
        assert not np.array_equal(words(turned["range"]), words(plain["range"])), "the frames are live"
        frame_case(accel, (name, form, "rotations as (n, 3, 3)"), o, rot.reshape(n, 3, 3), b)
        shear = np.array([[2.0, 0.5, 0.0], [0.0, 0.5, 0.25], [0.0, 0.0, 3.0]])
        frame_case(accel, (name, form, "scale and shear"), o, np.ascontiguousarray((rot.reshape(n, 3, 3) @ shear).reshape(n, 9)), b)
        # frames of NaNs and zero frames, on some of the poses (all of them would leave one class empty)
        odd = rot.copy()
        odd[1::5] = np.nan
        odd[3::5] = 0.0
        odd[4::10, 4] = np.nan  # one NaN entry
        frame_case(accel, (name, form, "NaN and zero frames"), o, odd, b)
    finally:
        reset(accel)


def test_an_identity_frame_is_not_null_frames():
    accel, poses, beams = setup("instanced")
    n, m = 65, 130
    o, b = np.ascontiguousarray(poses[spread(NP, n)]), np.ascontiguousarray(beams[spread(NB, m)])
    inf, nan = np.inf, np.nan
    special = np.array([[-0.0, 0.6, 0.8], [0.6, -0.0, 0.8], [0.6, 0.8, -0.0], [inf, 0.0, 1.0], [0.0, -inf, 1.0], [nan, 0.0, 1.0], [0.0, 1.0, nan], [-0.0, -0.0, -1.0]])
    at = np.arange(len(special)) * 9 + 2
    b[at] = special
    ident = np.ascontiguousarray(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    r_null, r_id = explicit_rays(o, None, b), explicit_rays(o, ident, b)
    differs = (r_null.view(np.uint64) != r_id.view(np.uint64)).any(axis=1).reshape(n, m)
    expect = np.zeros(m, dtype=bool)
    expect[at[:7]] = True  # (the last one is -0.0 in a product sum of -0.0s: the same bits through the identity)
    assert np.array_equal(differs, np.tile(expect, (n, 1))), "the rays differ exactly at the beams with a -0.0, infinite or NaN component"
    d = r_id[:m, 3:]
    assert not np.signbit(d[at[0], 0]) and d[at[0], 0] == 0.0 and not np.signbit(d[at[2], 2]), "-0.0 comes out as +0.0"
    assert np.isinf(d[at[3], 0]) and np.isnan(d[at[3], 1:]).all() and np.isnan(d[at[5]]).all() and np.isnan(d[at[6]]).all(), "0 * inf and NaN"
    assert np.signbit(d[at[7], 0]) and np.signbit(d[at[7], 1]) and d[at[7], 2] == -1.0, "-0.0 survives where both other products are -0.0"
    want_null = frame_case(accel, ("identity", "NULL frames"), o, None, b)
    want_id = frame_case(accel, ("identity", "identity frames"), o, ident, b)
    same = ~expect
    assert np.array_equal(words(want_null["range"][:, same]), words(want_id["range"][:, same]))


# ---- 5: outputs ------------------------------------------------------------------------------------------------------------------------
def empty_pose(accel, poses, beams):
    """A pose none of whose beams hits anything: far behind the camera, with the beams that look away from the scene (asserted on the
    reference's answer)."""
    cam = SCENES["instanced"](pyref.Api).camera
    view = np.array(cam.view, dtype=np.float64)
    o = (np.array(cam.origin, dtype=np.float64) - 1000.0 * view)[None, :]
    away = np.ascontiguousarray(beams[beams @ view < -0.5 * np.linalg.norm(view)])
    assert len(away) > 64
    assert (G.intersect(accel, explicit_rays(o, None, away))["kind"] == 0).all()
    return o, away


def test_outputs_alone_in_subsets_over_garbage_and_twice():
    accel, poses, beams = setup("instanced")
    n, m = 66, 130
    far, away = empty_pose(accel, poses, beams)
    o = np.ascontiguousarray(np.concatenate([poses[spread(NP, n - 1)], far]))
    b = np.ascontiguousarray(np.concatenate([away[:m // 2], beams[spread(NB, m - m // 2)]]))
    want = restate(G.intersect(accel, explicit_rays(o, None, b)), n, m)
    not_vacuous(want, "outputs", share=0.10)
    assert want["hits"][-1] == 0 and np.isposinf(want["nearest"][-1]), "a pose with no hit"
    assert len(np.unique(want["hits"])) > 8 and (want["hits"][:-1] > 0).all() and np.isfinite(want["nearest"][:-1]).all()
    shapes = {p: want[p].shape for p in PLANES}
    rng = np.random.default_rng(5)
    subsets = [(p,) for p in PLANES] + [("range", "hits"), ("hits", "nearest"), ("point", "id"), ("range", "normal", "nearest"), PLANES]
    for lanes in (BEAM, POSE):
        for planes in subsets:
            # every buffer exists and is garbage; only those asked for are named to the library (so the others stay by construction,
            # and the host form stages: what garbage and a repeated call really test is the device form's business, case 6)
            bufs = {p: rng.integers(1, 2 ** 32, int(np.prod(shapes[p])), dtype=np.uint64).astype(np.uint32).view(want[p].dtype).reshape(shapes[p]) for p in PLANES}
            for p in PLANES:
                if p not in planes:
                    bufs[p].view(np.uint32)[...] = 0xA5A5A5A5
            for _ in range(2):  # the same call twice: the same bytes, nothing accumulated
                got = G.range_scan(accel, o, b, None, planes, lanes, into={p: bufs[p] for p in planes})
                assert all(got[p] is bufs[p] for p in planes)
                compare(("outputs", lanes, planes), got, want, planes)
            assert all((words(bufs[p]) == 0xA5A5A5A5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", lanes, planes)
    got = accel.range_scan(o, b)
    assert list(got) == ["range"]
    compare("the default plane", got, want, ("range",))


# ---- 6: device form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel, poses, beams = setup(name)
    n, m = 129, NB
    o = np.ascontiguousarray(poses[spread(NP, n)])
    frames = rotations(n, 3)
    set_form(accel, form)
    try:
        for fr in (None, frames):
            want = restate(G.intersect(accel, explicit_rays(o, fr, beams)), n, m)
            not_vacuous(want, ("device form", name, fr is not None), share=0.10)
            host = scan(accel, o, beams, fr)
            compare(("host form", name), host, want)
            do, db = torch.from_numpy(o).cuda(), torch.from_numpy(beams).cuda()
            dfr = torch.from_numpy(fr).cuda() if fr is not None else None
            stream = torch.cuda.Stream()
            for lanes in (BEAM, POSE):
                dev = {p: torch.full((int(np.prod(want[p].shape)),), 0x25A5A5A5, dtype=torch.int32, device="cuda") for p in PLANES}
                few = {p: torch.full((int(np.prod(want[p].shape)),), 0x25A5A5A5, dtype=torch.int32, device="cuda") for p in PLANES}
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    s = torch.cuda.current_stream().cuda_stream
                    assert s != 0
                    ptr = lambda t: t.data_ptr()  # noqa: E731
                    for _ in range(2):  # the second call runs over the first one's results: written, not accumulated
                        G.range_scan_device(accel, n, ptr(do), ptr(dfr) if dfr is not None else None, m, ptr(db), *[ptr(dev[p]) for p in PLANES], lanes=lanes, stream=s)
                    G.range_scan_device(accel, n, ptr(do), ptr(dfr) if dfr is not None else None, m, ptr(db), range_ptr=ptr(few["range"]),
                                        nearest_ptr=ptr(few["nearest"]), lanes=lanes, stream=s)
                stream.synchronize()
                for p in PLANES:
                    assert dev[p].cpu().numpy().view(np.uint32).tobytes() == host[p].tobytes(), (name, lanes, p)
                    if p in ("range", "nearest"):
                        assert few[p].cpu().numpy().view(np.uint32).tobytes() == host[p].tobytes(), (name, lanes, p, "a subset")
                    else:
                        assert (few[p].cpu().numpy() == 0x25A5A5A5).all(), (name, lanes, p, "not asked for")
    finally:
        reset(accel)


# ---- 7: errors and empty sets ----------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_empty_sets_are_a_no_op():
    torch = pytest.importorskip("torch")
    accel, poses, beams = setup("cornell_glass")
    n, m = 70, 20
    o, b, fr = np.ascontiguousarray(poses[:n + 1]), np.ascontiguousarray(beams[:m + 1]), rotations(n + 1, 1)
    do, db, dfr = torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(fr).cuda()
    sizes = {"range": n * m, "point": n * m * 3, "normal": n * m * 3, "id": n * m * 4, "hits": n, "nearest": n}
    dev = {p: torch.full((sizes[p],), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for p in PLANES}
    hst = {p: np.full(sizes[p], 0x5A5A5A5A, dtype=np.uint32) for p in PLANES}
    torch.cuda.synchronize()
    O, F, B = do.data_ptr(), dfr.data_ptr(), db.data_ptr()
    D = {p: dev[p].data_ptr() for p in PLANES}
    H = {p: hst[p].ctypes.data for p in PLANES}

    def V(n_poses, origins, frames, n_beams, beams_, lanes=0, **out):
        ptrs = dict(D)
        ptrs.update(out)
        G.range_scan_device(accel, n_poses, origins, frames, n_beams, beams_, *[ptrs[p] for p in PLANES], lanes=lanes, stream=0)

    bad = [lambda: V(n, o.ctypes.data, F, m, B),                          # host pointers
           lambda: V(n, O, fr.ctypes.data, m, B),
           lambda: V(n, O, F, m, b.ctypes.data)]
    bad += [lambda p=p: V(n, O, F, m, B, **{p: H[p]}) for p in PLANES]
    bad += [lambda: V(n, O + 4, F, m, B),                                 # misaligned
            lambda: V(n, O, F + 4, m, B),
            lambda: V(n, O, F, m, B + 4)]
    bad += [lambda p=p: V(n, O, F, m, B, **{p: D[p] + 2}) for p in PLANES]
    bad += [lambda: V(n, O, F, m, B, id=D["id"] + 8),                     # id is 16-byte aligned
            lambda: V(n, O, F, m, B, **{p: None for p in PLANES}),        # all six outputs NULL
            lambda: V(n, None, F, m, B),                                  # NULL tables with non-zero counts
            lambda: V(n, O, F, m, None),
            lambda: V(n, O, F, m, B, lanes=3),                            # a bad lanes
            lambda: V(n, O, F, m, B, lanes=-1),
            lambda: V(n, O, F, 1 << 32, B, lanes=BEAM),                   # n_beams > 2^32 - 1
            lambda: V(n, O, F, 1 << 32, B, lanes=POSE),
            lambda: V(1 << 32, O, None, 64, B, lanes=BEAM),               # 2^32 tiles of one pose x 64 beams
            lambda: V((1 << 32) - 1, O, None, 65, B, lanes=BEAM),
            lambda: V(1 << 38, O, None, 8, B, lanes=POSE),                # 2^32 tiles of 64 poses x 8 beams
            lambda: V(1 << 36, O, None, 1 << 30, B),                      # 2^66 pairs
            lambda: V(1 << 24, O, None, 1, B, **{p: None for p in PLANES if p != "hits"})]  # 384 MiB of origins: the buffer ends long before
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    ho, hf, hb = o.ctypes.data, fr.ctypes.data, b.ctypes.data
    full = _capi.CScanOut(*[H[p] for p in PLANES])
    none = _capi.CScanOut()
    A = ctypes.addressof
    host = [(accel.h, ho, hf, n, hb, m, 0, A(none)),
            (accel.h, ho, hf, n, hb, m, 0, None),
            (accel.h, None, hf, n, hb, m, 0, A(full)),
            (accel.h, ho, hf, n, None, m, 0, A(full)),
            (None, ho, hf, n, hb, m, 0, A(full)),
            (accel.h, ho, hf, n, hb, m, 3, A(full)),
            (accel.h, ho, hf, n, hb, m, -7, A(full)),
            (accel.h, ho, hf, n, hb, 1 << 32, 0, A(full)),
            (accel.h, ho, hf, 1 << 32, hb, 64, BEAM, A(full)),
            (accel.h, ho, hf, 1 << 38, hb, 8, POSE, A(full)),
            (accel.h, ho, hf, 1 << 36, hb, 1 << 30, 0, A(full))]
    for k, args in enumerate(host):
        assert G.call("range_scan", *args) != 0 and G.last_error(), k
    # empty sets: success, nothing written (whatever the pointers)
    for n_, m_ in ((0, m), (n, 0), (0, 0)):
        V(n_, O, F, m_, B)
        assert G.call("range_scan", accel.h, ho, hf, n_, hb, m_, 0, A(full)) == 0
    assert G.call("range_scan", accel.h, None, None, 0, None, 0, 0, None) == 0
    assert scan(accel, np.zeros((0, 3)), b)["range"].shape == (0, m + 1) and scan(accel, o, np.zeros((0, 3)))["hits"].shape == (n + 1,)
    torch.cuda.synchronize()
    assert all((dev[p].cpu().numpy() == 0x5A5A5A5A).all() for p in PLANES) and all((hst[p] == 0x5A5A5A5A).all() for p in PLANES)
    # and the call still works afterwards
    V(n, O, F, m, B)
    torch.cuda.synchronize()
    want = scan(accel, o[:n], b[:m], fr[:n])
    for p in PLANES:
        assert dev[p].cpu().numpy().view(np.uint32).tobytes() == want[p].tobytes(), p
