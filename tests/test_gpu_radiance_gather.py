"""Radiance gathers (include/lasgun_hip.h: lg_radiance_gather, lg_radiance_gather_device, lg_radiance_gather_lanes): li() along K shared
directions from N poses, the rays made in the kernel, the answer as a plane and / or reduced per pose by the caller's weights.

The contract is restated here in numpy over lg_radiance and NOTHING is tolerated: both outputs are compared as uint64 views with every NaN
canonicalised (bits, tests/test_gpu_radiance_query.py).  The explicit rays are explicit_rays of tests/test_gpu_range_scan.py (the header's
expression, or the given bits without frames); radiance[i, k] = lg_radiance of ray (i, k); sums[i, c] = the loop acc = acc + L[i, k] * W[k, c]
over k in order from +0.0, one numpy product and one numpy sum a step.

  1  every traversal form x lanes 1, 2, 0 on the 257 x 1031 matrix of scan_inputs and its sub-shapes, n_weights 9 (both planes: li is the
     caller's plane), 3 and 1 (sums alone: li is parked); in the LDS form more tiles than twice the grid's waves per lane form;
  2  no vacuous comparison, asserted on the reference before anything is compared: hits and misses (lg_intersect) are each at least 15 % of
     every full matrix; on cornell_glass and mesh_glass at least 1 % of the rays' radiance differs from the same scene at recursion 0 (level
     0's child append and combine are live); `instanced` has no glass or mirror and covers the one-level path; 1 x 1 runs for a hit and a miss;
  3  pinned to the CPU oracle: three perspective cameras translated by dyadic offsets share their directions -- poses = their eyes, dirs =
     camera 0's 48 x 32 directions, NULL frames -- and the radiance plane equals the oracle's capture_radiance of each camera;
  4  frames (rotations, a sheared scale, the identity against NULL on -0.0, +-inf and NaN directions, NaN and zero frames) and weights (a zero
     column, +-inf and NaN entries, -0.0);
  5  each plane alone and both, the same call twice, and a child process whose parked li is cut into >= 3 batches of >= 2 chunks each (read
     from its LASGUN_DEBUG lines): the one-batch bytes;
  6  the device form on a stream that is not the default one: the host form's bytes over a prefill, buffers not asked for untouched, a render
     and a gather on one accel;
  7  every error of the contract refused with the outputs at their prefill; empty sets a no-op."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import _capi
from lasgun_amd import scenes as S
from test_gpu_radiance_query import L0_CASES, L0_FORMS, L0_IDS, bits, each_form, l0_scene, mixed_rays, oracle_radiance, with_camera, many_lights_scene
from test_gpu_range_scan import NP, NB, explicit_rays, fib, rotations, setup as scan_setup
from test_gpu_visibility import SCENES, FORMS, set_form, reset, spread

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
DIR, POSE = 1, 2
SHAPES = [(1, 63), (1, 64), (1, 65), (63, 1), (64, 1), (65, 1), (65, 9), (17, 130), (NP, NB)]
WEIGHTS = np.ascontiguousarray(np.random.default_rng(16).normal(size=(NB, 9)))  # seeded normal weights; n_weights c uses the first c columns
WEIGHTS.setflags(write=False)


def seq_sums(L, W):
    """The contract's reduction: acc = +0.0, then acc = acc + L[:, k] * W[k] for k in order; (n, k, 3) x (k, c) -> (n, c, 3)."""
    acc = np.zeros((L.shape[0], W.shape[1], 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(L.shape[1]):
            acc = acc + L[:, k, None, :] * W[k, :, None]
    return acc


def same(ctx, got, want):
    assert got.shape == want.shape and got.dtype == np.float64, (ctx, got.shape, want.shape)
    diff = bits(got) != bits(want)
    assert not diff.any(), (ctx, int(diff.sum()), "words differ; first at", np.argwhere(diff)[0].tolist())


def check_gather(ctx, accel, o, b, frames, W, L, lanes_set=(DIR, POSE, 0)):
    """Every lane form: n_weights 9 with both planes, 3 and 1 with sums alone, against radiance L (n, k, 3) and the sequential sums."""
    for c, planes in ((9, ("radiance", "sums")), (3, ("sums",)), (1, ("sums",))):
        Wc = np.ascontiguousarray(W[:, :c])
        want = seq_sums(L, Wc)
        for lanes in lanes_set:
            got = G.radiance_gather(accel, o, b, frames, Wc, planes, lanes)
            assert set(got) == set(planes)
            same(ctx + (c, lanes, "sums"), got["sums"], want)
            if "radiance" in planes:
                same(ctx + (c, lanes, "radiance"), got["radiance"], L)


_flat = {}


def recursion_is_live(name, rays, L):
    """At least 1 % of the rays' radiance differs from the same scene at recursion 0: level 0 appends children and combines them."""
    if name not in _flat:
        scene = SCENES[name](G)
        scene.set_max_recursion_depth(0)
        _flat[name] = G.radiance(G.Accel.from_scene(scene), rays)
    share = float((bits(_flat[name]) != bits(L.reshape(-1, 3))).any(axis=1).mean())
    assert share >= 0.01, ("the recursion does not show in these rays", name, share)


_full = {}


def full_reference(name, form, accel):
    """(hit mask, radiance) of the scene's full matrix by lg_intersect / lg_radiance in the accel's current form; once per (scene, form)."""
    if (name, form) not in _full:
        _, poses, dirs = scan_setup(name)
        rays = explicit_rays(poses, None, dirs)
        hit = (G.intersect(accel, rays)["kind"] != 0).reshape(NP, NB)
        L = G.radiance(accel, rays).reshape(NP, NB, 3)
        assert 0.15 <= hit.mean() <= 0.85, ("the comparison would be vacuous: hit share", float(hit.mean()), name, form)
        if name in ("cornell_glass", "mesh_glass"):
            recursion_is_live(name, rays, L)
        hit.setflags(write=False); L.setflags(write=False)
        _full[name, form] = (hit, L)
    return _full[name, form]


# ---- 1 and 2: the restatement, every form, both lane forms and auto -------------------------------------------------------------------
@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_radiance_and_sums_equal_the_restatement_over_lg_radiance(name, form):
    accel, poses, dirs = scan_setup(name)
    set_form(accel, form)
    try:
        hit, full = full_reference(name, form, accel)
        for n, m in SHAPES:
            rows, cols = spread(NP, n), spread(NB, m)
            if n == 1:
                rows = np.array([int(np.argmin(np.abs(hit[:, cols].mean(axis=1) - 0.5)))])
            if m == 1:
                cols = np.array([int(np.argmin(np.abs(hit[rows].mean(axis=0) - 0.5)))])
            o, b = np.ascontiguousarray(poses[rows]), np.ascontiguousarray(dirs[cols])
            L = np.ascontiguousarray(full[np.ix_(rows, cols)])
            part = hit[np.ix_(rows, cols)]
            assert 0.0 < part.mean() < 1.0, ("the comparison would be vacuous", name, form, n, m)
            if (n, m) != (NP, NB):
                same((name, form, n, m, "a function of the ray"), G.radiance(accel, explicit_rays(o, None, b)).reshape(n, m, 3), L)
            check_gather((name, form, n, m), accel, o, b, None, WEIGHTS[cols], L)
            assert G.radiance_gather_lanes(n, m) == (POSE if n >= m else DIR) == G.call("radiance_gather_lanes", n, m, 0)
        for cls in (True, False):  # 1 x 1: one ray, so once for a hit and once for a miss
            at = np.argwhere(hit == cls)
            i, k = at[len(at) // 2]
            o, b = poses[i:i + 1].copy(), dirs[k:k + 1].copy()
            assert bool(G.intersect(accel, explicit_rays(o, None, b))["kind"][0] != 0) == cls
            check_gather((name, form, "1 x 1", cls), accel, o, b, None, WEIGHTS[k:k + 1], G.radiance(accel, explicit_rays(o, None, b)).reshape(1, 1, 3))
    finally:
        reset(accel)


@pytest.mark.parametrize("lanes", [DIR, POSE], ids=["direction-lanes", "pose-lanes"])
def test_more_tiles_than_twice_the_grids_waves(lanes):
    """LDS form: one 1024-lane workgroup per CU, 16 waves each.  Direction lanes: 257 poses x ceil(K / 64) tiles; pose lanes: 5 blocks of 64
    poses x K tiles; K is the least count that passes 2 x 16 x CUs tiles."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = 64 * (2 * 16 * cus // NP) + 1 if lanes == DIR else 2 * 16 * cus // ((NP + 63) // 64) + 1
    tiles = NP * ((k + 63) // 64) if lanes == DIR else ((NP + 63) // 64) * k
    assert tiles > 2 * 16 * cus
    accel, poses, _ = scan_setup("cornell_glass")
    dirs = np.ascontiguousarray(fib(k))
    W = np.ascontiguousarray(np.random.default_rng(k).normal(size=(k, 3)))
    set_form(accel, "lds")
    try:
        rays = explicit_rays(poses, None, dirs)
        hit = G.intersect(accel, rays)["kind"] != 0
        assert 0.15 <= hit.mean() <= 0.85
        L = G.radiance(accel, rays).reshape(NP, k, 3)
        for planes in (("radiance", "sums"), ("sums",)):
            got = G.radiance_gather(accel, poses, dirs, None, W, planes, lanes)
            same(("lds", lanes, k, planes), got["sums"], seq_sums(L, W))
            if "radiance" in planes:
                same(("lds", lanes, k, "radiance"), got["radiance"], L)
    finally:
        reset(accel)


# ---- 3: pinned to the CPU oracle --------------------------------------------------------------------------------------------------------
CAMERAS = [
    ("cornell_glass", lambda api: S.cornell_scene(api, "glass"), True, 60.0, (0.0, 1.0, 0.0),
     [((2.0, 0.75, 6.0), (0.0, -0.5, 0.0)), ((1.0, 1.25, 5.0), (-1.0, 0.0, -1.0)), ((2.5, 0.25, 6.5), (0.5, -1.0, 0.5))]),
    ("instanced", lambda api: S.instanced_scene(api), False, 60.0, (0.0, 1.0, 0.0),  # (no glass or mirror: the one-level path)
     [((2.0, 0.75, 6.0), (0.0, -0.5, 0.0)), ((1.0, 1.25, 5.0), (-1.0, 0.0, -1.0)), ((2.5, 0.25, 6.5), (0.5, -1.0, 0.5))]),
    ("kitchen_sink", lambda api: S.kitchen_sink_scene(api, supersampling=0), True, 65.0, (0.0, 1.0, 0.125),
     [((-6.0, 3.0, 5.0), (0.5, -0.25, 0.0)), ((-5.0, 3.5, 6.0), (1.5, 0.25, 1.0)), ((-6.5, 2.5, 4.5), (0.0, -0.75, -0.5))]),
]


@pytest.mark.parametrize("name,builder,specular,fov,up,views", CAMERAS, ids=[c[0] for c in CAMERAS])
def test_translated_cameras_give_the_oracles_render_of_each(name, builder, specular, fov, up, views):
    w, h = 48, 32
    accel = G.Accel.from_scene(builder(G))
    cams = [("perspective", fov, eye, look, up) for eye, look in views]
    rays = [G.camera_rays(G.Accel.from_scene(with_camera(builder(G), cam)), w, h) for cam in cams]
    dirs = np.ascontiguousarray(rays[0][:, 3:])
    eyes = np.ascontiguousarray(np.array([r[0, :3] for r in rays]))
    for k, r in enumerate(rays):
        assert np.array_equal(r[:, 3:].view(np.uint64), dirs.view(np.uint64)), (name, k, "the cameras share their directions bit for bit")
        assert (r[:, :3].view(np.uint64) == eyes[k].view(np.uint64)).all() and np.array_equal(eyes[k], np.array(views[k][0])), (name, k, "one origin each")
        hit = G.intersect(accel, r)["kind"] != 0
        assert 0.2 <= hit.mean() <= 0.8, (name, k, float(hit.mean()))
    want = np.stack([oracle_radiance(lambda api, cam=cam: with_camera(builder(api), cam), w, h).reshape(-1, 3) for cam in cams])
    if specular:
        flat_accel = G.Accel.from_scene(with_camera(builder(G), cams[0], recursion=0))
        for k, r in enumerate(rays):
            share = float((bits(G.radiance(flat_accel, r)) != bits(want[k])).any(axis=1).mean())
            assert share >= 0.02, (name, k, "the recursion changes too few pixels", share)
    for lanes in (DIR, POSE):
        got = G.radiance_gather(accel, eyes, dirs, None, None, ("radiance",), lanes)["radiance"]
        same((name, lanes, "the oracle's render of each camera"), got, want)


# ---- 4: frames and weights --------------------------------------------------------------------------------------------------------------
def frame_case(accel, ctx, o, frames, b, W):
    rays = explicit_rays(o, frames, b)
    L = G.radiance(accel, rays).reshape(len(o), len(b), 3)
    check_gather(ctx, accel, o, b, frames, W, L, lanes_set=(DIR, POSE))
    return L


@pytest.mark.parametrize("name,form", [("instanced", "reference"), ("cornell_glass", "lds"), ("mesh_glass", "fast")])
def test_frames_follow_the_numpy_expression(name, form):
    accel, poses, dirs = scan_setup(name)
    n, m = 65, 130
    rows, cols = spread(NP, n), spread(NB, m)
    o, b, W = np.ascontiguousarray(poses[rows]), np.ascontiguousarray(dirs[cols]), WEIGHTS[cols]
    rot = rotations(n, 11)
    set_form(accel, form)
    try:
        plain = G.radiance(accel, explicit_rays(o, None, b)).reshape(n, m, 3)
        hit = G.intersect(accel, explicit_rays(o, rot, b))["kind"] != 0
        assert 0.10 <= hit.mean() <= 0.90, (name, form, float(hit.mean()))
        turned = frame_case(accel, (name, form, "rotations"), o, rot, b, W)
        assert not np.array_equal(bits(turned), bits(plain)), "the frames are live"
        same((name, form, "(n, 3, 3)"), G.radiance_gather(accel, o, b, rot.reshape(n, 3, 3), None, ("radiance",), POSE)["radiance"], turned)
        shear = np.array([[2.0, 0.5, 0.0], [0.0, 0.5, 0.25], [0.0, 0.0, 3.0]])
        frame_case(accel, (name, form, "scale and shear"), o, np.ascontiguousarray((rot.reshape(n, 3, 3) @ shear).reshape(n, 9)), b, W)
        odd = rot.copy()
        odd[1::5] = np.nan
        odd[3::5] = 0.0
        odd[4::10, 4] = np.nan  # one NaN entry
        frame_case(accel, (name, form, "NaN and zero frames"), o, odd, b, W)
    finally:
        reset(accel)


def test_an_identity_frame_is_not_null_frames_and_weights_follow_ieee():
    accel, poses, dirs = scan_setup("cornell_glass")
    n, m = 65, 130
    rows, cols = spread(NP, n), spread(NB, m)
    o, b = np.ascontiguousarray(poses[rows]), np.ascontiguousarray(dirs[cols])
    inf, nan = np.inf, np.nan
    special = np.array([[-0.0, 0.6, 0.8], [0.6, -0.0, 0.8], [0.6, 0.8, -0.0], [inf, 0.0, 1.0], [0.0, -inf, 1.0], [nan, 0.0, 1.0], [0.0, 1.0, nan], [-0.0, -0.0, -1.0]])
    at = np.arange(len(special)) * 9 + 2
    b[at] = special
    ident = np.ascontiguousarray(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    differs = (explicit_rays(o, None, b).view(np.uint64) != explicit_rays(o, ident, b).view(np.uint64)).any(axis=1).reshape(n, m)
    expect = np.zeros(m, dtype=bool)
    expect[at[:7]] = True  # (the last one is -0.0 in a product sum of -0.0s: the same bits through the identity)
    assert np.array_equal(differs, np.tile(expect, (n, 1))), "the rays differ exactly at the directions with a -0.0, infinite or NaN component"
    # weights: a zero column, +-inf and NaN entries, -0.0 -- on rows of their own, so that most sums stay finite
    W = WEIGHTS[cols].copy()
    W[:, 1] = 0.0
    W[5, 2], W[40, 3], W[77, 4], W[100, 5] = inf, -inf, nan, -0.0
    W[:, 6] = -0.0
    L_null = frame_case(accel, ("identity", "NULL frames"), o, None, b, W)
    L_id = frame_case(accel, ("identity", "identity frames"), o, ident, b, W)
    assert np.array_equal(bits(L_null[:, ~expect]), bits(L_id[:, ~expect]))
    want = seq_sums(L_null, W)
    # what the reference holds for these columns follows from IEEE alone (the comparison itself was frame_case's)
    finite = np.isfinite(L_null).all(axis=(1, 2))
    assert (want[finite][:, 1] == 0.0).all() and not np.signbit(want[finite][:, 1]).any(), "a zero column sums to +0.0 where the radiance is finite"
    assert np.isnan(want[~finite][:, 1]).all(), "... and to NaN where it is not: 0 * inf and 0 * NaN are not skipped"
    assert np.isnan(want[:, 4]).all() and not np.isfinite(want[:, 2]).any() and not np.isfinite(want[:, 3]).any(), "NaN and infinite weights reach the sum"


# ---- 5: planes and batching -------------------------------------------------------------------------------------------------------------
def test_planes_alone_together_and_twice():
    accel, poses, dirs = scan_setup("mesh_glass")
    n, m = 66, 130
    rows, cols = spread(NP, n), spread(NB, m)
    o, b, W = np.ascontiguousarray(poses[rows]), np.ascontiguousarray(dirs[cols]), np.ascontiguousarray(WEIGHTS[cols][:, :3])
    L = G.radiance(accel, explicit_rays(o, None, b)).reshape(n, m, 3)
    want = {"radiance": L, "sums": seq_sums(L, W)}
    rng = np.random.default_rng(5)
    for lanes in (DIR, POSE):
        for planes in (("radiance",), ("sums",), ("radiance", "sums"), ("sums", "radiance")):
            bufs = {p: rng.normal(size=want[p].shape) for p in la.GATHER_PLANES}
            keep = {p: bufs[p].copy() for p in la.GATHER_PLANES}
            for _ in range(2):  # the same call twice: the same bytes, nothing accumulated
                got = G.radiance_gather(accel, o, b, None, W, planes, lanes, into={p: bufs[p] for p in planes})
                for p in planes:
                    assert got[p] is bufs[p]
                    same((lanes, planes, p), got[p], want[p])
            assert all(np.array_equal(bufs[p], keep[p]) for p in la.GATHER_PLANES if p not in planes)
    got = accel.radiance_gather(o, b, weights=W)
    assert list(got) == ["sums"]
    same("the default plane", got["sums"], want["sums"])
    same("one column given as a vector", G.radiance_gather(accel, o, b, None, W[:, 0])["sums"], seq_sums(L, W[:, :1]))
    assert la.GATHER_PLANES == ("radiance", "sums")


CHILD = """import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import lasgun_amd as la
from test_gpu_visibility import SCENES
G = la.api
G.set_device(0)
z = np.load(%r)
a = G.Accel.from_scene(SCENES["cornell_glass"](G))
for lanes, n in ((1, 252), (2, 256)):
    np.save(%r %% lanes, G.radiance_gather(a, z["o"][:n], z["b"], z["m"][:n], z["w"], ("sums",), lanes)["sums"])
"""


def test_batches_of_a_parked_gather_give_the_one_batch_bytes():
    """A fresh process (both caps are read once): LASGUN_GATHER_PARK_MB=2 parks at most 84 poses x 1031 directions (direction lanes) or 64
    (pose lanes: whole blocks of 64), so 252 poses are three full batches and 256 poses four; LASGUN_WF_BUDGET_MB=64 cuts EVERY batch, the
    last included, into at least two chunks."""
    accel, poses, dirs = scan_setup("cornell_glass")
    frames = rotations(NP, 7)
    W = np.ascontiguousarray(WEIGHTS[:, :3])
    want = seq_sums(G.radiance(accel, explicit_rays(poses, frames, dirs)).reshape(NP, NB, 3), W)
    counts = {DIR: 252, POSE: 256}
    for lanes, n in counts.items():
        same(("one batch", lanes), G.radiance_gather(accel, poses[:n], dirs, frames[:n], W, ("sums",), lanes)["sums"], want[:n])
    with tempfile.TemporaryDirectory() as tmp:
        ip, op = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out%d.npy")
        np.savez(ip, o=poses, b=dirs, m=frames, w=W)
        env = dict(os.environ)
        env.update({"LASGUN_DEBUG": "1", "LASGUN_WF_BUDGET_MB": "64", "LASGUN_GATHER_PARK_MB": "2"})
        p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), ip, op)], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        lines = re.findall(r"radiance gather: levels \d+, (\d+) tiles in chunks of (\d+) \([^)]*\), batch (\d+) of (\d+), (direction|pose) lanes", p.stderr)
        for form, batches in (("direction", 3), ("pose", 4)):
            mine = [l for l in lines if l[4] == form]
            assert len(mine) == batches == int(mine[0][3]) and [int(l[2]) for l in mine] == list(range(1, batches + 1)), (form, mine)
            chunks = [(int(l[0]) + int(l[1]) - 1) // int(l[1]) for l in mine]
            assert all(c >= 2 for c in chunks), (form, mine)
        got = {lanes: np.load(op % lanes) for lanes in counts}
    for lanes, n in counts.items():
        same(("batched", lanes), got[lanes], want[:n])


# ---- 6: device form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel, poses, dirs = scan_setup(name)
    n, m, c = 129, NB, 9
    o = np.ascontiguousarray(poses[spread(NP, n)])
    dirs = dirs.copy()
    frames = rotations(n, 3)
    W = WEIGHTS.copy()
    set_form(accel, form)
    try:
        film = G.capture_radiance(accel, 64, 48).tobytes()
        for fr in (None, frames):
            host = G.radiance_gather(accel, o, dirs, fr, W, ("radiance", "sums"))
            L = G.radiance(accel, explicit_rays(o, fr, dirs)).reshape(n, m, 3)
            same(("host form", name), host["radiance"], L)
            same(("host form", name), host["sums"], seq_sums(L, W))
            do, db, dw = torch.from_numpy(o).cuda(), torch.from_numpy(dirs).cuda(), torch.from_numpy(W).cuda()
            dfr = torch.from_numpy(fr).cuda() if fr is not None else None
            stream = torch.cuda.Stream()
            for lanes in (DIR, POSE):
                fill = lambda k: torch.full((k,), 0x25A5A5A5A5A5A5A5, dtype=torch.int64, device="cuda")  # noqa: E731
                both = {"radiance": fill(n * m * 3), "sums": fill(n * c * 3)}
                only = {"radiance": fill(n * m * 3), "sums": fill(n * c * 3)}
                parked = {"radiance": fill(n * m * 3), "sums": fill(n * c * 3)}
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    s = torch.cuda.current_stream().cuda_stream
                    assert s != 0
                    args = (accel, n, do.data_ptr(), dfr.data_ptr() if dfr is not None else None, m, db.data_ptr())
                    for _ in range(2):  # the second call runs over the first one's results: written, not accumulated
                        G.radiance_gather_device(*args, dw.data_ptr(), c, both["radiance"].data_ptr(), both["sums"].data_ptr(), lanes=lanes, stream=s)
                    G.radiance_gather_device(*args, None, 0, radiance_ptr=only["radiance"].data_ptr(), lanes=lanes, stream=s)
                    G.radiance_gather_device(*args, dw.data_ptr(), c, sums_ptr=parked["sums"].data_ptr(), lanes=lanes, stream=s)
                stream.synchronize()
                cpu = lambda t: t.cpu().numpy().view(np.float64)  # noqa: E731
                for p in la.GATHER_PLANES:
                    same((name, lanes, p), cpu(both[p]).reshape(host[p].shape), host[p])
                same((name, lanes, "radiance alone"), cpu(only["radiance"]).reshape(host["radiance"].shape), host["radiance"])
                same((name, lanes, "sums alone"), cpu(parked["sums"]).reshape(host["sums"].shape), host["sums"])
                assert (only["sums"].cpu().numpy() == 0x25A5A5A5A5A5A5A5).all() and (parked["radiance"].cpu().numpy() == 0x25A5A5A5A5A5A5A5).all(), "not asked for"
            assert G.capture_radiance(accel, 64, 48).tobytes() == film, "a render after the gathers, on the same accel"
    finally:
        reset(accel)


# ---- 7: errors and empty sets -----------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_empty_sets_are_a_no_op():
    torch = pytest.importorskip("torch")
    accel, poses, dirs = scan_setup("cornell_glass")
    n, m, c = 70, 20, 3
    o, b, fr = np.ascontiguousarray(poses[:n + 1]), np.ascontiguousarray(dirs[:m + 1]), rotations(n + 1, 1)
    W = np.ascontiguousarray(WEIGHTS[:m + 1, :c])
    do, db, dfr, dw = (torch.from_numpy(x).cuda() for x in (o, b, fr, W))
    FILL = 0x5A5A5A5A5A5A5A5A
    dev = {"radiance": torch.full((n * m * 3,), FILL, dtype=torch.int64, device="cuda"), "sums": torch.full((n * c * 3,), FILL, dtype=torch.int64, device="cuda")}
    hst = {"radiance": np.full(n * m * 3, FILL, dtype=np.uint64), "sums": np.full(n * c * 3, FILL, dtype=np.uint64)}
    torch.cuda.synchronize()
    O, F, B, Wp = do.data_ptr(), dfr.data_ptr(), db.data_ptr(), dw.data_ptr()
    R, Z = dev["radiance"].data_ptr(), dev["sums"].data_ptr()

    def V(n_poses=n, origins=O, frames=F, n_dirs=m, dirs_=B, weights=Wp, n_weights=c, radiance=R, sums=Z, lanes=0, acc=accel):
        G.radiance_gather_device(acc, n_poses, origins, frames, n_dirs, dirs_, weights, n_weights, radiance, sums, lanes=lanes, stream=0)

    acc33 = G.Accel.from_scene(many_lights_scene(G, 33))
    deep = S.cornell_scene(G, "glass")
    deep.set_max_recursion_depth(20)
    acc20 = G.Accel.from_scene(deep)
    bad = [lambda: V(origins=o.ctypes.data), lambda: V(frames=fr.ctypes.data), lambda: V(dirs_=b.ctypes.data), lambda: V(weights=W.ctypes.data),  # host pointers
           lambda: V(radiance=hst["radiance"].ctypes.data), lambda: V(sums=hst["sums"].ctypes.data),
           lambda: V(origins=O + 4), lambda: V(frames=F + 4), lambda: V(dirs_=B + 4), lambda: V(weights=Wp + 4), lambda: V(radiance=R + 4), lambda: V(sums=Z + 4),  # misaligned
           lambda: V(radiance=None, sums=None),                               # both outputs NULL
           lambda: V(origins=None), lambda: V(dirs_=None),                    # NULL tables with non-zero counts
           lambda: V(weights=None), lambda: V(n_weights=0),                   # sums without weights
           lambda: V(lanes=3), lambda: V(lanes=-1),                           # a bad lanes
           lambda: V(n_dirs=1 << 32, lanes=DIR), lambda: V(n_dirs=1 << 32, lanes=POSE),                # n_dirs > 2^32 - 1
           lambda: V(n_poses=1 << 32, frames=None, n_dirs=64, lanes=DIR),                              # 2^32 tiles of one pose x 64 directions
           lambda: V(n_poses=(1 << 32) - 1, frames=None, n_dirs=65, lanes=DIR),
           lambda: V(n_poses=1 << 38, frames=None, n_dirs=1, lanes=POSE),                              # 2^32 tiles of 64 poses x one direction
           lambda: V(n_poses=1, frames=None, n_dirs=(1 << 32) - 1, lanes=DIR, n_weights=1 << 60),      # n_dirs * n_weights * 8
           lambda: V(n_poses=1 << 36, frames=None, n_dirs=1, lanes=POSE, n_weights=1 << 30),           # n_poses * n_weights * 24
           lambda: V(n_poses=1 << 24, frames=None, n_dirs=1, radiance=None),  # 384 MiB of origins: the buffer ends long before
           lambda: V(acc=acc33), lambda: V(acc=acc20)]                        # lg_radiance's two refusals
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
            raise AssertionError(("case %d of `bad` was not refused" % k))
        assert str(e.value), k
    with pytest.raises(la.LasgunError) as e:
        G.radiance_gather(acc33, o, b, None, W)
    assert "33 lights" in str(e.value)
    with pytest.raises(la.LasgunError) as e:
        G.radiance_gather(acc20, o, b, None, W)
    assert "recursion depth 20" in str(e.value)
    ho, hf, hb, hw = o.ctypes.data, fr.ctypes.data, b.ctypes.data, W.ctypes.data
    full = _capi.CGatherOut(hst["radiance"].ctypes.data, hst["sums"].ctypes.data)
    none = _capi.CGatherOut()
    A = ctypes.addressof
    host = [(accel.h, ho, hf, n, hb, m, hw, c, 0, A(none)),
            (accel.h, ho, hf, n, hb, m, hw, c, 0, None),
            (accel.h, None, hf, n, hb, m, hw, c, 0, A(full)),
            (accel.h, ho, hf, n, None, m, hw, c, 0, A(full)),
            (None, ho, hf, n, hb, m, hw, c, 0, A(full)),
            (accel.h, ho, hf, n, hb, m, None, c, 0, A(full)),
            (accel.h, ho, hf, n, hb, m, hw, 0, 0, A(full)),
            (accel.h, ho, hf, n, hb, m, hw, c, 3, A(full)),
            (accel.h, ho, hf, n, hb, m, hw, c, -7, A(full)),
            (accel.h, ho, hf, n, hb, 1 << 32, hw, c, 0, A(full)),
            (accel.h, ho, hf, 1 << 32, hb, 64, hw, c, DIR, A(full)),
            (accel.h, ho, hf, 1 << 38, hb, 1, hw, c, POSE, A(full)),
            (accel.h, ho, hf, 1 << 36, hb, 1 << 30, hw, c, 0, A(full)),
            (acc33.h, ho, hf, n, hb, m, hw, c, 0, A(full)),
            (acc20.h, ho, hf, n, hb, m, hw, c, 0, A(full))]
    for k, args in enumerate(host):
        assert G.call("radiance_gather", *args) != 0 and G.last_error(), k
    # empty sets: success, nothing written (whatever the pointers)
    for n_, m_ in ((0, m), (n, 0), (0, 0)):
        V(n_poses=n_, n_dirs=m_)
        assert G.call("radiance_gather", accel.h, ho, hf, n_, hb, m_, hw, c, 0, A(full)) == 0
    assert G.call("radiance_gather", None, None, None, 0, None, 0, None, 0, 9, None) == 0
    assert G.radiance_gather(accel, np.zeros((0, 3)), b, None, W)["sums"].shape == (0, c, 3)
    assert G.radiance_gather(accel, o, np.zeros((0, 3)), None, np.zeros((0, c)), ("radiance", "sums"))["radiance"].shape == (n + 1, 0, 3)
    torch.cuda.synchronize()
    assert all((dev[p].cpu().numpy() == FILL).all() for p in dev) and all((hst[p] == FILL).all() for p in hst)
    # weights are ignored where sums is not asked for; and the call still works afterwards
    V(weights=None, n_weights=0, sums=None)
    V()
    torch.cuda.synchronize()
    want = G.radiance_gather(accel, o[:n], b[:m], fr[:n], W[:m], ("radiance", "sums"))
    for p in dev:
        assert dev[p].cpu().numpy().view(np.uint64).tobytes() == want[p].tobytes(), p


# ---- level 0's shared bodies: two tiles, the last one partial, in every form, KIND and lane form (test_gpu_radiance_query.py, section 6) --
@pytest.mark.parametrize("name,builder,kind", L0_CASES, ids=L0_IDS)
def test_two_tiles_in_every_form_and_lane_form_equal_the_restatement(name, builder, kind):
    """2 poses x 65 directions and 65 poses x 2 directions: in direction lanes 2 x 2 tiles and 65 tiles of two rays, in pose lanes 65 tiles of
    two rays and 2 x 2 tiles -- against lg_radiance on the explicit rays (which section 6 there holds to the oracle) and the sequential sums."""
    accel = G.Accel.from_scene(l0_scene(builder, kind)(G))
    _, poses, dirs = scan_setup(name)
    checked = set()
    for n, m in ((2, 65), (65, 2)):
        o, b = np.ascontiguousarray(poses[spread(NP, n)]), np.ascontiguousarray(dirs[spread(NB, m)])
        rays = explicit_rays(o, None, b)
        mixed_rays(accel, rays, (name, kind, n, m))
        W = np.ascontiguousarray(WEIGHTS[spread(NB, m)])
        for form in each_form(accel):
            L = G.radiance(accel, rays).reshape(n, m, 3)
            check_gather((name, kind, form, n, m), accel, o, b, None, W, L, lanes_set=(DIR, POSE))
            checked.add(form)
    assert L0_FORMS[name] <= checked, (name, checked)
