"""Radiance queries (include/lasgun_hip.h: lg_radiance, lg_radiance_device): li() of caller-supplied rays through the render's
level-by-level pipeline.

  1  the render's own rays (lg_camera_rays) give the render's own radiance (lg_capture_radiance) and the oracle's, bit for bit;
  2  arbitrary rays pinned to the oracle by a SECOND CAMERA: scene B = scene A with another eye / look / up / fov (one orthographic, one
     inside the scene), lg_radiance(accel_A, camera rays of B) == the oracle's capture_radiance of B, bit for bit;
  3  arbitrary rays against the independent witness tests/pyref.py walking the reference's BVH (tests/pyref_bvh.py) (rtol 1e-12, atol 1e-15: what tests/test_pyref_witness.py grants pyref
     against the oracle -- its libm is not the portable trigonometry), non-finite rays included (NaN matches NaN);
  4  every form gives the same bytes: prune, LDS-resident scene, fast mode, sorted order, host / device form, many chunks, a permuted batch;
  5  sizes and errors; a render after a query and a query after a render on the same accel and stream.
Radiance is compared as bit patterns with every NaN canonicalised (tests/test_gpu_parity.py, bits)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import edge_rays as E
import pyref
import pyref_bvh

import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from query_witness import Witness
from test_gpu_ray_query import seeded_rays, world_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference accepts it and never reads it, camera.rs:142)
    pyref.Camera.set_aperture_radius = lambda self, radius: self


def bits(a):
    """Bit patterns with every NaN canonicalised (x86 and gfx950 disagree on the sign bit of a generated NaN): NaN positions must coincide."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def oracle_radiance(scene_of, w, h):
    """The oracle's f64 radiance of the film in portable-trig mode (the algorithms the device runs)."""
    o = oracle()
    oacc = o.Accel(scene_of(o))
    o.set_trig_mode(1)
    try:
        return o.capture_radiance(oacc, w, h, nthreads=8)
    finally:
        o.set_trig_mode(0)


def resolve(rad, samples):
    """A pixel from its samples' radiance as integrate() sums them (integrate.rs:16-20): in camera order from zero, times 1 / S."""
    r = rad.reshape(-1, samples, 3)
    color = np.zeros((r.shape[0], 3), dtype=np.float64)
    for s in range(samples):
        color = color + r[:, s, :]
    return color * (1.0 / float(samples))


# ---- 1: the render's own rays -----------------------------------------------------------------------------------------------------
OWN = [("kitchen_sink_perspective_ss1", lambda api: S.kitchen_sink_scene(api, camera="perspective", supersampling=0)),
       ("kitchen_sink_perspective_ss2", lambda api: S.kitchen_sink_scene(api, camera="perspective", supersampling=1)),
       ("kitchen_sink_orthographic_ss1", lambda api: S.kitchen_sink_scene(api, camera="orthographic", supersampling=0)),
       ("kitchen_sink_orthographic_ss2", lambda api: S.kitchen_sink_scene(api, camera="orthographic", supersampling=1)),
       ("cornell_glass", lambda api: S.cornell_scene(api, "glass")),
       ("mesh_glass", lambda api: S.mesh_scene(api, nu=48, nv=48, material="glass")),
       ("mirror", lambda api: S.simple_scene(api, 0, reflect=True))] + \
      [("random_%d" % s, (lambda s: lambda api: S.random_scene(api, s))(s)) for s in (1, 2, 3, 4)]


@pytest.mark.parametrize("name,builder", OWN, ids=[n for n, _ in OWN])
def test_the_renders_own_rays_give_the_renders_own_radiance(name, builder):
    w, h = 96, 64
    accel = G.Accel.from_scene(builder(G))
    samples = G.camera_samples(accel)
    if "_ss" in name:
        assert samples == {"1": 1, "2": 4}[name[-1]]
    rays = G.camera_rays(accel, w, h)
    assert rays.shape == (w * h * samples, 6)
    rad = G.radiance(accel, rays)
    assert rad.shape == (w * h * samples, 3) and rad.dtype == np.float64
    got = rad if samples == 1 else resolve(rad, samples)
    if samples == 4:  # the order the issue spells out
        r = rad.reshape(-1, 4, 3)
        assert np.array_equal(bits(((r[:, 0] + r[:, 1]) + r[:, 2] + r[:, 3]) * 0.25), bits(got))
    want = G.capture_radiance(accel, w, h).reshape(-1, 3)
    assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).any(axis=1).sum()))
    if samples == 1:
        assert np.array_equal(rad.view(np.int64), want.view(np.int64)), name  # the very bytes, signed zeros and NaN payloads included
    assert np.array_equal(bits(got), bits(oracle_radiance(builder, w, h).reshape(-1, 3))), name


# ---- 2: arbitrary rays pinned to the oracle by a second camera -----------------------------------------------------------------------
def with_camera(scene, cam, recursion=None):
    """The scene with its camera replaced (and its recursion, for the degenerate-view check): same aggregate, lights and background."""
    kind, par, eye, look, up = cam
    c = scene.set_orthographic_camera(par) if kind == "orthographic" else scene.set_perspective_camera(par)
    c.look_at(list(eye), list(look), list(up))
    if recursion is not None:
        scene.set_max_recursion_depth(recursion)
    return scene


# scene A, whether it shades glass / mirror (the recursion must then show in the view), and three B cameras: another perspective view, an
# orthographic one, and one INSIDE the scene's bounds, between its objects.  Chosen on the CPU with the oracle for the conditions asserted below.
SECOND = [
    ("kitchen_sink", lambda api: S.kitchen_sink_scene(api, supersampling=0), True, [
        ("perspective", 65.0, (-6.0, 3.0, 5.0), (0.5, -0.3, 0.0), (0.0, 1.0, 0.1)),
        ("orthographic", 5.5, (3.0, 3.0, 8.0), (0.0, -0.5, 0.5), (0.0, 1.0, 0.0)),
        ("perspective", 80.0, (0.9, -0.2, 0.9), (-2.2, -0.4, 0.5), (0.0, 1.0, 0.0))]),
    ("cornell_glass", lambda api: S.cornell_scene(api, "glass"), True, [
        ("perspective", 60.0, (2.0, 0.8, 6.0), (0.0, -0.5, 0.0), (0.0, 1.0, 0.0)),
        ("orthographic", 3.0, (0.5, 0.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        ("perspective", 95.0, (-0.3, 0.2, -1.5), (0.8, -1.0, 3.0), (0.0, 1.0, 0.0))]),
    ("mirror", lambda api: S.simple_scene(api, 0, reflect=True), True, [
        ("perspective", 50.0, (-500.0, 200.0, 600.0), (0.0, 0.0, -200.0), (0.0, 1.0, 0.0)),
        ("orthographic", 900.0, (300.0, 300.0, 800.0), (0.0, 0.0, -200.0), (0.0, 1.0, 0.0)),
        ("perspective", 90.0, (20.0, 30.0, -180.0), (200.0, 50.0, -100.0), (0.0, 1.0, 0.0))]),
    ("random_2", lambda api: S.random_scene(api, 2), False, [
        ("perspective", 60.0, (6.0, 2.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        ("orthographic", 9.0, (-3.0, 5.0, 8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        ("perspective", 85.0, (0.3, 0.2, 0.5), (2.0, 0.0, -2.0), (0.0, 1.0, 0.0))]),
]


@pytest.mark.parametrize("name,builder,specular,cameras", SECOND, ids=[s[0] for s in SECOND])
def test_a_second_cameras_rays_give_the_oracles_render_of_that_camera(name, builder, specular, cameras):
    w, h = 96, 64
    accel_a = G.Accel.from_scene(builder(G))
    assert len(cameras) >= 3 and any(c[0] == "orthographic" for c in cameras)
    for k, cam in enumerate(cameras):
        accel_b = G.Accel.from_scene(with_camera(builder(G), cam))
        rays_b = G.camera_rays(accel_b, w, h)
        assert not np.array_equal(rays_b, G.camera_rays(accel_a, w, h))
        want = oracle_radiance(lambda api: with_camera(builder(api), cam), w, h).reshape(-1, 3)
        # a degenerate view must not pass silently: hits, background, and (glass / mirror) pixels that the recursion changes
        hit = G.intersect(accel_a, rays_b)["kind"] != 0
        assert hit.mean() >= 0.20 and (~hit).mean() >= 0.05, (name, k, hit.mean())
        if specular:
            flat = oracle_radiance(lambda api: with_camera(builder(api), cam, recursion=0), w, h).reshape(-1, 3)
            assert (bits(flat) != bits(want)).any(axis=1).mean() >= 0.02, (name, k)
        got = G.radiance(accel_a, rays_b)
        assert np.array_equal(bits(got), bits(want)), (name, k, int((bits(got) != bits(want)).any(axis=1).sum()))


# ---- 3: arbitrary rays against the independent witness -------------------------------------------------------------------------------
WITNESS = [("kitchen_sink", lambda api: S.kitchen_sink_scene(api)), ("instanced", lambda api: S.instanced_scene(api)),
           ("exotic_obj", lambda api: S.exotic_obj_scene(api))]
RTOL, ATOL = 1e-12, 1e-15


def inside_sphere_rays(pscene, seed):
    """Rays that start inside the root's spheres (the glass ones among them: the first event is leaving the medium), eight each."""
    rng = np.random.default_rng(seed)
    out = []
    for c, r in world_points(pscene):
        if r == float("inf") or r > 10.0:
            continue
        for _ in range(8):
            out.append(np.concatenate([np.array(c) + rng.normal(0.0, 0.2 * r, 3), rng.normal(0.0, 1.0, 3)]))
    return np.array(out, dtype=np.float64).reshape(-1, 6)


def pyref_li(pscene, rays):
    with np.errstate(all="ignore"):
        return np.array([pyref.li(pscene, tuple(r[:3]), tuple(r[3:]), 0) for r in rays], dtype=np.float64).reshape(-1, 3)


def close(got, want):
    """NaN matches NaN; everything else within rtol / atol."""
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        near = np.abs(got - want) <= ATOL + RTOL * np.abs(want)
    return both_nan | (near & ~np.isnan(got) & ~np.isnan(want)) | (got == want)


@pytest.mark.parametrize("name,builder", WITNESS, ids=[n for n, _ in WITNESS])
def test_arbitrary_rays_match_the_witness(name, builder):
    gscene, pscene = builder(G), builder(pyref.Api)
    # li() through the reference's BVH, not pyref's brute-force loop over the primitives: which primitives a degenerate ray (a zero or
    # non-finite direction) is tested against at all is decided by the walk's slab tests, and the two differ on exactly those rays
    pyref_bvh.install(pscene)
    accel = G.Accel.from_scene(gscene)
    seeded = seeded_rays(pscene, 2000 + len(name))
    finite = np.concatenate([seeded[np.isfinite(seeded).all(axis=1)], inside_sphere_rays(pscene, 5)])
    hit = G.intersect(accel, finite)["kind"] != 0
    assert hit.sum() * 5 >= len(finite), (name, int(hit.sum()), len(finite))
    got, want = G.radiance(accel, finite), pyref_li(pscene, finite)
    ok = close(got, want).all(axis=1)
    assert ok.all(), (name, np.where(~ok)[0][:8], got[~ok][:4], want[~ok][:4])
    # non-finite rays: the call succeeds and says what the witness says
    lo, hi, boxes = E.scene_geometry(Witness(pscene), pscene)
    edge, _ = E.edge_rays(lo, hi, boxes=boxes, seed=len(name))
    odd = np.concatenate([edge[~np.isfinite(edge).all(axis=1)], seeded[-6:]])
    assert len(odd) >= 12
    got, want = G.radiance(accel, odd), pyref_li(pscene, odd)
    ok = close(got, want).all(axis=1)
    assert ok.all(), (name, odd[~ok][:4], got[~ok][:4], want[~ok][:4])


# ---- 4: every form gives the same bytes -----------------------------------------------------------------------------------------------
FORM_SCENES = [("cornell_glass", lambda api: S.cornell_scene(api, "glass")),
               ("mesh_glass", lambda api: S.mesh_scene(api, nu=48, nv=48, material="glass"))]
BATCH = (1 << 18) + 37


def batch(accel, seed):
    """The camera's rays of a 512 x 512 film, then random rays from around the camera."""
    rng = np.random.default_rng(seed)
    cam = G.camera_rays(accel, 512, 512)
    assert cam.shape[0] == 1 << 18
    extra = BATCH - cam.shape[0]
    o = cam[0, :3] + rng.normal(0.0, 0.5, (extra, 3))
    d = rng.normal(0.0, 1.0, (extra, 3))
    return np.concatenate([cam, np.concatenate([o, d], axis=1)])


def run_child(name, rays, budget_mb):
    """The query in a fresh process under LASGUN_WF_BUDGET_MB = budget_mb (None: the default): (radiance, chunks the library cut)."""
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.npy"), os.path.join(tmp, "out.npy")
        np.save(rp, rays)
        env = dict(os.environ)
        env["LASGUN_DEBUG"] = "1"
        env.pop("LASGUN_WF_BUDGET_MB", None)
        if budget_mb is not None:
            env["LASGUN_WF_BUDGET_MB"] = str(budget_mb)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "radiance_child.py"), name, rp, op], capture_output=True, text=True,
                           timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        m = re.findall(r"radiance query: levels \d+, (\d+) tiles in chunks of (\d+)", p.stderr)
        assert m, p.stderr[-3000:]
        tiles, per_chunk = int(m[-1][0]), int(m[-1][1])
        return np.load(op), (tiles + per_chunk - 1) // per_chunk


@pytest.mark.parametrize("name,builder", FORM_SCENES, ids=[n for n, _ in FORM_SCENES])
def test_every_form_gives_identical_bytes(name, builder):
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(builder(G))
    rays = batch(accel, 13)
    G.set_prune(accel, False)
    fits = G.set_lds_scene(accel, False)
    ref = G.radiance(accel, rays)
    ref_bytes = ref.tobytes()
    assert len(np.unique(ref[:, 0])) > 1000  # (a picture, not a constant)
    checked = []

    def check(form):
        assert G.radiance(accel, rays).tobytes() == ref_bytes, (name, form)
        checked.append(form)

    G.set_prune(accel, True); check("prune")
    if name == "cornell_glass":
        assert fits, "a scene of a few dozen triangles fits the LDS"
    if fits:
        G.set_prune(accel, False); G.set_lds_scene(accel, True); check("lds")
        G.set_prune(accel, True); check("lds+prune")
    G.set_prune(accel, None)
    try:
        G.set_mode(accel, True)
    except la.LasgunError:
        assert name != "mesh_glass", "the small torus scene admits the fast mode"
    else:
        check("fast")
        G.set_mode(accel, False)
    # the organisation is the level-by-level pipeline whatever the accel is told to render with
    for org in (0, 3, 1):
        G.set_streaming(accel, org)
        check("streaming %d" % org)
    # sorted order, on the reference walk and on the accel's defaults
    G.set_query_order(accel, 1)
    check("order 1")
    G.set_lds_scene(accel, False); check("order 1, tables in L2"); G.set_lds_scene(accel, True)
    # device form on a stream that is not the default one, both orders
    stream = torch.cuda.Stream()
    dr = torch.from_numpy(rays.copy()).cuda()
    for order in (1, 0):
        G.set_query_order(accel, order)
        do = torch.full((BATCH * 3,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            G.radiance_device(accel, BATCH, dr.data_ptr(), do.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        stream.synchronize()
        assert do.cpu().numpy().tobytes() == ref_bytes, (name, "device", order)
    # a permuted copy of the batch, un-permuted afterwards (every ray in another wave, beside other rays), both orders
    perm = np.random.default_rng(3).permutation(BATCH)
    for order in (0, 1):
        G.set_query_order(accel, order)
        out = np.empty_like(ref)
        out[perm] = G.radiance(accel, rays[perm])
        assert out.tobytes() == ref_bytes, (name, "permuted", order)
    # many chunks against one, each in a fresh process (the budget is read once)
    one, n_one = run_child(name, rays, None)
    many, n_many = run_child(name, rays, 64)
    assert n_one == 1 and n_many >= 8, (n_one, n_many)
    assert one.tobytes() == ref_bytes and many.tobytes() == ref_bytes, name
    assert {"prune", "order 1"} <= set(checked)


def test_sorted_order_in_many_chunks_gives_identical_bytes():
    """The chunks of a sorted query are cut from the sorted order: a shuffled batch, 64 MiB budget, in a child whose accel sorts."""
    name, builder = FORM_SCENES[0]
    accel = G.Accel.from_scene(builder(G))
    rays = batch(accel, 21)
    rays = rays[np.random.default_rng(4).permutation(BATCH)]
    ref = G.radiance(accel, rays)
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.npy"), os.path.join(tmp, "out.npy")
        np.save(rp, rays)
        code = ("import sys, numpy as np\nsys.path.insert(0, %r)\nsys.path.insert(0, %r)\nimport lasgun_amd as la\n"
                "from test_gpu_radiance_query import FORM_SCENES\nG = la.api\nG.set_device(0)\n"
                "a = G.Accel.from_scene(FORM_SCENES[0][1](G))\nG.set_query_order(a, 1)\nnp.save(%r, G.radiance(a, np.load(%r)))\n"
                % (ROOT, os.path.join(ROOT, "tests"), op, rp))
        env = dict(os.environ)
        env.update({"LASGUN_DEBUG": "1", "LASGUN_WF_BUDGET_MB": "64"})
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        m = re.findall(r"radiance query: levels \d+, (\d+) tiles in chunks of (\d+) \([^)]*\), sorted order", p.stderr)
        assert m and (int(m[-1][0]) + int(m[-1][1]) - 1) // int(m[-1][1]) >= 8, p.stderr[-3000:]
        assert np.load(op).tobytes() == ref.tobytes()


# ---- 5: sizes and errors -----------------------------------------------------------------------------------------------------------------
def test_sizes():
    accel = G.Accel.from_scene(S.kitchen_sink_scene(G, supersampling=0))
    rays = G.camera_rays(accel, 128, 64)
    ref = G.radiance(accel, rays)
    for order in (0, 1):
        G.set_query_order(accel, order)
        for n in (0, 1, 63, 64, 65, 4097):
            got = G.radiance(accel, rays[:n])
            assert got.shape == (n, 3) and got.tobytes() == ref[:n].tobytes(), (order, n)
    assert la.api.call("radiance", accel.h, None, 0, None) == 0  # n == 0: a no-op whatever the pointers


def many_lights_scene(api, nlights):
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 0.0, 6.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    for i in range(nlights):
        scene.add_point_light([-4.0 + 0.25 * i, 4.0, 3.0], [0.05, 0.05, 0.05], [1.0, 0.0, 0.0])
    scene.root.add_sphere([0.0, 0.0, 0.0], 1.0, api.Material.matte([0.8, 0.7, 0.6], 0.0))
    return scene


def test_errors_are_reported_and_nothing_is_launched():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    n = 100
    rays = G.camera_rays(accel, 16, 16)[: n + 1]
    dr = torch.from_numpy(rays.copy()).cuda()
    do = torch.full(((n + 1) * 3,), float("nan"), dtype=torch.float64, device="cuda")
    host_out = np.zeros((n, 3))
    torch.cuda.synchronize()
    bad = [lambda: G.radiance_device(accel, n, 0, do.data_ptr(), stream=0),
           lambda: G.radiance_device(accel, n, dr.data_ptr(), 0, stream=0),
           lambda: G.radiance_device(accel, n, dr.data_ptr() + 4, do.data_ptr(), stream=0),
           lambda: G.radiance_device(accel, n, dr.data_ptr(), do.data_ptr() + 4, stream=0),
           lambda: G.radiance_device(accel, n, rays.ctypes.data, do.data_ptr(), stream=0),      # host pointers
           lambda: G.radiance_device(accel, n, dr.data_ptr(), host_out.ctypes.data, stream=0)]
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    for args in ((accel.h, None, n, host_out.ctypes.data), (accel.h, rays.ctypes.data, n, None), (None, rays.ctypes.data, n, host_out.ctypes.data)):
        assert la.api.call("radiance", *args) != 0 and G.last_error()
    # the sorted order's indices are 32-bit: refused by count alone, before a buffer is looked at
    G.set_query_order(accel, 1)
    with pytest.raises(la.LasgunError) as e:
        G.radiance_device(accel, 1 << 32, dr.data_ptr(), do.data_ptr(), stream=0)
    assert "2^32" in str(e.value)
    G.set_query_order(accel, 0)
    torch.cuda.synchronize()
    assert np.isnan(do.cpu().numpy()).all()
    # 33 lights: the pipeline's visibility word holds 32 -- an error, not a wrong picture; 32 lights are served
    acc33 = G.Accel.from_scene(many_lights_scene(G, 33))
    with pytest.raises(la.LasgunError) as e:
        G.radiance(acc33, rays[:n])
    assert "33 lights" in str(e.value)
    with pytest.raises(la.LasgunError):
        G.radiance_device(acc33, n, dr.data_ptr(), do.data_ptr(), stream=0)
    torch.cuda.synchronize()
    assert np.isnan(do.cpu().numpy()).all()
    acc32 = G.Accel.from_scene(many_lights_scene(G, 32))
    r32 = G.camera_rays(acc32, 32, 32)
    assert np.array_equal(bits(G.radiance(acc32, r32)), bits(G.capture_radiance(acc32, 32, 32).reshape(-1, 3)))


def test_renders_and_queries_share_an_accel_and_its_stream():
    w, h = 160, 96
    builder = lambda api: S.kitchen_sink_scene(api, supersampling=0)  # noqa: E731
    want = oracle_radiance(builder, w, h).reshape(-1, 3)
    for streaming in (2, 1):
        accel = G.Accel.from_scene(builder(G))
        G.set_streaming(accel, streaming)  # (2: the render uses the very arrays the query uses)
        rays = G.camera_rays(accel, w, h)
        small = rays[: 64 * 7 + 5]
        a = G.radiance(accel, small)                                  # a query first (the context's arrays sized for it) ...
        r1 = G.capture_radiance(accel, w, h).reshape(-1, 3)           # ... a bigger render after it ...
        b = G.radiance(accel, rays)                                   # ... a query after the render ...
        r2 = G.capture_radiance(accel, w, h).reshape(-1, 3)           # ... and a render again
        for got in (r1, b, r2):
            assert np.array_equal(bits(got), bits(want)), streaming
        assert np.array_equal(bits(a), bits(want[: len(small)])), streaming


# ---- 6: two tiles, the last one partial, through every form, KIND and order of level 0's shared bodies -----------------------------------
# level0.h's three bodies serve five families, so a form that no test launches is a blind spot they share.  The cases below are the least
# that can go wrong in one: 65 rays (a full tile and a tile of one ray) and 130 (two and a tile of two), hits and misses among them,
# on a scene with no recursion at all (KIND 0: level 0 finishes every ray itself, the misses in the closest pass) and as it is (KIND 1: a
# level below), in every traversal form the scene admits, as given and in the sorted order -- bit for bit against the CPU oracle.
TWO_TILES = ((13, 5), (13, 10))
L0_CASES = [(name, builder, kind) for name, builder in FORM_SCENES for kind in (0, 1)]
L0_IDS = ["%s-KIND%d" % (name, kind) for name, _, kind in L0_CASES]
L0_FORMS = {"cornell_glass": {"reference", "prune", "lds", "lds+prune"}, "mesh_glass": {"reference", "prune", "fast"}}  # what each scene must admit


def l0_scene(builder, kind):
    """builder's scene with no recursion at all (KIND 0) or as it is (KIND 1)."""
    def scene_of(api):
        scene = builder(api)
        if kind == 0:
            scene.set_max_recursion_depth(0)
        return scene
    return scene_of


def each_form(accel):
    """Sets every traversal form the accel admits on it, one after the other, and yields its name; the accel's defaults afterwards."""
    fits = G.set_lds_scene(accel, False)
    for lds in (False, True) if fits else (False,):
        G.set_lds_scene(accel, lds)
        for prune in (False, True):
            G.set_prune(accel, prune)
            yield ("lds+prune" if prune else "lds") if lds else ("prune" if prune else "reference")
    G.set_prune(accel, None)
    G.set_lds_scene(accel, True)
    try:
        G.set_mode(accel, True)
    except la.LasgunError:
        return
    yield "fast"
    G.set_mode(accel, False)


def mixed_rays(accel, rays, ctx):
    """A case whose rays all hit, or all miss, would pass without running half of the closest pass."""
    hit = G.intersect(accel, rays)["kind"] != 0
    assert hit.any() and not hit.all(), ("the comparison would be vacuous: hits", int(hit.sum()), "of", len(hit), ctx)


@pytest.mark.parametrize("name,builder,kind", L0_CASES, ids=L0_IDS)
def test_two_tiles_in_every_form_and_order_give_the_oracles_radiance(name, builder, kind):
    scene_of = l0_scene(builder, kind)
    accel = G.Accel.from_scene(scene_of(G))
    assert G.camera_samples(accel) == 1
    checked = set()
    for w, h in TWO_TILES:
        rays = G.camera_rays(accel, w, h)
        mixed_rays(accel, rays, (name, kind, w, h))
        want = bits(oracle_radiance(scene_of, w, h).reshape(-1, 3))
        for form in each_form(accel):
            for order in (0, 1):
                G.set_query_order(accel, order)
                got = bits(G.radiance(accel, rays))
                assert np.array_equal(got, want), (name, kind, form, order, w * h, int((got != want).any(axis=1).sum()))
            G.set_query_order(accel, 0)
            checked.add(form)
    assert L0_FORMS[name] <= checked, (name, checked)
