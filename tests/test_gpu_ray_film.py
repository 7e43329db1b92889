"""Ray films (include/lasgun_hip.h: lg_capture_rays*, lg_lens_rays*): the caller's rays rendered into a film.

  1  the render's own rays (lg_camera_rays, samples = lg_camera_samples) give the render's own film and radiance, and the oracle's;
  2  a second camera's rays give the oracle's film of that camera (SECOND / with_camera of tests/test_gpu_radiance_query.py);
  3  the two outputs of one call agree: RGBA8 is the device's to_byte of the f64 output, which is resolve(lg_radiance(rays));
  4  offsets: tile order, a random order, a subset into prefilled buffers, slots behind the film, guard bytes;
  5  every form gives the same bytes, many chunks against one for a 9-sample film included;
  6  sizes and errors, renders and film queries on one accel and stream;
  7  lens rays against their formulas in numpy float64, and a lens film end to end.
Radiance is compared as bit patterns with every NaN canonicalised (bits); the oracle is taken in portable-trig mode."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_radiance_query import FORM_SCENES, L0_CASES, L0_FORMS, L0_IDS, SECOND, TWO_TILES, bits, each_form, l0_scene, many_lights_scene, mixed_rays, oracle_radiance, resolve, with_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
W, H = 96, 64


def oracle_film(scene_of, w, h):
    """The oracle's RGBA8 film in portable-trig mode (the algorithms the device runs)."""
    o = oracle()
    oacc = o.Accel(scene_of(o))
    film = o.Film(w, h)
    o.set_trig_mode(1)
    try:
        o.capture_subset_mt(0, 1, oacc, film, 8)
    finally:
        o.set_trig_mode(0)
    return film.pixels()


def to_byte(rgb):
    """The device's own to_byte (lg_math_eval op 8) of an f64 array, as uint8."""
    return G.math_eval(8, np.ascontiguousarray(rgb, dtype=np.float64).ravel()).astype(np.uint8).reshape(np.shape(rgb))


def regroup(rays, samples, order):
    """The rays of the pixel slots `order` names, slot-major."""
    return np.ascontiguousarray(rays.reshape(-1, samples, 6)[order].reshape(-1, 6))


# ---- 1: the render's own rays ---------------------------------------------------------------------------------------------------------
OWN = [("kitchen_sink_%s_ss%d" % (cam, ss), (lambda cam, ss: lambda api: S.kitchen_sink_scene(api, camera=cam, supersampling=ss))(cam, ss), (ss + 1) ** 2 if ss else 1)
       for cam in ("perspective", "orthographic") for ss in (0, 1, 2)] + \
      [("cornell_glass", lambda api: S.cornell_scene(api, "glass"), 1),
       ("mesh_glass", lambda api: S.mesh_scene(api, nu=48, nv=48, material="glass"), 1),
       ("mirror", lambda api: S.simple_scene(api, 0, reflect=True), 1)]


def own_rays_check(name, builder, samples, w, h):
    accel = G.Accel.from_scene(builder(G))
    assert G.camera_samples(accel) == samples, name
    rays = G.camera_rays(accel, w, h)
    assert rays.shape == (w * h * samples, 6)
    rgba, rgb = G.capture_rays(accel, rays, w, h, samples=samples, rgb=True)
    film = G.Film.new(w, h)
    G.capture_subset(0, 1, accel, film)
    assert np.array_equal(rgba, film.pixels()), (name, "lg_capture")
    assert np.array_equal(rgba, G.render(builder(G), (w, h)).pixels()), (name, "render")
    assert np.array_equal(rgba, oracle_film(builder, w, h)), (name, "oracle film")
    assert np.array_equal(bits(rgb), bits(G.capture_radiance(accel, w, h))), (name, "lg_capture_radiance")
    assert np.array_equal(bits(rgb), bits(oracle_radiance(builder, w, h))), (name, "oracle radiance")


@pytest.mark.parametrize("name,builder,samples", OWN, ids=[n for n, _, _ in OWN])
def test_the_renders_own_rays_give_the_renders_own_film(name, builder, samples):
    own_rays_check(name, builder, samples, W, H)


def test_the_renders_own_rays_at_an_odd_size_with_nine_samples():
    """50 x 38 at 9 samples: 17,100 rays, not a multiple of 64, and 9 does not divide 64."""
    own_rays_check("kitchen_sink_50x38_ss3", lambda api: S.kitchen_sink_scene(api, supersampling=2), 9, 50, 38)


# ---- 2: a second camera ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,specular,cameras", SECOND, ids=[s[0] for s in SECOND])
def test_a_second_cameras_rays_give_the_oracles_film_of_that_camera(name, builder, specular, cameras):
    accel_a = G.Accel.from_scene(builder(G))
    assert len(cameras) >= 3
    for k, cam in enumerate(cameras):
        accel_b = G.Accel.from_scene(with_camera(builder(G), cam))
        rays_b = G.camera_rays(accel_b, W, H)
        hit = G.intersect(accel_a, rays_b)["kind"] != 0
        assert hit.mean() >= 0.20 and (~hit).mean() >= 0.05, (name, k, hit.mean())
        got = G.capture_rays(accel_a, rays_b, W, H)
        want = oracle_film(lambda api: with_camera(builder(api), cam), W, H)
        assert np.array_equal(got, want), (name, k, int((got != want).any(axis=2).sum()))


# ---- 3: the two outputs agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", (0, 2))
def test_the_two_outputs_agree(ss):
    samples = (ss + 1) ** 2 if ss else 1
    accel = G.Accel.from_scene(S.kitchen_sink_scene(G, supersampling=ss))
    rays = G.camera_rays(accel, W, H)
    rgba, rgb = G.capture_rays(accel, rays, W, H, samples=samples, rgb=True)
    assert np.array_equal(rgba[..., :3], to_byte(rgb))
    assert (rgba[..., 3] == 255).all()
    assert np.array_equal(bits(rgb.reshape(-1, 3)), bits(resolve(G.radiance(accel, rays), samples)))
    # each output alone is the same bytes
    assert np.array_equal(G.capture_rays(accel, rays, W, H, samples=samples), rgba)
    assert np.array_equal(bits(G.capture_rays(accel, rays, W, H, samples=samples, rgba=False, rgb=True)), bits(rgb))


# ---- 4: offsets ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", (0, 1))
def test_offsets(ss):
    torch = pytest.importorskip("torch")
    samples = (ss + 1) ** 2 if ss else 1
    accel = G.Accel.from_scene(S.kitchen_sink_scene(G, supersampling=ss))
    rays = G.camera_rays(accel, W, H)
    ref_a, ref_d = G.capture_rays(accel, rays, W, H, samples=samples, rgb=True)
    tiles = la.tile_order_offsets(W, H)
    assert tiles.dtype == np.uint64 and np.array_equal(np.sort(tiles), np.arange(W * H, dtype=np.uint64))
    assert tiles[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, W] and tiles[64] == 8
    shuffled = np.random.default_rng(11).permutation(W * H).astype(np.uint64)
    for order in (tiles, shuffled):
        a, d = G.capture_rays(accel, regroup(rays, samples, order), W, H, samples=samples, offsets=order, rgb=True)
        assert np.array_equal(a, ref_a) and np.array_equal(bits(d), bits(ref_d))
    # a subset (every 7th slot of the tile order, and three slots behind the film) into prefilled buffers: host form ...
    sub = tiles[::7].copy()
    behind = np.array([W * H, W * H + 5, 2 ** 63], dtype=np.uint64)
    offs = np.concatenate([sub[:10], behind[:1], sub[10:], behind[1:]])
    srays = np.zeros((len(offs) * samples, 6))
    inside = offs < W * H
    srays.reshape(-1, samples, 6)[inside] = rays.reshape(-1, samples, 6)[offs[inside]]
    srays.reshape(-1, samples, 6)[~inside] = rays.reshape(-1, samples, 6)[:3]  # (real rays: were they written, it would show)
    named = np.zeros(W * H, dtype=bool)
    named[sub] = True
    film = np.full((H, W, 4), 0xA5, dtype=np.uint8)
    rgb = np.frombuffer(bytes([0xA5]) * (W * H * 24), dtype=np.float64).reshape(H, W, 3).copy()
    G.capture_rays(accel, srays, W, H, samples=samples, offsets=offs, into=(film, rgb))

    def check(film, rgb, what):
        f, r = film.reshape(-1, 4), rgb.reshape(-1, 3)
        assert np.array_equal(f[named], ref_a.reshape(-1, 4)[named]), what
        assert (f[~named] == 0xA5).all(), what
        assert np.array_equal(bits(r[named]), bits(ref_d.reshape(-1, 3)[named])), what
        assert (r[~named].view(np.uint8) == 0xA5).all(), what

    check(film, rgb, "host")
    # ... and the device form, with 64 guard bytes behind each output
    dr = torch.from_numpy(srays).cuda()
    do = torch.from_numpy(offs.view(np.int64)).cuda()
    da = torch.full((W * H * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dd = torch.full((W * H * 24 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    G.capture_rays_device(accel, len(offs), dr.data_ptr(), W, H, samples=samples, offsets_ptr=do.data_ptr(), rgba_ptr=da.data_ptr(), rgb_ptr=dd.data_ptr(), stream=0)
    torch.cuda.synchronize()
    ha, hd = da.cpu().numpy(), dd.cpu().numpy()
    assert (ha[-64:] == 0xA5).all() and (hd[-64:] == 0xA5).all()
    check(ha[:-64].reshape(H, W, 4), hd[:-64].view(np.float64).reshape(H, W, 3), "device")
    # without offsets, slots behind the film write nothing either: w*h + 3 slots into a w x h film
    more = np.concatenate([rays, rays[:3 * samples]])
    da.fill_(0xA5)
    dr2 = torch.from_numpy(more).cuda()
    torch.cuda.synchronize()
    G.capture_rays_device(accel, W * H + 3, dr2.data_ptr(), W, H, samples=samples, rgba_ptr=da.data_ptr(), stream=0)
    torch.cuda.synchronize()
    ha = da.cpu().numpy()
    assert (ha[-64:] == 0xA5).all() and np.array_equal(ha[:-64].reshape(H, W, 4), ref_a)
    assert np.array_equal(G.capture_rays(accel, more, W, H, samples=samples), ref_a)


# ---- 5: every form gives the same bytes ---------------------------------------------------------------------------------------------------------
def nine_sample_rays(builder, w, h):
    """The rays of the scene's camera at supersampling 2 (9 samples per pixel, camera order)."""
    scene = builder(G)
    scene.camera.set_supersampling(2)
    accel9 = G.Accel.from_scene(scene)
    assert G.camera_samples(accel9) == 9
    return accel9, G.camera_rays(accel9, w, h)


def run_child(name, rays, samples, w, h, order, budget_mb):
    """The film in a fresh process under LASGUN_WF_BUDGET_MB = budget_mb (None: the default): (rgba, rgb, chunks the library cut, sorted?)."""
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.npy"), os.path.join(tmp, "out.npz")
        np.save(rp, rays)
        env = dict(os.environ)
        env["LASGUN_DEBUG"] = "1"
        env.pop("LASGUN_WF_BUDGET_MB", None)
        if budget_mb is not None:
            env["LASGUN_WF_BUDGET_MB"] = str(budget_mb)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ray_film_child.py"), name, rp, str(samples), str(w), str(h), str(order), op],
                           capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        m = re.findall(r"ray film: levels \d+, (\d+) tiles in chunks of (\d+) \([^)]*\), (sorted order|as given)", p.stderr)
        assert m, p.stderr[-3000:]
        tiles, per_chunk = int(m[-1][0]), int(m[-1][1])
        out = np.load(op)
        return out["rgba"], out["rgb"], (tiles + per_chunk - 1) // per_chunk, m[-1][2] == "sorted order"


@pytest.mark.parametrize("name,builder", FORM_SCENES, ids=[n for n, _ in FORM_SCENES])
def test_every_form_gives_identical_bytes(name, builder):
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(builder(G))
    accel9, rays9 = nine_sample_rays(builder, 128, 128)
    batches = [(G.camera_rays(accel, 512, 512), 1, 512, 512), (rays9, 9, 128, 128)]
    G.set_prune(accel, False)
    fits = G.set_lds_scene(accel, False)
    refs = [G.capture_rays(accel, r, w, h, samples=s, rgb=True) for r, s, w, h in batches]
    assert len(np.unique(refs[0][1][..., 0])) > 1000  # (a picture, not a constant)
    assert np.array_equal(bits(refs[1][1]), bits(G.capture_radiance(accel9, 128, 128)))
    checked = []

    def check(form):
        for (r, s, w, h), (ref_a, ref_d) in zip(batches, refs):
            a, d = G.capture_rays(accel, r, w, h, samples=s, rgb=True)
            assert a.tobytes() == ref_a.tobytes() and d.tobytes() == ref_d.tobytes(), (name, form, s)
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
    for org in (0, 3, 1):
        G.set_streaming(accel, org)
        check("streaming %d" % org)
    G.set_query_order(accel, 1)
    check("order 1")
    # host form against the device form on a stream that is not the default one, both orders
    stream = torch.cuda.Stream()
    for (r, s, w, h), (ref_a, ref_d) in zip(batches, refs):
        dr = torch.from_numpy(r).cuda()
        for order in (1, 0):
            G.set_query_order(accel, order)
            da = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
            dd = torch.full((w * h * 3,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                G.capture_rays_device(accel, w * h, dr.data_ptr(), w, h, samples=s, rgba_ptr=da.data_ptr(), rgb_ptr=dd.data_ptr(),
                                      stream=torch.cuda.current_stream().cuda_stream)
            stream.synchronize()
            assert da.cpu().numpy().tobytes() == ref_a.tobytes() and dd.cpu().numpy().tobytes() == ref_d.tobytes(), (name, "device", s, order)
    assert {"prune", "order 1"} <= set(checked)


@pytest.mark.parametrize("name,builder", FORM_SCENES, ids=[n for n, _ in FORM_SCENES])
def test_a_nine_sample_film_in_many_chunks_gives_identical_bytes(name, builder):
    """Chunks are 64-ray tiles and 9 does not divide 64: a pixel's samples straddle chunk boundaries, and the sorted order scatters them.
    The film is 160 x 128 -- at four recursion levels a 64 MiB budget holds 337 tiles, so a 128 x 128 film of 9 samples (2,304 tiles) is 7
    chunks, one short of the 8 asked for; 160 x 128 (2,880 tiles) is 9."""
    w, h = 160, 128
    accel = G.Accel.from_scene(builder(G))
    _, rays9 = nine_sample_rays(builder, w, h)
    ref_a, ref_d = G.capture_rays(accel, rays9, w, h, samples=9, rgb=True)
    one = run_child(name, rays9, 9, w, h, 0, None)
    assert one[2] == 1 and not one[3]
    assert one[0].tobytes() == ref_a.tobytes() and one[1].tobytes() == ref_d.tobytes()
    for order in (0, 1):
        a, d, chunks, was_sorted = run_child(name, rays9, 9, w, h, order, 64)
        assert chunks >= 8 and was_sorted == bool(order), (order, chunks, was_sorted)
        assert a.tobytes() == ref_a.tobytes() and d.tobytes() == ref_d.tobytes(), (name, order)


# ---- 6: sizes and errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", (0, 1, 2))
def test_sizes(ss):
    samples = (ss + 1) ** 2 if ss else 1
    accel = G.Accel.from_scene(S.kitchen_sink_scene(G, supersampling=ss))
    w, h = 128, 64
    rays = G.camera_rays(accel, w, h)
    ref_a, ref_d = G.capture_rays(accel, rays, w, h, samples=samples, rgb=True)
    for order in (0, 1):
        G.set_query_order(accel, order)
        for n in (0, 1, 7, 63, 64, 65, 4097):
            film = np.full((h, w, 4), 0xA5, dtype=np.uint8)
            rgb = np.full((h, w, 3), -7.0)
            G.capture_rays(accel, rays[: n * samples], w, h, samples=samples, into=(film, rgb))
            assert film.reshape(-1, 4)[:n].tobytes() == ref_a.reshape(-1, 4)[:n].tobytes(), (order, n)
            assert rgb.reshape(-1, 3)[:n].tobytes() == ref_d.reshape(-1, 3)[:n].tobytes(), (order, n)
            assert (film.reshape(-1, 4)[n:] == 0xA5).all() and (rgb.reshape(-1, 3)[n:] == -7.0).all(), (order, n)
    assert la.api.call("capture_rays", accel.h, None, 0, samples, None, None, None, w, h) == 0  # pixels == 0: a no-op whatever the pointers
    assert la.api.call("capture_rays_device", accel.h, None, 0, samples, None, w, h, None, None, None) == 0


def test_errors_are_reported_and_nothing_is_launched():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    w, h, n = 16, 16, 100
    rays = G.camera_rays(accel, w, h)
    dr = torch.from_numpy(rays.copy()).cuda()
    do = torch.arange(w * h, dtype=torch.int64, device="cuda")
    da = torch.full((w * h * 4 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    dd = torch.full((w * h * 3 + 1,), float("nan"), dtype=torch.float64, device="cuda")
    host_a, host_d = np.full((h, w, 4), 0xA5, dtype=np.uint8), np.full((h, w, 3), np.nan)
    host_off = np.arange(n, dtype=np.uint64)
    torch.cuda.synchronize()

    def dev(rays_ptr=dr.data_ptr(), pixels=n, samples=1, off=None, a=da.data_ptr(), d=dd.data_ptr(), acc=accel):
        return lambda: G.capture_rays_device(acc, pixels, rays_ptr, w, h, samples=samples, offsets_ptr=off, rgba_ptr=a, rgb_ptr=d, stream=0)

    bad = [dev(rays_ptr=None),                                       # NULL rays
           dev(a=None, d=None),                                      # both outputs NULL
           dev(rays_ptr=dr.data_ptr() + 4), dev(off=do.data_ptr() + 4), dev(d=dd.data_ptr() + 4), dev(a=da.data_ptr() + 2),  # misaligned
           dev(rays_ptr=rays.ctypes.data), dev(off=host_off.ctypes.data), dev(a=host_a.ctypes.data), dev(d=host_d.ctypes.data),  # host pointers
           dev(samples=0),
           dev(pixels=1 << 62, samples=4), dev(pixels=(1 << 38) + 1)]  # an overflowing count
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    film = G.Film.new_with_output(w, h, host_a)
    small = G.Film.new(w, h - 1)
    for args in ((None, rays.ctypes.data, n, 1, None, film.h, host_d.ctypes.data, w, h),
                 (accel.h, None, n, 1, None, film.h, host_d.ctypes.data, w, h),
                 (accel.h, rays.ctypes.data, n, 1, None, None, None, w, h),
                 (accel.h, rays.ctypes.data, n, 0, None, film.h, host_d.ctypes.data, w, h),
                 (accel.h, rays.ctypes.data, 1 << 62, 4, None, film.h, host_d.ctypes.data, w, h),
                 (accel.h, rays.ctypes.data, n, 1, None, small.h, host_d.ctypes.data, w, h)):   # a film of another size
        assert la.api.call("capture_rays", *args) != 0 and G.last_error(), args[2:4]
    # 33 lights: the pipeline's visibility word holds 32 -- an error, not a wrong picture; 32 lights are served
    acc33 = G.Accel.from_scene(many_lights_scene(G, 33))
    with pytest.raises(la.LasgunError) as e:
        G.capture_rays(acc33, rays[:n], w, h, into=(host_a, host_d))
    assert "33 lights" in str(e.value)
    with pytest.raises(la.LasgunError):
        dev(acc=acc33)()
    torch.cuda.synchronize()
    assert (da.cpu().numpy() == 0xA5).all() and np.isnan(dd.cpu().numpy()).all()
    assert (host_a == 0xA5).all() and np.isnan(host_d).all()
    acc32 = G.Accel.from_scene(many_lights_scene(G, 32))
    r32 = G.camera_rays(acc32, 32, 32)
    a32, d32 = G.capture_rays(acc32, r32, 32, 32, rgb=True)
    f32 = G.Film.new(32, 32)
    G.capture_subset(0, 1, acc32, f32)
    assert np.array_equal(a32, f32.pixels()) and np.array_equal(bits(d32), bits(G.capture_radiance(acc32, 32, 32)))


def test_renders_and_film_queries_share_an_accel_and_its_stream():
    w, h = 160, 96
    builder = lambda api: S.kitchen_sink_scene(api, supersampling=0)  # noqa: E731
    want_d, want_a = oracle_radiance(builder, w, h), oracle_film(builder, w, h)
    for streaming in (2, 1):
        accel = G.Accel.from_scene(builder(G))
        G.set_streaming(accel, streaming)
        rays = G.camera_rays(accel, w, h)
        a0 = G.capture_rays(accel, rays[: 64 * 7 + 5], w, h)     # a film query first (the context's arrays sized for it) ...
        r1 = G.capture_radiance(accel, w, h)                      # ... a bigger render after it ...
        a1, d1 = G.capture_rays(accel, rays, w, h, rgb=True)      # ... a film query after the render ...
        r2 = G.capture_radiance(accel, w, h)                      # ... and a render again
        film = G.Film.new(w, h)
        G.capture_subset(0, 1, accel, film)
        for got in (r1, d1, r2):
            assert np.array_equal(bits(got), bits(want_d)), streaming
        assert np.array_equal(a1, want_a) and np.array_equal(film.pixels(), want_a), streaming
        assert np.array_equal(a0.reshape(-1, 4)[: 64 * 7 + 5], want_a.reshape(-1, 4)[: 64 * 7 + 5]), streaming


# ---- 7: lens rays --------------------------------------------------------------------------------------------------------------------------------
def rotated_basis():
    """An orthonormal basis that is no axis permutation: rotations about z, x and y composed."""
    def rot(axis, t):
        c, s = np.cos(t), np.sin(t)
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    m = rot(1, 0.7) @ rot(0, -0.4) @ rot(2, 1.1)
    return m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()  # right, up, forward


ORIGIN = (0.3, -1.25, 2.5)
FOV = 170.0


def lens_of(kind):
    right, up, forward = rotated_basis()
    return la.Lens(kind, ORIGIN, right, up, forward, FOV)


def lens_formula(kind, w, h, root, offsets=None):
    """The issue's formulas in numpy float64: (slots * root^2, 6)."""
    right, up, forward = rotated_basis()
    off = np.arange(w * h, dtype=np.uint64) if offsets is None else np.asarray(offsets, dtype=np.uint64)
    ok = off < w * h
    o = np.where(ok, off, 0).astype(np.int64)
    x, y = (o % w).astype(np.float64), (o // w).astype(np.float64)
    i, j = np.divmod(np.arange(root * root), root)
    u = (x[:, None] + (j[None, :] + 0.5) / root) / w
    v = (y[:, None] + (i[None, :] + 0.5) / root) / h
    if kind == 0:
        phi, theta = (u - 0.5) * (2.0 * np.pi), (0.5 - v) * np.pi
        cr, cu, cf = np.cos(theta) * np.sin(phi), np.sin(theta), np.cos(theta) * np.cos(phi)
    else:
        m = min(w, h)
        a, b = (2.0 * u - 1.0) * w / m, (1.0 - 2.0 * v) * h / m
        r, psi = np.sqrt(a * a + b * b), np.arctan2(b, a)
        theta = r * np.radians(FOV) / 2.0
        cr, cu, cf = np.sin(theta) * np.cos(psi), np.sin(theta) * np.sin(psi), np.cos(theta)
    d = cr[..., None] * right + cu[..., None] * up + cf[..., None] * forward
    rays = np.concatenate([np.broadcast_to(np.array(ORIGIN), d.shape), d], axis=2)
    rays[~ok] = 0.0
    return rays.reshape(-1, 6)


def angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b))


@pytest.mark.parametrize("kind", (0, 1), ids=("equirectangular", "fisheye"))
@pytest.mark.parametrize("w,h", ((64, 32), (33, 47)))
@pytest.mark.parametrize("root", (1, 3))
def test_lens_rays_match_their_formulas(kind, w, h, root):
    torch = pytest.importorskip("torch")
    lens = lens_of(kind)
    rays = G.lens_rays(lens, w, h, root)
    want = lens_formula(kind, w, h, root)
    assert rays.shape == want.shape == (w * h * root * root, 6)
    assert np.array_equal(rays[:, :3], want[:, :3])  # origins are exact
    assert np.abs(rays[:, 3:] - want[:, 3:]).max() <= 1e-14
    if root == 3:  # sample order is idx = i*root + j (the formula's, compared above); j and i are not interchangeable: samples 1 and 3 differ
        px = want.reshape(w * h, 9, 6)[w + 1, :, 3:]
        assert np.abs(px[1] - px[3]).max() > 1e-4
    # with offsets: slot g is pixel offsets[g]; slots behind the film are all zero
    offs = np.concatenate([np.random.default_rng(kind + w).permutation(w * h)[: 200], [w * h, w * h + 9, 2 ** 40]]).astype(np.uint64)
    sub = G.lens_rays(lens, w, h, root, offsets=offs)
    S2 = root * root
    full = rays.reshape(w * h, S2, 6)
    assert sub.shape == (len(offs) * S2, 6)
    assert np.array_equal(sub.reshape(len(offs), S2, 6)[:200], full[offs[:200]])
    assert (sub.reshape(len(offs), S2, 6)[200:] == 0.0).all()
    # host and device forms: identical bytes
    for o in (None, offs):
        slots = w * h if o is None else len(o)
        dr = torch.full((slots * S2 * 6,), float("nan"), dtype=torch.float64, device="cuda")
        do = torch.from_numpy(o.view(np.int64)).cuda() if o is not None else None
        torch.cuda.synchronize()
        G.lens_rays_device(torch.cuda.current_device(), lens, w, h, root, slots, dr.data_ptr(), offsets_ptr=do.data_ptr() if do is not None else None, stream=0)
        torch.cuda.synchronize()
        assert dr.cpu().numpy().tobytes() == (rays if o is None else sub).tobytes()


def test_lens_rays_look_where_they_should():
    right, up, forward = rotated_basis()
    w, h = 33, 47  # odd: pixel (16, 23) holds the film's centre at its own centre
    pano = G.lens_rays(lens_of(0), w, h, 1).reshape(h, w, 6)[..., 3:]
    assert np.abs(pano[23, 16] - forward).max() <= 1e-12
    # the left and right edges meet at -forward: the middle row's outermost samples sit phi = +-(pi - pi/w) from forward, mirror images about it
    seam = pano[23, 0] + pano[23, w - 1]
    assert np.abs(seam / np.linalg.norm(seam) + forward).max() <= 1e-12
    assert abs(angle(pano[23, 0], -forward) - np.pi / w) <= 1e-12 and abs(angle(pano[23, w - 1], -forward) - np.pi / w) <= 1e-12
    assert abs(np.dot(pano[23, 0], right) + np.dot(pano[23, w - 1], right)) <= 1e-12
    fish = G.lens_rays(lens_of(1), w, h, 1).reshape(h, w, 6)[..., 3:]
    assert np.abs(fish[23, 16] - forward).max() <= 1e-12
    # the inscribed circle (the shorter side, w) has its rim at u = 0 and u = 1: theta is linear in the distance from the centre, so the
    # middle row's outermost pixel centre is (1 - 1/w) * fov/2 from forward, and half a pixel further out lies the rim at fov/2
    half = np.radians(FOV) / 2.0
    for x in (0, w - 1):
        assert abs(angle(fish[23, x], forward) - (1.0 - 1.0 / w) * half) <= 1e-12
        step = angle(fish[23, x], forward) - angle(fish[23, x + (1 if x == 0 else -1)], forward)
        assert abs(angle(fish[23, x], forward) + step / 2.0 - half) <= 1e-12


def test_a_lens_film_end_to_end():
    pytest.importorskip("torch")
    w, h, root = 64, 32, 3
    accel = G.Accel.from_scene(S.kitchen_sink_scene(G, supersampling=0))
    lens = la.Lens(la.LENS_EQUIRECTANGULAR, (0.9, -0.2, 0.9), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))  # between the scene's objects
    rays = G.lens_rays(lens, w, h, root)
    hit = G.intersect(accel, rays)["kind"] != 0
    assert hit.mean() >= 0.20 and (~hit).mean() >= 0.05, hit.mean()
    want = to_byte(resolve(G.radiance(accel, rays), root * root)).reshape(h, w, 3)
    got = G.capture_rays(accel, rays, w, h, samples=root * root)
    assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all()
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 50  # (a picture, not a constant)
    for tile_order in (True, False):
        assert np.array_equal(G.capture_lens(accel, lens, w, h, samples_root=root, tile_order=tile_order), got), tile_order
    fish = la.Lens(la.LENS_FISHEYE, (0.9, -0.2, 0.9), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 160.0)
    frays = G.lens_rays(fish, w, h, 1)
    assert np.array_equal(G.capture_lens(accel, fish, w, h), G.capture_rays(accel, frays, w, h))


# ---- level 0's shared bodies: two tiles, the last one partial, in every form, KIND and order (test_gpu_radiance_query.py, section 6) -----
@pytest.mark.parametrize("name,builder,kind", L0_CASES, ids=L0_IDS)
def test_two_tiles_in_every_form_and_order_give_the_oracles_film(name, builder, kind):
    scene_of = l0_scene(builder, kind)
    accel = G.Accel.from_scene(scene_of(G))
    assert G.camera_samples(accel) == 1
    checked = set()
    for w, h in TWO_TILES:
        rays = G.camera_rays(accel, w, h)
        mixed_rays(accel, rays, (name, kind, w, h))
        want_a, want_d = oracle_film(scene_of, w, h), bits(oracle_radiance(scene_of, w, h))
        for form in each_form(accel):
            for order in (0, 1):
                G.set_query_order(accel, order)
                rgba, rgb = G.capture_rays(accel, rays, w, h, samples=1, rgb=True)  # (one sample a slot: the film forms of the three kernels)
                assert np.array_equal(rgba, want_a) and np.array_equal(bits(rgb), want_d), (name, kind, form, order, w * h)
            G.set_query_order(accel, 0)
            checked.add(form)
    assert L0_FORMS[name] <= checked, (name, checked)
