"""View batches (include/lasgun_hip.h, lg_view_look_at .. lg_capture_views_device; lasgun_amd/csrc/k_views.hip): one accel from K cameras
into K films in one call.  Every comparison is bit for bit: the scene's own view against lg_capture and lg_capture_radiance; view_rays against
camera_rays of an accel rebuilt with that camera; three cameras in one call against the oracle's render of a scene rebuilt per camera; odd
film sizes, many one-tile views, every traversal form, many chunks, and the errors, against lg_capture_rays on the views' rays written out."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import scenes as S
from test_gpu_radiance_query import FORM_SCENES, L0_CASES, L0_FORMS, L0_IDS, SECOND, bits, each_form, l0_scene, many_lights_scene, mixed_rays, oracle_radiance, with_camera
from test_gpu_ray_film import oracle_film
from test_gpu_visibility import reset, set_form

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
W, H = 96, 64


def view_of(cam, supersampling=0):
    """The View of a camera of SECOND: (kind, fov or scale, eye, look, up)."""
    kind, par, eye, look, up = cam
    return la.view_look_at(eye, look, up, supersampling=supersampling, **({"scale": par} if kind == "orthographic" else {"fov": par}))


def by_rays(accel, views, w, h):
    """The K films and their doubles from lg_capture_rays on the views' rays written out, film after film: (K, h, w, 4), (K, h, w, 3)."""
    samples = int(views[0].samples_root) ** 2
    rays = np.concatenate([G.view_rays(accel, v, w, h) for v in views])
    a, d = G.capture_rays(accel, rays, w, h * len(views), samples=samples, rgb=True)
    return a.reshape(len(views), h, w, 4), d.reshape(len(views), h, w, 3)


# ---- 1: the scene's own view ---------------------------------------------------------------------------------------------------------
OWN = [("perspective", 0, 96, 64), ("perspective", 1, 96, 64), ("orthographic", 0, 96, 64), ("perspective", 2, 45, 27)]


@pytest.mark.parametrize("cam,ss,w,h", OWN, ids=["%s_ss%d_%dx%d" % o for o in OWN])
def test_the_scenes_own_view_is_the_capture(cam, ss, w, h):
    scene = S.kitchen_sink_scene(G, camera=cam, supersampling=ss)
    accel = G.Accel.from_scene(scene)
    view = G.accel_view(accel)
    assert view.samples_root == ss + 1 and bytes(view) == bytes(G.scene_view(scene))
    rgba, rgb = G.capture_views(accel, [view], w, h, rgb=True)
    assert rgba.shape == (1, h, w, 4) and rgb.shape == (1, h, w, 3)
    film = G.Film.new(w, h)
    G.capture(scene, film)
    assert np.array_equal(rgba[0], film.pixels()), "lg_capture"
    assert np.array_equal(bits(rgb[0]), bits(G.capture_radiance(accel, w, h))), "lg_capture_radiance(0, 1, ..)"
    assert np.array_equal(accel.views([view], w, h), rgba)


# ---- 2: view_rays against a rebuilt accel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,specular,cameras", SECOND, ids=[s[0] for s in SECOND])
def test_view_rays_are_the_camera_rays_of_an_accel_rebuilt_with_that_camera(name, builder, specular, cameras):
    accel_a = G.Accel.from_scene(builder(G))
    for k, cam in enumerate(cameras):
        scene_b = with_camera(builder(G), cam)
        scene_b.camera.set_supersampling(1)
        accel_b = G.Accel.from_scene(scene_b)
        view = view_of(cam, supersampling=1)
        assert bytes(view) == bytes(G.accel_view(accel_b)), (name, k)
        whole = G.view_rays(accel_a, view, W, H)
        assert whole.shape == (W * H * 4, 6) and whole.tobytes() == G.camera_rays(accel_b, W, H).tobytes(), (name, k)
        rect = G.view_rays(accel_a, view, W, H, 3, 5, 41, 29)
        assert rect.shape == (38 * 24 * 4, 6) and rect.tobytes() == G.camera_rays(accel_b, W, H, 3, 5, 41, 29).tobytes(), (name, k)


# ---- 3: three cameras in one call, pinned to the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,specular,cameras", SECOND, ids=[s[0] for s in SECOND])
def test_three_cameras_in_one_call_give_the_oracles_renders(name, builder, specular, cameras):
    accel_a = G.Accel.from_scene(builder(G))
    assert len(cameras) == 3 and any(c[0] == "orthographic" for c in cameras) and any(c[0] == "perspective" for c in cameras)
    views = [view_of(cam) for cam in cameras]
    rgba, rgb = G.capture_views(accel_a, views, W, H, rgb=True)  # ONE call, the kinds mixed
    for k, cam in enumerate(cameras):
        hit = G.intersect(accel_a, G.view_rays(accel_a, views[k], W, H))["kind"] != 0
        assert hit.mean() >= 0.20 and (~hit).mean() >= 0.05, (name, k, hit.mean())
        want = oracle_film(lambda api: with_camera(builder(api), cam), W, H)
        assert np.array_equal(rgba[k], want), (name, k, int((rgba[k] != want).any(axis=2).sum()))
        want_d = oracle_radiance(lambda api: with_camera(builder(api), cam), W, H)
        assert np.array_equal(bits(rgb[k]).reshape(-1), bits(want_d).reshape(-1)), (name, k)
        alone_a, alone_d = G.capture_views(accel_a, [views[k]], W, H, rgb=True)
        assert alone_a[0].tobytes() == rgba[k].tobytes() and alone_d[0].tobytes() == rgb[k].tobytes(), (name, k)
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(rgba[i], rgba[j]), (name, i, j)


# ---- 4: shapes where the mapping can go wrong -------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (7, 9), (8, 8), (9, 8), (13, 5), (13, 11), (64, 1), (1, 64)]
GUARD = 64


@pytest.mark.parametrize("ss", (0, 1), ids=["S1", "S4"])
def test_film_shapes_and_guard_bytes(ss):
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    _, _, _, cameras = SECOND[1]
    views = [view_of(cameras[0], ss), view_of(cameras[2], ss)]
    for w, h in SHAPES:
        want_a, want_d = by_rays(accel, views, w, h)
        na, nd = 2 * w * h * 4, 2 * w * h * 3
        for ask_a, ask_d in ((True, False), (False, True), (True, True)):
            buf_a = np.full(na + GUARD, 0xA5, dtype=np.uint8)
            buf_d = np.full(nd + GUARD // 8, -7.0, dtype=np.float64)
            into = (buf_a[:na].reshape(2, h, w, 4) if ask_a else None, buf_d[:nd].reshape(2, h, w, 3) if ask_d else None)
            G.capture_views(accel, views, w, h, into=into)
            assert (buf_a[na:] == 0xA5).all() and (buf_d[nd:] == -7.0).all(), (w, h, "guard")
            if ask_a:
                assert buf_a[:na].tobytes() == want_a.tobytes(), (w, h, ss, ask_a, ask_d)
            else:
                assert (buf_a == 0xA5).all()
            if ask_d:
                assert buf_d[:nd].tobytes() == want_d.tobytes(), (w, h, ss, ask_a, ask_d)
            else:
                assert (buf_d == -7.0).all()


# ---- 5: many one-tile views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", (8, 9))
def test_many_small_views(side):
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    views = la.orbit_views((0.0, 0.0, 0.0), 5.0, 15.0, 130, 50.0)
    assert len(views) == 130
    want_a, want_d = by_rays(accel, views, side, side)
    rgba, rgb = G.capture_views(accel, views, side, side, rgb=True)
    assert rgba.tobytes() == want_a.tobytes() and rgb.tobytes() == want_d.tobytes()
    assert len({rgba[k].tobytes() for k in range(130)}) > 1, "the 130 films are not all equal"


# ---- 6: every form gives identical bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", FORM_SCENES, ids=[n for n, _ in FORM_SCENES])
def test_every_form_gives_identical_bytes(name, builder):
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(builder(G))
    w, h = 40, 24
    eye = np.array(G.accel_view(accel).origin[:])
    look = eye + np.array(G.accel_view(accel).view[:])
    batches = []
    for ss in (0, 1):
        views = la.orbit_views(look, float(np.linalg.norm(eye - look)), 20.0, 5, 55.0, supersampling=ss)
        set_form(accel, "reference")
        G.set_lds_scene(accel, False)
        batches.append((views, G.capture_views(accel, views, w, h, rgb=True)))
        want_a, want_d = by_rays(accel, views, w, h)
        assert batches[-1][1][0].tobytes() == want_a.tobytes() and batches[-1][1][1].tobytes() == want_d.tobytes(), (name, ss)
        assert len(np.unique(batches[-1][1][1])) > 100  # (pictures, not a constant)
    checked = []
    try:
        fits = G.set_lds_scene(accel, True)
        G.set_lds_scene(accel, False)
        if name == "cornell_glass":
            assert fits, "a scene of a few dozen triangles fits the LDS"
        for form in ["prune"] + (["lds"] if fits else []) + ["fast"]:
            try:
                set_form(accel, form)
            except la.LasgunError:
                assert not (form == "fast" and name == "mesh_glass"), "the small torus scene admits the fast mode"
                continue
            if form != "lds":
                G.set_lds_scene(accel, False)
            for views, (ref_a, ref_d) in batches:
                a, d = G.capture_views(accel, views, w, h, rgb=True)
                assert a.tobytes() == ref_a.tobytes() and d.tobytes() == ref_d.tobytes(), (name, form, views[0].samples_root)
            checked.append(form)
    finally:
        reset(accel)
    assert "prune" in checked and ("lds" in checked or name != "cornell_glass")
    # the host form against the device form on a stream that is not the default one
    stream = torch.cuda.Stream()
    for views, (ref_a, ref_d) in batches:
        da = torch.zeros(5 * w * h * 4, dtype=torch.uint8, device="cuda")
        dd = torch.full((5 * w * h * 3,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            G.capture_views_device(accel, views, w, h, rgba_ptr=da.data_ptr(), rgb_ptr=dd.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        stream.synchronize()
        a, d = G.capture_views(accel, views, w, h, rgb=True)
        assert da.cpu().numpy().tobytes() == a.tobytes() and dd.cpu().numpy().tobytes() == d.tobytes(), (name, "device")
        assert a.tobytes() == ref_a.tobytes() and d.tobytes() == ref_d.tobytes(), (name, "the accel's defaults")


# ---- 7: many chunks --------------------------------------------------------------------------------------------------------------------------
def run_child(name, views, w, h, budget_mb):
    """The batch in a fresh process under LASGUN_WF_BUDGET_MB = budget_mb (None: the default): (rgba, rgb, pixel tiles, tiles per chunk, tiles per view)."""
    with tempfile.TemporaryDirectory() as tmp:
        vp, op = os.path.join(tmp, "views.npy"), os.path.join(tmp, "out.npz")
        np.save(vp, np.stack([np.frombuffer(bytes(v), dtype=np.uint8) for v in views]))
        env = dict(os.environ)
        env["LASGUN_DEBUG"] = "1"
        env.pop("LASGUN_WF_BUDGET_MB", None)
        if budget_mb is not None:
            env["LASGUN_WF_BUDGET_MB"] = str(budget_mb)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "views_child.py"), name, vp, str(w), str(h), op], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        m = re.findall(r"view batch: levels \d+, (\d+) tiles in chunks of (\d+) \([^)]*\), (\d+) views of (\d+) tiles x (\d+) samples", p.stderr)
        assert m, p.stderr[-3000:]
        tiles, per_chunk, k, per_view, samples = (int(x) for x in m[-1])
        assert k == len(views) and tiles == k * per_view and samples == int(views[0].samples_root) ** 2
        out = np.load(op)
        return out["rgba"], out["rgb"], tiles, per_chunk, per_view


def test_a_nine_sample_batch_in_many_chunks_gives_identical_bytes():
    name, builder = FORM_SCENES[0]
    w, h = 128, 128
    accel = G.Accel.from_scene(builder(G))
    _, _, _, cameras = SECOND[1]
    views = [view_of(cam, 2) for cam in cameras]
    ref_a, ref_d = G.capture_views(accel, views, w, h, rgb=True)
    one_a, one_d, tiles, per_chunk, per_view = run_child(name, views, w, h, None)
    assert tiles == 3 * 256 and per_view == 256 and per_chunk == tiles, "the default budget holds the batch in one chunk"
    assert one_a.tobytes() == ref_a.tobytes() and one_d.tobytes() == ref_d.tobytes()
    a, d, tiles, per_chunk, per_view = run_child(name, views, w, h, 64)
    starts = list(range(0, tiles, per_chunk))
    assert len(starts) >= 3, (tiles, per_chunk)
    assert any(min(s + per_chunk, tiles) % per_view for s in starts), ("no chunk ends inside a view", per_chunk)
    assert any(s // per_view != (min(s + per_chunk, tiles) - 1) // per_view for s in starts), ("no chunk spans two views", per_chunk)
    assert a.tobytes() == ref_a.tobytes() and d.tobytes() == ref_d.tobytes()


# ---- 8: sharing the accel ---------------------------------------------------------------------------------------------------------------------
def test_renders_and_view_batches_share_an_accel():
    scene = S.cornell_scene(G, "glass")
    accel = G.Accel.from_scene(scene)
    _, _, _, cameras = SECOND[1]
    views = [view_of(cam, 1) for cam in cameras]
    w, h = 64, 48
    want_v = by_rays(accel, views, w, h)
    film0 = G.Film.new(w, h)
    G.capture_subset(0, 1, accel, film0)
    want_r = film0.pixels()
    for _ in range(2):
        a, d = G.capture_views(accel, views, w, h, rgb=True)  # a view batch after a render ...
        assert a.tobytes() == want_v[0].tobytes() and d.tobytes() == want_v[1].tobytes()
        film = G.Film.new(w, h)
        G.capture_subset(0, 1, accel, film)  # ... and a render after a view batch
        assert np.array_equal(film.pixels(), want_r)
        G.set_streaming(accel, 2)  # (the render level by level too: the same launch context's arrays)
    G.set_streaming(accel, 1)


# ---- 9: errors --------------------------------------------------------------------------------------------------------------------------------
def table(views):
    return (la.View * len(views))(*views)


def test_errors_are_reported_and_nothing_is_launched():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    _, _, _, cameras = SECOND[1]
    w, h = 16, 16
    good = [view_of(cameras[0]), view_of(cameras[1])]

    def edited(**kw):
        v = la.View.from_buffer_copy(bytes(good[1]))
        for k, x in kw.items():
            setattr(v, k, x)
        return [good[0], v]

    host_a, host_d = np.full((2, h, w, 4), 0xA5, dtype=np.uint8), np.full((2, h, w, 3), -7.0)
    da = torch.full((2 * w * h * 4 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    dd = torch.full((2 * w * h * 3 + 1,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    adr = ctypes.addressof

    def host(acc, views, k, ww, hh, a=host_a.ctypes.data, d=host_d.ctypes.data):
        return G.call("capture_views", acc, adr(views) if views is not None else None, k, ww, hh, a, d)

    def device(acc, views, k, ww, hh, a=da.data_ptr(), d=dd.data_ptr()):
        return G.call("capture_views_device", acc, adr(views) if views is not None else None, k, ww, hh, a, d, None)

    t = table(good)
    accel_many = G.Accel.from_scene(many_lights_scene(G, 33))
    deep_scene = S.cornell_scene(G, "glass")
    deep_scene.set_max_recursion_depth(20)
    deep = G.Accel.from_scene(deep_scene)
    big = table([good[0]] * 4)
    for call in (host, device):
        cases = [(None, t, 2, w, h), (accel.h, None, 2, w, h), (accel.h, t, 2, 0, h), (accel.h, t, 2, w, 0),
                 (accel.h, table(edited(samples_root=0)), 2, w, h), (accel.h, table(edited(samples_root=257)), 2, w, h),
                 (accel.h, table(edited(reserved=1)), 2, w, h), (accel.h, table(edited(samples_root=2)), 2, w, h),
                 (accel.h, big, 4, 1 << 18, 1 << 18),   # 4 * 2^15 * 2^15 = 2^32 work tiles: one above the limit
                 (accel.h, t, (1 << 62), 8, 8),         # a byte size beyond SIZE_MAX (and more tiles than 2^32 - 1)
                 (accel_many.h, t, 2, w, h), (deep.h, t, 2, w, h)]
        for k, args in enumerate(cases):
            assert call(*args) != 0 and G.last_error(), (call.__name__, k)
        assert call(accel.h, t, 2, w, h, None, None) != 0 and "both NULL" in G.last_error(), call.__name__
        assert call(accel.h, None, 0, w, h) == 0 and call(accel.h, t, 0, 0, 0, None, None) == 0, "n_views == 0 is a successful no-op"
    # the device form's own: host memory, a misaligned dev_rgb / dev_rgba, a dev_rgba one film too short
    assert device(accel.h, t, 2, w, h, a=host_a.ctypes.data) != 0 and "device memory" in G.last_error()
    assert device(accel.h, t, 2, w, h, d=host_d.ctypes.data) != 0 and "device memory" in G.last_error()
    assert device(accel.h, t, 2, w, h, d=dd.data_ptr() + 4) != 0 and "8-byte aligned" in G.last_error()
    assert device(accel.h, t, 2, w, h, a=da.data_ptr() + 2) != 0 and "4-byte aligned" in G.last_error()
    torch.cuda.empty_cache()
    bw, bh = 2048, 1536  # one film is 12 MiB: an allocation of its own, and the call asks for two
    short = torch.full((bw * bh * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert device(accel.h, t, 2, bw, bh, a=short.data_ptr(), d=None) != 0 and "ends beyond its allocation" in G.last_error()
    torch.cuda.synchronize()
    assert (host_a == 0xA5).all() and (host_d == -7.0).all(), "an error touched a host output"
    assert (da.cpu().numpy() == 0xA5).all() and (dd.cpu().numpy() == -7.0).all() and bool((short == 0xA5).all()), "an error touched a device output"
    with pytest.raises(la.LasgunError):
        G.capture_views(accel, edited(samples_root=2), w, h)
    with pytest.raises(la.LasgunError):
        G.view_rays(accel, edited(reserved=1)[1], w, h)
    with pytest.raises(la.LasgunError):
        G.view_rays(accel, good[0], w, h, 0, 0, w + 1, h)
    # and the calls still work afterwards
    a, d = G.capture_views(accel, good, w, h, rgb=True)
    want_a, want_d = by_rays(accel, good, w, h)
    assert a.tobytes() == want_a.tobytes() and d.tobytes() == want_d.tobytes()
    G.capture_views_device(accel, good, w, h, rgba_ptr=da.data_ptr(), rgb_ptr=dd.data_ptr(), stream=0)
    torch.cuda.synchronize()
    assert da.cpu().numpy()[:2 * w * h * 4].tobytes() == a.tobytes() and (da.cpu().numpy()[2 * w * h * 4:] == 0xA5).all()
    assert dd.cpu().numpy()[:2 * w * h * 3].tobytes() == d.tobytes() and dd.cpu().numpy()[-1] == -7.0


# ---- level 0's shared bodies: two tiles, the last one partial, in every form and KIND, one sample and four (test_gpu_radiance_query.py, section 6)
@pytest.mark.parametrize("name,builder,kind", L0_CASES, ids=L0_IDS)
def test_two_views_of_two_tiles_in_every_form_are_the_films_of_their_rays(name, builder, kind):
    """2 views of 9 x 9 pixels: four tiles a view, three of them partial, at samples_root 1 and 2 -- against lg_capture_rays on the views' rays
    written out (which test_gpu_ray_film.py holds to the oracle) and against the oracle's own renders of the scene rebuilt with each camera."""
    scene_of = l0_scene(builder, kind)
    accel = G.Accel.from_scene(scene_of(G))
    w = h = 9
    cameras = [s[3] for s in SECOND if s[0] == "cornell_glass"][0][:2]  # (both scenes stand in the same shell: a perspective and an orthographic view of it)
    checked = set()
    for ss in (0, 1):
        views = [view_of(cam, supersampling=ss) for cam in cameras]
        mixed_rays(accel, np.concatenate([G.view_rays(accel, v, w, h) for v in views]), (name, kind, ss))
        def rebuilt(cam):
            def scene_b(api):
                scene = with_camera(scene_of(api), cam)
                scene.camera.set_supersampling(ss)
                return scene
            return scene_b
        films = [oracle_film(rebuilt(cam), w, h) for cam in cameras]
        for form in each_form(accel):
            want_a, want_d = by_rays(accel, views, w, h)
            a, d = G.capture_views(accel, views, w, h, rgb=True)
            assert a.tobytes() == want_a.tobytes() and d.tobytes() == want_d.tobytes(), (name, kind, form, ss)
            for k in range(len(cameras)):
                assert np.array_equal(a[k], films[k]), (name, kind, form, ss, k, "oracle")
            checked.add(form)
    assert L0_FORMS[name] <= checked, (name, checked)
