"""View features (include/lasgun_hip.h: lg_capture_view_features, lg_capture_view_features_device; lasgun_amd/csrc/k_view_features.hip):
depth, normal, albedo, coverage, ids and the world-space hit point of the primary hits of K cameras over one accel, K whole films' planes
in one call.

The expected planes are computed in numpy from the library's older entry points -- hits = lg_intersect(lg_view_rays(view v)), view after
view, reshaped to (pixels, S) -- by the contract's loop written out (test_gpu_features.expected for the five shared planes, `restate`
below adds point: a Python `for s`, vectorised over the pixels, in f64, astype(float32)) and compared as BIT PATTERNS (NaNs
canonicalised): no tolerance, no mismatch.

  1  the accel's own view: the five shared planes are capture_features' full-film bytes, point the restatement over
     lg_intersect(lg_camera_rays);
  2  three mixed cameras in ONE call per scene of SECOND against the contract's loop, each view alone giving its slice's bytes; and
     against the CPU oracle's closest hits of those rays (portable-trig mode), a sphere scene and a mesh scene;
  3  film shapes (1,1) .. (1,64), two views, S = 1 and 4, every plane alone, depth + id + point and all six, over a 0xA5 prefill with 64
     guard bytes behind each plane; twice the same bytes;
  4  view boundaries and the tile claim's other path: 130 views of one tile and of four tiles, 66 views of 128 x 128 (16,896 tiles), on a
     scene resident in LDS (claims per XCD band) and on one with a single head, against ONE lg_intersect over the concatenated rays;
  5  supersampling: the own view and a look-at view in one call at S = 4 and 9 -- the sums in order, id from sample 0, depth's and
     point's divisor;
  6  every traversal form of FORM_SCENES: the reference's bytes in that form;
  7  the device form on a torch stream that is not the default one: the host form's bytes;
  8  every error of the contract refused with every plane at its prefill; n_views == 0 a no-op even with a NULL accel; a 40-light scene
     accepted.
Non-vacuity is asserted on lg_intersect's / the oracle's answer before anything is compared."""
import ctypes

import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_features import bits32, expected, pod_rgb, table_rgb
from test_gpu_radiance_query import FORM_SCENES, SECOND, many_lights_scene, with_camera  # noqa: F401  (with_camera: the cameras' own convention)
from test_gpu_visibility import reset, set_form

pytestmark = pytest.mark.gpu

G = la.api
W, H = 96, 64
PLANES = la.VIEW_FEATURE_PLANES
SHAPE = {"depth": (), "normal": (3,), "albedo": (3,), "coverage": (), "id": (4,), "point": (3,)}
GUARD = 64


def view_of(cam, supersampling=0):
    """The View of a camera of SECOND: (kind, fov or scale, eye, look, up)."""
    kind, par, eye, look, up = cam
    return la.view_look_at(eye, look, up, supersampling=supersampling, **({"scale": par} if kind == "orthographic" else {"fov": par}))


def restate(hits, samples, ray_rgb, id_material=None):
    """The contract's loop: test_gpu_features.expected for depth, normal, albedo, coverage and id, and point beside them -- psum from +0.0,
    a hit adds lg_hit::p per component for s ascending, point = nhit ? (float)(psum * (1.0 / (double)nhit)) : 0.0f."""
    out = expected(hits, samples, ray_rgb, id_material)
    h = hits.reshape(-1, samples)
    n = h.shape[0]
    psum, nhit = np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(samples):
            hs = h[:, s]
            hit = hs["kind"] != 0
            psum = np.where(hit[:, None], psum + hs["p"], psum)
            nhit = nhit + hit
        mean_p = (psum * (1.0 / np.maximum(nhit, 1).astype(np.float64))[:, None]).astype(np.float32)
    out["point"] = np.where((nhit > 0)[:, None], mean_p, np.float32(0.0)).astype(np.float32)
    return out


def view_hits(accel, views, w, h):
    """ONE lg_intersect over the views' rays written out, view after view: (K * w * h * S) lg_hit records."""
    return G.intersect(accel, np.concatenate([G.view_rays(accel, v, w, h) for v in views]))


def random_table(accel, seed=11):
    return np.random.default_rng(seed).random((G.material_count(accel), 3))


def compare(got, want, ctx, planes=PLANES):
    """got: (K, h, w, ...) planes; want: (K * h * w, ...) planes of the restatement.  The bits."""
    for p in planes:
        a, b = bits32(got[p].reshape((-1,) + SHAPE[p])), bits32(want[p])
        assert a.shape == b.shape, (ctx, p, a.shape, b.shape)
        assert np.array_equal(a, b), (ctx, p, int((a != b).sum()), "of", a.size, "words differ; first at", np.argwhere(a != b)[:1].tolist())


# ---- 1: the accel's own view -----------------------------------------------------------------------------------------------------------
OWN = [("perspective", 0, 96, 64), ("perspective", 1, 96, 64), ("perspective", 2, 45, 27), ("orthographic", 0, 96, 64), ("orthographic", 1, 45, 27)]


@pytest.mark.parametrize("cam,ss,w,h", OWN, ids=["%s_ss%d_%dx%d" % o for o in OWN])
def test_the_accels_own_view_gives_capture_features_bytes(cam, ss, w, h):
    accel = G.Accel.from_scene(S.kitchen_sink_scene(G, camera=cam, supersampling=ss))
    view = G.accel_view(accel)
    samples = (ss + 1) ** 2
    assert view.samples_root == ss + 1 and G.camera_samples(accel) == samples
    table = random_table(accel)
    got = G.capture_view_features(accel, [view], w, h, material_rgb=table)
    assert set(got) == set(PLANES) and got["point"].shape == (1, h, w, 3) and got["id"].shape == (1, h, w, 4) and got["depth"].shape == (1, h, w)
    own = G.capture_features(accel, w, h, material_rgb=table)
    for p in la.FEATURE_PLANES:
        assert got[p][0].tobytes() == own[p].tobytes(), (cam, ss, p, "lg_capture_features' full-film bytes")
    hits = G.intersect(accel, G.camera_rays(accel, w, h))
    assert (hits["kind"] != 0).any() and (hits["kind"] == 0).any(), (cam, ss)
    compare(got, restate(hits, samples, table_rgb(hits, table)), (cam, ss, w, h))
    assert got["point"].any() and (got["point"][0][np.isinf(got["depth"][0])] == 0.0).all()
    again = accel.view_features([view], w, h, material_rgb=table)
    assert all(again[p].tobytes() == got[p].tobytes() for p in PLANES)


# ---- 2: three mixed cameras in one call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,specular,cameras", SECOND, ids=[s[0] for s in SECOND])
def test_three_mixed_cameras_in_one_call(name, builder, specular, cameras):
    accel = G.Accel.from_scene(builder(G))
    assert len(cameras) == 3 and any(c[0] == "orthographic" for c in cameras) and any(c[0] == "perspective" for c in cameras)
    views = [view_of(cam) for cam in cameras]
    hits = view_hits(accel, views, W, H)
    per_view = (hits["kind"] != 0).reshape(3, -1)
    for k in range(3):
        assert per_view[k].mean() >= 0.20 and (~per_view[k]).mean() >= 0.05, (name, k, per_view[k].mean())
    assert len(np.unique(hits["kind"][hits["kind"] != 0])) >= 2, (name, "kinds among the hits")
    table = random_table(accel)
    want = restate(hits, 1, table_rgb(hits, table))
    got = G.capture_view_features(accel, views, W, H, material_rgb=table)  # ONE call, the kinds mixed
    compare(got, want, name)
    for k in range(3):
        alone = G.capture_view_features(accel, [views[k]], W, H, material_rgb=table)
        for p in PLANES:
            assert alone[p][0].tobytes() == got[p][k].tobytes(), (name, k, p, "a view alone gives its slice's bytes")
    for i in range(3):
        for j in range(i + 1, 3):
            assert got["point"][i].tobytes() != got["point"][j].tobytes() and got["id"][i].tobytes() != got["id"][j].tobytes(), (name, i, j)


ORACLE_SCENES = [("spheres", SECOND[2][1], SECOND[2][3]), ("mesh", lambda api: S.instanced_scene(api), SECOND[1][3])]


@pytest.mark.parametrize("name,builder,cameras", ORACLE_SCENES, ids=[s[0] for s in ORACLE_SCENES])
def test_three_mixed_cameras_equal_the_cpu_oracles_hits(name, builder, cameras):
    accel = G.Accel.from_scene(builder(G))
    views = [view_of(cam) for cam in cameras]
    rays = np.concatenate([G.view_rays(accel, v, W, H) for v in views])
    o = oracle()
    oaccel = o.Accel.from_scene(builder(o))
    o.set_trig_mode(True)  # the sphere's trigonometry the device runs (its normals compare bit for bit)
    try:
        ohits, omats = o.intersect(oaccel, rays, 16)
    finally:
        o.set_trig_mode(False)
    hit = ohits["kind"] != 0
    per_view = hit.reshape(3, -1)
    for k in range(3):
        assert per_view[k].mean() >= 0.20 and (~per_view[k]).mean() >= 0.05, (name, k, per_view[k].mean())
    assert len(np.unique(ohits["kind"][hit])) >= 2, (name, "kinds among the hits")
    keys = np.concatenate([omats["kind"][:, None].astype(np.float64), omats["p"]], axis=1)
    colour = {row.tobytes(): pod_rgb(int(row[0]), row[1:]) for row in np.unique(keys[hit], axis=0)}
    ray_rgb = np.zeros((len(ohits), 3))
    for i in np.nonzero(hit)[0]:
        ray_rgb[i] = colour[keys[i].tobytes()]
    lib = [G.accel_material(accel, i) for i in range(G.material_count(accel))]
    table = np.array([pod_rgb(m["kind"], m["p"]) for m in lib])
    got = G.capture_view_features(accel, views, W, H, material_rgb=table)
    # id's material column: the library's index must name the POD the oracle's ray hit
    mat = got["id"][..., 3].reshape(-1).view(np.int32)
    assert np.array_equal(mat == -1, ~hit)
    for i in np.nonzero(hit)[0]:
        m = lib[mat[i]]
        assert np.array([float(m["kind"])] + list(m["p"])).tobytes() == keys[i].tobytes(), (name, i)
    compare(got, restate(ohits, 1, ray_rgb, id_material=mat), (name, "oracle"))


# ---- 3: film shapes with guard bytes ------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (7, 9), (8, 8), (9, 8), (13, 5), (13, 11), (64, 1), (1, 64)]
SUBSETS = [(p,) for p in PLANES] + [("depth", "id", "point"), PLANES]


def guarded(pixels):
    """Per plane a byte buffer of its size plus GUARD, all 0xA5."""
    return {p: np.full(pixels * int(np.prod(SHAPE[p], dtype=np.int64)) * 4 + GUARD, 0xA5, dtype=np.uint8) for p in PLANES}


@pytest.mark.parametrize("ss", (0, 1), ids=["S1", "S4"])
def test_film_shapes_and_guard_bytes(ss):
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    _, _, _, cameras = SECOND[1]
    views = [view_of(cameras[0], ss), view_of(cameras[2], ss)]
    tab = (la.View * 2)(*views)
    samples = (ss + 1) ** 2
    table = random_table(accel)
    for w, h in SHAPES:
        pixels = 2 * w * h
        hits = view_hits(accel, views, w, h)
        want = restate(hits, samples, table_rgb(hits, table))
        for subset in SUBSETS:
            runs = []
            for _ in range(2):
                buf = guarded(pixels)
                f = la.CViewFeatures(*[buf[p].ctypes.data if p in subset else None for p in PLANES])
                rc = G.call("capture_view_features", accel.h, ctypes.addressof(tab), 2, w, h, ctypes.addressof(f), table.ctypes.data if "albedo" in subset else None)
                assert rc == 0, G.last_error()
                for p in PLANES:
                    if p in subset:
                        assert (buf[p][-GUARD:] == 0xA5).all(), (w, h, ss, subset, p, "guard")
                        dt = np.uint32 if p == "id" else np.float32
                        plane = buf[p][:-GUARD].view(dt).reshape((-1,) + SHAPE[p])
                        a, b = bits32(plane), bits32(want[p])
                        assert np.array_equal(a, b), (w, h, ss, subset, p, int((a != b).sum()))
                    else:
                        assert (buf[p] == 0xA5).all(), (w, h, ss, subset, p, "a plane that was not asked for was written")
                runs.append({p: buf[p].tobytes() for p in subset})
            assert runs[0] == runs[1], (w, h, ss, subset, "the same call twice")


# ---- 4: view boundaries and the tile claim's other path ---------------------------------------------------------------------------------
ORBIT_RADIUS = 8.0  # (test_gpu_views' radius 5 stands inside the Cornell shell's silhouette: 99.6 % of an orbit's pixels hit)
BOUNDARY_SCENES = {"cornell_glass": lambda api: S.cornell_scene(api, "glass"),   # resident in LDS: tiles are claimed per XCD band
                   "instanced": lambda api: S.instanced_scene(api)}               # a single head
BATCHES = [(130, 8), (130, 9), (66, 128)]


@pytest.mark.parametrize("n,side", BATCHES, ids=["%dx%d^2" % b for b in BATCHES])
@pytest.mark.parametrize("name", list(BOUNDARY_SCENES))
def test_view_boundaries_and_more_tiles_than_twice_the_grids_waves(name, n, side):
    """130 views of one tile (8 x 8) and of four partial tiles (9 x 9): consecutive tiles belong to different views; 66 views of 128 x 128
    are 16,896 tiles, more than twice the waves of any grid.  The orbit is test_gpu_views' on the Cornell shell (centre 0, elevation 15
    degrees, fov 50) at radius 8 instead of 5: at radius 5 only 0.4 % of the batch's pixels miss (0.7 % at 128 x 128).  Shares found on the
    CPU, with a numpy restatement of the header's ray expression and the oracle's intersect, the same for both scenes (the shell decides):
    130 x 8 x 8: 44.2 % hit, 25 .. 30 hits a view; 130 x 9 x 9: 47.4 % hit, 35 .. 42 a view; 66 x 128 x 128: 47.5 % hit, 7468 .. 7991 a view."""
    accel = G.Accel.from_scene(BOUNDARY_SCENES[name](G))
    if name == "cornell_glass":
        assert G.set_lds_scene(accel, True), "a scene of a few dozen triangles fits the LDS"
    views = la.orbit_views((0.0, 0.0, 0.0), ORBIT_RADIUS, 15.0, n, 50.0)
    assert len(views) == n and (n * ((side + 7) // 8) ** 2 == 16896 or side < 10)
    hits = view_hits(accel, views, side, side)
    per_view = (hits["kind"] != 0).reshape(n, -1)
    assert per_view.mean() >= 0.10 and (~per_view).mean() >= 0.10, (name, n, side, per_view.mean())
    assert len(np.unique(per_view.sum(axis=1))) > 1, "the views' hit counts are not all equal"
    table = random_table(accel)
    want = restate(hits, 1, table_rgb(hits, table))
    got = G.capture_view_features(accel, views, side, side, material_rgb=table)
    compare(got, want, (name, n, side))
    assert len({got["depth"][k].tobytes() for k in range(n)}) > 1


# ---- 5: supersampling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", (1, 2), ids=["S4", "S9"])
def test_supersampled_pixels_sum_their_samples_in_order(ss):
    accel = G.Accel.from_scene(S.simple_scene(G, ss))
    samples = (ss + 1) ** 2
    own = G.accel_view(accel)
    assert own.samples_root == ss + 1
    views = [own, view_of(SECOND[2][3][0], ss)]
    hits = view_hits(accel, views, W, H)
    h = hits.reshape(2, W * H, samples)
    nhit = (h["kind"] != 0).sum(axis=2)
    part = (nhit > 0) & (nhit < samples)
    assert part[0].mean() >= 0.02, ("the own view's pixels with 0 < coverage < 1", part[0].mean())
    assert part[1].sum() >= 8, "the look-at view's pixels on an edge"
    first_differs = part & ((h["kind"][:, :, 0] != 0) != (h["kind"][:, :, -1] != 0))
    assert first_differs[0].any(), "id must come from sample 0 where the samples disagree"
    table = random_table(accel)
    want = restate(hits, samples, table_rgb(hits, table))
    got = G.capture_view_features(accel, views, W, H, material_rgb=table)
    compare(got, want, ("supersampling", ss))
    # depth's and point's own divisor: on an edge pixel sum / nhit differs from sum / S
    k = np.nonzero(part.reshape(-1))[0]
    hk, nk = h.reshape(-1, samples)[k], nhit.reshape(-1)[k]
    tsum = np.where(hk["kind"] != 0, hk["t"], 0.0).sum(axis=1)
    psum = np.where((hk["kind"] != 0)[:, :, None], hk["p"], 0.0).sum(axis=1)
    depth, point = got["depth"].reshape(-1)[k], got["point"].reshape(-1, 3)[k]
    assert np.allclose(depth, tsum / nk, rtol=1e-6) and not np.allclose(depth, tsum / samples, rtol=1e-3)
    assert np.allclose(point, psum / nk[:, None], rtol=1e-5, atol=1e-4) and not np.allclose(point, psum / samples, rtol=1e-3, atol=1e-4)
    assert np.array_equal(got["coverage"].reshape(-1), (nhit.reshape(-1) / float(samples)).astype(np.float32))
    own_planes = G.capture_features(accel, W, H, material_rgb=table)
    for p in la.FEATURE_PLANES:
        assert got[p][0].tobytes() == own_planes[p].tobytes(), (ss, p)


# ---- 6: every traversal form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", FORM_SCENES, ids=[n for n, _ in FORM_SCENES])
def test_every_traversal_form_gives_the_references_bytes_in_that_form(name, builder):
    accel = G.Accel.from_scene(builder(G))
    w, h = 40, 24
    eye = np.array(G.accel_view(accel).origin[:])
    look = eye + np.array(G.accel_view(accel).view[:])
    table = random_table(accel)
    batches = [la.orbit_views(look, float(np.linalg.norm(eye - look)), 20.0, 5, 55.0, supersampling=ss) for ss in (0, 1)]
    checked = []
    try:
        fits = G.set_lds_scene(accel, True)
        if name == "cornell_glass":
            assert fits, "a scene of a few dozen triangles fits the LDS"
        for form in ["reference", "prune"] + (["lds"] if fits else []) + ["fast"]:
            try:
                set_form(accel, form)
            except la.LasgunError:
                assert not (form == "fast" and name == "mesh_glass"), "the small torus scene admits the fast mode"
                continue
            for views in batches:
                samples = int(views[0].samples_root) ** 2
                hits = view_hits(accel, views, w, h)  # (lg_intersect in this form)
                assert (hits["kind"] != 0).any() and (hits["kind"] == 0).any(), (name, form)
                got = G.capture_view_features(accel, views, w, h, material_rgb=table)
                compare(got, restate(hits, samples, table_rgb(hits, table)), (name, form, samples))
            checked.append(form)
    finally:
        reset(accel)
    assert "reference" in checked and "prune" in checked and ("lds" in checked or name != "cornell_glass") and ("fast" in checked or name != "mesh_glass")


# ---- 7: device form -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", (0, 1), ids=["S1", "S4"])
def test_device_form_on_a_torch_stream(ss):
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    views = [view_of(cam, ss) for cam in SECOND[1][3]]
    w, h = 45, 27
    table = random_table(accel)
    host = G.capture_view_features(accel, views, w, h, material_rgb=table)
    dtable = torch.from_numpy(table).cuda()
    dev = {p: torch.full((host[p].size * 4,), 0xA5, dtype=torch.uint8, device="cuda") for p in PLANES}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        G.capture_view_features_device(accel, views, w, h, dev["depth"].data_ptr(), dev["normal"].data_ptr(), dev["albedo"].data_ptr(), dev["coverage"].data_ptr(),
                                       dev["id"].data_ptr(), dev["point"].data_ptr(), dtable.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    stream.synchronize()
    for p in PLANES:
        assert dev[p].cpu().numpy().tobytes() == host[p].tobytes(), (ss, p)
    assert np.isinf(host["depth"]).any() and host["point"].any()


# ---- 8: errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_an_empty_batch_is_a_no_op():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(S.cornell_scene(G, "glass"))
    _, _, _, cameras = SECOND[1]
    w, h = 16, 16
    good = [view_of(cameras[0]), view_of(cameras[1])]
    pixels = 2 * w * h

    def edited(**kw):
        v = la.View.from_buffer_copy(bytes(good[1]))
        for k, x in kw.items():
            setattr(v, k, x)
        return (la.View * 2)(good[0], v)

    table = random_table(accel)
    dtable = torch.from_numpy(table).cuda()
    hbuf = guarded(pixels)
    dbuf = {p: torch.full((hbuf[p].size,), 0xA5, dtype=torch.uint8, device="cuda") for p in PLANES}
    torch.cuda.synchronize()
    hp = {p: hbuf[p].ctypes.data for p in PLANES}
    dp = {p: dbuf[p].data_ptr() for p in PLANES}
    ptr = lambda d, skip=(), shift={}: la.CViewFeatures(*[None if p in skip else d[p] + shift.get(p, 0) for p in PLANES])  # noqa: E731
    none = la.CViewFeatures()
    adr = ctypes.addressof
    t = (la.View * 2)(*good)
    big = (la.View * 4)(*([good[0]] * 4))

    def host(acc, views, k, ww, hh, f, tab):
        return G.call("capture_view_features", acc, adr(views) if views is not None else None, k, ww, hh, adr(f) if f is not None else None, tab)

    def device(acc, views, k, ww, hh, f, tab):
        return G.call("capture_view_features_device", acc, adr(views) if views is not None else None, k, ww, hh, adr(f) if f is not None else None, tab, None)

    for call, planes, tab in ((host, hp, table.ctypes.data), (device, dp, dtable.data_ptr())):
        f = ptr(planes)
        cases = [(None, t, 2, w, h, f, tab), (accel.h, None, 2, w, h, f, tab), (accel.h, t, 2, w, h, None, tab), (accel.h, t, 2, w, h, none, tab),
                 (accel.h, t, 2, w, h, f, None),                                            # albedo without material_rgb
                 (accel.h, t, 2, 0, h, f, tab), (accel.h, t, 2, w, 0, f, tab),
                 (accel.h, t, 1, 0xFFFFFFF9, 1, f, tab), (accel.h, t, 1, 1, 0xFFFFFFF9, f, tab),  # above 2^32 - 8
                 (accel.h, edited(samples_root=0), 2, w, h, f, tab), (accel.h, edited(samples_root=257), 2, w, h, f, tab),
                 (accel.h, edited(reserved=1), 2, w, h, f, tab), (accel.h, edited(samples_root=2), 2, w, h, f, tab),
                 (accel.h, big, 4, 1 << 18, 1 << 18, f, tab),   # 4 * 2^15 * 2^15 = 2^32 pixel tiles: one above the limit
                 (accel.h, t, (1 << 62), 8, 8, f, tab)]         # a byte size beyond SIZE_MAX (and more tiles than 2^32 - 1)
        for k, args in enumerate(cases):
            assert call(*args) != 0 and G.last_error(), (call.__name__, k)
        assert call(accel.h, t, 2, w, h, none, tab) != 0 and "every plane" in G.last_error(), call.__name__
        # n_views == 0: a successful no-op, answered before every other check
        assert call(None, None, 0, 0, 0, None, None) == 0 and call(accel.h, t, 0, w, h, f, tab) == 0 and call(None, t, 0, w, h, none, None) == 0, call.__name__
    # the device form's own: host memory where device memory is due, misaligned pointers, a plane that ends beyond its allocation
    dev_cases = [(t, 2, w, h, la.CViewFeatures(*[hp[q] if q == p else dp[q] for q in PLANES]), dtable.data_ptr()) for p in PLANES]
    dev_cases += [(t, 2, w, h, ptr(dp), table.ctypes.data)]
    dev_cases += [(t, 2, w, h, ptr(dp, shift={"id": 4}), dtable.data_ptr()), (t, 2, w, h, ptr(dp, shift={"id": 8}), dtable.data_ptr()),
                  (t, 2, w, h, ptr(dp, shift={"depth": 2}), dtable.data_ptr()), (t, 2, w, h, ptr(dp, shift={"normal": 1}), dtable.data_ptr()),
                  (t, 2, w, h, ptr(dp, shift={"albedo": 2}), dtable.data_ptr()), (t, 2, w, h, ptr(dp, shift={"coverage": 3}), dtable.data_ptr()),
                  (t, 2, w, h, ptr(dp, shift={"point": 2}), dtable.data_ptr()), (t, 2, w, h, ptr(dp), dtable.data_ptr() + 4)]
    # two films of 4096 x 4096: every plane would be 128 MiB and more, these buffers end long before
    dev_cases += [(t, 2, 4096, 4096, la.CViewFeatures(*[dp[q] if q == p else None for q in PLANES]), dtable.data_ptr()) for p in PLANES]
    for k, args in enumerate(dev_cases):
        assert device(accel.h, *args) != 0 and G.last_error(), ("device", k)
    torch.cuda.synchronize()
    for p in PLANES:
        assert (hbuf[p] == 0xA5).all() and (dbuf[p].cpu().numpy() == 0xA5).all(), (p, "an error or an empty batch touched an output")
    with pytest.raises(la.LasgunError):
        G.capture_view_features(accel, list(edited(samples_root=2)), w, h)
    with pytest.raises(ValueError):
        G.capture_view_features(accel, good, w, h, planes=("depth", "colour"))
    # material_rgb is ignored without albedo; and the calls still work after the errors: the restatement's bytes, the guards in place
    hits = view_hits(accel, good, w, h)
    want = restate(hits, 1, table_rgb(hits, table))
    for call, planes in ((host, hp), (device, dp)):
        assert call(accel.h, t, 2, w, h, ptr(planes, skip=("albedo",)), None) == 0, G.last_error()
    torch.cuda.synchronize()
    for p in PLANES:
        for got in (hbuf[p], dbuf[p].cpu().numpy()):
            assert (got[-GUARD:] == 0xA5).all(), p
            if p == "albedo":
                assert (got == 0xA5).all()
            else:
                a = bits32(got[:-GUARD].view(np.uint32 if p == "id" else np.float32).reshape((-1,) + SHAPE[p]))
                assert np.array_equal(a, bits32(want[p])), p
    # more than 32 lights is not an error here: nothing is shaded
    many = G.Accel.from_scene(many_lights_scene(G, 40))
    v = G.accel_view(many)
    got = G.capture_view_features(many, [v, v], w, h)
    mh = view_hits(many, [v, v], w, h)
    assert (mh["kind"] != 0).any() and (mh["kind"] == 0).any()
    compare(got, restate(mh, 1, table_rgb(mh, G.default_albedo_table(many))), "40 lights")
