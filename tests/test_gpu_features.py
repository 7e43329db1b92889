"""Feature buffers (include/lasgun_hip.h: lg_capture_features, lg_capture_features_device, lg_accel_material_count): depth, normal, albedo,
coverage and ids of the camera's primary hits, the rays made in the kernel.

The expected planes are computed in numpy from the library's older entry points -- hits = lg_intersect(lg_camera_rays(rect)), reshaped to
(pixels, S) -- by the contract's loop written out (a Python `for s`, vectorised over the pixels, in f64) and astype(float32), and compared
as BIT PATTERNS (NaNs canonicalised): no tolerance, no mismatch.

  1  every traversal form (the five (scene, form) pairs of test_gpu_visibility.FORMS), the full film, all planes, a random material_rgb;
  2  rectangles over a 0xA5 prefill: the whole film, partial tiles on all four sides, exactly one tile, a single pixel (one that hits, one
     that misses), one row, one column, and a 1032 x 1032 film (129 x 129 tiles: more than twice the waves of any grid -- the tile claim's
     other path), on a scene whose tiles are claimed per XCD band (resident in LDS) and on one with a single head;
  3  supersampling: S = 4 and S = 9 on the full film, S = 16 on a pixel set -- the sums in order, id from sample 0, the depth's own
     divisor.  (Camera::set_supersampling(n) makes (n + 1)^2 samples: simple_scene(supersampling=1, 2, 3).)
  4  the same planes from the CPU oracle's closest hits of the camera rays (orc_intersect in portable-trig mode, the entry
     tests/test_gpu_ray_query_edges.py pins lg_intersect to), a sphere scene and a mesh scene: bit for bit as well;
  5  plane subsets: each plane alone and depth + id give the all-planes bytes, unrequested planes keep their prefill, twice the same bytes;
  6  the device form on a torch stream that is not the default one: the host form's bytes;
  7  every error of the contract refused with every plane at its prefill; the empty rectangle a no-op; material_count;
  8  the wrapper's default_albedo_table against lg_accel_material.
Non-vacuity, asserted on lg_intersect's / the oracle's answer before anything is compared: in every scene of 1, 3 and 4 at least 10 % of
the pixels hit and at least 10 % miss, at least two kinds and three materials appear among the hits; in 3 at least 2 % of the pixels have
0 < coverage < 1.  (The Cornell shell's camera stands in front of the open box and sees past its walls: 23 % of the pixels miss.)"""
import ctypes
import hashlib

import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_visibility import FORMS, SCENES, reset, set_form

pytestmark = pytest.mark.gpu

G = la.api
W, H = 96, 64
PLANES = la.FEATURE_PLANES
SHAPE = {"depth": (), "normal": (3,), "albedo": (3,), "coverage": (), "id": (4,)}
BUILDERS = dict(SCENES)
BUILDERS.update({"simple_ss%d" % n: (lambda n: lambda api: S.simple_scene(api, n))(n) for n in (1, 2, 3)})


def bits32(a):
    """Bit patterns of a float32 / uint32 plane with every NaN canonicalised (as test_gpu_radiance_query.bits does for f64)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return a
    assert a.dtype == np.float32, a.dtype
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = np.uint32(0x7FC00000)
    return b


def prefill(w=W, h=H, planes=PLANES):
    """Planes full of 0xA5 bytes."""
    return {p: np.full((h, w) + SHAPE[p], 0xA5A5A5A5, dtype=np.uint32).view(np.uint32 if p == "id" else np.float32) for p in planes}


def untouched(arr):
    return np.ascontiguousarray(arr).view(np.uint8) == 0xA5


def expected(hits, samples, ray_rgb, id_material=None):
    """The contract's loop: hits (pixels * S) lg_hit records pixel-major, ray_rgb (pixels * S, 3) the colour a hit of that ray adds (rows
    of misses are never read), id_material: the material column of id (default: the hits' own).  Returns the five planes, (pixels, ...)."""
    h = hits.reshape(-1, samples)
    rgb = np.asarray(ray_rgb, dtype=np.float64).reshape(-1, samples, 3)
    n = h.shape[0]
    tsum, nsum, asum, nhit = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(samples):
            hs = h[:, s]
            hit = hs["kind"] != 0
            tsum = np.where(hit, tsum + hs["t"], tsum)
            nsum = np.where(hit[:, None], nsum + hs["ns"], nsum)
            asum = np.where(hit[:, None], asum + rgb[:, s, :], asum)
            nhit = nhit + hit
        inv = 1.0 / float(samples)
        mean_t = (tsum * (1.0 / np.maximum(nhit, 1).astype(np.float64))).astype(np.float32)
        out = {"depth": np.where(nhit > 0, mean_t, np.float32(np.inf)).astype(np.float32),
               "normal": (nsum * inv).astype(np.float32), "albedo": (asum * inv).astype(np.float32),
               "coverage": (nhit.astype(np.float64) * inv).astype(np.float32)}
    first = h[:, 0]
    mat = first["material"] if id_material is None else id_material
    out["id"] = np.stack([first["kind"], first["prim"], first["instance"], mat.astype(np.int32).view(np.uint32)], axis=1).astype(np.uint32)
    return out


def table_rgb(hits, table):
    """What a hit adds to asum by the contract: material_rgb[material], nothing for an index outside the table."""
    m = hits["material"].astype(np.int64)
    ok = (m >= 0) & (m < len(table))
    return np.where(ok[:, None], table[np.clip(m, 0, max(len(table) - 1, 0))], 0.0)


def random_table(accel, seed=11):
    return np.random.default_rng(seed).random((G.material_count(accel), 3))


def not_vacuous(hits, samples, ctx, partial=False):
    h = hits.reshape(-1, samples)
    cov = (h["kind"] != 0).mean(axis=1)
    assert (cov > 0).mean() >= 0.10 and (cov == 0).mean() >= 0.10, ("hit / miss fractions", (cov > 0).mean(), (cov == 0).mean(), ctx)
    hit = hits[hits["kind"] != 0]
    assert len(np.unique(hit["kind"])) >= 2, ("kinds among the hits", np.unique(hit["kind"]), ctx)
    if partial:
        assert ((cov > 0) & (cov < 1)).mean() >= 0.02, ("pixels with 0 < coverage < 1", ((cov > 0) & (cov < 1)).mean(), ctx)


def compare(got, want, rect, w, ctx, planes=PLANES):
    """got: film-shaped planes written over a prefill; want: compact planes of the rectangle.  Inside: the bits; outside: the prefill."""
    x0, y0, x1, y1 = rect
    for p in planes:
        g = got[p]
        inside = np.ascontiguousarray(g[y0:y1, x0:x1]).reshape((-1,) + SHAPE[p])
        a, b = bits32(inside), bits32(want[p])
        assert np.array_equal(a, b), (ctx, p, int((a != b).sum()), "of", a.size, "words differ; first at", np.argwhere(a != b)[:1].tolist())
        mask = np.ones(g.shape[:2], dtype=bool)
        mask[y0:y1, x0:x1] = False
        assert untouched(g[mask]).all(), (ctx, p, "a pixel outside the rectangle was touched")


_accels = {}


def accel_of(name):
    if name not in _accels:
        _accels[name] = G.Accel.from_scene(BUILDERS[name](G))
    return _accels[name]


_reference = {}


def reference(name, form="default", w=W, h=H, rect=None):
    """(hits of the rectangle's camera rays, S, table, expected planes), computed once per case and shared."""
    rect = (0, 0, w, h) if rect is None else rect
    key = (name, form, w, h, rect)
    if key not in _reference:
        accel = accel_of(name)
        samples = G.camera_samples(accel)
        hits = G.intersect(accel, G.camera_rays(accel, w, h, *rect))
        table = random_table(accel)
        _reference[key] = (hits, samples, table, expected(hits, samples, table_rgb(hits, table)))
    return _reference[key]


# ---- 1: every traversal form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_every_traversal_form_gives_the_contracts_planes(name, form):
    accel = accel_of(name)
    set_form(accel, form)
    try:
        hits, samples, table, want = reference(name, form)
        not_vacuous(hits, samples, (name, form))
        assert len(np.unique(hits["material"][hits["kind"] != 0])) >= 3, (name, "materials among the hits")
        got = G.capture_features(accel, W, H, material_rgb=table, into=prefill())
        compare(got, want, (0, 0, W, H), W, (name, form))
        assert np.isinf(got["depth"]).any() and (got["coverage"] == 1.0).any() and got["albedo"].any()
    finally:
        reset(accel)


# ---- 2: rectangles -----------------------------------------------------------------------------------------------------------------------
RECTS = [(0, 0, 96, 64), (3, 5, 20, 14), (8, 8, 16, 16), (0, 31, 96, 32), (47, 0, 48, 64), (41, 29, 50, 36), (41, 29, 54, 34)]  # (the last two: 63 and 65 pixels)


@pytest.mark.parametrize("name", ["cornell_glass", "instanced"])
def test_rectangles_leave_every_other_pixel_untouched(name):
    accel = accel_of(name)
    full = reference(name)[3]
    table = random_table(accel)
    cov = full["coverage"].reshape(H, W)
    ys, xs = np.nonzero(cov == 1.0)
    hit_px = (int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))
    ys, xs = np.nonzero(cov == 0.0)
    miss_px = (int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))
    singles = [(x, y, x + 1, y + 1) for x, y in (hit_px, miss_px)]
    for rect in RECTS + singles:
        x0, y0, x1, y1 = rect
        want = reference(name, rect=rect)[3]
        for p in PLANES:  # lg_intersect is a function of the ray: the rectangle's hits are the full film's
            sub = full[p].reshape((H, W) + SHAPE[p])[y0:y1, x0:x1].reshape((-1,) + SHAPE[p])
            assert np.array_equal(bits32(sub), bits32(want[p])), (name, rect, p)
        got = G.capture_features(accel, W, H, rect=rect, material_rgb=table, into=prefill())
        compare(got, want, rect, W, (name, rect))
    assert np.isfinite(full["depth"].reshape(H, W)[hit_px[1], hit_px[0]]) and np.isinf(full["depth"].reshape(H, W)[miss_px[1], miss_px[0]])


@pytest.mark.parametrize("name", ["cornell_glass", "instanced"])
def test_a_film_of_more_tiles_than_twice_the_grids_waves(name):
    w = h = 1032  # 129 x 129 tiles, a partial tile on the right and at the bottom
    accel = accel_of(name)
    assert G.camera_samples(accel) == 1
    hits = G.intersect(accel, G.camera_rays(accel, w, h))
    hit = hits[hits["kind"] != 0]  # (a square film of the Cornell shell sees next to no miss: the 96 x 64 cases carry the miss condition)
    assert len(np.unique(hit["kind"])) >= 2 and len(np.unique(hit["material"])) >= 3 and len(hit) >= len(hits) // 10, (name, len(hit))
    table = random_table(accel)
    want = expected(hits, 1, table_rgb(hits, table))
    got = G.capture_features(accel, w, h, material_rgb=table, into=prefill(w, h))
    compare(got, want, (0, 0, w, h), w, (name, w))


# ---- 3: supersampling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,samples,rect", [("simple_ss1", 4, None), ("simple_ss2", 9, None), ("simple_ss3", 16, (21, 9, 62, 40))],
                         ids=["S4", "S9", "S16-pixel-set"])
def test_supersampled_pixels_sum_their_samples_in_order(name, samples, rect):
    accel = accel_of(name)
    assert G.camera_samples(accel) == samples
    full_hits, _, table, _ = reference(name)
    not_vacuous(full_hits, samples, name, partial=True)
    assert len(np.unique(full_hits["material"][full_hits["kind"] != 0])) >= 3, (name, "materials among the hits")
    rect = (0, 0, W, H) if rect is None else rect
    hits, _, _, want = reference(name, rect=rect)
    h = hits.reshape(-1, samples)
    nhit = (h["kind"] != 0).sum(axis=1)
    part = (nhit > 0) & (nhit < samples)
    assert part.sum() >= 8, (name, rect, "pixels on an edge")
    first_differs = part & ((h["kind"][:, 0] != 0) != (h["kind"][:, -1] != 0))
    assert first_differs.any(), "id must come from sample 0 where the samples disagree"
    got = G.capture_features(accel, W, H, rect=rect, material_rgb=table, into=prefill())
    compare(got, want, rect, W, (name, rect))
    # the depth's own divisor: on an edge pixel tsum / nhit differs from tsum / S
    x0, y0, x1, y1 = rect
    depth = got["depth"][y0:y1, x0:x1].reshape(-1)
    tsum = np.where(h["kind"] != 0, h["t"], 0.0).sum(axis=1)
    k = np.nonzero(part)[0]
    assert np.allclose(depth[k], tsum[k] / nhit[k], rtol=1e-6) and not np.allclose(depth[k], tsum[k] / samples, rtol=1e-3)
    cov = got["coverage"][y0:y1, x0:x1].reshape(-1)
    assert np.array_equal(cov, (nhit / float(samples)).astype(np.float32))


# ---- 4: against the CPU oracle -------------------------------------------------------------------------------------------------------------
def pod_rgb(kind, p):
    """A colour that is a function of the material's POD alone (the oracle names a hit's material by its POD, the library by an index)."""
    d = hashlib.sha256(np.int64(kind).tobytes() + np.ascontiguousarray(p, dtype=np.float64).tobytes()).digest()
    return np.frombuffer(d[:24], dtype=np.uint64).astype(np.float64) / 2.0 ** 64


@pytest.mark.parametrize("name", ["simple_ss1", "instanced"], ids=["spheres", "mesh"])
def test_planes_equal_those_of_the_cpu_oracles_hits(name):
    accel = accel_of(name)
    samples = G.camera_samples(accel)
    rays = G.camera_rays(accel, W, H)
    o = oracle()
    oaccel = o.Accel.from_scene(BUILDERS[name](o))
    o.set_trig_mode(True)  # the sphere's trigonometry the device runs (its normals compare bit for bit)
    try:
        ohits, omats = o.intersect(oaccel, rays, 16)
    finally:
        o.set_trig_mode(False)
    not_vacuous(ohits, samples, (name, "oracle"), partial=samples > 1)
    hit = ohits["kind"] != 0
    pods = np.unique(np.concatenate([omats["kind"][hit, None].astype(np.float64), omats["p"][hit]], axis=1), axis=0)
    assert len(pods) >= 3, (name, "materials among the hits")
    colour = {row.tobytes(): pod_rgb(int(row[0]), row[1:]) for row in pods}
    ray_rgb = np.zeros((len(ohits), 3))
    keys = np.concatenate([omats["kind"][:, None].astype(np.float64), omats["p"]], axis=1)
    for i in np.nonzero(hit)[0]:
        ray_rgb[i] = colour[keys[i].tobytes()]
    lib = [G.accel_material(accel, i) for i in range(G.material_count(accel))]
    table = np.array([pod_rgb(m["kind"], m["p"]) for m in lib])
    got = G.capture_features(accel, W, H, material_rgb=table, into=prefill())
    # id's material column: the library's index must name the POD the oracle's sample 0 hit
    mat = got["id"][..., 3].reshape(-1).view(np.int32)
    first_hit, first_pod = hit.reshape(-1, samples)[:, 0], keys.reshape(-1, samples, 11)[:, 0]
    assert np.array_equal(mat == -1, ~first_hit)
    for i in np.nonzero(first_hit)[0]:
        m = lib[mat[i]]
        assert np.array([float(m["kind"])] + list(m["p"])).tobytes() == first_pod[i].tobytes(), (name, i)
    want = expected(ohits, samples, ray_rgb, id_material=mat)
    compare(got, want, (0, 0, W, H), W, (name, "oracle"))


# ---- 5: plane subsets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["instanced", "simple_ss1"])
def test_plane_subsets_give_the_all_planes_bytes(name):
    accel = accel_of(name)
    _, _, table, want = reference(name)
    rect = (5, 3, 90, 61)
    x0, y0, x1, y1 = rect
    every = G.capture_features(accel, W, H, rect=rect, material_rgb=table, into=prefill())
    again = G.capture_features(accel, W, H, rect=rect, material_rgb=table, into=prefill())
    for p in PLANES:
        assert every[p].tobytes() == again[p].tobytes(), (name, p, "the same call twice")
        sub = want[p].reshape((H, W) + SHAPE[p])[y0:y1, x0:x1]
        assert np.array_equal(bits32(every[p][y0:y1, x0:x1]), bits32(sub)), (name, p)
    for subset in [(p,) for p in PLANES] + [("depth", "id")]:
        buf = prefill()
        f = la.CFeatures(*[buf[p].ctypes.data if p in subset else None for p in PLANES])
        assert G.call("capture_features", accel.h, W, H, x0, y0, x1, y1, ctypes.addressof(f), table.ctypes.data if "albedo" in subset else None) == 0, G.last_error()
        for p in PLANES:
            if p in subset:
                assert buf[p].tobytes() == every[p].tobytes(), (name, subset, p)
            else:
                assert untouched(buf[p]).all(), (name, subset, p, "a plane that was not asked for was written")


# ---- 6: device form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference"), ("simple_ss1", "reference")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel = accel_of(name)
    set_form(accel, form)
    try:
        table = random_table(accel)
        dtable = torch.from_numpy(table).cuda()
        stream = torch.cuda.Stream()
        for rect in ((0, 0, W, H), (3, 5, 20, 14)):
            host = G.capture_features(accel, W, H, rect=rect, material_rgb=table, into=prefill())
            dev = {p: torch.from_numpy(a.view(np.uint8).copy()).cuda() for p, a in prefill().items()}
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                G.capture_features_device(accel, W, H, rect, dev["depth"].data_ptr(), dev["normal"].data_ptr(), dev["albedo"].data_ptr(), dev["coverage"].data_ptr(),
                                          dev["id"].data_ptr(), dtable.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            stream.synchronize()
            for p in PLANES:
                assert dev[p].cpu().numpy().tobytes() == host[p].tobytes(), (name, form, rect, p)
    finally:
        reset(accel)


# ---- 7: errors, the empty rectangle, material_count ----------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_an_empty_rectangle_is_a_no_op():
    torch = pytest.importorskip("torch")
    accel = accel_of("instanced")
    table = random_table(accel)
    dtable = torch.from_numpy(table).cuda()
    hbuf = prefill()
    dbuf = {p: torch.from_numpy(a.view(np.uint8).copy()).cuda() for p, a in prefill().items()}
    torch.cuda.synchronize()
    ptr = lambda d, skip=(), shift={}: la.CFeatures(*[None if p in skip else d[p] + shift.get(p, 0) for p in PLANES])  # noqa: E731
    hp = {p: hbuf[p].ctypes.data for p in PLANES}
    dp = {p: dbuf[p].data_ptr() for p in PLANES}
    none = la.CFeatures()
    full = (W, H, 0, 0, W, H)
    adr = ctypes.addressof

    def host(accel_h, dims, f, tab):
        return G.call("capture_features", accel_h, *dims, adr(f) if f is not None else None, tab)

    def device(accel_h, dims, f, tab):
        return G.call("capture_features_device", accel_h, *dims, adr(f) if f is not None else None, tab, None)

    bad_rects = [(W, H, 0, 0, W + 1, H), (W, H, 0, 0, W, H + 1), (W, H, 20, 0, 10, H), (W, H, 0, 30, W, 20), (0, 0, 0, 0, 1, 1)]
    huge = (8 << 16, 8 << 16, 0, 0, 8 << 16, 8 << 16)  # 65536 x 65536 tiles = 2^32
    for call, planes, tab in ((host, hp, table.ctypes.data), (device, dp, dtable.data_ptr())):
        f = ptr(planes)
        cases = [(None, full, f, tab), (accel.h, full, None, tab), (accel.h, full, none, tab), (accel.h, full, f, None), (accel.h, huge, f, tab)]
        cases += [(accel.h, r, f, tab) for r in bad_rects]
        for k, args in enumerate(cases):
            assert call(*args) != 0 and G.last_error(), (call.__name__, k)
        # the empty rectangle: success, nothing written, whatever the pointers
        for r in ((W, H, 5, 5, 5, 9), (W, H, 5, 5, 9, 5), (W, H, W, H, W, H), (0, 0, 0, 0, 0, 0)):
            assert call(accel.h, r, f, tab) == 0, (r, G.last_error())
    torch.cuda.synchronize()
    for p in PLANES:
        assert untouched(hbuf[p]).all() and untouched(dbuf[p].cpu().numpy()).all(), (p, "an error or an empty rectangle touched an output")
    hbuf2, dbuf2 = prefill(), {p: torch.from_numpy(a.view(np.uint8).copy()).cuda() for p, a in prefill().items()}
    hp2, dp2 = {p: hbuf2[p].ctypes.data for p in PLANES}, {p: dbuf2[p].data_ptr() for p in PLANES}
    torch.cuda.synchronize()
    # device form: host memory where device memory is due, misaligned pointers, a plane that ends beyond its allocation
    dev_cases = [(full, la.CFeatures(*[hp2[q] if q == p else dp2[q] for q in PLANES]), dtable.data_ptr()) for p in PLANES]
    dev_cases += [(full, ptr(dp2), table.ctypes.data)]
    dev_cases += [(full, ptr(dp2, shift={"id": 4}), dtable.data_ptr()), (full, ptr(dp2, shift={"id": 8}), dtable.data_ptr()),
                  (full, ptr(dp2, shift={"depth": 2}), dtable.data_ptr()), (full, ptr(dp2, shift={"normal": 1}), dtable.data_ptr()),
                  (full, ptr(dp2, shift={"albedo": 2}), dtable.data_ptr()), (full, ptr(dp2, shift={"coverage": 3}), dtable.data_ptr()),
                  (full, ptr(dp2), dtable.data_ptr() + 4)]
    big = (8192, 8192, 0, 0, 8, 1)  # eight pixels of a film whose planes would be 256 MiB and more: these buffers end long before
    dev_cases += [(big, la.CFeatures(*[dp2[q] if q == p else None for q in PLANES]), dtable.data_ptr()) for p in PLANES]
    for k, (dims, f, tab) in enumerate(dev_cases):
        assert device(accel.h, dims, f, tab) != 0 and G.last_error(), ("device", k)
    torch.cuda.synchronize()
    for p in PLANES:
        assert untouched(hbuf2[p]).all() and untouched(dbuf2[p].cpu().numpy()).all(), (p, "an error touched an output")
    # material_rgb is ignored without albedo
    for call, planes in ((host, hp2), (device, dp2)):
        assert call(accel.h, full, ptr(planes, skip=("albedo",)), None) == 0, G.last_error()
    torch.cuda.synchronize()
    assert untouched(hbuf2["albedo"]).all() and untouched(dbuf2["albedo"].cpu().numpy()).all()
    assert hbuf2["depth"].tobytes() == dbuf2["depth"].cpu().numpy().tobytes() and not untouched(hbuf2["depth"]).all()
    with pytest.raises(la.LasgunError):
        G.capture_features(accel, W, H, rect=(0, 0, W + 1, H))
    with pytest.raises(ValueError):
        G.capture_features(accel, W, H, planes=("depth", "colour"))
    # material_count: the first index lg_accel_material refuses
    n = G.material_count(accel)
    assert n >= 3
    G.accel_material(accel, n - 1)
    with pytest.raises(la.LasgunError):
        G.accel_material(accel, n)
    assert G.call("accel_material_count", None) == 0
    # and the call still works afterwards
    got = G.capture_features(accel, W, H, material_rgb=table, into=prefill())
    compare(got, reference("instanced")[3], (0, 0, W, H), W, "after the errors")


# ---- 8: the wrapper's default table ----------------------------------------------------------------------------------------------------------
def test_default_albedo_table_follows_the_materials():
    kinds = set()
    for name in ("instanced", "mesh_glass"):
        accel = accel_of(name)
        table = G.default_albedo_table(accel)
        assert table.shape == (G.material_count(accel), 3) and table.dtype == np.float64
        for i, row in enumerate(table):
            m = G.accel_material(accel, i)
            kinds.add(m["kind"])
            want = {0: m["p"][0:3], 1: m["p"][0:3], 2: (1.0, 1.0, 1.0), 3: m["p"][3:6], 4: m["p"][0:3]}[m["kind"]]
            assert tuple(row) == tuple(want), (name, i, m)
        hits, samples, _, _ = reference(name)
        got = G.capture_features(accel, W, H, planes=("albedo",))  # material_rgb=None: the default table
        want = expected(hits, samples, table_rgb(hits, table))["albedo"]
        assert np.array_equal(bits32(got["albedo"].reshape(-1, 3)), bits32(want)), name
        assert np.array_equal(accel.features(W, H, planes=("albedo",))["albedo"], got["albedo"])
    assert kinds == {0, 1, 2, 3, 4}, kinds  # matte, plastic, metal, glass, mirror
