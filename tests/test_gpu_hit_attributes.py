"""Hit attributes (include/lasgun_hip.h: lg_hit_attributes*, lg_hit_attributes_of*) on the device.

  1  every plane against the reference evaluator (tests/attr_ref.py, with the device's own atan2 / acos / sin / cos) on the films of
     tests/attr_cases.py, bit for bit under the NaN rule; hits against lg_intersect's bytes;
  2  three restatements in numpy from the planes alone, bit for bit: ts == cross(ns, ss); ng == face_forward(normalize(cross(gu, gv)), wo);
     lg_scatter's transmitted direction through pyref's BSDF from frame + ns;
  3  the three closed forms (barycentric sum, vertex blend, local -> world) within the witness's own worst on the same film plus 4 ulps;
  4  _of on lg_intersect's records and on lg_hit_layers' layers 0-2 equals the walking form; a wrong ray gives NO_HIT, a record that
     names nothing BAD_RECORD, with the guard words around the planes intact;
  5  shapes, both orders, every traversal form, more tiles than twice the grid's waves, each plane alone and subsets over garbage, the
     device forms on a second stream between guard words, the edge-case rays, 40 lights;
  6  every error of the contract -- a buffer that ends beyond its allocation and the limits on n included --, nothing touched."""
import ctypes
import functools

import numpy as np
import pytest

import attr_cases as C
import attr_ref as R
import edge_rays as E
import lasgun_amd as la
import pyref
from test_gpu_radiance_query import each_form, many_lights_scene

pytestmark = pytest.mark.gpu

G = la.api
PLANES = la.ATTR_PLANES
OF_PLANES = PLANES[1:]
WORDS = {"hits": 24, "flags": 1, "bary": 6, "uv": 4, "local": 6, "frame": 12, "dp": 12}  # uint32 words a row
GUARD, FILL = 64, 0x25A5A5A5
ULP = 2.0 ** -52


def words(a):
    return a.view(np.uint32) if a.dtype != np.uint32 else a


def same(ctx, got, want, planes):
    """Bit for bit, except that a NaN is SOME NaN (the header's NaN rule); hits compare as bytes where asked to (same_bytes)."""
    for p in planes:
        if p == "hits":
            for f in ("t", "p", "ng", "ns"):
                assert R.same_planes(got[p][f], want[p][f]), (ctx, p, f)
            for f in ("kind", "prim", "instance", "material"):
                assert np.array_equal(got[p][f], want[p][f]), (ctx, p, f)
        else:
            assert R.same_planes(got[p], want[p]), (ctx, p, np.nonzero(np.atleast_2d((words(np.ascontiguousarray(got[p])) != words(np.ascontiguousarray(want[p]))).reshape(len(got[p]), -1)).any(axis=1))[0][:5])


@functools.lru_cache(maxsize=None)
def film(name):
    """(accel, catalog, rays, lg_intersect's hits, the walking form's planes, the reference's planes) of a scene of attr_cases, once."""
    builder, (w, h) = next((b, wh) for n, b, wh in C.SCENES if n == name)
    pscene = builder(pyref.Api)
    accel = G.Accel.from_scene(builder(G))
    cat = R.Catalog(pscene)
    rays = C.film_rays(pscene, w, h)
    hits = G.intersect(accel, rays)
    got = G.hit_attributes(accel, rays)
    with R.trig(G):
        want = R.planes(cat, rays, hits)
    return accel, cat, rays, hits, got, want


ALL = [s[0] for s in C.SCENES]


# ---- 1: the planes are the reference's, the record is lg_intersect's --------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_every_plane_is_the_references_and_hits_is_lg_intersects(name):
    accel, cat, rays, hits, got, want = film(name)
    hit = hits["kind"] != 0
    assert hit.any() and (name == "extra" or not hit.all()), name  # (the extra scene's camera sits inside a sphere: every ray hits)
    assert got["hits"].tobytes() == hits.tobytes(), (name, "hits is lg_intersect's record, the same bytes")
    assert np.array_equal(got["flags"], np.where(hit, la.ATTR_HIT, 0)), name
    same(name, got, want, OF_PLANES)
    for p in OF_PLANES[1:]:
        assert not words(np.ascontiguousarray(got[p][~hit])).any(), (name, p, "a miss writes +0.0")
    assert not np.isnan(got["uv"]).all() and not np.isnan(got["frame"][hit]).any(), name


def test_the_device_films_hold_every_class():
    seen = set()
    for name in ALL:
        accel, cat, rays, hits, _, _ = film(name)
        seen |= C.classes(cat, rays, hits)
        r1 = C.continuation(rays, hits)
        seen |= C.classes(cat, r1, G.intersect(accel, r1))
    assert seen >= C.WANTED, sorted(C.WANTED - seen)


# ---- 2: restatements from the planes alone -------------------------------------------------------------------------------------------------
def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize(a):
    return a * (1.0 / np.sqrt(dot(a, a)))[:, None]


@pytest.mark.parametrize("name", ALL)
def test_the_frame_and_the_geometric_normal_restate_from_the_planes(name):
    _, _, rays, hits, got, _ = film(name)
    hit = hits["kind"] != 0
    ns, ng = hits["ns"][hit], hits["ng"][hit]
    ss, ts = got["frame"][hit, :3], got["frame"][hit, 3:]
    gu, gv = got["dp"][hit, :3], got["dp"][hit, 3:]
    assert R.same_planes(ts, cross(ns, ss)), (name, "ts == cross(ns, ss)")
    wo = -normalize(rays[hit, 3:])
    n = normalize(cross(gu, gv))
    n = np.where((dot(n, wo) < 0.0)[:, None], -n, n)
    assert R.same_planes(ng, n), (name, "ng == face_forward(normalize(cross(gu, gv)), wo)")


def test_lg_scatters_transmitted_direction_restates_through_the_bsdf():
    """The one round 22 could not pin: refract's direction is bsdf.sample_f(wo, TRANSMISSION | SPECULAR).wi, and the BSDF's frame is
    (ss, ts, ns) -- here ss and ts come from lg_hit_attributes' frame, ns from the record."""
    from test_gpu_scatter import classes_scene
    accel = G.Accel.from_scene(classes_scene(G))
    rays = G.camera_rays(accel, 96, 64)
    sc = G.scatter(accel, rays, ("hits", "flags", "refract"))
    at = G.hit_attributes(accel, rays, ("hits", "frame"))
    assert at["hits"].tobytes() == sc["hits"].tobytes()
    idx = np.nonzero(sc["flags"] & la.SCATTER_REFRACT)[0]
    assert len(idx) >= 100
    checked = 0
    for i in idx:
        h = sc["hits"][i]
        m = G.accel_material(accel, int(h["material"]))
        assert m["kind"] == 3
        p = [float(v) for v in m["p"]]
        bx = pyref.scattering(pyref.Material.glass(p[0:3], p[3:6], p[6]))
        ns, ss = tuple(map(float, h["ns"])), tuple(map(float, at["frame"][i, :3]))
        bsdf = pyref.BSDF(tuple(map(float, h["ng"])), ns, ss, bx)
        assert np.array(bsdf.ts).tobytes() == at["frame"][i, 3:].tobytes()
        wo = pyref.neg(pyref.normalize(tuple(map(float, rays[i, 3:]))))
        _, wi, pdf = bsdf.sample_f(wo, 2 | 16)
        assert pdf > 0.0 and np.array(wi).tobytes() == sc["refract"][i, 3:].tobytes(), (i, wi, sc["refract"][i, 3:])
        checked += 1
    assert checked == len(idx)


# ---- 3: the closed forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.FILMS)
def test_the_closed_forms_stay_within_the_witness_worst_plus_4_ulps(name):
    _, cat, rays, hits, got, want = film(name)
    device, witness = R.closed_forms(cat, hits, got), R.closed_forms(cat, hits, want)
    print("closed forms, %s: device %r witness %r" % (name, device, witness))
    scale = max(1.0, float(np.abs(hits["p"][hits["kind"] != 0]).max()))  # an ulp of the largest coordinate compared
    for key in device:
        margin = 4 * ULP * (1.0 if key == "bary_sum" else scale)
        assert device[key] <= witness[key] + margin, (name, key, device[key], witness[key])


# ---- 4: the _of form --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_of_on_lg_intersects_records_is_the_walking_form(name):
    accel, _, rays, hits, got, _ = film(name)
    of = G.hit_attributes_of(accel, rays, hits)
    for p in OF_PLANES:
        assert of[p].tobytes() == got[p].tobytes(), (name, p)
    scrubbed = hits.copy()  # only kind, prim and instance are read
    scrubbed["t"], scrubbed["p"], scrubbed["ng"], scrubbed["ns"], scrubbed["material"] = np.nan, 7.0, -1.0, 0.0, 12345
    again = G.hit_attributes_of(accel, rays, scrubbed)
    assert all(again[p].tobytes() == got[p].tobytes() for p in OF_PLANES), name


@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass"])
def test_of_on_the_layers_of_lg_hit_layers_is_the_walking_form_on_the_segments(name):
    accel, _, rays, hits, _, _ = film(name)
    layers = G.hit_layers(accel, rays, 3, ("hits",))["hits"]
    assert layers[0].tobytes() == hits.tobytes()
    seg, alive, deeper = rays, np.arange(len(rays)), 0
    for j in range(3):
        rec = np.ascontiguousarray(layers[j][alive])
        walked = G.hit_attributes(accel, seg)
        assert walked["hits"].tobytes() == rec.tobytes(), (name, j, "the segment rebuilt in numpy is the one the layers walked")
        of = G.hit_attributes_of(accel, seg, rec)
        assert all(of[p].tobytes() == walked[p].tobytes() for p in OF_PLANES), (name, j)
        deeper += int((rec["kind"] != 0).sum()) if j else 0
        keep = rec["kind"] != 0
        seg = np.ascontiguousarray(np.concatenate([rec["p"][keep] - rec["ng"][keep] * C.STEP, seg[keep, 3:]], axis=1))
        alive = alive[keep]
    assert deeper > 200, (name, deeper)


def test_a_wrong_ray_gives_no_hit_and_a_bad_record_bad_record_between_guard_words():
    torch = pytest.importorskip("torch")
    accel, cat, rays, hits, got, _ = film("kitchen_sink")
    pick = np.concatenate([np.nonzero(hits["kind"] == k)[0][:40] for k in (1, 2, 3)])
    r, rec = rays[pick].copy(), hits[pick].copy()
    n = len(pick)
    # wrong rays: far away, pointing off
    wrong = r.copy()
    wrong[:, :3] = [60.0, 70.0, 80.0]
    wrong[:, 3:] = [0.0, 1.0, 0.0]
    of = G.hit_attributes_of(accel, wrong, rec)
    assert (of["flags"] == la.ATTR_NO_HIT).all()
    assert all(not words(np.ascontiguousarray(of[p])).any() for p in OF_PLANES[1:])
    # bad records: the ones attr_record_ok refused on the CPU (tools/attributes_host_check.cpp): kind 7, prim == the count, instance == the count, a sphere in the wrong instance
    bad = rec.copy()
    tri = int(np.nonzero(rec["kind"] == 3)[0][0])
    faces = len(cat.accels[int(rec[tri]["instance"])]["mesh"][0].polys)
    bad["kind"][0::4] = 7
    bad["prim"][1::4] = np.where(bad["kind"][1::4] == 1, len(cat.spheres), np.where(bad["kind"][1::4] == 2, len(cat.cuboids), 0xFFFFFFFF))
    bad["instance"][2::4] = len(cat.accels)
    third = np.arange(n)[3::4]
    bad["instance"][third] = np.where(bad["instance"][third] == 0, 1, 0)  # the primitive in an accel it does not sit in (a mesh's face count differs, or it is a group)
    bad["kind"][tri], bad["prim"][tri], bad["instance"][tri] = 3, faces, rec[tri]["instance"]
    expect = np.array([R.attributes(cat, r[i], int(bad[i]["kind"]), int(bad[i]["prim"]), int(bad[i]["instance"]))[0] for i in range(n)], dtype=np.uint32)
    assert (expect == R.BAD_RECORD).sum() >= n - n // 4 - 2 and expect[tri] == R.BAD_RECORD, expect
    host = G.hit_attributes_of(accel, r, bad)
    assert np.array_equal(host["flags"], expect)
    isbad = expect == R.BAD_RECORD
    assert all(not words(np.ascontiguousarray(host[p][isbad])).any() for p in OF_PLANES[1:])
    # ... and on the device between guard words
    dr, dh = torch.from_numpy(r).cuda(), torch.from_numpy(bad.view(np.uint8).reshape(n, 96)).cuda()
    dev = {p: torch.full((GUARD + n * WORDS[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in OF_PLANES}
    torch.cuda.synchronize()
    G.hit_attributes_of_device(accel, n, dr.data_ptr(), dh.data_ptr(), stream=0, **{p + "_ptr": dev[p].data_ptr() + 4 * GUARD for p in OF_PLANES})
    torch.cuda.synchronize()
    for p in OF_PLANES:
        back = dev[p].cpu().numpy().view(np.uint32)
        assert (back[:GUARD] == FILL).all() and (back[GUARD + n * WORDS[p]:] == FILL).all(), (p, "the guard words are intact")
        assert back[GUARD:GUARD + n * WORDS[p]].tobytes() == host[p].tobytes(), p


# ---- 5: shapes, orders, forms, subsets, streams, edge rays -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4097])
def test_shapes_and_both_orders(n):
    accel, _, rays, hits, got, _ = film("instanced")
    idx = (np.arange(n) * 37) % len(rays)
    r = np.ascontiguousarray(rays[idx])
    for order in (0, 1):
        G.set_query_order(accel, order)
        try:
            out = G.hit_attributes(accel, r)
            of = G.hit_attributes_of(accel, r, hits[idx])
        finally:
            G.set_query_order(accel, 0)
        for p in PLANES:
            assert out[p].tobytes() == got[p][idx].tobytes(), (n, order, p)
        for p in OF_PLANES:
            assert of[p].tobytes() == got[p][idx].tobytes(), (n, order, p)


@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass"])
def test_every_traversal_form_gives_the_same_bytes(name):
    """In every form the record is lg_intersect's in that form and the planes are _of's on those records (which walks nothing); the exact
    forms give the reference form's bytes; where the fast mode settles an exact tie its own way, those rows are held to attr_ref."""
    builder = next(b for n, b, _ in C.SCENES if n == name)
    accel = G.Accel.from_scene(builder(G))
    _, cat, rays, _, got, _ = film(name)
    forms = []
    for form in each_form(accel):
        forms.append(form)
        out = G.hit_attributes(accel, rays)
        hits = G.intersect(accel, rays)
        assert out["hits"].tobytes() == hits.tobytes(), (name, form, "hits is lg_intersect's record in the same form")
        of = G.hit_attributes_of(accel, rays, hits)
        assert all(out[p].tobytes() == of[p].tobytes() for p in OF_PLANES), (name, form, "the planes are _of's on those records")
        if form == "fast":
            rows = (out["hits"].view(np.uint8).reshape(len(rays), 96) == got["hits"].view(np.uint8).reshape(len(rays), 96)).all(axis=1)
            assert rows.mean() > 0.99, (name, form)
            assert all(out[p][rows].tobytes() == got[p][rows].tobytes() for p in PLANES), (name, form)
            other = np.nonzero(~rows)[0]
            print("fast form, %s: %d rows whose record differs from the reference form's" % (name, len(other)))
            if len(other):
                with R.trig(G):
                    want = R.planes(cat, rays[other], hits[other])
                same((name, form, "the rows the fast mode settles its own way"), {p: out[p][other] for p in OF_PLANES}, want, OF_PLANES)
        else:
            assert all(out[p].tobytes() == got[p].tobytes() for p in PLANES), (name, form)
    assert "reference" in forms and "prune" in forms, forms


def test_more_tiles_than_twice_the_grids_waves():
    """LDS form: one 1024-lane workgroup per CU, 16 waves each; the film repeated until its 64-ray tiles pass 2 x 16 x CUs."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    accel, _, rays, _, got, _ = film("cornell_glass")
    reps = 1
    while (reps * len(rays) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    big = np.ascontiguousarray(np.tile(rays, (reps, 1)))
    out = G.hit_attributes(accel, big, ("hits", "uv", "bary", "frame"))
    for p in out:
        assert out[p].tobytes() == np.tile(got[p], (reps,) + (1,) * (got[p].ndim - 1)).tobytes(), (p, reps)


SUBSETS = [(p,) for p in PLANES] + [("uv", "bary"), ("hits", "dp"), ("flags", "local", "frame")]


def test_each_plane_alone_and_subsets_over_garbage():
    accel, _, rays, hits, got, _ = film("kitchen_sink")
    n = 64 * 20 + 9
    r = np.ascontiguousarray(rays[1000:1000 + n])
    rng = np.random.default_rng(5)
    for planes in SUBSETS:
        bufs = {p: rng.integers(1, 2 ** 32, n * WORDS[p], dtype=np.uint64).astype(np.uint32).view(got[p].dtype).reshape((n,) + got[p].shape[1:]) for p in PLANES}
        for p in PLANES:
            if p not in planes:
                words(bufs[p])[...] = 0xA5A5A5A5
        out = G.hit_attributes(accel, r, planes, into={p: bufs[p] for p in planes})
        assert all(out[p] is bufs[p] and out[p].tobytes() == got[p][1000:1000 + n].tobytes() for p in planes), planes
        assert all((words(bufs[p]) == 0xA5A5A5A5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", planes)
        if "hits" not in planes:
            for p in planes:
                words(bufs[p])[...] = 0x5A5A5A5A
            of = G.hit_attributes_of(accel, r, hits[1000:1000 + n], planes, into={p: bufs[p] for p in planes})
            assert all(of[p].tobytes() == got[p][1000:1000 + n].tobytes() for p in planes), planes
    assert list(accel.hit_attributes(r[:5], ("uv", "bary"))) == ["uv", "bary"]


@pytest.mark.parametrize("name", ["cornell_glass", "instanced"])
def test_the_device_forms_on_a_second_stream_between_guard_words(name):
    torch = pytest.importorskip("torch")
    accel, _, rays, hits, got, _ = film(name)
    n = len(rays)
    drays = torch.from_numpy(rays).cuda()
    dhits = torch.from_numpy(hits.view(np.uint8).reshape(n, 96).copy()).cuda()
    stream = torch.cuda.Stream()
    for of_form in (False, True):
        for planes in ((OF_PLANES if of_form else PLANES), ("uv", "bary"), ("frame",)):
            dev = {p: torch.full((GUARD + n * WORDS[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                s = torch.cuda.current_stream().cuda_stream
                assert s != 0
                ptrs = {p + "_ptr": dev[p].data_ptr() + 4 * GUARD for p in planes}
                for _ in range(2):  # the second call runs over the first one's results
                    if of_form:
                        G.hit_attributes_of_device(accel, n, drays.data_ptr(), dhits.data_ptr(), stream=s, **ptrs)
                    else:
                        G.hit_attributes_device(accel, n, drays.data_ptr(), stream=s, **ptrs)
            stream.synchronize()
            for p in PLANES:
                back = dev[p].cpu().numpy().view(np.uint32)
                if p in planes:
                    assert (back[:GUARD] == FILL).all() and (back[GUARD + n * WORDS[p]:] == FILL).all(), (name, of_form, p, "nothing is written outside the plane")
                    assert back[GUARD:GUARD + n * WORDS[p]].tobytes() == got[p].tobytes(), (name, of_form, planes, p)
                else:
                    assert (back == FILL).all(), (name, of_form, planes, p, "not asked for")


@pytest.mark.parametrize("case", ["f3", "f7", "grid"])
def test_the_edge_case_rays(case):
    """tests/edge_rays.py's families: the record is lg_intersect's, _of on it is the walking form, the frame restates -- NaNs as NaNs --, and
    every hit of a ray whose components are all finite is held to attr_ref (the witness computes in Python floats: a ray on which Python
    raises where IEEE answers is counted, and there are few)."""
    scene, bounds, boxes = {"f3": (E.f3_scene, E.F3_BOUNDS, E.F3_BOXES), "f7": (E.f7_scene, E.F7_BOUNDS, E.F7_BOXES), "grid": (E.grid_scene, E.GRID_BOUNDS, E.GRID_BOXES)}[case]
    accel = G.Accel.from_scene(scene(G))
    rays = np.ascontiguousarray(E.edge_rays(*bounds, boxes=boxes, mesh=(case == "grid"), huge=(case == "f7"), seed=3)[0])
    hits = G.intersect(accel, rays)
    out = G.hit_attributes(accel, rays)
    same(case, out, {"hits": hits}, ("hits",))
    hit = hits["kind"] != 0
    assert hit.any(), case
    assert np.array_equal(out["flags"], np.where(hit, la.ATTR_HIT, 0))
    of = G.hit_attributes_of(accel, rays, hits)
    same((case, "_of"), of, out, OF_PLANES)
    assert R.same_planes(out["frame"][hit, 3:], cross(hits["ns"][hit], out["frame"][hit, :3])), (case, "ts == cross(ns, ss)")
    for p in OF_PLANES[1:]:
        assert not words(np.ascontiguousarray(out[p][~hit])).any(), (case, p)
    # ... and against the reference evaluator
    cat = R.Catalog(scene(pyref.Api))
    finite = np.nonzero(hit & np.isfinite(rays).all(axis=1))[0]
    assert len(finite) >= 100, (case, len(finite))
    raised, kinds = 0, set()
    with R.trig(G):
        for i in finite:
            h = hits[i]
            try:
                flags, at = R.attributes(cat, rays[i], int(h["kind"]), int(h["prim"]), int(h["instance"]))
            except (ZeroDivisionError, OverflowError, ValueError):
                raised += 1
                continue
            assert flags == R.HIT, (case, i, rays[i], flags)
            kinds.add(int(h["kind"]))
            for p, _ in R.PLANES:
                assert R.same_planes(out[p][i], np.array(at[p], dtype=np.float64)), (case, i, p, rays[i], out[p][i], at[p])
    print("edge rays, %s: %d finite hits against attr_ref, Python raised on %d" % (case, len(finite), raised))
    assert raised * 20 <= len(finite), (case, raised, len(finite))
    assert kinds >= ({1, 2, 3} if case == "grid" else {1, 2}), (case, kinds)


def test_a_scene_of_40_lights_is_accepted():
    accel = G.Accel.from_scene(many_lights_scene(G, 40))
    rays = G.camera_rays(accel, 16, 16)
    out = G.hit_attributes(accel, rays)
    hit = out["hits"]["kind"] != 0
    assert hit.any() and not hit.all() and (out["flags"][hit] == la.ATTR_HIT).all()
    assert ((out["uv"][hit] >= 0.0) & (out["uv"][hit] <= 1.0)).all()


# ---- 6: errors ------------------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_and_nothing_is_touched():
    torch = pytest.importorskip("torch")
    accel, _, rays, hits, _, _ = film("cornell_glass")
    n = 100
    r, h = np.ascontiguousarray(rays[:n]), np.ascontiguousarray(hits[:n])
    dr = torch.from_numpy(rays[:n + 1].copy()).cuda()
    dh = torch.from_numpy(hits[:n + 1].view(np.uint8).reshape(n + 1, 96).copy()).cuda()
    dev = {p: torch.full(((n + 1) * WORDS[p],), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
    host = {p: np.full(n * WORDS[p], 0xA5A5A5A5, dtype=np.uint32) for p in PLANES}
    torch.cuda.synchronize()
    ptrs = {p + "_ptr": dev[p].data_ptr() for p in PLANES}
    of_ptrs = {k: v for k, v in ptrs.items() if k != "hits_ptr"}
    # For "a buffer that ends beyond its allocation" the buffer has to BE an allocation: torch hands small tensors out of blocks of its own,
    # and the library can only see where a block ends (hipMemGetAddressRange).  12 MiB are a block of their own (tests/test_gpu_scatter.py
    # does the same): 2^17 records, 2^18 rows of dp; the call asks for one row more.
    torch.cuda.empty_cache()
    many, many_dp = 1 << 17, 1 << 18
    short_hits = torch.full((many * 24,), FILL, dtype=torch.int32, device="cuda")
    short_dp = torch.full((many_dp * 12,), FILL, dtype=torch.int32, device="cuda")
    long_rays = torch.zeros((many_dp + 1, 6), dtype=torch.float64, device="cuda")
    long_rays[:, 5] = 1.0
    long_recs = torch.zeros(((many_dp + 1) * 24,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    shorts = [("hits", lambda: G.hit_attributes_device(accel, many + 1, long_rays, hits_ptr=short_hits, stream=0)),
              ("dp", lambda: G.hit_attributes_device(accel, many_dp + 1, long_rays, dp_ptr=short_dp, stream=0)),
              ("hits", lambda: G.hit_attributes_of_device(accel, many + 1, long_rays, short_hits, flags_ptr=long_recs, stream=0)),     # short records
              ("dp", lambda: G.hit_attributes_of_device(accel, many_dp + 1, long_rays, long_recs, dp_ptr=short_dp, stream=0))]
    for k, (what, call) in enumerate(shorts):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert what + " ends beyond its allocation" in str(e.value), (k, str(e.value))
    G.hit_attributes_device(accel, many, long_rays, hits_ptr=short_hits, stream=0)  # (exactly its size is accepted ...
    torch.cuda.synchronize()
    assert not bool((short_hits == FILL).all())
    short_hits.fill_(FILL)                                                           # ... and the refusals below leave it alone)
    torch.cuda.synchronize()
    walk = lambda rp, count=n, **kw: G.hit_attributes_device(accel, count, rp, stream=0, **dict(ptrs, **kw))  # noqa: E731
    of_ = lambda rp, hp, count=n, **kw: G.hit_attributes_of_device(accel, count, rp, hp, stream=0, **dict(of_ptrs, **kw))  # noqa: E731
    bad = [lambda: walk(0),
           lambda: G.hit_attributes_device(accel, n, dr.data_ptr(), stream=0),                    # all planes NULL
           lambda: walk(dr.data_ptr() + 4),                                                       # rays: 8 bytes
           lambda: walk(r.ctypes.data),                                                           # host rays
           lambda: walk(dr, count=0xFFFFFFFF * 64 + 1),                                           # n > (2^32 - 1) * 64
           lambda: walk(dr, count=1 << 62),                                                       # a plane's bytes do not fit size_t
           lambda: of_(dr, 0),                                                                    # no records
           lambda: of_(dr, dh.data_ptr() + 8),                                                    # records: 16 bytes
           lambda: of_(dr, h.ctypes.data),                                                        # host records
           lambda: of_(dr, dh, count=0xFFFFFFFF * 64 + 1),
           lambda: of_(dr, dh, count=1 << 62),
           lambda: G.hit_attributes_of_device(accel, n, dr.data_ptr(), dh.data_ptr(), stream=0)]  # all planes NULL
    for p in PLANES:
        align = 16 if p == "hits" else 4 if p == "flags" else 8
        bad.append(lambda p=p, align=align: walk(dr, **{p + "_ptr": dev[p].data_ptr() + align // 2}))   # misaligned
        bad.append(lambda p=p: walk(dr, **{p + "_ptr": host[p].ctypes.data}))                             # a host pointer
        if p != "hits":
            bad.append(lambda p=p, align=align: of_(dr, dh, **{p + "_ptr": dev[p].data_ptr() + align // 2}))
            bad.append(lambda p=p: of_(dr, dh, **{p + "_ptr": host[p].ctypes.data}))
    for k, call in enumerate(bad + [c for _, c in shorts]):
        try:
            call()
        except la.LasgunError as e:
            assert str(e), k
        else:
            raise AssertionError("call %d of the list was not refused" % k)
    torch.cuda.synchronize()
    assert bool((short_hits == FILL).all()) and bool((short_dp == FILL).all()) and not bool(long_recs.any()), "the short buffers and their neighbours keep their fill"
    with_hits = la.CAttrOut(*[dev[p].data_ptr() for p in PLANES])  # the _of form with a hits plane
    assert G.call("hit_attributes_of_device", accel.h, dr.data_ptr(), dh.data_ptr(), n, ctypes.addressof(with_hits), None) != 0 and "out->hits" in G.last_error()
    host_out = la.CAttrOut(*[host[p].ctypes.data for p in PLANES])
    assert G.call("hit_attributes_of", accel.h, r.ctypes.data, h.ctypes.data, n, ctypes.addressof(host_out)) != 0 and "out->hits" in G.last_error()
    assert G.call("hit_attributes", accel.h, None, n, ctypes.addressof(host_out)) != 0 and "rays is NULL" in G.last_error()
    assert G.call("hit_attributes", accel.h, r.ctypes.data, n, None) != 0 and "out is NULL" in G.last_error()
    torch.cuda.synchronize()
    assert all((dev[p].cpu().numpy().view(np.uint32) == FILL).all() for p in PLANES), "no device output touched"
    assert all((host[p] == 0xA5A5A5A5).all() for p in PLANES)
    with pytest.raises(ValueError):
        G.hit_attributes_of(accel, r, h[:5])
    # and after all that the accel still answers
    assert G.hit_attributes(accel, r, ("hits",))["hits"].tobytes() == h.tobytes()
