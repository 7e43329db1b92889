"""Closest points (include/lasgun_hip.h: lg_closest_points*) on the device, bit for bit against the brute force over all primitives
(tests/closest_ref.py) on the scenes and points of tests/closest_cases.py -- nothing is tolerated.

   1  every plane equals the brute force, with radius in {+INF, 0, the median distance, 2^-20};
   2  n in {0, 1, 63, 64, 65, 129, 4097};
   3  one call of more tiles than twice the grid's waves equals its 4097-point pieces;
   4  every traversal mode of the accel, and the sorted query order, give the same bytes;
   5  each plane alone, and subsets over garbage, leave the other buffers intact;
   6  the device form on a second stream between guard words;
   7  the material of every row is the brute force's (case 1); material equals lg_intersect's on the ray from q to point, wherever that ray's first hit names the same primitive (count printed);
      lg_intersect's own hit points as query points equal the brute force too;
   8  signed_distance against the closed form for one sphere and one box;
   9  a scene with 40 lights is accepted;
  10  every error leaves its outputs untouched; the depth-8 scenes match the brute force or are refused exactly where the gate says."""
import functools

import numpy as np
import pytest

import closest_cases as C
import closest_ref as R
import lasgun_amd as la
import pyref
from test_gpu_radiance_query import each_form, many_lights_scene
from test_gpu_ray_query import same_material

pytestmark = pytest.mark.gpu

G = la.api
PLANES = la.CLOSEST_PLANES
WORDS = {"distance": 2, "point": 6, "id": 4}  # uint32 words a row
GUARD, FILL = 64, 0x25A5A5A5
INF = float("inf")


@functools.lru_cache(maxsize=None)
def accel_of(name):
    return G.Accel.from_scene(C.builder(name)(G))


def same(ctx, got, want, accel=None, brute=None):
    """distance and point bit for bit; kind, prim, instance against the brute force; with (accel, brute) the material word of EVERY row too:
    the Material behind the library's index is the brute force's for that winner (a table index itself is the library's own)."""
    if accel is not None:
        table = {int(i): G.accel_material(accel, int(i)) for i in np.unique(got["id"][:, 3]) if i != 0xFFFFFFFF}
        rows = want["winner"] >= 0
        for index, winner in sorted(set(zip(got["id"][rows, 3].tolist(), want["winner"][rows].tolist()))):  # every row, each distinct pair once
            m = brute.materials[winner]
            assert index in table and same_material(table[index], pyref.DEFAULT_MATERIAL if m is None else m), (ctx, "material", index, winner)
    assert R.same_bits(got["distance"], want["distance"]), (ctx, "distance", np.nonzero(got["distance"].view(np.uint64) != want["distance"].view(np.uint64))[0][:5])
    assert R.same_bits(got["point"], want["point"]), (ctx, "point", np.nonzero((got["point"].view(np.uint64) != want["point"].view(np.uint64)).any(axis=1))[0][:5])
    assert np.array_equal(got["id"][:, :3], want["id"][:, :3]), (ctx, "id", np.nonzero((got["id"][:, :3] != want["id"][:, :3]).any(axis=1))[0][:5])
    miss = want["id"][:, 0] == 0
    assert (got["id"][miss, 3] == 0xFFFFFFFF).all() and (got["id"][~miss, 3] != 0xFFFFFFFF).all(), (ctx, "material: -1 for a miss alone")


# ---- 1: the brute force, four radii -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SCENES))
def test_every_plane_is_the_brute_forces_at_four_radii(name):
    _, b, pts, want = C.case(name)
    accel = accel_of(name)
    for radius in C.radii(want):
        ref = want if radius == INF else b.closest(pts, radius)
        got = G.closest_points(accel, pts, radius)
        same((name, radius), got, ref, accel, b)
        hits = int((ref["id"][:, 0] != 0).sum())
        print("closest points, %s, radius %r: %d of %d points have a surface within it" % (name, radius, hits, len(pts)))
        assert 0 < hits < len(pts), (name, radius, "a radius that excludes some winners and not all")
    assert accel.closest_points(pts[:5], radius=1.0, planes=("distance",))["distance"].tobytes() == G.closest_points(accel, pts[:5], 1.0)["distance"].tobytes()


# ---- 2: shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own", "torus"])
def test_every_count_from_none_to_4097(name):
    _, _, pts, want = C.case(name)
    accel = accel_of(name)
    for n in (0, 1, 63, 64, 65, 129, 4097):
        got = G.closest_points(accel, pts[:n])
        assert all(len(got[p]) == n for p in PLANES)
        same((name, n), got, {p: want[p][:n] for p in PLANES})


# ---- 3: more tiles than twice the grid's waves -------------------------------------------------------------------------------------------
def test_one_big_call_is_its_4097_point_pieces():
    torch = pytest.importorskip("torch")
    _, _, pts, want = C.case("own")
    accel = accel_of("own")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = 1
    while (reps * len(pts) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    big = np.ascontiguousarray(np.tile(pts, (reps, 1)))
    got = G.closest_points(accel, big)
    piece = G.closest_points(accel, pts)
    same("piece", piece, want)
    for p in PLANES:
        assert got[p].tobytes() == np.tile(piece[p], (reps,) + (1,) * (piece[p].ndim - 1)).tobytes(), (p, reps)


# ---- 4: every traversal mode, the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own", "torus"])
def test_every_traversal_mode_and_order_gives_the_same_bytes(name):
    _, _, pts, want = C.case(name)
    accel = G.Accel.from_scene(C.builder(name)(G))  # (an accel of its own: the modes are the accel's)
    first = G.closest_points(accel, pts)
    same(name, first, want)
    forms = []
    for form in each_form(accel):
        for order in (0, 1):
            G.set_query_order(accel, order)
            got = G.closest_points(accel, pts)
            assert all(got[p].tobytes() == first[p].tobytes() for p in PLANES), (name, form, order)
        G.set_query_order(accel, 0)
        forms.append(form)
    assert "reference" in forms and "prune" in forms, forms


# ---- 5: each plane alone, subsets over garbage -------------------------------------------------------------------------------------------
def test_each_plane_alone_and_subsets_over_garbage():
    _, _, pts, want = C.case("own")
    accel = accel_of("own")
    n = 64 * 20 + 9
    q = np.ascontiguousarray(pts[500:500 + n])
    full = G.closest_points(accel, q)
    same("slice", full, {p: want[p][500:500 + n] for p in PLANES})
    rng = np.random.default_rng(5)
    dt = {"distance": np.float64, "point": np.float64, "id": np.uint32}
    for planes in (("distance",), ("point",), ("id",), ("distance", "id"), ("point", "id"), ("distance", "point"), PLANES):
        bufs = {p: rng.integers(1, 2 ** 32, n * WORDS[p], dtype=np.uint64).astype(np.uint32).view(dt[p]).reshape(full[p].shape) for p in PLANES}
        for p in PLANES:
            if p not in planes:
                bufs[p].view(np.uint32)[...] = 0xA5A5A5A5
        out = G.closest_points(accel, q, INF, planes, into={p: bufs[p] for p in planes})
        assert all(out[p] is bufs[p] and out[p].tobytes() == full[p].tobytes() for p in planes), planes
        assert all((bufs[p].view(np.uint32) == 0xA5A5A5A5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", planes)


# ---- 6: the device form on a second stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "torus"])
def test_the_device_form_on_a_second_stream_between_guard_words(name):
    torch = pytest.importorskip("torch")
    _, b, pts, want = C.case(name)
    accel = accel_of(name)
    n = len(pts)
    radius = C.radii(want)[2]
    ref = G.closest_points(accel, pts, radius)
    same((name, radius), ref, b.closest(pts, radius))
    dpts = torch.from_numpy(pts).cuda()
    stream = torch.cuda.Stream()
    for planes in (PLANES, ("distance",), ("point", "id")):
        dev = {p: torch.full((GUARD + n * WORDS[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            assert s != 0
            ptrs = {p + "_ptr": dev[p].data_ptr() + 4 * GUARD for p in planes}
            for _ in range(2):  # the second call runs over the first one's results
                G.closest_points_device(accel, n, dpts.data_ptr(), radius, stream=s, **ptrs)
        stream.synchronize()
        for p in PLANES:
            back = dev[p].cpu().numpy().view(np.uint32)
            if p in planes:
                assert (back[:GUARD] == FILL).all() and (back[GUARD + n * WORDS[p]:] == FILL).all(), (name, p, "nothing is written outside the plane")
                assert back[GUARD:GUARD + n * WORDS[p]].tobytes() == ref[p].tobytes(), (name, planes, p)
            else:
                assert (back == FILL).all(), (name, planes, p, "not asked for")


# ---- 7: the material is lg_intersect's; lg_intersect's hit points as query points --------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SCENES))
def test_material_is_lg_intersects_on_the_ray_to_the_point(name):
    _, b, pts, want = C.case(name)
    accel = accel_of(name)
    got = G.closest_points(accel, pts)
    ok = (got["id"][:, 0] != 0) & (got["distance"] > 1e-9)
    q, x = pts[ok], got["point"][ok]
    rays = np.ascontiguousarray(np.concatenate([q, x - q], axis=1))
    hits = G.intersect(accel, rays)
    ids = got["id"][ok]
    named = (hits["kind"] == ids[:, 0]) & (hits["prim"] == ids[:, 1]) & (hits["instance"] == ids[:, 2])
    print("closest points, %s: the ray from q to its closest point names the same primitive for %d of %d points" % (name, int(named.sum()), int(ok.sum())))
    assert named.sum() >= ok.sum() // 2, (name, int(named.sum()), int(ok.sum()))
    assert np.array_equal(hits["material"][named].astype(np.uint32), ids[named, 3]), name
    kinds = set(ids[named, 0].tolist())
    assert kinds >= set(np.unique(want["id"][:, 0]).tolist()) - {0}, (name, kinds)
    # lg_intersect's hit points are surface points: their closest point is themselves up to rounding, and the brute force agrees bit for bit
    cam = G.camera_rays(accel, 32, 24)
    h = G.intersect(accel, cam)
    surf = np.ascontiguousarray(h["p"][h["kind"] != 0])
    assert len(surf) >= 50, name
    on = G.closest_points(accel, surf)
    same((name, "hit points"), on, b.closest(surf))
    assert on["distance"].max() < 1e-9, (name, float(on["distance"].max()))


# ---- 8: signed distance ------------------------------------------------------------------------------------------------------------------
def sphere_and_box(api):
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 0.0, 9.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    scene.root.add_sphere([-2.0, 0.0, 0.0], 1.0, api.Material.matte([0.8, 0.7, 0.6], 0.0))
    scene.root.add_box([1.0, -1.0, -1.0], [3.0, 1.0, 1.0], api.Material.matte([0.6, 0.7, 0.8], 0.0))
    return scene


def test_signed_distance_against_the_closed_form():
    accel = G.Accel.from_scene(sphere_and_box(G))
    rng = np.random.default_rng(8)
    q = rng.uniform(-4.0, 4.0, (2000, 3)) * [1.0, 0.5, 0.5]
    ds = np.sqrt(((q - [-2.0, 0.0, 0.0]) ** 2).sum(axis=1)) - 1.0
    d = np.abs(q - [2.0, 0.0, 0.0]) - 1.0
    db = np.sqrt((np.maximum(d, 0.0) ** 2).sum(axis=1)) + np.minimum(d.max(axis=1), 0.0)
    want = np.minimum(ds, db)  # the two solids are disjoint: the union's signed distance is the smaller
    got = accel.signed_distance(q)
    assert not np.isnan(got).any() and (got < 0).sum() >= 100 and (got > 0).sum() >= 100
    assert np.abs(got - want).max() <= 1e-12, float(np.abs(got - want).max())
    assert np.isnan(accel.signed_distance(q[got < 0][:4], max_layers=1)).all(), "the count reached max_layers: the parity is unknown"
    assert np.isnan(G.signed_distance(accel, np.array([[np.nan, 0.0, 0.0]]))).all()


# ---- 9: 40 lights ------------------------------------------------------------------------------------------------------------------------
def test_a_scene_with_40_lights_is_accepted():
    import pyref
    accel = G.Accel.from_scene(many_lights_scene(G, 40))
    b = R.Brute(many_lights_scene(pyref.Api, 40))
    q = np.random.default_rng(9).uniform(-3.0, 3.0, (257, 3))
    same("40 lights", G.closest_points(accel, q), b.closest(q))


# ---- 10: errors; the depth-8 scenes ---------------------------------------------------------------------------------------------------------
def test_every_error_leaves_its_outputs_untouched():
    torch = pytest.importorskip("torch")
    _, _, pts, _ = C.case("own")
    accel = accel_of("own")
    n = 100
    q = np.ascontiguousarray(pts[:n])
    host = {"distance": np.full(n, 7.0), "point": np.full((n, 3), 7.0), "id": np.full((n, 4), 7, dtype=np.uint32)}
    dq = torch.from_numpy(pts[:n + 1].copy()).cuda()
    dev = {p: torch.full(((n + 1) * WORDS[p],), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
    ptr = {p + "_ptr": dev[p].data_ptr() for p in PLANES}
    cpu = torch.zeros(n * 3, dtype=torch.float64)
    # For "a buffer that ends beyond its allocation" the buffer has to BE an allocation: torch hands small tensors out of blocks of its own,
    # and the library can only see where a block ends.  12 MiB are a block of their own (tests/test_gpu_hit_attributes.py does the same)
    torch.cuda.empty_cache()
    many = 1 << 19
    short_point = torch.full((many * 6,), FILL, dtype=torch.int32, device="cuda")
    long_point = torch.full(((many + 1) * 6,), FILL, dtype=torch.int32, device="cuda")
    short_pts = torch.zeros((many, 3), dtype=torch.float64, device="cuda")
    long_pts = torch.zeros((many + 1, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    refused = C.builder("chain8_shallow")(G)
    bad = [lambda: G.closest_points(accel, q, -1.0, into=host),
           lambda: G.closest_points(accel, q, float("nan"), into=host),
           lambda: G.closest_points(accel, q, -INF, into=host),
           lambda: G.closest_points(accel, q, INF, (), into=host),
           lambda: G.closest_points(G.Accel.from_scene(refused), q, INF, into=host),
           lambda: G.closest_points_device(accel, n, 0, INF, stream=0, **ptr),
           lambda: G.closest_points_device(accel, n, dq.data_ptr(), INF, stream=0),
           lambda: G.closest_points_device(accel, n, dq.data_ptr(), -1.0, stream=0, **ptr),
           lambda: G.closest_points_device(accel, n, dq.data_ptr() + 4, INF, stream=0, **ptr),
           lambda: G.closest_points_device(accel, n, dq.data_ptr(), INF, stream=0, **dict(ptr, id_ptr=dev["id"].data_ptr() + 8)),
           lambda: G.closest_points_device(accel, n, dq.data_ptr(), INF, stream=0, **dict(ptr, distance_ptr=dev["distance"].data_ptr() + 4)),
           lambda: G.closest_points_device(accel, many + 1, long_pts, INF, point_ptr=short_point, stream=0),
           lambda: G.closest_points_device(accel, many + 1, short_pts, INF, point_ptr=long_point, stream=0),
           lambda: G.closest_points_device(accel, n, cpu.data_ptr(), INF, stream=0, **ptr),
           lambda: G.closest_points_device(accel, (2 ** 32 - 1) * 64 + 1, dq.data_ptr(), INF, stream=0, **ptr),
           lambda: G.closest_points_device(accel, 2 ** 63, dq.data_ptr(), INF, stream=0, **ptr)]
    for i, f in enumerate(bad):
        with pytest.raises(la.LasgunError):
            f()
        assert G.last_error(), i
    torch.cuda.synchronize()
    assert (host["distance"] == 7.0).all() and (host["point"] == 7.0).all() and (host["id"] == 7).all(), "an error touches no host output"
    assert all((dev[p].cpu().numpy().view(np.uint32) == FILL).all() for p in PLANES), "nor a device output"
    assert bool((short_point == FILL).all()) and bool((long_point == FILL).all())
    for what, call in (("point", bad[11]), ("points", bad[12])):
        with pytest.raises(la.LasgunError, match=what + " ends beyond its allocation"):
            call()
    with pytest.raises(la.LasgunError, match="instance 1 "):
        G.closest_points(G.Accel.from_scene(refused), q)
    G.closest_points_device(accel, 0, 0, -1.0, stream=0)  # n == 0 is answered before every other check
    assert all(len(v) == 0 for v in G.closest_points(accel, np.zeros((0, 3)), -1.0).values())


@pytest.mark.parametrize("name", list(C.LIMIT_SCENES))
def test_the_depth_8_scenes_match_the_brute_force_or_are_refused_where_the_gate_says(name):
    _, b, pts, want = C.case(name)
    verdict = C.gate(b.cat)
    assert G.scene_closest_gate(C.builder(name)(G))[0] == verdict, name
    accel = accel_of(name)
    if verdict >= 0:
        with pytest.raises(la.LasgunError, match="instance %d " % verdict):
            G.closest_points(accel, pts)
        return
    depth = G.scene_closest_depth(C.builder(name)(G))
    print("closest points, %s: a per-lane stack of %d entries, %d KiB of dynamic LDS" % (name, depth, depth * 2))
    assert depth <= G.CLOSEST_MAX_DEPTH
    if name == "deep_a":
        assert depth > 32, "this scene takes the launch beyond the default 64 KiB of dynamic LDS: the raised limit runs on the hardware"
    same(name, G.closest_points(accel, pts), want, accel, b)
    r = C.radii(want)[2]
    same((name, r), G.closest_points(accel, pts, r), b.closest(pts, r))
