"""Proximity queries (include/lasgun_hip.h: lg_nearest*) on the device, bit for bit against the brute force over all primitives
(tests/nearest_ref.py over tests/closest_ref.py) on the scenes and points of tests/closest_cases.py -- nothing is tolerated.

   1  all five planes equal the brute force: own, cornell, torus x k in {1, 2, 3, 8} x radius in {+INF, 0, the median distance, 2^-20},
      the material of every filled slot included;
   2  slot 0 is lg_closest_points' planes byte for byte, for k = 1 and k = 8;
   3  touch == (count > 0);
   4  the touch-only form (its plane alone) gives the same bytes;
   5  count alone and the list alone each equal the all-planes call: the three forms and their different prune limits, one answer;
   6  per-point radii: a seeded mix of +INF, 0, -0.0, the median, 2^-20, NaN, -1 and random values against the brute force row by row; a
      radii array filled with one value against the shared-radius call, the same bytes;
   7  n in {0, 1, 63, 64, 65, 129, 4097};
   8  one call of more tiles than twice the grid's waves equals its 4097-point pieces;
   9  every traversal mode of the accel and both query orders give the same bytes;
  10  each plane alone, and subsets over garbage, leave the other buffers intact;
  11  the device form on a second stream between guard words;
  12  the depth-8 scenes at k = 1 and 8 match the brute force or are refused exactly where the gate and lg_scene_nearest_lds say; one of
      those answered needs more than 64 KiB of dynamic LDS;
  13  a scene with 40 lights is accepted;
  14  every error leaves its outputs untouched."""
import functools

import numpy as np
import pytest

import closest_cases as C
import closest_ref as R
import lasgun_amd as la
import nearest_ref as N
import pyref
from test_gpu_radiance_query import each_form, many_lights_scene
from test_gpu_ray_query import same_material

pytestmark = pytest.mark.gpu

G = la.api
PLANES = la.NEAREST_PLANES
SLOTS = la.NEAREST_SLOT_PLANES
DT = {"touch": np.uint8, "count": np.uint32, "distance": np.float64, "point": np.float64, "id": np.uint32}
BYTES = {"touch": 1, "count": 4, "distance": 8, "point": 24, "id": 16}  # a row
GUARD, FILL = 64, 0xA5
INF = float("inf")
LDS_LIMIT = 160 << 10


@functools.lru_cache(maxsize=None)
def accel_of(name):
    return G.Accel.from_scene(C.builder(name)(G))


def same(ctx, got, want, accel=None, brute=None):
    """touch, count, distance and point bit for bit; kind, prim, instance against the brute force; with (accel, brute) the material word of
    EVERY filled slot too: the Material behind the library's index is the brute force's for that candidate."""
    for p in ("touch", "count", "distance", "point"):
        if p in got:
            assert R.same_bits(got[p], want[p]), (ctx, p, np.argwhere(got[p].reshape(want[p].shape) != want[p])[:5] if got[p].shape == want[p].shape else got[p].shape)
    if "touch" in got and "count" in got:
        assert ((got["touch"] == 1) == (got["count"] > 0)).all() and (got["touch"] <= 1).all(), (ctx, "touch == (count > 0)")
    if "id" not in got:
        return
    assert got["id"].shape == want["id"].shape and np.array_equal(got["id"][..., :3], want["id"][..., :3]), (ctx, "id", np.argwhere((got["id"][..., :3] != want["id"][..., :3]).any(axis=-1))[:5])
    miss = want["id"][..., 0] == 0
    assert (got["id"][miss][:, 3] == 0xFFFFFFFF).all() and (got["id"][~miss][:, 3] != 0xFFFFFFFF).all(), (ctx, "material: -1 for an empty slot alone")
    if accel is not None:
        table = {int(i): G.accel_material(accel, int(i)) for i in np.unique(got["id"][..., 3]) if i != 0xFFFFFFFF}
        filled = want["winner"] >= 0
        for index, winner in sorted(set(zip(got["id"][..., 3][filled].tolist(), want["winner"][filled].tolist()))):  # every filled slot, each distinct pair once
            m = brute.materials[winner]
            assert index in table and same_material(table[index], pyref.DEFAULT_MATERIAL if m is None else m), (ctx, "material", index, winner)


def cut(want, n):
    """The answer for the first n points."""
    return {p: (want[p][:, :n] if want[p].ndim >= 2 and p not in ("touch", "count", "next_d2") else want[p][:n]) for p in want}


# ---- 1, 3: the brute force, four k, four radii ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("name", list(C.SCENES))
def test_all_five_planes_are_the_brute_forces(name, k):
    _, b, pts, closest = C.case(name)
    accel = accel_of(name)
    for index, radius in enumerate(C.radii(closest)):
        want = N.first(N.reference(name, index), k)
        got = G.nearest(accel, pts, radius=radius, k=k)
        assert [got[p].shape for p in PLANES] == [(len(pts),), (len(pts),), (k, len(pts)), (k, len(pts), 3), (k, len(pts), 4)]
        same((name, k, radius), got, want, accel, b)
        hits = int(got["touch"].sum())
        print("nearest, %s, k %d, radius %r: %d of %d points touch, the largest count is %d" % (name, k, radius, hits, len(pts), int(got["count"].max())))
        assert 0 < hits < len(pts), (name, radius, "a radius that excludes some points and not all")
    assert accel.nearest(pts[:5], radius=1.0, k=2, planes=("count",))["count"].tobytes() == G.nearest(accel, pts[:5], radius=1.0, k=2)["count"].tobytes()
    assert accel.touching(pts[:70], 1.0).tolist() == (G.nearest(accel, pts[:70], radius=1.0)["count"] > 0).tolist()


# ---- 2: slot 0 is lg_closest_points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("name", list(C.SCENES))
def test_slot_0_is_closest_points_byte_for_byte(name, k):
    _, _, pts, closest = C.case(name)
    accel = accel_of(name)
    for radius in C.radii(closest):
        got = G.nearest(accel, pts, radius=radius, k=k, planes=SLOTS)
        ref = G.closest_points(accel, pts, radius)
        for p in SLOTS:
            assert got[p][0].tobytes() == ref[p].tobytes(), (name, k, radius, p)


# ---- 4, 5: the three forms, one answer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("name", list(C.SCENES))
def test_the_three_forms_give_one_answer(name, k):
    _, _, pts, closest = C.case(name)
    accel = accel_of(name)
    for index in (0, 2, 3):  # +INF (count walks everything), the median, 2^-20
        radius = C.radii(closest)[index]
        full = G.nearest(accel, pts, radius=radius, k=k)
        same((name, k, radius), full, N.first(N.reference(name, index), k))
        for planes in (("touch",), ("count",), SLOTS, ("touch", "count"), ("touch", "distance"), ("distance",), ("count", "id")):
            got = G.nearest(accel, pts, radius=radius, k=k, planes=planes)
            assert all(got[p].tobytes() == full[p].tobytes() for p in planes), (name, k, radius, planes)
        # k plays no part without a slot plane, and may then be 0
        for kk in (0, 5):
            got = G.nearest(accel, pts, radius=radius, k=kk, planes=("touch", "count"))
            assert got["touch"].tobytes() == full["touch"].tobytes() and got["count"].tobytes() == full["count"].tobytes(), (name, kk, radius)


# ---- 6: per-point radii ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("own", 8), ("cornell", 3), ("torus", 8), ("torus", 1)])
def test_a_radius_per_point_against_the_brute_force(name, k):
    _, b, pts, closest = C.case(name)
    accel = accel_of(name)
    radii = N.mixed_radii(name, 60 + k)
    assert np.isnan(radii).sum() >= 10 and (radii == -1.0).sum() >= 10 and (np.signbit(radii) & (radii == 0.0)).sum() >= 10 and np.isinf(radii).sum() >= 10
    want = N.nearest(b, pts, radii=radii, k=k)
    got = G.nearest(accel, pts, radii=radii, radius=float("nan"), k=k)  # (with radii the shared radius is neither read nor checked)
    same((name, k, "mixed radii"), got, want, accel, b)
    bad = np.isnan(radii) | (radii < 0.0)
    assert (got["count"][bad] == 0).all() and np.isinf(got["distance"][:, bad]).all(), "a NaN or negative radius of its own: a miss, not an error"
    zero = (radii == 0.0) & np.signbit(radii)
    assert got["count"][zero].tobytes() == G.nearest(accel, pts[zero], radius=0.0, k=k, planes=("count",))["count"].tobytes(), "-0.0 is zero"
    for planes in (("touch",), ("count",), SLOTS):  # each form reads the radius plane
        part = G.nearest(accel, pts, radii=radii, k=k, planes=planes)
        assert all(part[p].tobytes() == got[p].tobytes() for p in planes), (name, k, planes)
    # one value in every entry: the shared-radius call's bytes
    for radius in C.radii(closest):
        shared = G.nearest(accel, pts, radius=radius, k=k)
        filled = G.nearest(accel, pts, radii=np.full(len(pts), radius), radius=-1.0, k=k)
        assert all(shared[p].tobytes() == filled[p].tobytes() for p in PLANES), (name, k, radius)


# ---- 7: shapes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own", "torus"])
def test_every_count_from_none_to_4097(name):
    _, _, pts, closest = C.case(name)
    accel = accel_of(name)
    radius = C.radii(closest)[2]
    want = N.first(N.reference(name, 2), 3)
    for n in (0, 1, 63, 64, 65, 129, 4097):
        got = G.nearest(accel, pts[:n], radius=radius, k=3)
        assert got["touch"].shape == (n,) and got["count"].shape == (n,) and got["distance"].shape == (3, n) and got["point"].shape == (3, n, 3) and got["id"].shape == (3, n, 4)
        same((name, n), got, cut(want, n))
        per_point = G.nearest(accel, pts[:n], radii=np.full(n, radius), k=3)
        assert all(per_point[p].tobytes() == got[p].tobytes() for p in PLANES), (name, n)


# ---- 8: more tiles than twice the grid's waves -----------------------------------------------------------------------------------------------
def test_one_big_call_is_its_4097_point_pieces():
    torch = pytest.importorskip("torch")
    _, _, pts, closest = C.case("own")
    accel = accel_of("own")
    radius = C.radii(closest)[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = 1
    while (reps * len(pts) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    big = np.ascontiguousarray(np.tile(pts, (reps, 1)))
    got = G.nearest(accel, big, radius=radius, k=2)
    piece = G.nearest(accel, pts, radius=radius, k=2)
    same("piece", piece, N.first(N.reference("own", 2), 2))
    for p in PLANES:
        tiled = np.tile(piece[p], (1, reps) + (1,) * (piece[p].ndim - 2)) if p in SLOTS else np.tile(piece[p], reps)
        assert got[p].tobytes() == tiled.tobytes(), (p, reps)


# ---- 9: every traversal mode, both query orders: the same bytes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own", "torus"])
def test_every_traversal_mode_and_order_gives_the_same_bytes(name):
    _, _, pts, closest = C.case(name)
    radius = C.radii(closest)[2]
    accel = G.Accel.from_scene(C.builder(name)(G))  # (an accel of its own: the modes are the accel's)
    first = G.nearest(accel, pts, radius=radius, k=4)
    same(name, first, N.first(N.reference(name, 2), 4))
    forms = []
    for form in each_form(accel):
        for order in (0, 1):
            G.set_query_order(accel, order)
            got = G.nearest(accel, pts, radius=radius, k=4)
            assert all(got[p].tobytes() == first[p].tobytes() for p in PLANES), (name, form, order)
        G.set_query_order(accel, 0)
        forms.append(form)
    assert "reference" in forms and "prune" in forms, forms


# ---- 10: each plane alone, subsets over garbage ----------------------------------------------------------------------------------------------
def test_each_plane_alone_and_subsets_over_garbage():
    _, _, pts, closest = C.case("own")
    accel = accel_of("own")
    radius, k = C.radii(closest)[2], 3
    n = 64 * 20 + 9
    q = np.ascontiguousarray(pts[500:500 + n])
    full = G.nearest(accel, q, radius=radius, k=k)
    same("slice", full, {p: (v[:, 500:500 + n] if p in SLOTS + ("winner", "d2") else v[500:500 + n]) for p, v in N.first(N.reference("own", 2), k).items()})
    rng = np.random.default_rng(5)
    subsets = [(p,) for p in PLANES] + [("touch", "id"), ("count", "distance"), ("point", "id"), ("touch", "count", "point"), PLANES]
    for planes in subsets:
        bufs = {p: rng.integers(1, 256, full[p].nbytes, dtype=np.uint8).view(DT[p]).reshape(full[p].shape) for p in PLANES}
        for p in PLANES:
            if p not in planes:
                bufs[p].view(np.uint8)[...] = 0xA5
        out = G.nearest(accel, q, radius=radius, k=k, planes=planes, into={p: bufs[p] for p in planes})
        assert all(out[p] is bufs[p] and out[p].tobytes() == full[p].tobytes() for p in planes), planes
        assert all((bufs[p].view(np.uint8) == 0xA5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", planes)


# ---- 11: the device form on a second stream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "torus"])
def test_the_device_form_on_a_second_stream_between_guard_words(name):
    torch = pytest.importorskip("torch")
    _, b, pts, closest = C.case(name)
    accel = accel_of(name)
    n, k = len(pts), 3
    radii = N.mixed_radii(name, 11)
    ref = G.nearest(accel, pts, radii=radii, k=k)
    same((name, "mixed radii"), ref, N.nearest(b, pts, radii=radii, k=k))
    dpts, dradii = torch.from_numpy(pts).cuda(), torch.from_numpy(radii).cuda()
    stream = torch.cuda.Stream()
    rows = {p: (k * n if p in SLOTS else n) for p in PLANES}
    for planes in (PLANES, ("touch",), ("count", "distance"), ("point", "id")):
        dev = {p: torch.full((GUARD + rows[p] * BYTES[p] + GUARD,), FILL, dtype=torch.uint8, device="cuda") for p in PLANES}
        assert all(dev[p].data_ptr() % 16 == 0 for p in PLANES)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            assert s != 0
            ptrs = {p + "_ptr": dev[p].data_ptr() + GUARD for p in planes}
            for _ in range(2):  # the second call runs over the first one's results
                G.nearest_device(accel, n, dpts.data_ptr(), dradii.data_ptr(), k=k, stream=s, **ptrs)
        stream.synchronize()
        for p in PLANES:
            back = dev[p].cpu().numpy()
            if p in planes:
                assert (back[:GUARD] == FILL).all() and (back[GUARD + rows[p] * BYTES[p]:] == FILL).all(), (name, p, "nothing is written outside the plane")
                assert back[GUARD:GUARD + rows[p] * BYTES[p]].tobytes() == ref[p].tobytes(), (name, planes, p)
            else:
                assert (back == FILL).all(), (name, planes, p, "not asked for")


# ---- 12: the depth-8 scenes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("name", list(C.LIMIT_SCENES))
def test_the_depth_8_scenes_match_the_brute_force_or_are_refused_where_the_rules_say(name, k):
    _, b, pts, closest = C.case(name)
    verdict = C.gate(b.cat)
    lds = G.scene_nearest_lds(C.builder(name)(G), k)
    assert lds == 256 * (8 * G.scene_closest_depth(C.builder(name)(G)) + 20 * k)
    accel = accel_of(name)
    if verdict >= 0:
        with pytest.raises(la.LasgunError, match="instance %d " % verdict):
            G.nearest(accel, pts, k=k)
        return
    if lds > LDS_LIMIT:
        with pytest.raises(la.LasgunError, match="lg_scene_nearest_lds"):
            G.nearest(accel, pts, k=k)
        return
    print("nearest, %s, k %d: %d KiB of dynamic LDS a workgroup" % (name, k, lds // 1024))
    if name == "deep_a" and k == 8:
        assert lds > (64 << 10), "this case takes the launch beyond the default 64 KiB of dynamic LDS: the raised limit runs on the hardware"
    radius = C.radii(closest)[2]
    same((name, k, radius), G.nearest(accel, pts, radius=radius, k=k), N.nearest(b, pts, radius=radius, k=k), accel, b)
    slots = G.nearest(accel, pts, k=k, planes=SLOTS)  # +INF through the list form: the k-th best alone prunes
    same((name, k, INF), slots, N.nearest(b, pts, k=k))
    assert all(slots[p][0].tobytes() == G.closest_points(accel, pts)[p].tobytes() for p in SLOTS)


# ---- 13: 40 lights ------------------------------------------------------------------------------------------------------------------------------
def test_a_scene_with_40_lights_is_accepted():
    accel = G.Accel.from_scene(many_lights_scene(G, 40))
    b = R.Brute(many_lights_scene(pyref.Api, 40))
    q = np.random.default_rng(9).uniform(-3.0, 3.0, (257, 3))
    same("40 lights", G.nearest(accel, q, radius=2.0, k=4), N.nearest(b, q, radius=2.0, k=4))


# ---- 14: errors ---------------------------------------------------------------------------------------------------------------------------------
def test_every_error_leaves_its_outputs_untouched():
    torch = pytest.importorskip("torch")
    _, _, pts, _ = C.case("own")
    accel = accel_of("own")
    n, k = 100, 2
    q = np.ascontiguousarray(pts[:n])
    host = {"touch": np.full(n, 7, dtype=np.uint8), "count": np.full(n, 7, dtype=np.uint32), "distance": np.full((k, n), 7.0), "point": np.full((k, n, 3), 7.0),
            "id": np.full((k, n, 4), 7, dtype=np.uint32)}
    flags = {p: host[p] for p in ("touch", "count")}
    dq = torch.from_numpy(pts[:n + 1].copy()).cuda()
    dr = torch.ones(n + 1, dtype=torch.float64, device="cuda")
    dev = {p: torch.full((((k if p in SLOTS else 1) * n + 1) * BYTES[p],), FILL, dtype=torch.uint8, device="cuda") for p in PLANES}
    ptr = {p + "_ptr": dev[p].data_ptr() for p in PLANES}
    cpu = torch.zeros(n * 3, dtype=torch.float64)
    # For "a buffer that ends beyond its allocation" the buffer has to BE an allocation: torch hands small tensors out of blocks of its own,
    # and the library can only see where a block ends.  12 MiB are a block of their own (tests/test_gpu_closest_points.py does the same)
    torch.cuda.empty_cache()
    many = 1 << 19
    short_point = torch.full((many * 24,), FILL, dtype=torch.uint8, device="cuda")
    long_point = torch.full(((many + 1) * 24,), FILL, dtype=torch.uint8, device="cuda")
    long_pts = torch.zeros((many * 3 + 1, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    refused = C.builder("chain8_shallow")(G)
    bad = [lambda: G.nearest(accel, q, radius=-1.0, k=k, into=host),
           lambda: G.nearest(accel, q, radius=float("nan"), k=k, into=host),
           lambda: G.nearest(accel, q, radius=-INF, k=k, into=host),
           lambda: G.nearest(accel, q, k=k, planes=(), into=host),
           lambda: G.nearest(G.Accel.from_scene(refused), q, k=k, into=host),
           lambda: G.nearest_device(accel, n, 0, None, INF, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, k, stream=0),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, -1.0, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, 9, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, 0, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, 9, stream=0, touch_ptr=dev["touch"].data_ptr()),
           lambda: G.nearest_device(accel, n, dq.data_ptr() + 4, None, INF, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), dr.data_ptr() + 4, INF, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, k, stream=0, **dict(ptr, id_ptr=dev["id"].data_ptr() + 8)),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, k, stream=0, **dict(ptr, count_ptr=dev["count"].data_ptr() + 2)),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), None, INF, k, stream=0, **dict(ptr, distance_ptr=dev["distance"].data_ptr() + 4)),
           lambda: G.nearest_device(accel, many + 1, long_pts, None, INF, 1, point_ptr=short_point, stream=0),
           lambda: G.nearest_device(accel, many // 2 + 1, long_pts, None, INF, 2, point_ptr=short_point, stream=0),  # (n * k rows: one too many)
           lambda: G.nearest_device(accel, many * 3 + 1, long_pts, short_point, INF, 0, touch_ptr=long_point, stream=0),  # (as radii: 8 bytes a point)
           lambda: G.nearest_device(accel, n, cpu.data_ptr(), None, INF, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, n, dq.data_ptr(), cpu.data_ptr(), INF, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, (2 ** 32 - 1) * 64 + 1, dq.data_ptr(), None, INF, k, stream=0, **ptr),
           lambda: G.nearest_device(accel, 2 ** 63, dq.data_ptr(), None, INF, 8, stream=0, **ptr)]
    for i, f in enumerate(bad):
        with pytest.raises(la.LasgunError):
            f()
        assert G.last_error(), i
    for f in (lambda: G.nearest(accel, q, k=9, into=host), lambda: G.nearest(accel, q, k=0, into=host), lambda: G.nearest(accel, q, radii=np.ones(n - 1), k=k, into=host)):
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()
    assert all((host[p] == 7).all() for p in PLANES), "an error touches no host output"
    assert all((dev[p].cpu().numpy() == FILL).all() for p in PLANES), "nor a device output"
    assert bool((short_point == FILL).all()) and bool((long_point == FILL).all())
    for what, call in (("point", bad[16]), ("point", bad[17]), ("radii", bad[18])):
        with pytest.raises(la.LasgunError, match=what + " ends beyond its allocation"):
            call()
    with pytest.raises(la.LasgunError, match="instance 1 "):
        G.nearest(G.Accel.from_scene(refused), q)
    G.nearest_device(accel, 0, 0, None, -1.0, 99, stream=0)  # n == 0 is answered before every other check
    assert all(len(v.reshape(-1)) == 0 for v in G.nearest(accel, np.zeros((0, 3)), radius=-1.0, k=2).values())
    # legal: k == 0 without a slot plane; a NaN shared radius beside radii
    ok = G.nearest(accel, q, radii=np.ones(n), radius=float("nan"), k=0, planes=("touch", "count"), into=flags)
    assert (ok["touch"] <= 1).all() and not (ok["count"] == 7).all()
