"""Segment proximity (include/lasgun_hip.h: lg_closest_segments*) on the device, bit for bit against the brute force over all primitives
(tests/segment_ref.py over tests/closest_ref.py) on the scenes of tests/closest_cases.py and the segments of tests/segment_cases.py --
nothing is tolerated unless stated.

   1  all five planes equal the brute force: own, cornell, torus x radius in {+INF, 0, the median distance, 2^-20}, plus one per-segment
      radii array that holds NaN, negative and -0.0 entries; the material of every winner included;
   2  degenerate segments (p0 == p1) give lg_nearest's k = 1 bytes for the same points and radii;
   3  distance(segment) <= min(lg_closest_points' distance at p0, at p1): exactly where that endpoint's winner is a box or a triangle (the
      segment's candidate of that primitive has the endpoint's own candidate among its sub-candidates); where it is a sphere, within the
      CPU brute force's own worst excess on the same segments plus 4 ulps -- SPHERE_EXCESS below, measured 3.05e-11 (torus, a segment
      with an endpoint at 1e6: an ulp of that distance is 1.2e-10), 1.42e-11 on own, 0 on cornell;
   4  a segment whose ray form o = p0, d = p1 - p0 hits (lg_intersect) at t in [0.01, 0.99] with lg_hit_attributes' barycentrics all at
      least 0.01 answers distance == +0.0 and touch == 1 (tests/test_segments_witness.py: at least 200 a mesh scene);
   5  the two forms agree: touch alone is touch beside the other planes, and is isfinite(distance);
   6  n in {0, 1, 63, 64, 65, 129, 4097};
   7  one call of 3 x 4097 equals its three pieces;
   8  every traversal mode of the accel and both query orders give the same bytes;
   9  each plane alone, and subsets over garbage, leave the other buffers intact;
  10  the device form on a second stream between guard words;
  11  the depth-8 scenes match the brute force or are refused exactly where the gate and the depth rule say;
  12  a scene with 40 lights is accepted;
  13  every error leaves its outputs untouched."""
import functools

import numpy as np
import pytest

import closest_cases as C
import closest_ref as R
import lasgun_amd as la
import pyref
import segment_cases as SC
import segment_ref as SR
from test_gpu_radiance_query import each_form, many_lights_scene
from test_gpu_ray_query import same_material

pytestmark = pytest.mark.gpu

G = la.api
PLANES = la.SEGMENT_PLANES
DT = {"touch": np.uint8, "distance": np.float64, "param": np.float64, "point": np.float64, "id": np.uint32}
BYTES = {"touch": 1, "distance": 8, "param": 8, "point": 24, "id": 16}  # a row
GUARD, FILL = 64, 0xA5
INF = float("inf")
SPHERE_EXCESS = 3.1e-11  # the brute force's worst distance(segment) - distance(endpoint) where the endpoint's winner is a sphere (docstring, 3)


@functools.lru_cache(maxsize=None)
def accel_of(name):
    return G.Accel.from_scene(C.builder(name)(G))


def same(ctx, got, want, accel=None, brute=None):
    """touch, distance, param and point bit for bit; kind, prim, instance against the brute force; with (accel, brute) the material word of
    EVERY winner too: the Material behind the library's index is the brute force's for that candidate."""
    for p in ("touch", "distance", "param", "point"):
        if p in got:
            assert R.same_bits(got[p], want[p]), (ctx, p, np.argwhere(got[p].reshape(want[p].shape) != want[p])[:5] if got[p].shape == want[p].shape else got[p].shape)
    if "touch" in got and "distance" in got:
        assert ((got["touch"] == 1) == np.isfinite(got["distance"])).all() and (got["touch"] <= 1).all(), (ctx, "touch == isfinite(distance)")
    if "id" not in got:
        return
    assert got["id"].shape == want["id"].shape and np.array_equal(got["id"][:, :3], want["id"][:, :3]), (ctx, "id", np.argwhere((got["id"][:, :3] != want["id"][:, :3]).any(axis=-1))[:5])
    miss = want["id"][:, 0] == 0
    assert (got["id"][miss][:, 3] == 0xFFFFFFFF).all() and (got["id"][~miss][:, 3] != 0xFFFFFFFF).all(), (ctx, "material: -1 for a miss alone")
    if accel is not None:
        table = {int(i): G.accel_material(accel, int(i)) for i in np.unique(got["id"][:, 3]) if i != 0xFFFFFFFF}
        filled = want["winner"] >= 0
        for index, winner in sorted(set(zip(got["id"][:, 3][filled].tolist(), want["winner"][filled].tolist()))):
            m = brute.materials[winner]
            assert index in table and same_material(table[index], pyref.DEFAULT_MATERIAL if m is None else m), (ctx, "material", index, winner)


def cut(want, lo, hi):
    return {p: v[lo:hi] for p, v in want.items()}


# ---- 1: the brute force, four shared radii and a radius per segment ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SCENES))
def test_all_five_planes_are_the_brute_forces(name):
    _, b, segs, want, _ = SC.case(name)
    accel = accel_of(name)
    refs = SC.references(name)
    for index, radius in enumerate(C.radii(want)):
        got = G.closest_segments(accel, segs, radius=radius)
        assert [got[p].shape for p in PLANES] == [(len(segs),), (len(segs),), (len(segs),), (len(segs), 3), (len(segs), 4)]
        same((name, radius), got, refs[index], accel, b)
        hits = int(got["touch"].sum())
        print("closest segments, %s, radius %r: %d of %d segments touch" % (name, radius, hits, len(segs)))
        assert 0 < hits < len(segs)
    radii = SC.mixed_radii(name, 30)
    got = G.closest_segments(accel, segs, radii=radii, radius=float("nan"))  # (with radii the shared radius is neither read nor checked)
    same((name, "mixed radii"), got, refs[4], accel, b)
    dead = np.isnan(radii) | (radii < 0.0)
    assert dead.sum() >= 20 and (got["touch"][dead] == 0).all() and np.isinf(got["distance"][dead]).all(), "a NaN or negative radius of its own: a miss, not an error"
    zero = (radii == 0.0) & np.signbit(radii)
    assert zero.sum() >= 10 and got["touch"][zero].tobytes() == G.closest_segments(accel, segs[zero], radius=0.0, planes=("touch",))["touch"].tobytes(), "-0.0 is zero"
    filled = G.closest_segments(accel, segs, radii=np.full(len(segs), C.radii(want)[2]), radius=-1.0)
    shared = G.closest_segments(accel, segs, radius=C.radii(want)[2])
    assert all(filled[p].tobytes() == shared[p].tobytes() for p in PLANES), "one value in every entry: the shared-radius call's bytes"
    assert accel.closest_segments(segs[:5], radius=1.0, planes=("distance",))["distance"].tobytes() == G.closest_segments(accel, segs[:5], radius=1.0)["distance"].tobytes()
    r = np.abs(np.where(np.isfinite(radii), radii, 1.0))
    touching = accel.capsules_touching(segs[:70, :3], segs[:70, 3:], r[:70])
    assert touching.tolist() == (G.closest_segments(accel, segs[:70], radii=r[:70])["touch"] == 1).tolist()
    assert accel.sweep_touching(segs[:70, :3], segs[:70, 3:], 0.25).tolist() == (G.closest_segments(accel, segs[:70], radius=0.25)["touch"] == 1).tolist()


# ---- 2: degenerate segments are lg_nearest at k = 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SCENES))
def test_degenerate_segments_give_nearests_k_1_bytes(name):
    _, _, pts, closest = C.case(name)
    accel = accel_of(name)
    segs = np.ascontiguousarray(np.concatenate([pts, pts], axis=1))
    rng = np.random.default_rng(2)
    med = C.radii(closest)[2]
    mixed = np.where(rng.integers(0, 8, len(pts)) == 0, rng.choice([float("nan"), -1.0, -0.0, INF], len(pts)), rng.uniform(0.0, 2.0 * med, len(pts)))
    for radii, radius in [(None, r) for r in C.radii(closest)] + [(mixed, float("nan"))]:
        got = G.closest_segments(accel, segs, radii=radii, radius=radius)
        ref = G.nearest(accel, pts, radii=radii, radius=radius, k=1, planes=("touch", "distance", "point", "id"))
        assert got["touch"].tobytes() == ref["touch"].tobytes(), (name, radius)
        for p in ("distance", "point", "id"):
            assert got[p].tobytes() == ref[p][0].tobytes(), (name, radius, p)
        assert not got["param"].any() and not np.signbit(got["param"]).any(), "s = +0.0"


# ---- 3: the segment is no farther than either endpoint -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SCENES))
def test_a_segment_is_no_farther_than_its_endpoints(name):
    _, b, segs, want, _ = SC.case(name)
    accel = accel_of(name)
    fin = np.isfinite(segs).all(axis=1)
    got = G.closest_segments(accel, segs, planes=("distance",))["distance"]
    cpu_worst, gpu_worst = 0.0, 0.0
    for end in (segs[:, :3], segs[:, 3:]):
        pt = G.closest_points(accel, np.ascontiguousarray(end))
        exact = fin & (pt["id"][:, 0] >= 2)
        sphere = fin & (pt["id"][:, 0] == 1)
        assert (got[exact] <= pt["distance"][exact]).all(), (name, np.nonzero(exact & ~(got <= pt["distance"]))[0][:5])
        cpu = b.closest(end)
        assert cpu["distance"].tobytes() == pt["distance"].tobytes()
        if sphere.any():
            cpu_worst = max(cpu_worst, float((want["distance"][sphere] - cpu["distance"][sphere]).max()))
            gpu_worst = max(gpu_worst, float((got[sphere] - pt["distance"][sphere]).max()))
            assert (got[sphere] <= pt["distance"][sphere] + SPHERE_EXCESS + 4.0 * np.spacing(pt["distance"][sphere])).all(), name
    print("closest segments, %s: distance(segment) - distance(endpoint) where a sphere wins the endpoint: brute force %.3e, device %.3e at worst" % (name, cpu_worst, gpu_worst))
    assert cpu_worst <= SPHERE_EXCESS, "the recorded excess is the brute force's own"


# ---- 4: a pierced triangle is at distance zero ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.MESH_SCENES))
def test_a_segment_whose_ray_form_hits_well_inside_is_at_distance_zero(name):
    _, _, segs, _, _ = SC.case(name)
    accel = accel_of(name)
    fin = np.isfinite(segs).all(axis=1)
    rays = np.ascontiguousarray(np.concatenate([segs[:, :3], segs[:, 3:] - segs[:, :3]], axis=1)[fin])
    at = G.hit_attributes(accel, rays, planes=("hits", "flags", "bary"))
    hits = G.intersect(accel, rays)
    assert hits.tobytes() == at["hits"].tobytes()
    keep = (hits["kind"] == 3) & (hits["t"] >= 0.01) & (hits["t"] <= 0.99) & (at["flags"] == la.ATTR_HIT) & (at["bary"].min(axis=1) >= 0.01)
    print("closest segments, %s: %d segments pass the ray-form filter" % (name, keep.sum()))
    assert keep.sum() >= 200
    got = G.closest_segments(accel, segs[fin][keep], planes=("touch", "distance"))
    assert (got["distance"] == 0.0).all() and not np.signbit(got["distance"]).any() and (got["touch"] == 1).all()


# ---- 5: the two forms, one answer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SCENES))
def test_the_two_forms_agree(name):
    _, _, segs, want, _ = SC.case(name)
    accel = accel_of(name)
    radii = SC.mixed_radii(name, 30)
    for kw in [dict(radius=r) for r in C.radii(want)] + [dict(radii=radii)]:
        full = G.closest_segments(accel, segs, **kw)
        alone = G.closest_segments(accel, segs, planes=("touch",), **kw)
        assert alone["touch"].tobytes() == full["touch"].tobytes(), (name, kw.get("radius"))
        assert ((alone["touch"] == 1) == np.isfinite(full["distance"])).all()
        for planes in (("touch", "distance"), ("distance",), ("param", "id"), ("point",)):
            got = G.closest_segments(accel, segs, planes=planes, **kw)
            assert all(got[p].tobytes() == full[p].tobytes() for p in planes), (name, planes)


# ---- 6: shapes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own", "torus"])
def test_every_count_from_none_to_4097(name):
    _, _, segs, want, _ = SC.case(name)
    accel = accel_of(name)
    radius = C.radii(want)[2]
    ref = SC.references(name)[2]
    for n in (0, 1, 63, 64, 65, 129, 4097):
        got = G.closest_segments(accel, segs[:n], radius=radius)
        assert [got[p].shape for p in PLANES] == [(n,), (n,), (n,), (n, 3), (n, 4)]
        same((name, n), got, cut(ref, 0, n))
        alone = G.closest_segments(accel, segs[:n], radius=radius, planes=("touch",))
        assert alone["touch"].tobytes() == got["touch"].tobytes(), (name, n)


# ---- 7: one call of three pieces ---------------------------------------------------------------------------------------------------------------------
def test_one_call_of_3_x_4097_is_its_three_pieces():
    _, _, segs, want, _ = SC.case("own")
    accel = accel_of("own")
    radius = C.radii(want)[2]
    piece = G.closest_segments(accel, segs, radius=radius)
    same("piece", piece, SC.references("own")[2])
    big = np.ascontiguousarray(np.concatenate([segs, segs[::-1], segs]))
    got = G.closest_segments(accel, big, radius=radius)
    for p in PLANES:
        assert got[p].tobytes() == np.concatenate([piece[p], piece[p][::-1], piece[p]]).tobytes(), p
    touch = G.closest_segments(accel, big, radius=radius, planes=("touch",))["touch"]
    assert touch.tobytes() == got["touch"].tobytes()


# ---- 8: every traversal mode, both query orders: the same bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own", "torus"])
def test_every_traversal_mode_and_order_gives_the_same_bytes(name):
    _, _, segs, want, _ = SC.case(name)
    radius = C.radii(want)[2]
    accel = G.Accel.from_scene(C.builder(name)(G))  # (an accel of its own: the modes are the accel's)
    first = G.closest_segments(accel, segs, radius=radius)
    same(name, first, SC.references(name)[2])
    forms = []
    for form in each_form(accel):
        for order in (0, 1):
            G.set_query_order(accel, order)
            got = G.closest_segments(accel, segs, radius=radius)
            assert all(got[p].tobytes() == first[p].tobytes() for p in PLANES), (name, form, order)
        G.set_query_order(accel, 0)
        forms.append(form)
    assert "reference" in forms and "prune" in forms, forms


# ---- 9: each plane alone, subsets over garbage -------------------------------------------------------------------------------------------------------
def test_each_plane_alone_and_subsets_over_garbage():
    _, _, segs, want, _ = SC.case("own")
    accel = accel_of("own")
    radius = C.radii(want)[2]
    n = 64 * 20 + 9
    q = np.ascontiguousarray(segs[500:500 + n])
    full = G.closest_segments(accel, q, radius=radius)
    same("slice", full, cut(SC.references("own")[2], 500, 500 + n))
    rng = np.random.default_rng(5)
    subsets = [(p,) for p in PLANES] + [("touch", "id"), ("distance", "param"), ("point", "id"), ("touch", "param", "point"), PLANES]
    for planes in subsets:
        bufs = {p: rng.integers(1, 256, full[p].nbytes, dtype=np.uint8).view(DT[p]).reshape(full[p].shape) for p in PLANES}
        for p in PLANES:
            if p not in planes:
                bufs[p].view(np.uint8)[...] = 0xA5
        out = G.closest_segments(accel, q, radius=radius, planes=planes, into={p: bufs[p] for p in planes})
        assert all(out[p] is bufs[p] and out[p].tobytes() == full[p].tobytes() for p in planes), planes
        assert all((bufs[p].view(np.uint8) == 0xA5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", planes)


# ---- 10: the device form on a second stream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "torus"])
def test_the_device_form_on_a_second_stream_between_guard_words(name):
    torch = pytest.importorskip("torch")
    _, _, segs, _, _ = SC.case(name)
    accel = accel_of(name)
    n = len(segs)
    radii = SC.mixed_radii(name, 30)
    ref = G.closest_segments(accel, segs, radii=radii)
    same((name, "mixed radii"), ref, SC.references(name)[4])
    dsegs, dradii = torch.from_numpy(segs).cuda(), torch.from_numpy(radii).cuda()
    stream = torch.cuda.Stream()
    for planes in (PLANES, ("touch",), ("distance", "param"), ("point", "id")):
        dev = {p: torch.full((GUARD + n * BYTES[p] + GUARD,), FILL, dtype=torch.uint8, device="cuda") for p in PLANES}
        assert all(dev[p].data_ptr() % 16 == 0 for p in PLANES)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            assert s != 0
            ptrs = {p + "_ptr": dev[p].data_ptr() + GUARD for p in planes}
            for _ in range(2):  # the second call runs over the first one's results
                G.closest_segments_device(accel, n, dsegs.data_ptr(), dradii.data_ptr(), stream=s, **ptrs)
        stream.synchronize()
        for p in PLANES:
            back = dev[p].cpu().numpy()
            if p in planes:
                assert (back[:GUARD] == FILL).all() and (back[GUARD + n * BYTES[p]:] == FILL).all(), (name, p, "nothing is written outside the plane")
                assert back[GUARD:GUARD + n * BYTES[p]].tobytes() == ref[p].tobytes(), (name, planes, p)
            else:
                assert (back == FILL).all(), (name, planes, p, "not asked for")


# ---- 11: the depth-8 scenes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.LIMIT_SCENES))
def test_the_depth_8_scenes_match_the_brute_force_or_are_refused_where_the_rules_say(name):
    _, b, pts, closest = C.case(name)
    verdict = C.gate(b.cat)
    depth = G.scene_closest_depth(C.builder(name)(G))
    accel = accel_of(name)
    rng = np.random.default_rng(12)
    n = 1025
    lo, hi = C.world_bounds(b)
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    p0 = pts[:n]
    reach = np.where(np.arange(n) % 4 == 0, 0.0, rng.uniform(0.01, 1.0, n) ** 3 * diag)[:, None]
    d = rng.normal(0.0, 1.0, (n, 3))
    segs = np.ascontiguousarray(np.concatenate([p0, p0 + d / np.sqrt((d * d).sum(axis=1))[:, None] * reach], axis=1))
    if verdict >= 0:
        with pytest.raises(la.LasgunError, match="instance %d " % verdict):
            G.closest_segments(accel, segs)
        return
    if depth > G.CLOSEST_MAX_DEPTH:
        with pytest.raises(la.LasgunError, match="need a stack of"):
            G.closest_segments(accel, segs)
        return
    radius = C.radii(closest)[2]
    want = SR.closest_segments(b, segs, [radius, INF])
    print("closest segments, %s: a stack of %d entries, %d KiB of dynamic LDS a workgroup" % (name, depth, 256 * 8 * depth // 1024))
    same((name, radius), G.closest_segments(accel, segs, radius=radius), want[0], accel, b)
    same((name, INF), G.closest_segments(accel, segs), want[1])
    assert G.closest_segments(accel, segs, radius=radius, planes=("touch",))["touch"].tobytes() == want[0]["touch"].tobytes()


# ---- 12: 40 lights -------------------------------------------------------------------------------------------------------------------------------------
def test_a_scene_with_40_lights_is_accepted():
    accel = G.Accel.from_scene(many_lights_scene(G, 40))
    b = R.Brute(many_lights_scene(pyref.Api, 40))
    rng = np.random.default_rng(9)
    p0 = rng.uniform(-3.0, 3.0, (257, 3))
    segs = np.ascontiguousarray(np.concatenate([p0, p0 + rng.normal(0.0, 1.0, (257, 3))], axis=1))
    same("40 lights", G.closest_segments(accel, segs, radius=2.0), SR.closest_segments(b, segs, [2.0])[0])


# ---- 13: errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_error_leaves_its_outputs_untouched():
    torch = pytest.importorskip("torch")
    _, _, segs, _, _ = SC.case("own")
    accel = accel_of("own")
    n = 100
    q = np.ascontiguousarray(segs[:n])
    host = {"touch": np.full(n, 7, dtype=np.uint8), "distance": np.full(n, 7.0), "param": np.full(n, 7.0), "point": np.full((n, 3), 7.0), "id": np.full((n, 4), 7, dtype=np.uint32)}
    dq = torch.from_numpy(segs[:n + 1].copy()).cuda()
    dr = torch.ones(n + 1, dtype=torch.float64, device="cuda")
    dev = {p: torch.full(((n + 1) * BYTES[p],), FILL, dtype=torch.uint8, device="cuda") for p in PLANES}
    ptr = {p + "_ptr": dev[p].data_ptr() for p in PLANES}
    cpu = torch.zeros(n * 6, dtype=torch.float64)
    # For "a buffer that ends beyond its allocation" the buffer has to BE an allocation: torch hands small tensors out of blocks of its own,
    # and the library can only see where a block ends.  12 MiB are a block of their own (tests/test_gpu_closest_points.py does the same)
    torch.cuda.empty_cache()
    many = 1 << 19
    short_point = torch.full((many * 24,), FILL, dtype=torch.uint8, device="cuda")
    long_point = torch.full(((many + 1) * 24,), FILL, dtype=torch.uint8, device="cuda")
    long_segs = torch.zeros((many * 3 + 1, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    refused = C.builder("chain8_shallow")(G)
    bad = [lambda: G.closest_segments(accel, q, radius=-1.0, into=host),
           lambda: G.closest_segments(accel, q, radius=float("nan"), into=host),
           lambda: G.closest_segments(accel, q, radius=-INF, into=host),
           lambda: G.closest_segments(accel, q, planes=(), into=host),
           lambda: G.closest_segments(G.Accel.from_scene(refused), q, into=host),
           lambda: G.closest_segments_device(accel, n, 0, None, INF, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), None, INF, stream=0),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), None, -1.0, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr() + 4, None, INF, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), dr.data_ptr() + 4, INF, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), None, INF, stream=0, **dict(ptr, id_ptr=dev["id"].data_ptr() + 8)),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), None, INF, stream=0, **dict(ptr, param_ptr=dev["param"].data_ptr() + 4)),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), None, INF, stream=0, **dict(ptr, distance_ptr=dev["distance"].data_ptr() + 4)),
           lambda: G.closest_segments_device(accel, many + 1, long_segs, None, INF, point_ptr=short_point, stream=0),
           lambda: G.closest_segments_device(accel, many * 3 + 1, long_segs, short_point, INF, touch_ptr=long_point, stream=0),  # (as radii: 8 bytes a segment)
           lambda: G.closest_segments_device(accel, many // 2 + 1, short_point, None, INF, touch_ptr=long_point, stream=0),  # (as segments: 48 bytes each, one too many)
           lambda: G.closest_segments_device(accel, n, cpu.data_ptr(), None, INF, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, n, dq.data_ptr(), cpu.data_ptr(), INF, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, (2 ** 32 - 1) * 64 + 1, dq.data_ptr(), None, INF, stream=0, **ptr),
           lambda: G.closest_segments_device(accel, 2 ** 63, dq.data_ptr(), None, INF, stream=0, **ptr)]
    for i, f in enumerate(bad):
        with pytest.raises(la.LasgunError):
            f()
        assert G.last_error(), i
    for f in (lambda: G.closest_segments(accel, q[:, :3], into=host), lambda: G.closest_segments(accel, q, radii=np.ones(n - 1), into=host),
              lambda: G.closest_segments(accel, q, planes=("count",), into=host)):
        with pytest.raises(ValueError):
            f()
    torch.cuda.synchronize()
    assert all((host[p] == 7).all() for p in PLANES), "an error touches no host output"
    assert all((dev[p].cpu().numpy() == FILL).all() for p in PLANES), "nor a device output"
    assert bool((short_point == FILL).all()) and bool((long_point == FILL).all())
    for what, call in (("point", bad[13]), ("radii", bad[14]), ("segments", bad[15])):
        with pytest.raises(la.LasgunError, match=what + " ends beyond its allocation"):
            call()
    with pytest.raises(la.LasgunError, match="instance 1 "):
        G.closest_segments(G.Accel.from_scene(refused), q)
    G.closest_segments_device(accel, 0, 0, None, -1.0, stream=0)  # n == 0 is answered before every other check
    assert all(len(v.reshape(-1)) == 0 for v in G.closest_segments(accel, np.zeros((0, 6)), radius=-1.0).values())
    ok = G.closest_segments(accel, q, radii=np.ones(n), radius=float("nan"), planes=("touch", "param"), into={p: host[p] for p in ("touch", "param")})
    assert (ok["touch"] <= 1).all() and not (ok["param"] == 7.0).all(), "legal: a NaN shared radius beside radii"
