"""The opt-in ray order of ray queries (include/lasgun_hip.h: lg_accel_set_query_order, lg_query_order*; k_sort.hip, raykey.h):
  1. the same bytes: every query answers with order 1 (rays keyed and sorted on the device, walked through the permutation) exactly what it
     answers with order 0, in the caller's slots -- every traversal form, closest hit and occlusion, output arrays prefilled with 0xA5 so
     that a slot never written, or written for the wrong ray, shows; a sample of the sorted answers against the independent witness;
  2. the order: perm is the stable ascending sort of the keys, the same on every call, the same from the host and the device form;
  3. the key is not degenerate (a constant key would pass 1 and 2);
  4. the setting: default, round trip, invalid values, bad buffers rejected before any launch."""
import numpy as np
import pytest

import pyref

import edge_rays as E
import lasgun_amd as la
from lasgun_amd import scenes as S
from query_witness import Witness, portable_trig, same
from test_gpu_ray_query import same_material, seeded_rays

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = la.api
INF = float("inf")
if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference never reads it, camera.rs:142)
    pyref.Camera.set_aperture_radius = lambda self, radius: self


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def query(accel, rays, order):
    """(hit bytes, occlusion bytes) of `rays` through the device entry points, both output arrays prefilled with 0xA5."""
    n = len(rays)
    G.set_query_order(accel, order)
    dr = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64).copy()).cuda()
    dh = torch.full((max(n, 1) * 96,), 0xA5, dtype=torch.uint8, device="cuda")
    do = torch.full((max(n, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    G.intersect_device(accel, n, dr.data_ptr(), dh.data_ptr(), stream=0)
    G.occluded_device(accel, n, dr.data_ptr(), do.data_ptr(), stream=0)
    torch.cuda.synchronize()
    G.set_query_order(accel, 0)
    return dh.cpu().numpy()[: n * 96].tobytes(), do.cpu().numpy()[:n].tobytes()


def scene_box(accel):
    """A box around what the camera sees of the scene (the hit points of a coarse film), for rays that have something to meet."""
    cam = G.camera_rays(accel, 48, 48)
    hits = G.intersect(accel, cam)
    p = hits["p"][hits["kind"] != 0]
    assert len(p) > 16
    return p.min(axis=0) - 0.25, p.max(axis=0) + 0.25


def ray_sets(accel, seed):
    """[(name, rays)]: shuffled camera rays, random rays through the bounds, the edge-case rays, identical rays, small and odd counts."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(accel)
    cam = G.camera_rays(accel, 96, 96)
    cam = cam[rng.permutation(len(cam))]
    cam[:, 3:] *= rng.uniform(0.05, 4.0, (len(cam), 1))  # (t < 1 and t >= 1 both occur)
    n = 6000
    o = rng.uniform(lo - (hi - lo), hi + (hi - lo), (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d[n // 2:] = rng.normal(0.0, 1.0, (n - n // 2, 3))
    rand = np.concatenate([o, d * rng.uniform(0.3, 3.0, (n, 1))], axis=1)
    edge, _ = E.edge_rays(lo, hi, seed=seed)
    same_ray = np.tile(cam[:1], (5000, 1))
    sets = [("camera, shuffled", cam), ("random", rand), ("edge", edge), ("identical", same_ray)]
    sets += [("n=%d" % k, rand[:k]) for k in (1, 63, 64, 65, 4133)]
    return sets


def traversal_forms(accel):
    """(name, setup) of every traversal form the accel accepts: reference, pruned, LDS-resident, LDS + pruned, fast."""
    def ref():
        G.set_mode(accel, False)
        G.set_prune(accel, False)
        G.set_lds_scene(accel, False)
    out = [("reference", ref), ("prune", lambda: (ref(), G.set_prune(accel, True)))]
    ref()
    if G.set_lds_scene(accel, True):
        out += [("lds", lambda: (ref(), G.set_lds_scene(accel, True))),
                ("lds+prune", lambda: (ref(), G.set_prune(accel, True), G.set_lds_scene(accel, True)))]
    ref()
    try:
        G.set_mode(accel, True)
    except la.LasgunError:
        pass  # (a scene the fast mode refuses)
    else:
        out.append(("fast", lambda: (ref(), G.set_mode(accel, True))))
    ref()
    return out


SCENES = [("spheres", lambda: S.spheres_scene(G), ("reference", "lds")),
          ("mesh", lambda: S.mesh_scene(G, nu=96, nv=96, material="metal"), ("reference", "prune")),
          ("mixed", lambda: S.mixed_scene(G, nspheres=256, nu=64, nv=64), ("reference", "prune")),
          ("instanced", lambda: S.instanced_scene(G), ("reference",)),
          ("kitchen_sink", lambda: S.kitchen_sink_scene(G), ("reference",))]


# ---- 1: the same bytes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder,required", SCENES, ids=[s[0] for s in SCENES])
def test_sorted_order_gives_identical_bytes_in_every_form(name, builder, required):
    accel = G.Accel.from_scene(builder())
    sets = ray_sets(accel, 100 + len(name))
    forms = traversal_forms(accel)
    assert set(required) <= set(f for f, _ in forms), (name, [f for f, _ in forms])
    some_hit = some_occ = False
    for form, setup in forms:
        for label, rays in sets:
            setup()
            h0, o0 = query(accel, rays, 0)
            setup()
            h1, o1 = query(accel, rays, 1)
            assert h1 == h0, (name, form, label, "closest hits differ")
            assert o1 == o0, (name, form, label, "occlusion bytes differ")
            assert set(o0) <= {0, 1}, (name, form, label)
            hits = np.frombuffer(h0, dtype=la.HIT_DTYPE)
            some_hit = some_hit or bool((hits["kind"] != 0).any())
            some_occ = some_occ or 1 in set(o0)
    assert some_hit and some_occ, name


def test_sorted_order_through_the_host_forms():
    accel = G.Accel.from_scene(S.mixed_scene(G, nspheres=256, nu=64, nv=64))
    for label, rays in ray_sets(accel, 5):
        G.set_query_order(accel, 0)
        h0, o0 = G.intersect(accel, rays), G.occluded(accel, rays)
        G.set_query_order(accel, 1)
        h1, o1 = G.intersect(accel, rays), G.occluded(accel, rays)
        assert h1.tobytes() == h0.tobytes() and np.array_equal(o0, o1), label
    assert G.get_query_order(accel) == 1
    # nothing to do is still nothing to do
    assert len(G.intersect(accel, np.zeros((0, 6)))) == 0 and len(G.occluded(accel, np.zeros((0, 6)))) == 0


@pytest.mark.parametrize("name,builder", [("kitchen_sink", lambda api: S.kitchen_sink_scene(api)), ("instanced", lambda api: S.instanced_scene(api))],
                         ids=["kitchen_sink", "instanced"])
def test_sorted_answers_match_the_witness(name, builder):
    gscene, pscene = builder(G), builder(pyref.Api)
    accel = G.Accel.from_scene(gscene)
    wit = Witness(pscene)
    rays = seeded_rays(pscene, 2000 + len(name))
    assert len(rays) > 128  # (several tiles: the rays are walked through the permutation)
    G.set_query_order(accel, 1)
    hits = G.intersect(accel, rays)
    occ = G.occluded(accel, rays)
    n_hit = 0
    with portable_trig():
        for i, ray in enumerate(rays):
            h, want = hits[i], wit.closest(ray[:3], ray[3:])
            if want is None:
                assert h["t"] == INF and h["kind"] == 0 and h["material"] == -1, (name, i, ray, h)
                assert not occ[i], (name, i)
                continue
            n_hit += 1
            assert same(h["t"], want["t"]), (name, i, ray, h["t"], want["t"])
            assert (int(h["kind"]), int(h["prim"]), int(h["instance"])) == want["id"], (name, i, ray, h, want["id"])
            assert same_material(G.accel_material(accel, int(h["material"])), want["mat"]), (name, i)
            for k in ("p", "ng", "ns"):
                assert all(same(a, b) for a, b in zip(h[k], want[k])), (name, i, k, list(h[k]), want[k])
            assert bool(occ[i]) == (want["t"] < 1.0), (name, i)
    assert n_hit >= len(rays) // 5, (name, n_hit, len(rays))


# ---- 2: the order -------------------------------------------------------------------------------------------------------------------
def test_perm_is_the_stable_sort_of_the_keys():
    accel = G.Accel.from_scene(S.mixed_scene(G, nspheres=256, nu=64, nv=64))
    stream = torch.cuda.Stream()
    for label, rays in ray_sets(accel, 9) + [("n=0", np.zeros((0, 6)))]:
        n = len(rays)
        perm, keys = G.query_order(accel, rays)
        assert perm.dtype == np.uint32 and keys.dtype == np.uint32 and len(perm) == n and len(keys) == n
        assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32)), label
        perm2, keys2 = G.query_order(accel, rays)
        assert np.array_equal(perm, perm2) and np.array_equal(keys, keys2), label
        # the device form on a torch stream; with and without the keys
        dr = torch.from_numpy(np.ascontiguousarray(rays).copy()).cuda()
        dp = torch.full((max(n, 1),), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
        dk = torch.full((max(n, 1),), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
        dp2 = dp.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            G.query_order_device(accel, n, dr.data_ptr(), dp.data_ptr(), dk.data_ptr(), stream=s)
            G.query_order_device(accel, n, dr.data_ptr(), dp2.data_ptr(), None, stream=s)
        stream.synchronize()
        if n:
            assert np.array_equal(dp.cpu().numpy().view(np.uint32), perm), label
            assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys), label
            assert np.array_equal(dp2.cpu().numpy().view(np.uint32), perm), label
        else:
            assert (dp.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all() and (dk.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()


def test_a_big_order_is_a_permutation_and_sorted():
    """More rays than one pass's chunks of the smallest size: several rounds per workgroup, a last partial round."""
    accel = G.Accel.from_scene(S.spheres_scene(G))
    rng = np.random.default_rng(3)
    cam = G.camera_rays(accel, 1200, 1000)
    rays = cam[rng.permutation(len(cam))][: 1150037]
    rays[: 300000, :3] += rng.normal(0.0, 2.0, (300000, 3))
    perm, keys = G.query_order(accel, rays)
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32))


# ---- 3: the key is not degenerate ---------------------------------------------------------------------------------------------------
def test_the_key_separates_directions_and_origins():
    accel = G.Accel.from_scene(S.spheres_scene(G))
    cam = G.camera_rays(accel, 256, 256)
    assert len(cam) == 256 * 256
    # identical rays, identical keys
    _, keys = G.query_order(accel, np.tile(cam[1234:1235], (300, 1)))
    assert len(set(keys.tolist())) == 1
    # the camera rays of opposite film corners
    _, keys = G.query_order(accel, cam[[0, len(cam) - 1]])
    assert keys[0] != keys[1]
    # the shuffled camera rays of a 256^2 film: more than one distinct key per 64 rays
    rng = np.random.default_rng(1)
    _, keys = G.query_order(accel, cam[rng.permutation(len(cam))])
    assert len(np.unique(keys)) > len(cam) // 64, len(np.unique(keys))
    # one direction from opposite corners of the scene's bounds
    grid = G.Accel.from_scene(E.grid_scene(G))
    lo, hi = E.GRID_BOUNDS
    d = (0.3, -0.2, -1.0)
    _, keys = G.query_order(grid, np.array([tuple(lo) + d, tuple(hi) + d]))
    assert keys[0] != keys[1]
    # degenerate input gets some key, the same one every time
    nan = float("nan")
    odd = np.array([(0.0,) * 6, (nan,) * 6, (INF, -INF, nan, 0.0, 0.0, 0.0), (1e300, -1e300, 0.0, INF, -INF, 1.0), (0.0, 0.0, 0.0, 5e-324, 0.0, 0.0)] * 30)
    p1, k1 = G.query_order(grid, odd)
    p2, k2 = G.query_order(grid, odd)
    assert np.array_equal(p1, p2) and np.array_equal(k1, k2) and np.array_equal(p1, np.argsort(k1, kind="stable").astype(np.uint32))
    assert all(len(set(k1[j::5].tolist())) == 1 for j in range(5))


# ---- 4: settings --------------------------------------------------------------------------------------------------------------------
def test_setting_round_trip_and_invalid_values():
    accel = G.Accel.from_scene(S.spheres_scene(G, nspheres=64))
    assert G.get_query_order(accel) == 0
    G.set_query_order(accel, 1)
    assert G.get_query_order(accel) == 1
    for bad in (2, -1, 7):
        with pytest.raises(la.LasgunError) as e:
            G.set_query_order(accel, bad)
        assert str(e.value)
        assert G.get_query_order(accel) == 1
    G.set_query_order(accel, 0)
    assert G.get_query_order(accel) == 0


def test_order_entry_points_reject_bad_buffers_and_launch_nothing():
    accel = G.Accel.from_scene(S.spheres_scene(G, nspheres=64))
    n = 1000
    rays = G.camera_rays(accel, 40, 26)[: n + 1]
    dr = torch.from_numpy(rays.copy()).cuda()
    dp = torch.full((n + 1,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
    dk = dp.clone()
    host = np.zeros(n, dtype=np.uint32)
    # an allocation of its own (nothing cached to carve it from; 32 MiB is a whole number of the allocator's 2 MiB units): its end is known
    torch.cuda.empty_cache()
    own_bytes = 32 << 20
    own = torch.full((own_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    short = own.data_ptr() + own_bytes - 4 * (n - 1)  # room for n - 1 words
    torch.cuda.synchronize()
    bad = [lambda: G.query_order_device(accel, n, 0, dp.data_ptr(), dk.data_ptr(), stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), 0, dk.data_ptr(), stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr() + 4, dp.data_ptr(), dk.data_ptr(), stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), dp.data_ptr() + 2, dk.data_ptr(), stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), dp.data_ptr(), dk.data_ptr() + 2, stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), host.ctypes.data, dk.data_ptr(), stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), dp.data_ptr(), host.ctypes.data, stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), short, dk.data_ptr(), stream=0),
           lambda: G.query_order_device(accel, n, dr.data_ptr(), dp.data_ptr(), short, stream=0)]
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    torch.cuda.synchronize()
    assert (dp.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all() and (dk.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
    assert (own.cpu().numpy() == 0xA5).all() and (host == 0).all()
    # the same buffers, rightly used, are accepted
    G.query_order_device(accel, n - 1, dr.data_ptr(), short, dk.data_ptr(), stream=0)
    torch.cuda.synchronize()
    assert np.array_equal(np.sort(own.cpu().numpy()[own_bytes - 4 * (n - 1):].view(np.uint32)), np.arange(n - 1, dtype=np.uint32))
