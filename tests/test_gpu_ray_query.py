"""Ray queries (include/lasgun_hip.h: lg_intersect*, lg_occluded*, lg_camera_rays*, lg_accel_material, lg_accel_instance) against the
independent witness: tests/pyref.py walking the reference's BVH (tests/pyref_bvh.py), wrapped (tests/query_witness.py) so that it says WHICH primitive
won -- (kind, prim, instance) in the numbering of lg_hit -- and with the sphere's trigonometry taken from the oracle's portable functions
(orc_math_eval ops 2-5, the algorithms the device runs) so that sphere normals compare bit for bit as well."""
import numpy as np
import pytest

import pyref

import lasgun_amd as la
from lasgun_amd import scenes as S
from query_witness import Witness, bits, pod, portable_trig, same

pytestmark = pytest.mark.gpu

G = la.api
INF = float("inf")
if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference accepts it and never reads it, camera.rs:142)
    pyref.Camera.set_aperture_radius = lambda self, radius: self


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def same_material(lib_mat, want):
    kind, flat = pod(want)
    return lib_mat["kind"] == kind and [bits(v) for v in lib_mat["p"][:len(flat)]] == flat


def scene_pair(builder, *args, **kw):
    return builder(G, *args, **kw), builder(pyref.Api, *args, **kw)


def world_points(scene):
    """Centres of the root aggregate's spheres and boxes in world space, and the spheres' radii (inf for boxes)."""
    out = []
    tr = scene.root.transform
    for node in scene.root.contents:
        if node[0] == "sphere":
            out.append((pyref.transform_point(tr.m, node[1]), node[2]))
        elif node[0] == "cuboid":
            out.append((pyref.transform_point(tr.m, tuple(0.5 * (a + b) for a, b in zip(node[1], node[2]))), INF))
    return out


def seeded_rays(pscene, seed, n_random=160, extent=4.0):
    """Random origins and directions; rays from inside spheres and boxes; axis-parallel directions with zero components; a few with
    infinite and NaN components."""
    rng = np.random.default_rng(seed)
    rays = []
    eye = np.array(pscene.camera.origin, dtype=np.float64)
    for _ in range(n_random):
        o = rng.uniform(-extent, extent, 3) if rng.random() < 0.5 else eye + rng.normal(0.0, 0.3, 3)
        target = rng.uniform(-extent / 2, extent / 2, 3)
        d = target - o if rng.random() < 0.7 else rng.normal(0.0, 1.0, 3)
        rays.append(np.concatenate([o, d * rng.uniform(0.2, 3.0)]))
    for c, r in world_points(pscene)[:24]:
        o = np.array(c) + (rng.normal(0.0, 0.05, 3) if r == INF else rng.normal(0.0, min(r, 1.0) * 0.2, 3))
        rays.append(np.concatenate([o, rng.normal(0.0, 1.0, 3)]))
    for k in range(24):
        d = np.zeros(3)
        d[k % 3] = (-1.0) ** k * rng.uniform(0.5, 2.0)
        if k >= 12:
            d[(k + 1) % 3] = rng.uniform(-0.5, 0.5)  # one zero component
        rays.append(np.concatenate([rng.uniform(-extent, extent, 3), d]))
    nan = float("nan")
    for o, d in [((0.0, 0.0, 9.0), (0.0, 0.0, -INF)), ((0.0, 0.5, 9.0), (INF, 0.0, -1.0)), ((0.0, 0.0, 9.0), (nan, 0.0, -1.0)),
                 ((nan, 0.0, 9.0), (0.0, 0.0, -1.0)), ((0.0, 0.0, 9.0), (0.0, 0.0, 0.0)), ((INF, 0.0, 0.0), (-1.0, 0.0, 0.0))]:
        rays.append(np.array(o + d))
    return np.array(rays, dtype=np.float64)


WITNESS_SCENES = [("kitchen_sink", lambda api: S.kitchen_sink_scene(api)),
                  ("instanced", lambda api: S.instanced_scene(api)),
                  ("tie_mesh", lambda api: S.tie_mesh_scene(api)),
                  ("exotic_obj", lambda api: S.exotic_obj_scene(api))] + \
                 [("random_%d" % s, (lambda s: lambda api: S.random_scene(api, s))(s)) for s in (1, 2, 3, 4)]


# ---- 1: closest hit (and 3b: occlusion) against the witness ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", WITNESS_SCENES, ids=[n for n, _ in WITNESS_SCENES])
def test_closest_hit_matches_the_witness(name, builder):
    gscene, pscene = builder(G), builder(pyref.Api)
    accel = G.Accel.from_scene(gscene)
    wit = Witness(pscene)
    rays = seeded_rays(pscene, 1000 + len(name))
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


# ---- 2 / 3: the render's own rays give the render's own hits and shadow verdicts ------------------------------------------------------
@pytest.mark.parametrize("camera", ["perspective", "orthographic"])
def test_camera_rays_and_the_renders_own_hits(camera):
    gscene, pscene = scene_pair(S.kitchen_sink_scene, camera=camera, supersampling=1)
    accel = G.Accel.from_scene(gscene)
    w, h, x0, y0, x1, y1 = 64, 48, 4, 6, 60, 42
    rays = G.camera_rays(accel, w, h, x0, y0, x1, y1)
    assert G.camera_samples(accel) == 4 and rays.shape == ((x1 - x0) * (y1 - y0) * 4, 6)
    want = np.array([np.concatenate([o, d]) for y in range(y0, y1) for x in range(x0, x1) for o, d in pscene.camera.sample(x, y, w, h)])
    assert np.array_equal(rays.view(np.int64), want.view(np.int64))
    first = rays[::4]
    hits = G.intersect(accel, first)
    segs, expect = [], []
    for k, (y, x) in enumerate((y, x) for y in range(y0, y1) for x in range(x0, x1)):
        tp = G.trace_pixel(accel, w, h, x, y)
        if tp["ref"] == 0xFFFFFFFF:
            assert hits[k]["kind"] == 0
            continue
        assert bits(hits[k]["t"]) == bits(tp["t"]) and int(hits[k]["instance"]) == tp["accel"], (x, y, hits[k], tp)
        o = np.array(tp["shadow_origin"])
        for (lpos, _, _), (st, _) in zip(pscene.lights, tp["shadow"]):
            segs.append(np.concatenate([o, np.array(lpos) - o]))
            expect.append(st < 1.0)
    assert len(segs) > 300 and len(segs) % len(pscene.lights) == 0, len(segs)
    assert np.array_equal(G.occluded(accel, np.array(segs)), np.array(expect))


# ---- 4: every traversal form gives the same bytes ----------------------------------------------------------------------------------
def big_batch(accel, seed, n=(1 << 20) + 37):
    """The camera's rays of a 1024 x 1024 film (coherent; every form of the walk meets hits, misses and near-ties of box faces), then
    random rays from near the camera (incoherent), each direction scaled by a random factor so that t < 1 and t >= 1 both occur."""
    rng = np.random.default_rng(seed)
    cam = G.camera_rays(accel, 1024, 1024)[: n]
    extra = n - cam.shape[0]
    o = cam[0, :3] + rng.normal(0.0, 0.3, (extra, 3))
    d = cam[rng.integers(0, cam.shape[0], extra), 3:] + rng.normal(0.0, 0.2, (extra, 3))
    rays = np.concatenate([cam, np.concatenate([o, d], axis=1)])
    rays[:, 3:] *= rng.uniform(0.05, 4.0, (n, 1))
    return rays


FORM_SCENES = [("spheres", lambda: S.spheres_scene(G)), ("mesh", lambda: S.mesh_scene(G, nu=96, nv=96, material="metal")),
               ("mixed", lambda: S.mixed_scene(G, nspheres=256, nu=64, nv=64))]


@pytest.mark.parametrize("name,builder", FORM_SCENES, ids=[n for n, _ in FORM_SCENES])
def test_every_traversal_form_gives_identical_bytes(name, builder):
    accel = G.Accel.from_scene(builder())
    rays = big_batch(accel, 7)
    G.set_prune(accel, False)
    fits = G.set_lds_scene(accel, False)
    ref_h, ref_o = G.intersect(accel, rays).tobytes(), G.occluded(accel, rays)
    assert ref_h and ref_o.any() and not ref_o.all()
    mid = (1 << 19) - 31  # (where the coherent rays of the batch both hit and miss)

    def small(form):
        """Launches of one tile, full or not, and of two: a ray's answer does not depend on the batch it comes in."""
        for n in (1, 63, 64, 65):
            assert G.intersect(accel, rays[mid:mid + n]).tobytes() == ref_h[96 * mid:96 * (mid + n)], (name, form, n)
            assert np.array_equal(G.occluded(accel, rays[mid:mid + n]), ref_o[mid:mid + n]), (name, form, n)

    small("reference")
    forms = [("prune", lambda: G.set_prune(accel, True))]
    if fits:
        forms += [("lds", lambda: (G.set_prune(accel, False), G.set_lds_scene(accel, True))),
                  ("lds+prune", lambda: (G.set_prune(accel, True), G.set_lds_scene(accel, True)))]
    checked = []
    for form, setup in forms:
        setup()
        assert G.intersect(accel, rays).tobytes() == ref_h, (name, form)
        assert np.array_equal(G.occluded(accel, rays), ref_o), (name, form)
        small(form)
        checked.append(form)
    if name != "spheres":
        G.set_prune(accel, None)
        G.set_lds_scene(accel, True)
        try:
            G.set_mode(accel, True)
        except la.LasgunError:
            pass  # (a scene the fast mode refuses)
        else:
            assert G.intersect(accel, rays).tobytes() == ref_h, (name, "fast")
            assert np.array_equal(G.occluded(accel, rays), ref_o), (name, "fast")
            small("fast")
            checked.append("fast")
            G.set_mode(accel, False)
    assert checked


# ---- 5: device entry points -----------------------------------------------------------------------------------------------------
def test_device_entry_points_on_a_torch_stream():
    torch = pytest.importorskip("torch")
    gscene, pscene = scene_pair(S.instanced_scene)
    accel = G.Accel.from_scene(gscene)
    rays_all = big_batch(accel, 11, n=64 * 1024 + 1)
    stream = torch.cuda.Stream()
    for n in (0, 1, 64 * 1024 + 1):
        rays = rays_all[:n]
        want_h, want_o = G.intersect(accel, rays), G.occluded(accel, rays)
        dr = torch.from_numpy(rays.copy()).cuda()
        dh = torch.full((max(n, 1) * 96,), 0xAB, dtype=torch.uint8, device="cuda")
        do = torch.full((max(n, 1),), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s = torch.cuda.current_stream().cuda_stream
            G.intersect_device(accel, n, dr.data_ptr(), dh.data_ptr(), stream=s)
            G.occluded_device(accel, n, dr.data_ptr(), do.data_ptr(), stream=s)
        stream.synchronize()
        if n:
            assert dh.cpu().numpy().tobytes() == want_h.tobytes(), n
            assert np.array_equal(do.cpu().numpy().astype(bool), want_o), n
        else:
            assert (dh.cpu().numpy() == 0xAB).all() and (do.cpu().numpy() == 0xAB).all()
    # the camera's rays, device form
    w, h = 64, 48
    cam = torch.zeros((w * h * G.camera_samples(accel), 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, w, h, 0, 0, w, h, cam.data_ptr(), stream=0)
    torch.cuda.synchronize()
    assert np.array_equal(cam.cpu().numpy().view(np.int64), G.camera_rays(accel, w, h).view(np.int64))


def test_device_entry_points_reject_bad_buffers_and_launch_nothing():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(S.spheres_scene(G, nspheres=64))
    n = 100
    dr = torch.from_numpy(big_batch(accel, 3, n=n + 1)).cuda()
    dh = torch.full(((n + 1) * 96,), 0xAB, dtype=torch.uint8, device="cuda")
    do = torch.full((n + 1,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = [lambda: G.intersect_device(accel, n, 0, dh.data_ptr(), stream=0),
           lambda: G.intersect_device(accel, n, dr.data_ptr(), 0, stream=0),
           lambda: G.occluded_device(accel, n, 0, do.data_ptr(), stream=0),
           lambda: G.occluded_device(accel, n, dr.data_ptr(), 0, stream=0),
           lambda: G.intersect_device(accel, n, dr.data_ptr() + 4, dh.data_ptr(), stream=0),
           lambda: G.intersect_device(accel, n, dr.data_ptr(), dh.data_ptr() + 8, stream=0),
           lambda: G.occluded_device(accel, n, dr.data_ptr() + 4, do.data_ptr(), stream=0),
           lambda: G.camera_rays_device(accel, 8, 8, 0, 0, 8, 8, dr.data_ptr() + 4, stream=0),
           lambda: G.camera_rays_device(accel, 8, 8, 0, 0, 8, 8, 0, stream=0),
           lambda: G.camera_rays_device(accel, 8, 8, 0, 0, 9, 8, dr.data_ptr(), stream=0)]
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    torch.cuda.synchronize()
    assert (dh.cpu().numpy() == 0xAB).all() and (do.cpu().numpy() == 0xAB).all()
    with pytest.raises(la.LasgunError):
        G.accel_material(accel, 10 ** 6)
    with pytest.raises(la.LasgunError):
        G.accel_instance(accel, 10 ** 6)


# ---- 6: lookups ---------------------------------------------------------------------------------------------------------------
def lookup_scene(api):
    """Every sphere and box with a material of its own, a mesh added without a material inside a group, one with a material."""
    scene = api.Scene.new()
    cam = scene.set_perspective_camera(50.0)
    cam.look_at([0.0, 0.0, 10.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    M = api.Material
    mesh = scene.parse_obj(S.PLANE_OBJ)
    for i in range(6):
        scene.root.add_sphere([-3.0 + 1.2 * i, 1.5, 0.0], 0.4, M.matte([0.1 * i, 0.5, 0.2], 3.0 * i))
        scene.root.add_box([-3.3 + 1.2 * i, -0.3, -0.3], [-2.7 + 1.2 * i, 0.3, 0.3], M.plastic([0.2, 0.1 * i, 0.3], [0.5, 0.5, 0.5], 0.05 * (i + 1)))
    g = api.Aggregate.new()
    g.rotate_x(90.0).translate([0.0, -2.0, 0.0])
    g.add_obj(mesh)
    inner = api.Aggregate.new()
    inner.translate([2.5, 0.0, 0.0])
    inner.add_obj_of(mesh, M.metal([0.2, 0.9, 1.1], [3.9, 2.4, 2.2], 0.1, 0.2))
    g.add_group(inner)
    scene.root.add_group(g)
    return scene, mesh


def test_material_and_instance_lookups():
    gscene, mesh = lookup_scene(G)
    pscene, _ = lookup_scene(pyref.Api)
    accel = G.Accel.from_scene(gscene)
    wit = Witness(pscene)
    targets = [c for c, _ in world_points(pscene)] + [(0.0, -2.0, 0.0), (2.5, -2.0, 0.0), (-0.5, -2.0, 0.4), (2.2, -2.0, -0.3)]
    rays = np.array([(0.0, 0.0, 10.0) + tuple(np.array(t) - np.array([0.0, 0.0, 10.0])) for t in targets])
    hits = G.intersect(accel, rays)
    kinds = set()
    for i, h in enumerate(hits):
        want = wit.closest(rays[i, :3], rays[i, 3:])
        assert want is not None and (int(h["kind"]), int(h["prim"]), int(h["instance"])) == want["id"], (i, h, want)
        assert same_material(G.accel_material(accel, int(h["material"])), want["mat"]), i
        kinds.add(int(h["kind"]))
        inst, steps = int(h["instance"]), 0
        parent, obj = G.accel_instance(accel, inst)
        if h["kind"] == 3:
            assert obj == mesh
        else:
            assert obj == -1
        while parent != -1:  # the chain ends at the root
            assert G.accel_instance(accel, parent)[1] == -1  # (every ancestor is a group)
            parent, _ = G.accel_instance(accel, parent)
            steps += 1
            assert steps < 8
    assert kinds == {1, 2, 3}
    assert G.accel_instance(accel, 0) == (-1, -1)
    # the mesh added without a material shades with Material::default() (bvh.rs:513-515)
    plain = hits[len(targets) - 4]
    assert same_material(G.accel_material(accel, int(plain["material"])), pyref.DEFAULT_MATERIAL)
