"""The oracle's ray queries (orc_intersect, orc_occluded) against the identity-tracking witness (tests/query_witness.py) on every family
of tests/edge_rays.py: t, p, ng and ns bit for bit (any NaN equals any NaN), the winner's (kind, prim, instance), its material POD, and
the shadow verdict t < 1 -- with glibc's trigonometry and with the portable one the device runs.  CPU only: this is what makes the
oracle a reference for tests/test_gpu_ray_query_edges.py."""
import contextlib

import numpy as np
import pytest

import pyref
import edge_rays as E
import limit_scenes as L
from lasgun_amd import scenes as S
from oracle_lib import oracle
from query_witness import Witness, bits, pod, portable_trig, same

if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference never reads it, camera.rs:142)
    pyref.Camera.set_aperture_radius = lambda self, radius: self

SCENES = [("kitchen_sink", lambda api: S.kitchen_sink_scene(api), {}),
          ("instanced", lambda api: S.instanced_scene(api), {}),
          ("tie_mesh", lambda api: S.tie_mesh_scene(api), {}),
          ("exotic_obj", lambda api: S.exotic_obj_scene(api), {}),
          ("random_1", lambda api: S.random_scene(api, 1), {}),
          ("random_3", lambda api: S.random_scene(api, 3), {}),
          ("f3", E.f3_scene, {}),
          ("f7", E.f7_scene, {"huge": True}),
          ("grid", E.grid_scene, {"mesh": True}),
          # the scene graph's limits (tests/limit_scenes.py): the oracle is pinned at eight levels and past 64 accels HERE.  "camera": the
          # scene's own camera rays beside the edge rays; "deepest": the accels at the end of the longest chains, in which some winners must lie
          ("chain8_shallow", L.chain8_shallow, {"camera": True, "deepest": (7, 9)}),
          ("accels65", L.accels65, {"camera": True, "deepest": (2, 4)})]


@contextlib.contextmanager
def oracle_trig(o, portable):
    o.set_trig_mode(portable)
    try:
        with (portable_trig() if portable else contextlib.nullcontext()):
            yield
    finally:
        o.set_trig_mode(False)


def scene_rays(pscene, wit, kw, seed):
    lo, hi, boxes = E.scene_geometry(wit, pscene)
    rays, fam = E.edge_rays(lo, hi, boxes=boxes, seed=seed, **{k: v for k, v in kw.items() if k not in ("camera", "deepest")})
    if kw.get("camera"):
        cam = np.array([[*od[0], *od[1]] for y in range(L.H // 2) for x in range(L.W // 2) for od in pscene.camera.sample(x, y, L.W // 2, L.H // 2)])
        rays, fam = np.concatenate([rays, cam]), np.concatenate([fam, np.array(["camera"] * len(cam))])
    return rays, fam


@pytest.mark.parametrize("portable", [False, True], ids=["libm", "portable"])
@pytest.mark.parametrize("name,builder,kw", SCENES, ids=[s[0] for s in SCENES])
def test_oracle_queries_match_the_witness(name, builder, kw, portable):
    o = oracle()
    oscene, pscene = builder(o), builder(pyref.Api)
    accel = o.Accel.from_scene(oscene)
    wit = Witness(pscene)
    rays, fam = scene_rays(pscene, wit, kw, seed=len(name))
    n_hit, n_nan, n_deepest = {}, 0, 0
    with oracle_trig(o, portable):
        hits, mats = o.intersect(accel, rays)
        occ = o.occluded(accel, rays)
        for i, ray in enumerate(rays):
            h, want, ctx = hits[i], wit.closest(ray[:3], ray[3:]), [name, fam[i], i, list(ray)]  # (a list: the messages below append to it)
            if want is None:
                assert h["t"] == np.inf and h["kind"] == 0 and h["prim"] == 0xFFFFFFFF and h["instance"] == 0xFFFFFFFF, ctx
                assert h["material"] == -1 and not occ[i], ctx
                assert not any(bits(v) for k in ("p", "ng", "ns") for v in h[k]), ctx
                continue
            n_hit[fam[i]] = n_hit.get(fam[i], 0) + 1
            n_nan += want["t"] != want["t"]
            n_deepest += want["id"][2] in kw.get("deepest", ())
            assert same(h["t"], want["t"]), ctx + [h["t"], want["t"]]
            assert (int(h["kind"]), int(h["prim"]), int(h["instance"])) == want["id"], ctx + [h, want["id"]]
            kind, flat = pod(want["mat"])
            assert int(mats[i]["kind"]) == kind and [bits(v) for v in mats[i]["p"][:len(flat)]] == flat, ctx
            for k in ("p", "ng", "ns"):
                assert all(same(a, b) for a, b in zip(h[k], want[k])), ctx + [k, list(h[k]), want[k]]
            assert bool(occ[i]) == (want["t"] < 1.0), ctx
    for f in ("F1", "F2", "F6") + (("F5",) if kw.get("mesh") else ()):
        assert n_hit.get(f, 0) >= 8, (name, f, n_hit)
    if kw.get("huge"):
        assert n_hit["F7"] >= 10 and n_nan >= 1, (n_hit, n_nan)
    if kw.get("camera"):
        assert n_hit["camera"] >= 64 and n_deepest >= 16, (name, n_hit, n_deepest)


def test_f7_the_nan_winner_is_not_an_occluder():
    """The lead of the finite-then-NaN family: a box accepted at t = 7e-160, then the sphere's overflowing quadratic at t = NaN, which
    wins (NaN passes both t < 0 and t >= isect.t): the closest hit is the sphere at t = NaN and the segment is NOT occluded -- while
    without the sphere the same ray is blocked by the box at t < 1."""
    o = oracle()
    ray = np.array([[0.0, 0.0, 10.0, 0.0, 0.0, -1e160]])
    h, _ = o.intersect(o.Accel.from_scene(E.f7_scene(o)), ray)
    assert np.isnan(h[0]["t"]) and int(h[0]["kind"]) == 1 and not o.occluded(o.Accel.from_scene(E.f7_scene(o)), ray)[0]
    h0, _ = o.intersect(o.Accel.from_scene(E.f7_scene(o, with_sphere=False)), ray)
    assert int(h0[0]["kind"]) == 2 and 0.0 < h0[0]["t"] < 1.0
    assert o.occluded(o.Accel.from_scene(E.f7_scene(o, with_sphere=False)), ray)[0]
    w = Witness(E.f7_scene(pyref.Api)).closest(ray[0, :3], ray[0, 3:])
    assert w["t"] != w["t"] and w["id"] == (1, 0, 0)


def test_f3_scene_transforms():
    """What the F3 scene's groups are, bit for bit: the root, the plain group and the group translated by zero have an exact-identity
    minv (the walk's AF_IDENTITY shortcut applies to them); the 360-degree turn equals the identity on its diagonal only.  (A minv equal
    to the identity in value but not in bits -- a -0.0 entry -- cannot be built through the scene API: every builder step is a matrix
    product, and its sums turn -0.0 into +0.0.)"""
    scene = E.f3_scene(pyref.Api)
    groups = [node[1] for node in scene.root.contents if node[0] == "group"]
    flat = lambda m: [bits(v) for row in m for v in row]  # noqa: E731
    ident = flat(pyref.mat_identity())
    assert [flat(g.transform.minv) == ident for g in groups] == [True, True, False]
    assert flat(scene.root.transform.minv) == ident
    turn = groups[2].transform.minv
    assert [turn[k][k] for k in range(4)] == [1.0] * 4 and turn[0][1] != 0.0


def test_edge_rays_are_deterministic_and_tiled():
    a, fa = E.edge_rays((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), boxes=[((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], mesh=True, huge=True)
    b, fb = E.edge_rays((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), boxes=[((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], mesh=True, huge=True)
    assert a.view(np.int64).tobytes() == b.view(np.int64).tobytes() and list(fa) == list(fb)
    assert set(fa) == {"F1", "F2", "F3", "F4", "F5", "F6", "F7"}
    first = np.where(fa == "F1")[0][0]
    assert first % E.TILE == 0 and (fa == "F1").sum() % E.TILE == 0 and (fa == "F2").sum() % E.TILE == 0
    assert len(E.mesh_grid_obj().splitlines()) - 1 - (E.MESH_N + 1) ** 2 == 2 * E.MESH_N ** 2 >= 4096
