"""The exact walk's level door (lg_accel_set_level_door): bit 0, a ray that has the thinnest slab of a nested accel's
root box wholly behind it does not enter; bit 1, a group that holds one untransformed mesh and nothing else is walked as one level with it.
Nothing may know: with masks 0, 1, 2 and 3 every film is compared bit for bit -- RGBA bytes and f64 radiance -- with the CPU oracle, in every
organisation (level by level with the scene in LDS and in L2, megakernel, queue, pruned), every hit record and occlusion byte of the edge-case
rays (tests/level_door_rays.py) likewise, and the work counters stay the reference's.  The oracle is the only yardstick: a mask is never
compared with another mask alone."""
import numpy as np
import pytest

import pyref
import lasgun_amd as la
import level_door_rays as R
import level_door_scenes as D
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_ray_query_edges import Expect

pytestmark = pytest.mark.gpu
G = la.api
MASKS = (0, 1, 2, 3)
ERR = 2.220446049250313e-16 * 65536.0  # the shading offset (integrate.rs:40)
# (name, lg_accel_set_streaming, scene tables in LDS, pruned walk)
ORGS = [("levels_lds", 2, True, False), ("levels_l2", 2, False, False), ("megakernel", 0, True, False), ("queue", 3, True, False),
        ("levels_pruned", 2, True, True), ("megakernel_pruned_l2", 0, False, True)]
if not hasattr(pyref.Camera, "set_aperture_radius"):
    pyref.Camera.set_aperture_radius = lambda self, radius: self

FILMS = {"cornell_plastic": (lambda api: S.cornell_scene(api, "plastic"), 96),
         "cornell_glass": (lambda api: S.cornell_scene(api, "glass"), 96),
         "srt_lone": (D.srt_lone_scene, 64), "nested": (D.nested_scene, 64), "mesh_and_sphere": (D.mesh_and_sphere_scene, 64),
         "identity_lone": (D.identity_lone_scene, 64)}
for _view, _cam in D.AXIS_VIEWS.items():  # orthographic views down an axis: local directions with a -0 component into a lone-mesh group
    FILMS["identity_lone_" + _view] = (lambda api, c=_cam: D.identity_lone_scene(api, c), 64)
    FILMS["srt_lone_" + _view] = (lambda api, c=_cam: D.srt_lone_scene(api, c), 64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_radiance(got, want):  # bit for bit; the bits of a NaN say which machine made it, not what was computed
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def setup(acc, org):
    _, streaming, lds, prune = org
    G.set_streaming(acc, streaming)
    G.set_prune(acc, prune)
    G.set_lds_scene(acc, lds)


@pytest.mark.parametrize("name", sorted(FILMS))
def test_films_match_the_oracle_with_every_mask(name):
    builder, size = FILMS[name]
    o = oracle()
    oacc = o.Accel(builder(o))
    o.set_trig_mode(1)
    try:
        ofilm = o.Film(size, size)
        o.capture_subset(0, 1, oacc, ofilm)
        want_rgba, want_rad = ofilm.pixels(), o.capture_radiance(oacc, size, size)
        o.stats_reset()
        o.capture_subset(0, 1, oacc, o.Film(size, size))
        want_stats = o.stats_read()
    finally:
        o.set_trig_mode(0)
    acc = G.Accel(builder(G))
    for org in ORGS:
        setup(acc, org)
        for mask in MASKS:
            G.set_level_door(acc, mask)
            film = G.Film(size, size)
            G.capture_subset(0, 1, acc, film)
            rad = G.capture_radiance(acc, size, size)
            assert np.array_equal(film.pixels(), want_rgba), (name, org[0], mask, int((film.pixels() != want_rgba).sum()))
            assert same_radiance(rad, want_rad), (name, org[0], mask, int((bits(rad) != bits(want_rad)).sum()))
    # The counting forms never take the shortcuts: the same counters with every mask.  Against the oracle: the ray and hit counts are the
    # reference's; the work counters are at most the reference's, as in test_gpu_parity.py -- a shadow ray here stops at its first t < 1 where
    # the reference walks on (walk.h, anyhit_exit_ok) -- and EQUAL the reference's where no shadow ray is cast (the next test).
    G.set_streaming(acc, 1); G.set_prune(acc, False); G.set_lds_scene(acc, True)
    stats = []
    for mask in MASKS:
        G.set_level_door(acc, mask)
        stats.append(G.capture_stats(acc, size, size))
    for mask, got in zip(MASKS, stats):
        assert got == stats[0], (name, mask)
        for key in ("primary_rays", "shadow_rays", "secondary_rays", "hits"):
            assert got[key] == want_stats[key], (name, mask, key)
        for key in ("nodes_tested", "spheres_tested", "cuboids_tested", "triangles_tested", "accel_entries"):
            assert got[key] <= want_stats[key], (name, mask, key)
    assert want_stats["accel_entries"] > want_stats["primary_rays"]  # (nested accels are reached at all)


class Dark:
    """A binding whose scenes ignore add_point_light: the same geometry, camera and materials, no shadow ray -- every traversal is a closest-hit
    walk, whose work the reference's counters state exactly."""

    def __init__(self, api):
        self.Material, self.Aggregate = api.Material, api.Aggregate

        class Scene:
            @staticmethod
            def new():
                s = api.Scene.new()
                s.add_point_light = lambda *a, **k: None
                return s
        self.Scene = Scene


@pytest.mark.parametrize("name", sorted(n for n in FILMS if "_down_" not in n and "_along_" not in n))
def test_counters_equal_the_oracle_with_every_mask(name):
    builder, size = FILMS[name]
    o = oracle()
    oacc = o.Accel(builder(Dark(o)))
    o.stats_reset()
    o.capture_subset(0, 1, oacc, o.Film(size, size))
    want = o.stats_read()
    assert want["shadow_rays"] == 0 and want["accel_entries"] > want["primary_rays"]
    acc = G.Accel(builder(Dark(G)))
    for lds in (True, False):
        G.set_lds_scene(acc, lds)
        for mask in MASKS:
            G.set_level_door(acc, mask)
            got = G.capture_stats(acc, size, size)
            assert got == want, (name, lds, mask, got, want)


def test_headline_crop_matches_the_oracle_with_every_mask():
    """The headline scene at 4096 x 4096, its central 128 x 128: the tiles the benchmark renders, as the benchmark renders them."""
    size, x0, x1 = 4096, 1984, 2112
    o = oracle()
    oacc = o.Accel(S.spheres_scene(o))
    o.set_trig_mode(1)
    try:
        want_rgba, want_rad = o.capture_rect(oacc, size, size, x0, x0, x1, x1, nthreads=16)
    finally:
        o.set_trig_mode(0)
    acc = G.Accel(S.spheres_scene(G))
    for org in ORGS:
        setup(acc, org)
        for mask in MASKS:
            G.set_level_door(acc, mask)
            rgba, rad = G.capture_rect(acc, size, size, x0, x0, x1, x1)
            assert np.array_equal(rgba, want_rgba) and same_radiance(rad, want_rad), (org[0], mask, int((rgba != want_rgba).sum()))


def wall_shadow_rays(builder):
    """Shadow rays leaving the walls: the oracle's primary hits on a 24 x 24 film, offset along the facing normal, towards the light."""
    o = oracle()
    pscene = builder(pyref.Api)
    rays = np.array([[*od[0], *od[1]] for y in range(24) for x in range(24) for od in pscene.camera.sample(x, y, 24, 24)], dtype=np.float64)
    hits, _ = o.intersect(o.Accel(builder(o)), rays)
    hit = hits["kind"] == 3  # triangles: the walls
    ng = hits["ng"][hit]
    ng = np.where((np.einsum("ij,ij->i", ng, -rays[hit, 3:]) < 0.0)[:, None], -ng, ng)
    p = hits["p"][hit] + ng * ERR
    light = np.array(pscene.lights[0][0])
    return np.concatenate([p, light - p], axis=1)


EDGE_SCENES = {"cornell_plastic": lambda api: S.cornell_scene(api, "plastic"), "identity_lone": D.identity_lone_scene,
               "srt_lone": D.srt_lone_scene, "nested": D.nested_scene, "mesh_and_sphere": D.mesh_and_sphere_scene}


@pytest.mark.parametrize("name", sorted(EDGE_SCENES))
def test_edge_rays_match_the_oracle_with_every_mask(name):
    builder = EDGE_SCENES[name]
    pscene = builder(pyref.Api)
    rays, fam = R.edge_rays(pscene, seed=len(name))
    shadow = wall_shadow_rays(builder)
    rays = np.concatenate([rays, shadow])
    fam = np.concatenate([fam, np.array(["shadow"] * len(shadow))])
    exp = Expect(oracle().Accel.from_scene(builder(oracle())), rays, fam)
    accel = G.Accel.from_scene(builder(G))
    perm = np.random.default_rng(3).permutation(len(rays))
    for prune in (False, True):
        for lds in (True, False):
            G.set_prune(accel, prune)
            G.set_lds_scene(accel, lds)
            for mask in MASKS:
                G.set_level_door(accel, mask)
                exp.check(accel, G.intersect(accel, rays), G.occluded(accel, rays), (name, prune, lds, mask))
                exp.check(accel, G.intersect(accel, rays[perm]), G.occluded(accel, rays[perm]), (name, prune, lds, mask, "shuffled"), sel=perm)
    # not vacuous: at some door the probe says "does not enter" for some rays of every exact family and "enters" for others; there are rays
    # that hit something although a door is shut to them, and rays that hit through an open door
    _, ds = R.doors(pscene)
    top = []
    for d in ds:  # every door sees the rays in the space it is reached in
        local = [R.parent_ray(d, tuple(r[:3]), tuple(r[3:])) for r in rays.tolist()]
        top.append(R.probe_numpy(d, np.array([l[0] for l in local]), np.array([l[1] for l in local])))
    hit = exp.hits["kind"] != 0
    for f in ("face", "dzero", "random"):
        sel = fam == f
        assert any((s & sel).any() and (~s & sel).any() for s in top), (name, f)
    assert any((hit & s).any() for s in top) and any((hit & ~s).any() for s in top) and exp.occ.any() and not exp.occ.all(), name
    if name == "cornell_plastic":
        assert len(shadow) >= 100 and (~exp.occ[fam == "shadow"]).any()


def test_the_switch_refuses_other_masks():
    acc = G.Accel(S.readme_scene(G))
    for bad in (-1, 4, 256):
        with pytest.raises(la.LasgunError):
            G.set_level_door(acc, bad)
    G.set_level_door(acc, 3)
