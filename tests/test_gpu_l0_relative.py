"""The level-0 closest pass's origin-relative form (lg_accel_set_l0_relative): where every ray of a launch leaves from
the same point, the workgroup that has copied the scene into LDS subtracts that point from the node boxes and sphere centres once.  Nothing may
know: with the switch on and off every film is the CPU oracle's, byte for byte, and the f64 radiance bit for bit, and the getter says which
form ran -- what the gate (tests/test_l0_relative_predicate.py) says for that scene and camera.  The oracle is the only yardstick: the two
forms are never compared with each other alone.  Level by level is forced with lg_accel_set_streaming(2) (films this small otherwise go to
the megakernel, which has no such form), the scene tables in LDS."""
import os

import numpy as np
import pytest

import lasgun_amd as la
import level_door_scenes as D
import pyref
import pyref_bvh
from lasgun_amd import scenes as S
from oracle_lib import oracle

pytestmark = pytest.mark.gpu
G = la.api
SIZES = ((64, 64), (96, 72))  # whole tiles; a film whose right and bottom tiles are cut
ENV_ON = os.environ.get("LASGUN_L0_RELATIVE", "1")[:1] != "0"
if not hasattr(pyref.Camera, "set_aperture_radius"):
    pyref.Camera.set_aperture_radius = lambda self, radius: self


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_radiance(got, want):  # bit for bit; the bits of a NaN say which machine made it, not what was computed
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def spheres64(api):
    return S.spheres_scene(api, nspheres=64)


def nested3_scene(api):
    """Groups nested to depth 3, each rotated, scaled unevenly and translated, each holding spheres AND cubes (and the innermost a small
    mesh); spheres and cubes side by side in the root's leaves as well; one glass sphere, so that deeper levels follow level 0."""
    scene = D._base(api)
    plastic, matte, glass = D._mats(api)
    A = api.Aggregate
    g3 = A.new(); g3.rotate_z(40.0); g3.scale(1.1, 0.6, 1.4); g3.translate([0.2, 0.3, -0.1])
    g3.add_sphere([0.0, 0.0, 0.0], 0.35, plastic); g3.add_cube([0.3, -0.2, 0.1], 0.3, matte); g3.add_sphere([-0.5, 0.2, 0.3], 0.2, matte)
    g3.add_obj_of(scene.parse_obj(S.torus_obj(8, 6, R=0.5, r=0.12, normals=False)), plastic)
    g2 = A.new(); g2.rotate_x(-30.0); g2.scale(0.9, 1.3, 0.7); g2.translate([-0.4, 0.1, 0.2])
    g2.add_sphere([0.6, 0.5, 0.0], 0.25, matte); g2.add_cube([-0.9, -0.6, -0.2], 0.35, plastic); g2.add_sphere([0.1, -0.7, 0.4], 0.2, plastic)
    g2.add_group(g3)
    g1 = A.new(); g1.scale(1.2, 0.8, 1.1); g1.rotate_y(25.0); g1.translate([0.3, -0.2, 0.1])
    g1.add_sphere([-0.9, 0.8, 0.2], 0.3, plastic); g1.add_cube([0.7, 0.4, -0.3], 0.4, matte); g1.add_cube([-0.2, -1.1, 0.5], 0.25, plastic)
    g1.add_group(g2)
    scene.root.add_group(g1)
    for i, (c, r) in enumerate((([-1.6, -0.9, 0.6], 0.3), ([1.5, 1.1, -0.4], 0.35), ([1.7, -1.2, 0.9], 0.25), ([-1.4, 1.3, -0.8], 0.3))):
        scene.root.add_sphere(c, r, glass if i == 0 else plastic)
    for o, dim in (([-2.1, 0.2, -0.5], 0.4), ([0.9, -1.9, -0.9], 0.5), ([-0.6, 1.5, 0.4], 0.3), ([1.9, 0.1, 0.2], 0.35)):
        scene.root.add_cube(o, dim, matte)
    return scene


def many_accels_scene(api):
    """Eight planes in transformed groups around a few spheres: 17 accels, one more than the form's table holds."""
    scene = D._base(api)
    plastic, matte, _ = D._mats(api)
    plane = scene.parse_obj(S.PLANE_OBJ)
    for k in range(8):
        g = api.Aggregate.new(); g.scale(1.5, 1.0, 1.5); g.rotate_z(45.0 * k); g.rotate_x(10.0 * k); g.translate([0.0, -1.8 + 0.1 * k, 0.0]); g.add_obj_of(plane, matte)
        scene.root.add_group(g)
    for c in ([0.0, 0.0, 0.0], [0.8, 0.4, 0.5], [-0.7, -0.3, 0.9]):
        scene.root.add_sphere(c, 0.4, plastic)
    return scene


def look(builder, origin, at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), ss=0):
    def build(api):
        scene = builder(api)
        if origin is not None:
            scene.camera.look_at(list(origin), list(at), list(up))
        if ss:
            scene.camera.set_supersampling(ss)
        return scene
    return build


def oracle_film(build, w, h, k=0, n=1):
    """(RGBA film, f64 radiance) of the oracle for subset (k, n) of a w x h film."""
    o = oracle()
    oacc = o.Accel(build(o))
    o.set_trig_mode(1)
    try:
        film = o.Film(w, h)
        o.capture_subset(k, n, oacc, film)
        return film.pixels(), o.capture_radiance(oacc, w, h)
    finally:
        o.set_trig_mode(0)


def expect_form(scene, acc, switch):
    """What the gate should say: the switch, the device-free part for this scene and camera, at most 16 accels."""
    return bool(ENV_ON and switch and G.l0_relative_origins(scene) is not None and G.accel_info(acc)["accels"] <= 16)


def levels(scene):
    acc = G.Accel(scene)
    G.set_streaming(acc, 2)
    G.set_prune(acc, False)
    assert G.set_lds_scene(acc, True), "the scene fits in LDS"
    return acc


def check_render(build, w, h, want, expect_on=None, tag=""):
    scene = build(G)
    acc = levels(scene)
    for switch in (True, False):
        G.set_l0_relative(acc, switch)
        film = G.Film(w, h)
        G.capture_subset(0, 1, acc, film)
        assert G.last_organisation(acc).startswith("wavefront"), tag
        form = G.last_l0_relative(acc)
        assert form == expect_form(scene, acc, switch), (tag, switch, form)
        if expect_on is not None and ENV_ON:
            assert form == (expect_on and switch), (tag, switch, form)
        assert np.array_equal(film.pixels(), want[0]), (tag, switch, int((film.pixels() != want[0]).sum()))
        rad = G.capture_radiance(acc, w, h)
        assert same_radiance(rad, want[1]), (tag, switch, int((bits(rad) != bits(want[1])).sum()))
    return scene, acc


# ---- 1, 2: the headline's kind of scene, and groups in groups with spheres and cubes ------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ("spheres64", "nested3"))
def test_films_match_the_oracle_in_both_forms(name, w, h):
    build = look({"spheres64": spheres64, "nested3": nested3_scene}[name], None)
    want = oracle_film(build, w, h)
    assert len(np.unique(want[0].reshape(-1, 4), axis=0)) > 50, "a picture"
    check_render(build, w, h, want, expect_on=True, tag=name)


# ---- 3: camera origins -----------------------------------------------------------------------------------------------------------------
def origins():
    pscene = spheres64(pyref.Api)
    bmin_x = pyref_bvh.build(pscene.root).bound()[0][0]  # the root box's bmin.x, as the reference's builder makes it
    centre = next(n[1] for n in pscene.root.contents if n[0] == "sphere")
    return {"zero_component": ((0.0, 0.4, 5.0), (0.0, 0.0, 0.0)),
            # on the plane x = bmin.x, looking along it: bmin.x - o.x is exactly 0 in every lane, the root's entry parameter on x a zero of either
            # sign.  (0 * inf needs d.x = 0 as well, which no ray through a pixel CENTRE of an even-width film has: its aux coefficient is
            # (x + 0.5 - w / 2) pixels.  That path is walked by the predicate test's planes through the origins of rays with zero components.)
            "on_bmin_x": ((bmin_x, 0.3, 1.5), (bmin_x, 0.0, 0.0)),
            "inside_a_sphere": (centre, (0.0, 0.0, 0.0)),
            "far": ((1e6, 2e5, 3e5), (0.0, 0.0, 0.0))}


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ("zero_component", "on_bmin_x", "inside_a_sphere", "far"))
def test_camera_origins(name, w, h):
    origin, at = origins()[name]
    build = look(spheres64, origin, at)
    check_render(build, w, h, oracle_film(build, w, h), expect_on=True, tag=name)


# ---- 4: nine samples a pixel, side by side and in a row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_nine_samples(w, h):
    build = look(spheres64, None, ss=2)
    want = oracle_film(build, w, h)
    scene = build(G)
    acc = levels(scene)
    for order in (0, 1):
        G.set_sample_order(acc, order)
        for switch in (True, False):
            G.set_l0_relative(acc, switch)
            film = G.Film(w, h)
            G.capture_subset(0, 1, acc, film)
            assert G.last_l0_relative(acc) == expect_form(scene, acc, switch) and (not ENV_ON or G.last_l0_relative(acc) == switch), (order, switch)
            assert np.array_equal(film.pixels(), want[0]), (order, switch)
            assert same_radiance(G.capture_radiance(acc, w, h), want[1]), (order, switch)


# ---- 5: the other addressing modes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_interleaved_rows_and_subsets(w, h):
    import torch
    build = look(spheres64, None)
    want = oracle_film(build, w, h)[0]
    o = oracle()
    oacc = o.Accel(build(o))
    scene = build(G)
    acc = levels(scene)
    rows = 4
    mine = np.concatenate([want[y:y + rows] for y in range(rows, h, 2 * rows)])  # rank 1 of 2: blocks 1, 3, ...
    for switch in (True, False):
        G.set_l0_relative(acc, switch)
        tile = torch.zeros((h // 2, w, 4), dtype=torch.uint8, device="cuda")
        G.capture_interleaved_device(acc, w, h, rows, 2, 1, tile.data_ptr())
        G.synchronize(acc)
        assert G.last_l0_relative(acc) == expect_form(scene, acc, switch), switch
        assert np.array_equal(tile.cpu().numpy(), mine), switch
        film, ofilm = G.Film(w, h), o.Film(w, h)
        G.capture_subset(3, 7, acc, film)
        o.capture_subset(3, 7, oacc, ofilm)
        assert G.last_l0_relative(acc) == expect_form(scene, acc, switch), switch
        assert np.array_equal(film.pixels(), ofilm.pixels()) and ofilm.pixels().any(), switch
        film = G.Film(w, h)
        G.capture_subsets([1, 3, 4], 7, acc, film)
        for k in (1, 4):
            o.capture_subset(k, 7, oacc, ofilm)
        assert np.array_equal(film.pixels(), ofilm.pixels()), switch


# ---- 6: no origin is stale ---------------------------------------------------------------------------------------------------------------
CAMERAS = (((0.3, 0.4, 5.0), (0.0, 0.0, 0.0)), ((-3.5, 1.2, 2.5), (0.2, -0.3, 0.0)))


@pytest.mark.parametrize("w,h", SIZES)
def test_two_cameras_on_one_accel(w, h):
    wants = [oracle_film(look(nested3_scene, c, at), w, h) for c, at in CAMERAS]
    assert not np.array_equal(wants[0][0], wants[1][0])
    scene = nested3_scene(G)
    acc = levels(scene)
    for switch in (True, False):
        G.set_l0_relative(acc, switch)
        for rounds in range(2):  # A, B, A, B: each call's origin is its own camera's
            for (c, at), want in zip(CAMERAS, wants):
                scene.camera.look_at(list(c), list(at), [0.0, 1.0, 0.0])
                film = G.Film(w, h)
                G.capture_subset(0, 1, acc, film)
                assert G.last_l0_relative(acc) == expect_form(scene, acc, switch), (switch, c)
                assert np.array_equal(film.pixels(), want[0]), (switch, rounds, c)
                assert same_radiance(G.capture_radiance(acc, w, h), want[1]), (switch, rounds, c)
        views = [G.view_look_at(c, at, (0.0, 1.0, 0.0), fov=50.0) for c, at in CAMERAS]
        rgba, rgb = G.capture_views(acc, views, w, h, rgb=True)
        for k in range(2):
            assert np.array_equal(rgba[k], wants[k][0]) and same_radiance(rgb[k], wants[k][1]), (switch, k)


# ---- 7: where the gate says no -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ("orthographic", "seventeen_accels"))
def test_the_absolute_form_runs_where_the_gate_says_no(name, w, h):
    build = (lambda api: D.srt_lone_scene(api, D.AXIS_VIEWS["down_z"])) if name == "orthographic" else many_accels_scene
    scene, acc = check_render(build, w, h, oracle_film(build, w, h), expect_on=False, tag=name)
    if name == "seventeen_accels":
        assert G.accel_info(acc)["accels"] == 17
    assert (G.l0_relative_origins(scene) is None) == (name == "orthographic")


def test_the_switch_refuses_other_values():
    acc = G.Accel(S.readme_scene(G))
    assert G.last_l0_relative(acc) is None
    for bad in (-1, 2):
        assert G.call("accel_set_l0_relative", acc.h, bad) != 0
    G.set_l0_relative(acc, True)
