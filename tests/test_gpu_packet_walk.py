"""The packet form of level 0's closest pass (lg_accel_set_packet_walk): the 64 rays of a wave walked with one
cursor, one stack and one slot counter.  Nothing may know: with the switch on and off every film is the CPU oracle's, byte for byte, the
two positions agree with each other, and the getter says which form the pass took -- what the gate (tests/test_packet_walk_predicate.py,
lasgun_amd/csrc/packet_host.h) allows.  Level by level is forced with lg_accel_set_streaming(2) (films this small otherwise go to the
megakernel, which has no such form), the scene tables in LDS."""
import os

import numpy as np
import pytest

import lasgun_amd as la
import level_door_scenes as D
import shadow_skip_scenes as K
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_l0_relative import look, nested3_scene, oracle_film, same_radiance, spheres64

pytestmark = pytest.mark.gpu
G = la.api
ENV_ON = os.environ.get("LASGUN_PACKET_WALK", "1")[:1] != "0"


def levels(scene):
    acc = G.Accel(scene)
    G.set_streaming(acc, 2)
    G.set_prune(acc, False)
    assert G.set_lds_scene(acc, True), "the scene fits in LDS"
    return acc


def both_positions(build, w, h, want, tag="", takes=True, relative=(True,), radiance=True):
    """Films (and radiance) in both switch positions against the oracle and each other; `takes`: the gate admits the scene."""
    scene = build(G)
    assert (G.scene_packet_walk_gate(scene) == 0) == takes, (tag, G.scene_packet_walk_gate(scene))
    acc = levels(scene)
    films = {}
    for rel in relative:
        G.set_l0_relative(acc, rel)
        for switch in (True, False):
            G.set_packet_walk(acc, switch)
            film = G.Film(w, h)
            G.capture_subset(0, 1, acc, film)
            assert G.last_organisation(acc).startswith("wavefront"), tag
            took = G.last_packet_walk(acc)
            assert took == (ENV_ON and switch and takes), (tag, rel, switch, took)
            px = film.pixels()
            assert np.array_equal(px, want[0]), (tag, rel, switch, int((px != want[0]).sum()))
            if radiance:
                assert same_radiance(G.capture_radiance(acc, w, h), want[1]), (tag, rel, switch)
            films[(rel, switch)] = px
    first = next(iter(films.values()))
    for k, v in films.items():
        assert np.array_equal(v, first), (tag, k)
    return scene, acc


def coincident_scene(api):
    """Two coincident spheres of different materials (the first in order[] wins the tie) and a sphere tangent to a cube's face on the camera's axis."""
    scene = D._base(api)
    scene.camera.look_at([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    plastic, matte, _ = D._mats(api)
    red = api.Material.plastic([1.0, 0.1, 0.1], [0.5, 0.7, 0.5], 0.25)
    scene.root.add_sphere([-1.0, 0.5, 0.0], 0.6, plastic)
    scene.root.add_sphere([-1.0, 0.5, 0.0], 0.6, red)
    scene.root.add_cube([-0.5, -0.5, -1.0], 1.0, matte)   # its front face: z = 0
    scene.root.add_sphere([0.0, 0.0, 0.5], 0.5, red)      # touches that face at the origin, on the camera's axis
    scene.root.add_sphere([1.2, -0.8, 0.3], 0.4, plastic)
    return scene


def every_door_scene(api, ortho=None):
    """Every shape of nested accel the gate admits, around a few spheres and a cube in the root: a group of spheres and a cube under a rotation
    and an uneven scale; a lone plane mesh in such a group; one in an identity group; a plane mesh straight in the root.  `ortho`: a view
    down an axis, whose rays -- exact zeros in two components -- are not plain in any level and take the lone meshes' groups as levels."""
    scene = D._base(api, ortho)
    plastic, matte, glass = D._mats(api)
    plane = scene.parse_obj(S.PLANE_OBJ)
    A = api.Aggregate
    g = A.new(); g.rotate_z(30.0); g.scale(1.2, 0.7, 1.1); g.translate([-0.9, 0.6, 0.3])
    # (one centroid, so that the builder leaves the three in one leaf: the group's tree is its root record)
    g.add_sphere([0.0, 0.0, 0.0], 0.4, plastic); g.add_cube([-0.33, -0.33, -0.33], 0.66, matte); g.add_sphere([0.0, 0.0, 0.0], 0.5, matte)
    scene.root.add_group(g)
    f = A.new(); f.scale(2.5, 1.0, 2.5); f.rotate_z(8.0); f.translate([0.0, -1.5, 0.0]); f.add_obj_of(plane, matte)
    scene.root.add_group(f)
    p = A.new(); p.add_obj_of(plane, plastic)
    scene.root.add_group(p)
    scene.root.add_obj_of(plane, matte)
    for c, r in (([1.2, 0.8, 0.5], 0.45), ([0.9, -0.7, 1.1], 0.3), ([-1.3, -0.6, 0.9], 0.35), ([0.2, 1.4, -0.5], 0.3), ([1.6, 0.1, -0.8], 0.3)):
        scene.root.add_sphere(c, r, plastic)
    scene.root.add_cube([-0.4, 0.2, 0.6], 0.5, matte)
    return scene


def _ortho(scene):
    camera = scene.set_orthographic_camera(4.5)
    camera.look_at([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    return scene


def two_lights_scene(api):
    scene = spheres64(api)
    scene.add_point_light([-1.5, 1.2, 1.0], [0.4, 0.5, 0.9], [1.0, 0.0, 0.0])
    return scene


def far_light_scene(api):
    """A light so far away that its shadow rays leave anyhit_exit_ok's range: the any-hit walk without the early exit."""
    scene = spheres64(api)
    scene.add_point_light([3e70, 1e70, 2e70], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0])
    return scene


CASES = {
    # name: (builder, w, h, the gate admits it, positions of the origin-relative form)
    "headline_64": (lambda api: S.spheres_scene(api, nspheres=1024), 64, 64, True, (True, False)),  # a tile spans several spheres: lanes diverge
    "headline_256": (lambda api: S.spheres_scene(api, nspheres=1024), 256, 256, True, (True,)),
    "one_sphere": (lambda api: S.spheres_scene(api, nspheres=1), 64, 64, True, (True,)),
    "two_spheres": (lambda api: S.spheres_scene(api, nspheres=2), 64, 64, True, (True,)),
    "down_minus_z_128": (spheres64, 128, 128, True, (True, False)),  # the shell's camera looks down -z: 2-4 octants in the centre tiles, d.y == 0 on a row
    "coincident_and_tangent": (coincident_scene, 64, 64, True, (True, False)),
    "cornell_plastic_128": (lambda api: S.cornell_scene(api, "plastic"), 128, 128, True, (True, False)),  # a cuboid slot, the walls
    "cornell_glass_128": (lambda api: S.cornell_scene(api, "glass"), 128, 128, True, (True,)),  # deeper levels: the per-lane walk
    "every_door": (every_door_scene, 64, 64, True, (True, False)),  # groups of spheres and cubes, lone meshes, a mesh straight in the root
    "orthographic_down_z": (lambda api: every_door_scene(api, D.AXIS_VIEWS["down_z"]), 64, 64, True, (True,)),  # absolute closest form, local rays that are not plain
    "orthographic_down_y": (lambda api: every_door_scene(api, D.AXIS_VIEWS["down_y"]), 64, 64, True, (True,)),
    "cornell_orthographic": (lambda api: _ortho(S.cornell_scene(api, "plastic")), 64, 64, True, (True,)),
    "srt_lone": (D.srt_lone_scene, 64, 64, False, (True,)),  # a mesh whose tree has interior nodes: the gate says no
    "shadow_skip_holes": (lambda api: K.terminator_scene(api, "plastic", "one"), 64, 64, True, (True,)),  # flagged holes inside a shadow tile
    "two_lights": (two_lights_scene, 64, 64, True, (True,)),
    "far_light": (far_light_scene, 64, 64, True, (True,)),
    "nested3": (nested3_scene, 96, 72, False, (True,)),  # groups in groups: the gate says no
    "mesh_and_sphere": (D.mesh_and_sphere_scene, 64, 64, False, (True,)),  # a mesh inside a group that is not its lone mesh's
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_films_match_the_oracle_in_both_positions(name):
    builder, w, h, takes, relative = CASES[name]
    build = look(builder, None)
    want = oracle_film(build, w, h)
    assert want[0].any(), "a picture"
    both_positions(build, w, h, want, tag=name, takes=takes, relative=relative, radiance=(w * h <= 128 * 128))


def test_the_tie_shows_in_the_colour():
    """The coincident spheres: the pixel at the first sphere's centre carries the FIRST sphere's (blue) material in both positions."""
    build = look(coincident_scene, None)
    want = oracle_film(build, 64, 64)[0]
    acc = levels(build(G))
    # the film's pixel over (-1.0, 0.5): blue dominates red there
    ys, xs = np.nonzero((want[..., 2].astype(int) - want[..., 0].astype(int)) > 40)
    assert len(ys) > 20, "the first sphere is seen"
    for switch in (True, False):
        G.set_packet_walk(acc, switch)
        film = G.Film(64, 64)
        G.capture_subset(0, 1, acc, film)
        assert np.array_equal(film.pixels(), want), switch


def test_nine_samples_in_both_orders():
    w, h = 64, 64
    build = look(spheres64, None, ss=2)
    want = oracle_film(build, w, h)
    acc = levels(build(G))
    for order in (0, 1):
        G.set_sample_order(acc, order)
        for switch in (True, False):
            G.set_packet_walk(acc, switch)
            film = G.Film(w, h)
            G.capture_subset(0, 1, acc, film)
            assert G.last_packet_walk(acc) == (ENV_ON and switch), (order, switch)
            assert np.array_equal(film.pixels(), want[0]), (order, switch)
            assert same_radiance(G.capture_radiance(acc, w, h), want[1]), (order, switch)


def test_interleaved_rows_and_a_strided_subset():
    """Partial tiles and inactive lanes: rows dealt in blocks, and every 7th pixel from the 3rd."""
    import torch
    w, h, rows = 96, 72, 4
    build = look(spheres64, None)
    want = oracle_film(build, w, h)[0]
    o = oracle()
    oacc = o.Accel(build(o))
    ofilm = o.Film(w, h)
    o.capture_subset(3, 7, oacc, ofilm)
    acc = levels(build(G))
    mine = np.concatenate([want[y:y + rows] for y in range(rows, h, 2 * rows)])  # rank 1 of 2: blocks 1, 3, ...
    for switch in (True, False):
        G.set_packet_walk(acc, switch)
        tile = torch.zeros((mine.shape[0], w, 4), dtype=torch.uint8, device="cuda")
        G.capture_interleaved_device(acc, w, h, rows, 2, 1, tile.data_ptr())
        G.synchronize(acc)
        assert np.array_equal(tile.cpu().numpy(), mine), switch
        film = G.Film(w, h)
        G.capture_subset(3, 7, acc, film)
        assert G.last_packet_walk(acc) == (ENV_ON and switch), switch
        assert np.array_equal(film.pixels(), ofilm.pixels()) and ofilm.pixels().any(), switch


def test_the_counting_walk_is_untouched():
    w, h = 64, 64
    acc = levels(spheres64(G))
    stats = []
    for switch in (True, False):
        G.set_packet_walk(acc, switch)
        stats.append(G.capture_stats(acc, w, h))
    assert stats[0] == stats[1]
    assert stats[0]["nodes_tested"] > 0


def test_the_switch_refuses_other_values():
    acc = G.Accel(S.readme_scene(G))
    assert G.last_packet_walk(acc) is None
    for bad in (-1, 2):
        assert G.call("accel_set_packet_walk", acc.h, bad) != 0
    G.set_packet_walk(acc, True)
