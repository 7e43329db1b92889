"""The exact walk from LDS over pair records (lg_accel_set_node_pairs): the closest and shadow passes of the
level-by-level pipeline test both children of an interior node in one trip and push only a far child that is hit.  Nothing may know: with
the switch on and off every film is the CPU oracle's, byte for byte, the f64 radiance bit for bit, the two positions agree with each other,
and the getter says which records the closest pass walked.  Level by level is forced with lg_accel_set_streaming(2) (films this small
otherwise go to the megakernel), the scene tables in LDS.  The megakernel, the queue organisation and the ray queries take the same
step from the same image (walk.h, walk<>) and are run in both positions too; the counting walk keeps the node tables and must not notice
the switch; the pruned walk is launched from the L2 tables while the accel holds pair records."""
import os

import numpy as np
import pytest

import lasgun_amd as la
import level_door_scenes as D
import edge_rays
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_l0_relative import bits, look, nested3_scene, oracle_film, same_radiance, spheres64

pytestmark = pytest.mark.gpu
G = la.api
ENV_ON = os.environ.get("LASGUN_NODE_PAIRS", "1")[:1] != "0"


def levels(scene):
    acc = G.Accel(scene)
    G.set_streaming(acc, 2)
    G.set_prune(acc, False)
    assert G.set_lds_scene(acc, True), "the scene fits in LDS"
    return acc


def both_positions(build, w, h, want, tag="", relative=(True,)):
    """Films and radiance in both switch positions (and the given positions of the origin-relative form) against the oracle and each other."""
    scene = build(G)
    acc = levels(scene)
    films = {}
    for rel in relative:
        G.set_l0_relative(acc, rel)
        for switch in (True, False):
            G.set_node_pairs(acc, switch)
            film = G.Film(w, h)
            G.capture_subset(0, 1, acc, film)
            assert G.last_organisation(acc).startswith("wavefront"), tag
            assert G.last_node_pairs(acc) == (switch and ENV_ON), (tag, rel, switch, G.last_node_pairs(acc))
            px = film.pixels()
            assert np.array_equal(px, want[0]), (tag, rel, switch, int((px != want[0]).sum()))
            rad = G.capture_radiance(acc, w, h)
            assert same_radiance(rad, want[1]), (tag, rel, switch, int((bits(rad) != bits(want[1])).sum()))
            films[(rel, switch)] = (px, rad)
    first = next(iter(films.values()))
    for k, v in films.items():
        assert np.array_equal(v[0], first[0]) and same_radiance(v[1], first[1]), (tag, k)
    return scene, acc


def one_sphere_scene(api):
    """A root accel whose node 0 is a leaf: the root record alone."""
    scene = D._base(api)
    plastic, _, _ = D._mats(api)
    scene.root.add_sphere([0.1, -0.2, 0.0], 0.8, plastic)
    return scene


def two_leaves_scene(api):
    """Two far-apart clusters: a tree of one interior node and two leaves (one pair record)."""
    scene = D._base(api)
    plastic, matte, _ = D._mats(api)
    scene.root.add_sphere([-1.2, 0.0, 0.0], 0.5, plastic)
    scene.root.add_sphere([1.2, 0.3, -0.2], 0.5, matte)
    return scene


CASES = {
    "headline": (lambda api: S.spheres_scene(api, nspheres=1024), 128, 128),
    "root_is_a_leaf": (one_sphere_scene, 64, 64),
    "two_leaves": (two_leaves_scene, 64, 64),
    "nested3": (nested3_scene, 96, 72),  # groups in groups, spheres and cubes and a mesh, a glass sphere: deeper levels follow
    "orthographic": (lambda api: D.srt_lone_scene(api, D.AXIS_VIEWS["down_z"]), 64, 64),  # non-plain rays: the general form
    "cornell_glass": (lambda api: S.cornell_scene(api, "glass"), 64, 64),  # deeper levels take the absolute pair form
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_films_match_the_oracle_in_both_positions(name):
    builder, w, h = CASES[name]
    build = look(builder, None)
    want = oracle_film(build, w, h)
    assert want[0].any(), "a picture"
    both_positions(build, w, h, want, tag=name, relative=(True, False))


def test_nine_samples_in_both_orders():
    w, h = 64, 64
    build = look(spheres64, None, ss=2)
    want = oracle_film(build, w, h)
    acc = levels(build(G))
    for order in (0, 1):
        G.set_sample_order(acc, order)
        for switch in (True, False):
            G.set_node_pairs(acc, switch)
            film = G.Film(w, h)
            G.capture_subset(0, 1, acc, film)
            assert G.last_node_pairs(acc) == (switch and ENV_ON), (order, switch)
            assert np.array_equal(film.pixels(), want[0]), (order, switch)
            assert same_radiance(G.capture_radiance(acc, w, h), want[1]), (order, switch)


def test_interleaved_rows_and_a_strided_subset():
    import torch
    w, h, rows = 96, 72, 4
    build = look(nested3_scene, None)
    want = oracle_film(build, w, h)[0]
    o = oracle()
    oacc = o.Accel(build(o))
    ofilm = o.Film(w, h)
    o.capture_subset(3, 7, oacc, ofilm)
    acc = levels(build(G))
    mine = np.concatenate([want[y:y + rows] for y in range(rows, h, 2 * rows)])  # rank 1 of 2: blocks 1, 3, ...
    for switch in (True, False):
        G.set_node_pairs(acc, switch)
        tile = torch.zeros((mine.shape[0], w, 4), dtype=torch.uint8, device="cuda")
        G.capture_interleaved_device(acc, w, h, rows, 2, 1, tile.data_ptr())
        G.synchronize(acc)
        assert np.array_equal(tile.cpu().numpy(), mine), switch
        film = G.Film(w, h)
        G.capture_subset(3, 7, acc, film)
        assert G.last_node_pairs(acc) == (switch and ENV_ON), switch
        assert np.array_equal(film.pixels(), ofilm.pixels()) and ofilm.pixels().any(), switch


def test_shadow_rays_outside_the_early_exit_range():
    """A light so far away that its shadow rays' directions exceed anyhit_exit_ok's range (2^199 here): the any-hit walk without
    the early exit."""
    def build(api):
        scene = spheres64(api)
        scene.add_point_light([3e70, 1e70, 2e70], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0])
        return scene
    w, h = 64, 64
    both_positions(build, w, h, oracle_film(build, w, h), tag="far_light")


@pytest.mark.parametrize("org", (0, 3))
def test_the_other_organisations_do_not_notice(org):
    """The megakernel (0) and the queue organisation (3) over an LDS-resident scene, in both positions against the oracle."""
    w, h = 64, 64
    build = look(lambda api: S.cornell_scene(api, "glass"), None)
    want = oracle_film(build, w, h)
    acc = G.Accel(build(G))
    G.set_streaming(acc, org)
    G.set_prune(acc, False)
    assert G.set_lds_scene(acc, True)
    for switch in (True, False):
        G.set_node_pairs(acc, switch)
        film = G.Film(w, h)
        G.capture_subset(0, 1, acc, film)
        assert not G.last_organisation(acc).startswith("wavefront"), org
        assert G.last_node_pairs(acc) == (switch and ENV_ON), (org, switch)
        assert np.array_equal(film.pixels(), want[0]), (org, switch, int((film.pixels() != want[0]).sum()))


def test_queries_on_the_edge_rays_in_both_positions():
    """lg_intersect* / lg_occluded* over the LDS-resident scene: every output byte is the same in both positions (the node form's bytes are
    pinned to the CPU oracle on these rays by tests/test_gpu_ray_query_edges.py)."""
    acc = G.Accel(nested3_scene(G))
    G.set_prune(acc, False)
    rays, _ = edge_rays.edge_rays((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0))
    out = {}
    for switch in (True, False):
        G.set_node_pairs(acc, switch)
        out[switch] = (G.intersect(acc, rays).tobytes(), G.occluded(acc, rays).tobytes())
        assert G.last_node_pairs(acc) == (switch and ENV_ON), switch
    assert out[True] == out[False] and len(out[True][1]) == len(rays)


def test_the_pruned_walk_leaves_lds_while_the_accel_holds_pair_records():
    """The image's form is decided when it is made: an accel that renders pruned keeps node records (the pruned walk reads them from LDS).
    One that holds pair records and is then switched to the pruned walk launches it from the L2 tables.  Same film every time."""
    w, h = 64, 64
    build = look(nested3_scene, None)
    want = oracle_film(build, w, h)

    def render(acc):
        film = G.Film(w, h)
        G.capture_subset(0, 1, acc, film)
        assert np.array_equal(film.pixels(), want[0])
        assert same_radiance(G.capture_radiance(acc, w, h), want[1])

    acc = levels(build(G))
    G.set_prune(acc, True)  # the tables are made again with the mesh leaves' records: node records in LDS, walked pruned
    render(acc)
    assert G.last_node_pairs(acc) is False
    G.set_prune(acc, False)
    G.set_node_pairs(acc, False)
    G.set_node_pairs(acc, True)  # the image made again, now for the plain exact walk
    render(acc)
    assert G.last_node_pairs(acc) == ENV_ON
    G.set_prune(acc, True)  # the records are there already: nothing is re-made, the pruned walk goes to the L2 tables
    render(acc)


def test_the_counting_walk_is_untouched():
    w, h = 64, 64
    acc = levels(nested3_scene(G))
    stats = []
    for switch in (True, False):
        G.set_node_pairs(acc, switch)
        stats.append(G.capture_stats(acc, w, h))
    assert stats[0] == stats[1]
    assert stats[0]["nodes_tested"] > 0


def test_the_switch_refuses_other_values():
    acc = G.Accel(S.readme_scene(G))
    assert G.last_node_pairs(acc) is None
    for bad in (-1, 2):
        assert G.call("accel_set_node_pairs", acc.h, bad) != 0
    G.set_node_pairs(acc, True)
