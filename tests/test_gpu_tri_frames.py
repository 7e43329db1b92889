"""The frame table of flat triangles (lg_accel_set_tri_frames): at the accel build the device makes one record per
triangle of every small mesh instance without vertex normals -- the normals and tangents of a hit's shading frame carried up the scene graph,
for both signs of the triangle's normal, and the material -- and the fused form's closest pass reads a hit's record instead of evaluating
those expressions again.  The film must not know: every case is compared bit for bit -- RGBA bytes and f64 radiance -- with the CPU oracle
AND with the same accel rendered with the switch off, and the getter says whether the table was read -- what the plan
(tests/test_tri_frames_gate.py, lasgun_amd/csrc/tri_frames_host.h) and the fused form's gate allow.  The table's rows themselves are
compared bit for bit with what lg_intersect and lg_hit_attributes, which read no table, return for rays onto the same triangles from both
sides.  Level by level is forced with lg_accel_set_streaming(2), the scene tables in LDS.  Films are 128 x 128 at most (the headline: 256)."""
import os

import numpy as np
import pytest

import lasgun_amd as la
import tri_frames_scenes as T
from lasgun_amd import scenes as S
from test_gpu_l0_relative import look, spheres64
from test_gpu_shadow_skip import bits, oracle_film, same_radiance

pytestmark = pytest.mark.gpu
G = la.api
ENV_ON = os.environ.get("LASGUN_TRI_FRAMES", "1")[:1] != "0" and os.environ.get("LASGUN_FUSED_SHADE", "1")[:1] != "0" and os.environ.get("LASGUN_PACKET_WALK", "1")[:1] != "0"
W = H = 64


def levels(scene):
    acc = G.Accel(scene)
    G.set_streaming(acc, 2)  # level by level whatever the launch size
    G.set_prune(acc, False)
    assert G.set_lds_scene(acc, True), "the scene fits in LDS"
    return acc


def both_switches(acc, w, h, takes, tag, k=0, n=1):
    """(RGBA, radiance) with the switch on and off; the getter after each of the four launches."""
    out = {}
    for switch in (True, False):
        G.set_tri_frames(acc, switch)
        film = G.Film(w, h)
        G.capture_subset(k, n, acc, film)
        assert G.last_organisation(acc).startswith("wavefront"), tag
        assert G.last_tri_frames(acc) == (ENV_ON and switch and takes), (tag, switch, G.last_tri_frames(acc))
        rad = G.capture_radiance(acc, w, h, k, n)
        assert G.last_tri_frames(acc) == (ENV_ON and switch and takes), (tag, switch, "radiance")
        out[switch] = (film.pixels(), rad)
    G.set_tri_frames(acc, True)
    return out


def check(build, w=W, h=H, takes=True, k=0, n=1, tag=""):
    want_rgba, want_rad = oracle_film(build, w, h, k, n)
    assert want_rgba.any(), "a picture"
    scene = build(G)
    assert (G.scene_tri_frames_gate(scene)[0] > 0 and G.scene_fused_shade_gate(scene) == 0) == takes, tag
    acc = levels(scene)
    r = both_switches(acc, w, h, takes, tag, k, n)
    on, off = r[True], r[False]
    assert np.array_equal(on[0], off[0]) and np.array_equal(bits(on[1]), bits(off[1])), ("switch on against switch off", tag)
    assert np.array_equal(on[0], want_rgba), (tag, int((on[0] != want_rgba).sum()))
    assert same_radiance(on[1], want_rad), (tag, int((bits(on[1]) != bits(want_rad)).sum()))
    return acc


def triangle_share(acc, w, h):
    """The share of a film's pixels whose closest hit is a triangle (lg_hit::kind 3)."""
    hits = G.intersect(acc, G.camera_rays(acc, w, h))
    return float((hits["kind"] == 3).mean())


SCENES = {
    "cornell_inside": (lambda api: S.cornell_scene(api, "plastic"), 128),
    # from behind the back wall, and from below the floor: the back of a wall, the other sign of its normal
    "cornell_behind": (look(lambda api: S.cornell_scene(api, "plastic"), (0.5, 0.4, -7.0)), 128),
    "cornell_below": (look(lambda api: S.cornell_scene(api, "plastic"), (0.3, -6.0, 1.0), up=(0.0, 0.0, -1.0)), 64),
    # a non-uniform scale and rotations above the mesh (xf_normal is not xf_vector), an instance without a material
    "scaled_rotated": (lambda api: T.walls_scene(api), 128),
    "scaled_rotated_behind": (lambda api: T.walls_scene(api, origin=(-1.0, -3.0, -6.0)), 64),
    "uv": (lambda api: T.walls_scene(api, T.strip_obj(6, uv="skew")), 64),
    "uv_backface_swapped": (lambda api: T.walls_scene(api, T.strip_obj(6, uv="skew"), backface=True), 64),
    "uv_determinant_0": (lambda api: T.walls_scene(api, T.strip_obj(4, uv="flat")), 64),  # dpdu, dpdv from coordinate_system
    "uv_determinant_0_behind": (lambda api: T.walls_scene(api, T.strip_obj(4, uv="flat"), origin=(-1.0, -3.0, -6.0)), 64),
    "along_a_wall": (T.along_wall_scene, 64),  # orthographic, in a wall's plane: dot(c, -lr.d) == 0 in every lane
    "at_the_instance_cap": (lambda api: T.capped_scene(api, 1024), 64),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_film_does_not_know(name):
    build, size = SCENES[name]
    acc = check(build, size, size, tag=name)
    if name != "along_a_wall":  # not vacuous: a good part of the film is triangles
        assert triangle_share(acc, size, size) > 0.05, name


REFUSED = {
    "vertex_normals": lambda api: T.capped_scene(api, 6, normals=True),
    "over_the_instance_cap": lambda api: T.capped_scene(api, 1025),
    "over_the_accels_cap": lambda api: T.capped_scene(api, 241, instances=17),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_scenes_without_a_table_still_match(name):
    acc = check(REFUSED[name], takes=False, tag=name)
    assert len(G.read_tri_frames(acc)) == 0
    assert triangle_share(acc, W, H) > 0.05, name


@pytest.mark.parametrize("size", [64, 256])
def test_the_headline(size):
    check(lambda api: S.spheres_scene(api, nspheres=1024), size, size, tag="headline_%d" % size)


def test_nine_samples_in_both_orders():
    build = look(spheres64, None, ss=2)
    want_rgba, want_rad = oracle_film(build, W, H)
    acc = levels(build(G))
    for order in (0, 1):
        G.set_sample_order(acc, order)
        r = both_switches(acc, W, H, True, ("order", order))
        for switch in (True, False):
            assert np.array_equal(r[switch][0], want_rgba), (order, switch)
            assert same_radiance(r[switch][1], want_rad), (order, switch)
        assert np.array_equal(bits(r[True][1]), bits(r[False][1])), order


def test_a_strided_subset_and_interleaved_rows():
    import torch
    build = lambda api: T.walls_scene(api)  # noqa: E731
    for k in (0, 3):
        check(build, W, H, k=k, n=7, tag="subset_%d" % k)
    want_rgba, _ = oracle_film(build, W, H)
    acc = levels(build(G))
    rows = 4
    mine = np.concatenate([want_rgba[y:y + rows] for y in range(rows, H, 2 * rows)])  # rank 1 of 2: blocks 1, 3, ...
    for switch in (True, False):
        G.set_tri_frames(acc, switch)
        tile = torch.zeros((mine.shape[0], W, 4), dtype=torch.uint8, device="cuda")
        G.capture_interleaved_device(acc, W, H, rows, 2, 1, tile.data_ptr())
        G.synchronize(acc)
        assert G.last_tri_frames(acc) == (ENV_ON and switch), switch
        assert np.array_equal(tile.cpu().numpy(), mine), switch
    G.set_tri_frames(acc, True)


def test_the_fused_forms_switch_is_the_tables_too():
    build = lambda api: T.walls_scene(api)  # noqa: E731
    want_rgba, want_rad = oracle_film(build, W, H)
    acc = levels(build(G))
    G.set_fused_shade(acc, False)
    r = both_switches(acc, W, H, False, "three kernels")
    for switch in (True, False):
        assert np.array_equal(r[switch][0], want_rgba) and same_radiance(r[switch][1], want_rad), switch


def test_counters_unchanged():
    acc = levels(T.walls_scene(G))
    stats = []
    for switch in (True, False):
        G.set_tri_frames(acc, switch)
        stats.append(G.capture_stats(acc, W, H))
    assert stats[0] == stats[1] and stats[0]["hits"] > 0 and stats[0]["triangles_tested"] > 0, stats


def test_the_switch_refuses_other_values():
    acc = G.Accel(S.readme_scene(G))
    assert G.last_tri_frames(acc) is None
    for bad in (-1, 2):
        assert G.call("accel_set_tri_frames", acc.h, bad) != 0
    G.set_tri_frames(acc, True)


def rays_from_all_around(n, seed):
    """n rays from a sphere of radius 7 around the scene, each aimed at a point of the box the scenes fill."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o *= 7.0 / np.linalg.norm(o, axis=1, keepdims=True)
    at = rng.uniform(-1.8, 1.8, size=(n, 3))
    return np.ascontiguousarray(np.concatenate([o, at - o], axis=1))


ROWS = {
    "cornell": lambda api: S.cornell_scene(api, "plastic"),
    "scaled_rotated": lambda api: T.walls_scene(api),
    "uv_backface_swapped": lambda api: T.walls_scene(api, T.strip_obj(6, uv="skew"), backface=True),
    "uv_determinant_0": lambda api: T.walls_scene(api, T.strip_obj(4, uv="flat")),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_the_rows_are_what_a_hit_on_the_triangle_gets(name):
    scene = ROWS[name](G)
    records, base = G.scene_tri_frames_gate(scene)
    acc = G.Accel(scene)
    rows = G.read_tri_frames(acc)
    assert len(rows) == records > 0
    rays = rays_from_all_around(8192, 11)
    out = G.hit_attributes(acc, rays, planes=("hits", "frame"))
    hits, frame = out["hits"], out["frame"]
    assert np.array_equal(hits.view(np.uint8), G.intersect(acc, rays).view(np.uint8))
    seen = np.zeros((records, 2), dtype=np.int64)
    for i in np.flatnonzero(hits["kind"] == 3):
        a, k = int(hits["instance"][i]), int(hits["prim"][i])
        assert base[a] is not None, (name, a)
        row = rows[base[a] + k]
        v = [v for v in (0, 1) if np.array_equal(bits(row["ns"][v]), bits(hits["ns"][i]))]
        assert len(v) == 1, (name, i, a, k, row["ns"], hits["ns"][i])
        v = v[0]
        assert np.array_equal(bits(row["ts"][v]), bits(frame[i, 3:])), (name, i, a, k)
        assert np.array_equal(bits(row["ss"]), bits(frame[i, :3])), (name, i, a, k)
        assert np.array_equal(bits(row["ng0"]), bits(hits["ng"][i])) or np.array_equal(bits(-row["ng0"]), bits(hits["ng"][i])), (name, i, a, k)
        assert int(row["mat"]) == int(hits["material"][i]), (name, i, a, k)
        assert row["pad"] == 0
        seen[base[a] + k, v] += 1
    # every triangle was hit from both sides: each variant of each row was compared
    assert (seen > 0).all(), (name, seen.tolist())
