"""The fused form of the camera's level 0 (lg_accel_set_fused_shade): for a scene of one level and one light the
closest pass shades in its epilogue -- a hit whose shadow ray decides nothing is finished there, every other hit parks its point, the
light's term and the ambient term -- and the shadow pass adds the light's term where the light is visible and writes the pixel; no shade
pass.  The film must not know: every case is compared bit for bit -- RGBA bytes and f64 radiance -- with the CPU oracle AND with the same
accel rendered with the switch off, and the getter says which form ran -- what the gate (tests/test_fused_shade_gate.py,
lasgun_amd/csrc/fused_host.h) allows.  Level by level is forced with lg_accel_set_streaming(2), the scene tables in LDS.

Scenes (fused_shade_scenes.py, shadow_skip_scenes.py): a sphere that fills the 64 x 64 film, lit from the side (tiles wholly lit, wholly
flagged, across the boundary; corners that miss), every material, the shadow skip on and off; a sphere shadowing another (walked hits whose
light is hidden); the guards of the skip's argument with one light; a small sphere in front of the background (appended hits, holes in
dense tiles); the headline at 64^2 and 256^2 with the origin-relative closest form on and off; 9 spp in both sample orders; a strided
subset, a crop, interleaved rows; scenes the gate refuses; the work counters."""
import os

import numpy as np
import pytest

import fused_shade_scenes as F
import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from shadow_skip_scenes import LIGHTS
from test_gpu_l0_relative import look, spheres64
from test_gpu_shadow_skip import ERR, bits, oracle_film, same_radiance

pytestmark = pytest.mark.gpu
G = la.api
ENV_ON = os.environ.get("LASGUN_FUSED_SHADE", "1")[:1] != "0"
W = H = 64


def levels(scene):
    acc = G.Accel(scene)
    G.set_streaming(acc, 2)  # level by level whatever the launch size
    G.set_prune(acc, False)
    assert G.set_lds_scene(acc, True), "the scene fits in LDS"
    return acc


def both_forms(acc, w, h, takes, tag, k=0, n=1):
    """(RGBA, radiance) with the switch on and off; the getter after each of the four launches."""
    out = {}
    for switch in (True, False):
        G.set_fused_shade(acc, switch)
        film = G.Film(w, h)
        G.capture_subset(k, n, acc, film)
        assert G.last_organisation(acc).startswith("wavefront"), tag
        assert G.last_fused_shade(acc) == (ENV_ON and switch and takes), (tag, switch, G.last_fused_shade(acc))
        rad = G.capture_radiance(acc, w, h, k, n)
        assert G.last_fused_shade(acc) == (ENV_ON and switch and takes), (tag, switch, "radiance")
        out[switch] = (film.pixels(), rad)
    G.set_fused_shade(acc, True)
    return out


def check(build, w=W, h=H, takes=True, k=0, n=1, skips=(True,), relative=(True,), tag=""):
    want_rgba, want_rad = oracle_film(build, w, h, k, n)
    assert want_rgba.any(), "a picture"
    scene = build(G)
    assert (G.scene_fused_shade_gate(scene) == 0) == takes, (tag, G.scene_fused_shade_gate(scene))
    acc = levels(scene)
    for rel in relative:
        G.set_l0_relative(acc, rel)
        for skip in skips:
            G.set_shadow_skip(acc, skip)
            r = both_forms(acc, w, h, takes, (tag, rel, skip), k, n)
            on, off = r[True], r[False]
            assert np.array_equal(on[0], off[0]) and np.array_equal(bits(on[1]), bits(off[1])), ("switch on against switch off", tag, rel, skip)
            assert np.array_equal(on[0], want_rgba), (tag, rel, skip, int((on[0] != want_rgba).sum()))
            assert same_radiance(on[1], want_rad), (tag, rel, skip, int((bits(on[1]) != bits(want_rad)).sum()))
    G.set_shadow_skip(acc, True)
    G.set_l0_relative(acc, True)
    return acc, want_rad


@pytest.mark.parametrize("kind", ["plastic", "matte0", "matte20", "metal"])
def test_every_material_across_the_terminator(kind):
    _, rad = check(lambda api: F.sphere_scene(api, kind, F.ONE), skips=(True, False), tag=kind)
    if kind == "plastic":  # the picture is the one the cases are about: tiles wholly lit, wholly unlit and across the boundary
        lit = (rad.sum(axis=2) > 0.45).reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3))
        assert (lit == 0.0).any() and (lit == 1.0).any() and ((lit > 0.0) & (lit < 1.0)).any(), lit


@pytest.mark.parametrize("kind", ["mirror", "glass"])
def test_specular_materials(kind):
    # with recursion the chain has levels below: the gate refuses and the three kernels run; without, BSDF::f of a specular material is
    # zero for every wi and the fused form carries zeros
    check(lambda api: F.sphere_scene(api, kind, F.ONE), takes=False, skips=(True, False), tag=kind)
    check(lambda api: F.sphere_scene(api, kind, F.ONE, recursion=0), takes=True, skips=(True, False), tag=kind + "_recursion_0")


def test_a_sphere_shadowing_another():
    _, rad = check(F.shadowed_scene, skips=(True, False), tag="shadowed")
    # not vacuous: the blocker is outside the view, so every pixel darker than in the scene without it is a walked hit whose light is hidden
    _, open_rad = oracle_film(lambda api: F.sphere_scene(api, "plastic", F.ONE), W, H)
    assert int((rad.sum(axis=2) < open_rad.sum(axis=2) - 0.05).sum()) > 20


@pytest.mark.parametrize("lights", ["inf_intensity", "zero_falloff"])
def test_guards(lights):
    which = {"inf_intensity": F.INF_INTENSITY, "zero_falloff": F.ZERO_FALLOFF}[lights]
    _, rad = check(lambda api: F.sphere_scene(api, "plastic", which), skips=(True, False), tag=lights)
    if lights == "zero_falloff":  # f_att == 0 at every hit: the light is skipped whatever its visibility -- the film of the scene without it
        _, dark = oracle_film(lambda api: F.sphere_scene(api, "plastic", []), W, H)
        assert np.array_equal(bits(rad), bits(dark))


def test_guard_light_at_a_hit_point():
    """The ONE light exactly at the point a pixel's shadow ray leaves from (p + p_err of the hit), with a falloff that is not zero there: d = 0,
    wi is NaN, the zero-length shadow ray hits nothing, so the light's term -- parked by the closest pass, added by the shadow pass -- is NaN."""
    o = oracle()
    base = G.Accel(F.sphere_scene(G, "plastic", F.ONE))
    ray = G.camera_rays(base, W, H, 20, 30, 21, 31)
    hit, _ = o.intersect(o.Accel(F.sphere_scene(o, "plastic", F.ONE)), ray)
    assert hit["kind"][0] != 0
    ng = hit["ng"][0] if np.dot(hit["ng"][0], -ray[0, 3:]) >= 0.0 else -hit["ng"][0]
    p = hit["p"][0] + ng * ERR
    at_hit = [([float(c) for c in p], [0.5, 0.5, 0.5], [1.0, 0.0, 0.0])]
    _, want_rad = check(lambda api: F.sphere_scene(api, "plastic", at_hit), skips=(True, False), tag="light_at_hit")
    assert np.isnan(want_rad[30, 20]).all(), want_rad[30, 20]  # d == 0 was hit: the case is not vacuous
    assert np.isnan(want_rad).sum() == 3, int(np.isnan(want_rad).sum())


def test_a_small_sphere_in_front_of_the_background():
    check(F.speck_scene, skips=(True, False), tag="speck")


@pytest.mark.parametrize("size", [64, 256])
def test_the_headline(size):
    check(lambda api: S.spheres_scene(api, nspheres=1024), size, size, relative=(True, False), tag="headline_%d" % size)


def test_nine_samples_in_both_orders():
    build = look(spheres64, None, ss=2)
    want_rgba, want_rad = oracle_film(build, W, H)
    acc = levels(build(G))
    for order in (0, 1):
        G.set_sample_order(acc, order)
        r = both_forms(acc, W, H, True, ("order", order))
        for switch in (True, False):
            assert np.array_equal(r[switch][0], want_rgba), (order, switch)
            assert same_radiance(r[switch][1], want_rad), (order, switch)
        assert np.array_equal(bits(r[True][1]), bits(r[False][1])), order


def test_a_strided_subset_a_crop_and_interleaved_rows():
    import torch
    build = lambda api: F.sphere_scene(api, "plastic", F.ONE)  # noqa: E731
    for k in (0, 3):
        check(build, W, H, k=k, n=7, tag="subset_%d" % k)  # holes in dense blocks, partially active tiles
    want_rgba, want_rad = oracle_film(build, W, H)
    acc = levels(build(G))
    rows = 4
    mine = np.concatenate([want_rgba[y:y + rows] for y in range(rows, H, 2 * rows)])  # rank 1 of 2: blocks 1, 3, ...
    for switch in (True, False):
        G.set_fused_shade(acc, switch)
        rgba, rad = G.capture_rect(acc, W, H, 5, 9, 61, 50)
        assert G.last_fused_shade(acc) == (ENV_ON and switch), switch
        assert np.array_equal(rgba, want_rgba[9:50, 5:61]) and same_radiance(rad, want_rad[9:50, 5:61]), switch
        tile = torch.zeros((mine.shape[0], W, 4), dtype=torch.uint8, device="cuda")
        G.capture_interleaved_device(acc, W, H, rows, 2, 1, tile.data_ptr())
        G.synchronize(acc)
        assert G.last_fused_shade(acc) == (ENV_ON and switch), switch
        assert np.array_equal(tile.cpu().numpy(), mine), switch


REFUSED = {
    "two_lights": lambda api: F.sphere_scene(api, "plastic", LIGHTS["two"]),
    "no_lights": lambda api: F.sphere_scene(api, "plastic", []),
    "nested_groups": F.nested_group_scene,  # the packet walk's gate says no
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_scenes_the_gate_refuses_still_match(name):
    check(REFUSED[name], takes=False, skips=(True, False), tag=name)


def test_the_packet_walks_switch_is_the_fused_forms_too():
    build = lambda api: F.sphere_scene(api, "plastic", F.ONE)  # noqa: E731
    want_rgba, want_rad = oracle_film(build, W, H)
    acc = levels(build(G))
    G.set_packet_walk(acc, False)
    r = both_forms(acc, W, H, False, "per-lane closest pass")
    for switch in (True, False):
        assert np.array_equal(r[switch][0], want_rgba) and same_radiance(r[switch][1], want_rad), switch


def test_counters_unchanged():
    acc = levels(F.sphere_scene(G, "plastic", F.ONE))
    stats = []
    for switch in (True, False):
        G.set_fused_shade(acc, switch)
        stats.append(G.capture_stats(acc, W, H))
    assert stats[0] == stats[1] and stats[0]["shadow_rays"] == stats[0]["hits"] > 0, stats


def test_the_switch_refuses_other_values():
    acc = G.Accel(S.readme_scene(G))
    assert G.last_fused_shade(acc) is None
    for bad in (-1, 2):
        assert G.call("accel_set_fused_shade", acc.h, bad) != 0
    G.set_fused_shade(acc, True)
