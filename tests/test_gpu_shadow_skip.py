"""The level-by-level pipeline's shadow skip (lg_accel_set_shadow_skip): the closest pass flags the hits at which no
light's term depends on the light being visible, the shadow pass does not walk them.  The film must not know: every case is compared bit
for bit -- RGBA bytes and f64 radiance -- with the CPU oracle AND with the same accel rendered with the switch off.

Scenes (shadow_skip_scenes.py): a sphere that fills a 64 x 64 film, lit from the side, so that 8 x 8 tiles lie wholly in the flagged
region, wholly outside it and across its boundary; every material; one, two, three and 33 lights; the guards of the flag's argument (an
infinite intensity, a light exactly at a hit point, a falloff of zero); kitchen_sink at recursion 2 (deeper levels, appended hits);
strided subsets and a crop (holes, partially active tiles); the work counters."""
import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from shadow_skip_scenes import H, W, terminator_scene

pytestmark = pytest.mark.gpu
G = la.api
ERR = 2.220446049250313e-16 * 65536.0  # the shading offset (integrate.rs:40)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_radiance(got, want):
    """Bit for bit, except that a NaN matches a NaN: IEEE 754 leaves the sign and payload of a NaN an operation GENERATES to the implementation
    (x86 makes 0xFFF8..., the GPU 0x7FF8...), so the bits of a NaN say which machine computed it, not what was computed.  (The film's bytes
    do not know: a NaN quantises to 0, img.rs:65-67.)"""
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def oracle_film(builder, w, h, k=0, n=1):
    o = oracle()
    oacc = o.Accel(builder(o))
    o.set_trig_mode(1)  # the portable trig the GPU uses: radiance is bit-comparable
    try:
        film = o.Film(w, h)
        o.capture_subset(k, n, oacc, film)
        return film.pixels(), o.capture_radiance(oacc, w, h, k, n)
    finally:
        o.set_trig_mode(0)


def gpu_film(acc, w, h, skip, k=0, n=1):
    G.set_streaming(acc, 2)  # level by level whatever the launch size
    G.set_shadow_skip(acc, skip)
    film = G.Film(w, h)
    G.capture_subset(k, n, acc, film)
    return film.pixels(), G.capture_radiance(acc, w, h, k, n)


def check(builder, w=W, h=H, k=0, n=1):
    want_rgba, want_rad = oracle_film(builder, w, h, k, n)
    acc = G.Accel(builder(G))
    on = gpu_film(acc, w, h, True, k, n)
    off = gpu_film(acc, w, h, False, k, n)
    G.set_shadow_skip(acc, True)
    assert np.array_equal(on[0], off[0]) and np.array_equal(bits(on[1]), bits(off[1])), "switch on against switch off"
    assert np.array_equal(on[0], want_rgba), int((on[0] != want_rgba).sum())
    assert same_radiance(on[1], want_rad), int((bits(on[1]) != bits(want_rad)).sum())
    return acc, want_rad


def test_terminator_across_tiles():
    _, rad = check(lambda api: terminator_scene(api, "plastic", "one"))
    # the picture is the one the cases are about: per 8 x 8 tile the share of pixels the light reaches (brighter than the ambient term alone
    # can make them) is 0 in some tiles, 1 in some and in between in others
    lit = (rad.sum(axis=2) > 0.45).reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3))
    assert (lit == 0.0).any() and (lit == 1.0).any() and ((lit > 0.0) & (lit < 1.0)).any(), lit


@pytest.mark.parametrize("kind", ["matte0", "matte20", "metal", "mirror", "glass"])
def test_every_material(kind):
    check(lambda api: terminator_scene(api, kind, "one"))


def test_kitchen_sink_recursion_2():
    check(lambda api: S.kitchen_sink_scene(api, recursion=2), 64, 64)


@pytest.mark.parametrize("lights", ["two", "three", "many"])
def test_several_lights(lights):
    check(lambda api: terminator_scene(api, "plastic", lights))


@pytest.mark.parametrize("lights", ["inf_intensity", "zero_falloff"])
def test_guards(lights):
    check(lambda api: terminator_scene(api, "plastic", lights))


def test_guard_light_at_a_hit_point():
    """A light exactly at the point a pixel's shadow rays leave from (p + p_err of the hit), with a falloff that is not zero there: d = 0, wi is
    NaN, the zero-length shadow ray hits nothing, so the light's term -- and the pixel -- is NaN.  `reflect` is false at that hit for both lights
    (NaN > 0 is false), so only the finiteness guard of wi_dot_n keeps the hit from being flagged; flagged, the pixel would be finite."""
    o = oracle()
    base = G.Accel(terminator_scene(G, "plastic", "one"))
    ray = G.camera_rays(base, W, H, 20, 30, 21, 31)
    hit, _ = o.intersect(o.Accel(terminator_scene(o, "plastic", "one")), ray)
    assert hit["kind"][0] != 0
    ng = hit["ng"][0] if np.dot(hit["ng"][0], -ray[0, 3:]) >= 0.0 else -hit["ng"][0]
    p = hit["p"][0] + ng * ERR
    extra = [([float(c) for c in p], [0.5, 0.5, 0.5], [1.0, 0.0, 0.0])]
    _, want_rad = check(lambda api: terminator_scene(api, "plastic", "one", extra))
    assert np.isnan(want_rad[30, 20]).all(), want_rad[30, 20]  # d == 0 was hit: the case is not vacuous
    assert np.isnan(want_rad).sum() == 3, int(np.isnan(want_rad).sum())


def test_counters_unchanged():
    acc = G.Accel(terminator_scene(G, "plastic", "two"))
    G.set_shadow_skip(acc, True)
    on = G.capture_stats(acc, W, H)
    G.set_shadow_skip(acc, False)
    off = G.capture_stats(acc, W, H)
    G.set_shadow_skip(acc, True)
    assert on == off and on["shadow_rays"] == 2 * on["hits"] > 0, (on, off)


def test_other_addressing_modes():
    builder = lambda api: terminator_scene(api, "plastic", "one")  # noqa: E731
    for k in (0, 3):
        check(builder, W, H, k, 7)  # a strided subset: holes in dense blocks, partially active tiles
    want_rgba, want_rad = oracle_film(builder, W, H)
    acc = G.Accel(builder(G))
    G.set_streaming(acc, 2)
    for skip in (True, False):
        G.set_shadow_skip(acc, skip)
        rgba, rad = G.capture_rect(acc, W, H, 5, 9, 61, 50)
        assert np.array_equal(rgba, want_rgba[9:50, 5:61]) and same_radiance(rad, want_rad[9:50, 5:61]), skip
