"""The exactness argument of the shadow skip, pinned on the CPU and independently of the device: where the light and
the viewer are on opposite sides of a hit's geometric normal (BSDF::f's `reflect` is false), the cosine is finite, the attenuation is
not NaN and PI * intensity is finite, the light's term of li() is +-0 whether or not the light is visible -- so a film rendered with the
shadow rays of exactly those (hit, light) pairs treated as unoccluded has the same bits.

li() is pyref's, restated here with that one change; the predicate is written from pyref's vectors."""
import math

import pytest

import pyref
from pyref import PI, ZERO, add, closest, cross, div, dot, magnitude, mul, mulv, neg, normalize, smul, sub
from shadow_skip_scenes import H, W, terminator_scene


def irrelevant(ng, wo, wi, wi_dot_n, f_att, intensity):
    reflect_ = dot(wi, ng) * dot(wo, ng) > 0.0
    return (not reflect_) and math.isfinite(wi_dot_n) and not math.isnan(f_att) and all(math.isfinite(PI * c) for c in intensity)


class Counts:
    hits = pairs = skipped_pairs = skipped_hits = occluded_skipped = guarded = 0


def li_skip(scene, o, d, depth, cnt):
    """pyref.li with the shadow ray of an irrelevant (hit, light) pair not traced: the light counts as visible."""
    hit = closest(scene, o, d)
    if hit is None:
        return pyref.background(scene, normalize(d))
    t, mat = hit["t"], hit["mat"]
    wo = neg(normalize(d))
    ng = normalize(cross(hit["g"][0], hit["g"][1]))
    if dot(ng, wo) < 0.0:
        ng = neg(ng)
    ns = normalize(hit["n"]) if hit["n"] is not None else normalize(cross(hit["s"][0], hit["s"][1]))
    err = 2.220446049250313e-16 * 2.0 ** 16
    p0 = add(o, mul(d, t))
    p_err = mul(ng, err)
    bsdf = pyref.BSDF(ng, ns, normalize(hit["s"][0]), pyref.scattering(mat))
    p = add(p0, p_err)
    output = ZERO
    cnt.hits += 1
    all_skipped = bool(scene.lights)
    for lpos, lint, fall in scene.lights:
        wi = sub(lpos, p)
        dist = magnitude(wi)
        f_att = fall[0] + fall[1] * dist + fall[2] * dist * dist
        wi = normalize(wi)
        wi_dot_n = dot(wi, ns)
        cnt.pairs += 1
        skipped = irrelevant(ng, wo, wi, wi_dot_n, f_att, lint)
        cnt.guarded += (not skipped) and not (dot(wi, ng) * dot(wo, ng) > 0.0)  # `reflect` is false and a guard keeps the walk
        if skipped:
            cnt.skipped_pairs += 1
            occ = closest(scene, p, sub(lpos, p))  # (traced only to count: the cases must include skipped rays that WERE occluded)
            cnt.occluded_skipped += occ is not None and occ["t"] < 1.0
        else:
            all_skipped = False
            occ = closest(scene, p, sub(lpos, p))
            if occ is not None and occ["t"] < 1.0:
                continue
        if f_att == 0.0:
            continue
        f = bsdf.f(wo, wi)
        term = div(mul(mulv(smul(PI, lint), f), wi_dot_n), f_att)
        if skipped:  # the device does not add the term at all (the hit's visibility word is 0): adding it must change no bit
            assert same_bits(add(output, term), output), (term, output)
        output = add(output, term)
    cnt.skipped_hits += all_skipped
    output = add(output, mulv(scene.ambient, bsdf.f(wo, ns)))
    refracted = reflected = ZERO
    if depth < scene.recursion:
        spectrum, wi, pdf = bsdf.sample_f(wo, pyref.TRANSMISSION | pyref.SPECULAR)
        if not (pdf <= 0.0 or spectrum == ZERO or abs(dot(wi, ns)) == 0.0):
            refracted = div(mul(mulv(spectrum, li_skip(scene, sub(p0, p_err), wi, depth + 1, cnt)), abs(dot(wi, ns))), pdf)
        spectrum, wi, pdf = bsdf.sample_f(wo, pyref.REFLECTION | pyref.SPECULAR)
        if not (pdf <= 0.0 or spectrum == ZERO or dot(wi, ns) <= 0.0):
            reflected = mulv(spectrum, li_skip(scene, add(p0, p_err), pyref.reflect(wo, ns), depth + 1, cnt))
    return add(add(output, reflected), refracted)


def same_bits(a, b):
    return all(math.copysign(1.0, x) == math.copysign(1.0, y) and (x == y or (x != x and y != y)) for x, y in zip(a, b))


@pytest.mark.parametrize("kind,lights", [("plastic", "one"), ("plastic", "two"), ("plastic", "three"), ("glass", "two"), ("matte20", "inf_intensity"),
                                         ("metal", "zero_falloff")])
def test_film_does_not_depend_on_skipped_shadow_rays(kind, lights):
    scene = terminator_scene(pyref.Api, kind, lights)
    want, _ = pyref.render(scene, W, H)
    cnt = Counts()
    for y in range(H):
        for x in range(W):
            (o, d), = scene.camera.sample(x, y, W, H)
            got = mul(add(ZERO, li_skip(scene, o, d, 0, cnt)), 1.0)
            assert same_bits(got, want[y][x]), (x, y, got, want[y][x])
    if lights == "inf_intensity":
        assert cnt.skipped_pairs == 0  # (the guard: 0 * inf is NaN, every walk is kept)
        return
    # not vacuous: many pairs are skipped, many are not, and some of the skipped rays were occluded (the sphere shadows its own far side)
    assert cnt.skipped_pairs > cnt.pairs // 10 and cnt.pairs - cnt.skipped_pairs > cnt.pairs // 10, vars(cnt)
    assert cnt.occluded_skipped > 0, vars(cnt)
    if lights != "one":
        assert 0 < cnt.skipped_hits < cnt.skipped_pairs  # hits at which only some of the lights are irrelevant


def test_light_at_a_hit_point_keeps_its_walk():
    """A light exactly where a pixel's shadow rays leave from: d = 0, wi and wi_dot_n are NaN, and so is the light's term when the zero-length
    shadow ray counts as visible -- `reflect` is false there (NaN > 0), so only the finiteness guard keeps the pair out of the skip."""
    x, y = 20, 30
    base = terminator_scene(pyref.Api, "plastic", "one")
    (o, d), = base.camera.sample(x, y, W, H)
    hit = closest(base, o, d)
    wo = neg(normalize(d))
    ng = normalize(cross(hit["g"][0], hit["g"][1]))
    if dot(ng, wo) < 0.0:
        ng = neg(ng)
    p = add(add(o, mul(d, hit["t"])), mul(ng, 2.220446049250313e-16 * 2.0 ** 16))
    scene = terminator_scene(pyref.Api, "plastic", "one", [(list(p), [0.5, 0.5, 0.5], [1.0, 0.0, 0.0])])
    want = pyref.li(scene, o, d, 0)
    assert all(c != c for c in want), want  # the case is the one meant: the pixel IS NaN
    cnt = Counts()
    got = li_skip(scene, o, d, 0, cnt)  # (asserts that no skipped term changes a bit)
    assert same_bits(got, want) and cnt.guarded == 1 and cnt.skipped_pairs == 1, vars(cnt)
