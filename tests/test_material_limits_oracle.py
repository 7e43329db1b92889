"""The conditions that keep tests/test_gpu_material_limits.py from being vacuous, checked on the CPU oracle alone (no GPU), and the
oracle against the independent witness tests/pyref.py at the same limits.  Scene, palette and light cases: tests/material_limits.py.

Measured on the oracle (portable trigonometry, 160 x 128; the assertions below are the bounds, these are the values):
  pixels that hold a NaN   plain lights, recursion 2: 5.8 %; every light case at recursion 1: 5.8 %, but 14.3 % for the two overflowing
                           intensities (inf in a channel, 1e308) and 39.2 % for the NaN falloff;
  a negative channel       2.3 % with plain lights (sigma 90 and 120, negative kd, metal roughness -0.2: their whole surface), 15.8 % with
                           the falloff that crosses zero;
  +-inf                    none with plain lights; 5,200 pixels with either overflowing intensity;
  exactly (0, 0, 0) on a hit   glass eta inf and NaN, glass and plastic with both colours zero, mirror kr 0;
  footprints               (the pixels where the entry alone differs from the floor alone) 109 .. 409 pixels; NaN-free share 100 % for 37
                           entries, 20 - 47 % for roughness 0, 1e-300, inf, NaN and metal u or v of 0, inf, NaN -- their surface is NaN
                           wherever the ambient term reaches it; the finite rest is the shadow they throw on the floor -- and 0 % for
                           metal eta = (1e200, 1e-200, 1): eta^2 overflows, fr_conductor's t1 - t2 is inf - inf in the x channel at
                           every hit.  Its twin eta = (1e70, 1e-70, 1) keeps eta^4 finite: 100 % NaN-free.  Where an entry stands matters:
                           before the solid background a specular entry whose weights clamp to one IS the background, bit for bit, and
                           an all-NaN surface is finite only in its shadow, so material_limits.palette puts those in the lowest rows;
  the two libm modes       no film byte differs; 0 to 3 pixels of 20,480 a case differ in the radiance's last bits (sphere.rs' atan2 / acos).
The witness: on a 48 x 36 film, plain lights and every light case, pyref's radiance and the oracle's are bit-identical on every pixel, NaN
positions included.  What the witness needed was in its Python, not its arithmetic: math.sqrt of a negative operand and a division by zero
raise where IEEE arithmetic (Rust's, C++'s) gives NaN or inf -- pyref._sqrt, pyref._div -- and max(-0.0, 0.0) hands back -0.0 where the
clamp of bsdf.rs:133, `maxsd x, 0.0` in an optimised x86-64 build, gives +0.0 -- pyref.max_const, pyref.min_const.
The backlit sheet (material_limits.sheet_scene, 64 x 48): 266 pixels of the sheet, every one NaN under the NaN falloff and the ambient term
alone under plain lights -- the one place where a shadow walk skipped in error would show."""
import functools

import numpy as np
import pytest

import material_limits as ML
import pyref
from oracle_lib import oracle

ROWS = (len(ML.NAMES) + ML.COLS - 1) // ML.COLS


@functools.lru_cache(maxsize=None)
def render(lights="plain", recursion=2, only=None, portable=True, w=ML.W, h=ML.H):
    """(radiance, film bytes) of the oracle; computed once, read-only."""
    o = oracle()
    acc = o.Accel(ML.limits_scene(o, lights=lights, recursion=recursion, only=only))
    o.set_trig_mode(1 if portable else 0)
    try:
        film = o.Film(w, h)
        o.capture_subset_mt(0, 1, acc, film, 8)
        rad, px = o.capture_radiance(acc, w, h, nthreads=8), film.pixels().copy()
    finally:
        o.set_trig_mode(0)
    rad.setflags(write=False)
    px.setflags(write=False)
    return rad, px


def nan_share(rad):
    return float(np.isnan(rad).any(axis=-1).mean())


def test_the_palette_holds_every_limit():
    n = set(ML.NAMES)
    assert len(ML.NAMES) == len(n) == 47 and ROWS == 6
    for r in ("0p0", "1em300", "1em08", "1p0", "50p0", "inf", "m0p25", "nan"):
        assert "plastic_rough_" + r in n
    for e in ("1p0", "0p5", "0p001", "1000000p0", "0p0", "m1p5", "inf", "nan"):
        assert "glass_eta_" + e in n
    for s in ("0p0", "1em09", "90p0", "120p0", "m5p0", "nan"):
        assert "matte_sigma_" + s in n
    assert sum(x.startswith("metal_uv_") for x in n) == 7 and sum(x.startswith("mirror") for x in n) == 3 and ML.ALL_NAN in n
    assert set(ML.LIGHT_CASES) >= {"falloff_crosses_zero", "falloff_nan", "falloff_zero", "falloff_inf", "intensity_zero", "intensity_1e308"}
    rec = ML.light_records("falloff_crosses_zero")
    assert rec.shape == (2,) and rec["falloff"][1].tolist() == [-1.0, 0.1, 0.0] and rec["position"][0].tolist() == [-6.0, 12.0, 9.0]


def test_nan_pixels_with_plain_lights():
    rad, _ = render()
    share = nan_share(rad)
    print("plain lights, recursion 2: %.2f %% of pixels hold a NaN" % (100 * share))
    assert 0.0 < share <= 0.10, share


@pytest.mark.parametrize("case", sorted(ML.LIGHT_CASES))
def test_nan_pixels_of_a_light_case(case):
    rad, _ = render(lights=case, recursion=1)
    share = nan_share(rad)
    print("%s, recursion 1: %.2f %% of pixels hold a NaN" % (case, 100 * share))
    assert 0.0 < share <= (0.50 if case == "falloff_nan" else 0.20), (case, share)
    if case == "falloff_crosses_zero":  # the attenuation is negative near the light, positive far from it: both signs of its term show
        plain, _ = render(recursion=1)
        with np.errstate(invalid="ignore"):
            assert (rad < plain).any() and (rad > plain).any()
    if case in ("intensity_inf_channel", "intensity_1e308"):
        assert np.isinf(rad).any(), case


@pytest.mark.parametrize("i", range(len(ML.NAMES)), ids=ML.NAMES)
def test_every_entry_has_a_footprint_that_is_not_all_nan(i):
    alone, floor = render(only=i)[0], render(only=-1)[0]
    foot = (ML.bits(alone) != ML.bits(floor)).any(axis=-1)
    clean = float((~np.isnan(alone[foot]).any(axis=-1)).mean()) if foot.any() else 0.0
    print("%s: footprint %d pixels, %.1f %% free of NaN" % (ML.NAMES[i], int(foot.sum()), 100 * clean))
    assert foot.sum() >= 100, (ML.NAMES[i], int(foot.sum()))
    if ML.NAMES[i] == ML.ALL_NAN:  # the single exception, by name: eta^2 overflows and every hit is NaN in x
        assert clean == 0.0
    else:
        assert clean >= 0.15, (ML.NAMES[i], clean)


def test_the_film_shows_every_class_of_behaviour():
    rad, px = render()
    hit = (ML.bits(rad) != ML.bits(np.broadcast_to(np.array(ML.BACKGROUND), rad.shape))).any(axis=-1)
    nan = np.isnan(rad).any(axis=-1)
    with np.errstate(invalid="ignore"):
        negative = (rad < 0.0).any(axis=-1)
        zero = hit & (rad == 0.0).all(axis=-1)
        finite = hit & np.isfinite(rad).all(axis=-1) & (rad > 0.0).all(axis=-1)
    over, _ = render(lights="intensity_1e308", recursion=1)
    assert nan.any() and negative.any() and zero.sum() >= 100 and finite.mean() >= 0.25, (nan.sum(), negative.sum(), zero.sum(), finite.mean())
    assert np.isposinf(over).any() and np.isneginf(over).any(), "both infinities, under the overflowing light"
    assert np.isnan(rad).any(axis=-1).sum() > np.isnan(rad).all(axis=-1).sum() > 0, "NaN in one channel and in all three"
    # the NaN positions are part of the answer: the film maps them to 0, channel by channel
    assert (px[..., :3][np.isnan(rad)] == 0).all()


# "No pixel" is the film: no byte of it differs.  In f64 radiance a few pixels differ in their last bits (sphere.rs' atan2 / acos, one ulp
# apart in the two modes); their number per case, measured here and pinned so that a change of either trigonometry shows:
LIBM_LAST_BIT_PIXELS = {"plain": 2, "falloff_crosses_zero": 3, "falloff_inf": 2, "falloff_nan": 0, "falloff_negative_quadratic": 3, "falloff_zero": 2,
                        "intensity_1e308": 0, "intensity_inf_channel": 2, "intensity_zero": 2, "negative_zero_intensity": 3}


def test_the_two_libm_modes_differ_on_no_pixel():
    for lights, recursion in [("plain", 2), ("plain", 0)] + [(c, 1) for c in sorted(ML.LIGHT_CASES)]:
        (rad, px), (rad_libm, px_libm) = render(lights, recursion), render(lights, recursion, portable=False)
        assert np.array_equal(px, px_libm), (lights, int((px != px_libm).any(axis=-1).sum()))
        assert np.array_equal(np.isnan(rad), np.isnan(rad_libm)), lights
        last_bits = int((ML.bits(rad) != ML.bits(rad_libm)).any(axis=-1).sum())
        assert np.allclose(rad, rad_libm, rtol=1e-12, atol=1e-15, equal_nan=True) and last_bits == LIBM_LAST_BIT_PIXELS[lights], (lights, last_bits)


def test_the_backlit_sheet_is_where_a_skipped_shadow_walk_would_show():
    """material_limits.sheet_scene under the NaN falloff: with the light in the sheet's plane every pixel of the sheet is NaN, and with the
    same light behind a closed solid's back none would be (the solid blocks it) -- the palette scene cannot show this."""
    o = oracle()
    rays = np.array([list(a) + list(b) for y in range(ML.SHEET_H) for x in range(ML.SHEET_W)
                     for a, b in ML.sheet_scene(pyref.Api).camera.sample(x, y, ML.SHEET_W, ML.SHEET_H)])
    out = {}
    for lights in ("plain", "falloff_nan"):
        oacc = o.Accel(ML.sheet_scene(o, lights))
        out[lights] = o.capture_radiance(oacc, ML.SHEET_W, ML.SHEET_H, nthreads=8).reshape(-1, 3)
    hits, _ = o.intersect(o.Accel(ML.sheet_scene(o)), rays)
    sheet = hits["kind"] == 3  # a triangle
    assert sheet.sum() >= 250 and not np.isnan(out["plain"]).any()
    assert np.isnan(out["falloff_nan"][sheet]).all(), "0 * (wi . n) / NaN at every hit of the sheet"
    ambient_alone = np.array(ML.AMBIENT) * np.array((0.6, 0.6, 0.6)) * pyref.FRAC_1_PI  # (in some order of its three products)
    assert (out["plain"][sheet] == out["plain"][sheet][0]).all() and np.allclose(out["plain"][sheet][0], ambient_alone, rtol=1e-14, atol=0.0), "no light is reflected"
    prad, _ = pyref.render(ML.sheet_scene(pyref.Api, "falloff_nan"), ML.SHEET_W, ML.SHEET_H)
    assert np.array_equal(ML.bits(np.asarray(prad).reshape(-1, 3)), ML.bits(out["falloff_nan"]))


# ---- the independent witness ---------------------------------------------------------------------------------------------------------------
RTOL, ATOL = 1e-12, 1e-15  # tests/test_pyref_witness.py


@pytest.mark.parametrize("lights", ["plain"] + sorted(ML.LIGHT_CASES))
def test_the_witness_agrees_with_the_oracle(lights):
    w, h = 48, 36
    recursion = 2 if lights == "plain" else 1
    orad, opx = render(lights, recursion, portable=False, w=w, h=h)  # libm trigonometry on both sides
    prad, prgba = pyref.render(ML.limits_scene(pyref.Api, lights=lights, recursion=recursion), w, h)
    prad, prgba = np.asarray(prad, dtype=np.float64), np.asarray(prgba, dtype=np.uint8)
    assert np.isnan(orad).any() and np.array_equal(np.isnan(prad), np.isnan(orad)), (lights, "NaN positions")
    assert np.array_equal(np.isinf(prad), np.isinf(orad))
    assert np.allclose(prad, orad, rtol=RTOL, atol=ATOL, equal_nan=True), lights
    assert np.array_equal(prgba, opx), (lights, int((prgba != opx).any(axis=-1).sum()))
    same = int((ML.bits(prad) == ML.bits(orad)).all(axis=-1).sum())
    print("%s: %d of %d pixels bit-identical in f64 radiance, %d hold a NaN" % (lights, same, w * h, int(np.isnan(orad).any(axis=-1).sum())))
    assert same >= (w * h * 99) // 100


def test_the_witness_takes_the_ieee_branches():
    """What Python would raise on and IEEE arithmetic answers: the two helpers the limits made necessary."""
    assert pyref._sqrt(-1.0) != pyref._sqrt(-1.0) and pyref._sqrt(-0.0) == 0.0 and pyref._sqrt(ML.INF) == ML.INF
    assert pyref._div(1.0, 0.0) == ML.INF and pyref._div(-1.0, 0.0) == -ML.INF and pyref._div(1.0, -0.0) == -ML.INF and pyref._div(0.0, 0.0) != pyref._div(0.0, 0.0)
    assert str(pyref.max_const(-0.0, 0.0)) == "0.0" and pyref.max_const(ML.NAN, 0.0) == 0.0 and pyref.min_const(pyref.max_const(-0.5, 0.0), 1.0) == 0.0
    assert pyref.min_const(ML.INF, 1.0) == 1.0 and str(pyref.min_const(pyref.max_const(-0.0, 0.0), 1.0)) == "0.0"  # maxsd / minsd x, const
    assert pyref.tr_d(0.0, 0.0, (0.0, 0.0, 1.0)) != pyref.tr_d(0.0, 0.0, (0.0, 0.0, 1.0))      # 1 / (pi * 0 * 0 * ...): 0 * (1 + NaN)
    assert pyref.tr_d(ML.INF, 0.3, pyref.normalize((0.3, 0.2, 0.9))) == 0.0                     # 1 / inf
    assert pyref.fr_dielectric(0.5, 1.0, ML.NAN) != pyref.fr_dielectric(0.5, 1.0, ML.NAN)       # NaN >= 1.0 is false: the formula runs
    assert pyref.fr_dielectric(0.5, 1.0, 0.0) == 1.0                                            # sin_t = inf >= 1.0
