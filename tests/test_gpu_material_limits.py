"""Shading at the limits of the material and light parameters (tests/material_limits.py), pinned to the CPU oracle:
every entry point that restates shade.h -- the render in each organisation and traversal form, with the shadow skip on and off, one and
four samples a pixel; lg_radiance, lg_radiance_groups, lg_scatter, lg_scatter_lit, lg_capture_rays, lg_capture_views and
lg_radiance_gather on the camera's own rays -- gives the oracle's film of a 47-material palette under plain lights and under nine lights
whose intensity or falloff is negative, zero, infinite, overflowing or NaN.  tests/test_material_limits_oracle.py shows on the CPU that the
comparison is not vacuous: 6 % of the plain film's pixels hold a NaN (39 % under the NaN falloff), 2 % a negative channel, and those
positions are part of the answer.  The palette's closed solids block every light they do not reflect, so one more scene, an open sheet
seen from behind with a light in its plane (material_limits.sheet_scene), holds the hits at which the shadow skip's NaN guard decides.

Every comparison is of bit patterns with NaNs canonicalised (material_limits.bits) and of RGBA8 bytes; nothing is tolerated, except where
the CPU witness tests/pyref.py (glibc's trigonometry, not the portable one) is the reference: the child weights of lg_scatter on the
spheres, under tests/test_pyref_witness.py's rtol 1e-12 / atol 1e-15 with presence, flags, NaN positions, signed zeros and clamped ones
compared exactly; on the cubes, whose frames hold no trigonometry, the weights are the witness's bit for bit.  A failure
names the palette entries whose primary hits hold the differing pixels."""
import functools

import numpy as np
import pytest

import lasgun_amd as la
import material_limits as ML
import pyref
import scatter_ref as R
from light_subsets import group_pairs, subset_scene
from oracle_lib import oracle
from test_gpu_fuzz import ORGANISATIONS
from test_gpu_radiance_query import each_form

pytestmark = pytest.mark.gpu
G = la.api
W, H = ML.W, ML.H
bits = ML.bits
CASES = [("plain", 0), ("plain", 2)] + [(c, 1) for c in sorted(ML.LIGHT_CASES)]
CASE_IDS = ["%s_r%d" % c for c in CASES]
LIT_CASES = ["plain"] + sorted(ML.LIGHT_CASES)
ENTRY_CENTRES = np.array([[(i % ML.COLS - 3.5) * 1.6, (i // ML.COLS) * 1.5, 0.0] for i in range(len(ML.NAMES))])


@functools.lru_cache(maxsize=None)
def oracle_film(lights="plain", recursion=2, supersampling=0, only=None, w=W, h=H, subset=None):
    """(radiance (h, w, 3), film bytes) of the oracle in portable-trig mode; subset: (light mask, ambient) of tests/light_subsets.py.
    Computed once, read-only."""
    o = oracle()
    build = ML.builder(lights=lights, recursion=recursion, supersampling=supersampling, only=only)
    oacc = o.Accel(build(o) if subset is None else subset_scene(o, build, *subset))
    o.set_trig_mode(1)
    try:
        film = o.Film(w, h)
        o.capture_subset_mt(0, 1, oacc, film, 8)
        rad, px = o.capture_radiance(oacc, w, h, nthreads=8), film.pixels().copy()
    finally:
        o.set_trig_mode(0)
    rad.setflags(write=False)
    px.setflags(write=False)
    return rad, px


@functools.lru_cache(maxsize=None)
def accel_of(lights="plain", recursion=2, no_lights=False):
    return G.Accel.from_scene(ML.limits_scene(G, lights=lights, recursion=recursion, no_lights=no_lights))


@functools.lru_cache(maxsize=None)
def camera_rays(w=W, h=H):
    rays = G.camera_rays(accel_of(), w, h)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def owners(w=W, h=H):
    """(w * h,) int: the palette entry the pixel's camera ray hits first, -1 the floor, -2 nothing; from the oracle's hits."""
    o = oracle()
    hits, _ = o.intersect(o.Accel(ML.limits_scene(o)), camera_rays(w, h))
    p = np.ascontiguousarray(hits["p"])
    d = np.linalg.norm(p[:, None, :] - ENTRY_CENTRES[None], axis=2)
    own = np.where(d.min(axis=1) < 0.9, d.argmin(axis=1), -1)
    own[hits["kind"] == 0] = -2
    return own


def blame(differs, w=W, h=H, own=None):
    """The names of the entries (floor, background) that hold the pixels of the mask `differs`, with the count of each."""
    own = owners(w, h) if own is None else own
    ids, counts = np.unique(own[np.asarray(differs).reshape(-1)], return_counts=True)
    return {(ML.NAMES[i] if i >= 0 else ("floor", "background")[-1 - i]): int(c) for i, c in zip(ids, counts)}


def same_radiance(ctx, got, want, **kw):
    got, want = np.asarray(got).reshape(-1, 3), np.asarray(want).reshape(-1, 3)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    differs = (bits(got) != bits(want)).any(axis=1)
    assert not differs.any(), (ctx, "radiance differs in %d pixels" % int(differs.sum()), blame(differs, **kw))


def same_film(ctx, got, want, **kw):
    differs = (np.asarray(got).reshape(-1, 4) != np.asarray(want).reshape(-1, 4)).any(axis=1)
    assert not differs.any(), (ctx, "film bytes differ in %d pixels" % int(differs.sum()), blame(differs, **kw))


def organisations(acc):
    """Sets each organisation and traversal form of the fuzz campaign on the accel and yields it; fast mode may refuse the scene."""
    try:
        for streaming, fast, _, prune in ORGANISATIONS:
            G.set_streaming(acc, streaming)
            G.set_prune(acc, prune)
            try:
                G.set_mode(acc, fast)
            except la.LasgunError as e:
                assert fast and ("inverse" in str(e) or "smallest triangle" in str(e)), str(e)
                continue
            yield (streaming, fast, prune)
    finally:
        G.set_mode(acc, False)
        G.set_prune(acc, None)
        G.set_streaming(acc, 1)


def render(acc, w, h):
    film = G.Film(w, h)
    G.capture_subset(0, 1, acc, film)
    return G.capture_radiance(acc, w, h), film.pixels()


# ---- the render -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("supersampling", [0, 1])
@pytest.mark.parametrize("lights,recursion", CASES, ids=CASE_IDS)
def test_the_render_is_the_oracles_in_every_organisation(lights, recursion, supersampling):
    want_rad, want_px = oracle_film(lights, recursion, supersampling)
    assert np.isnan(want_rad).any() and not np.isnan(want_rad).all(axis=-1).all()
    acc = G.Accel.from_scene(ML.limits_scene(G, lights=lights, recursion=recursion, supersampling=supersampling))
    assert G.camera_samples(acc) == (4 if supersampling else 1)
    done = 0
    try:
        for org in organisations(acc):
            for skip in (True, False):
                G.set_shadow_skip(acc, skip)
                rad, px = render(acc, W, H)
                same_film((lights, recursion, supersampling, org, skip), px, want_px)
                same_radiance((lights, recursion, supersampling, org, skip), rad, want_rad)
                done += 1
    finally:
        G.set_shadow_skip(acc, True)
    assert done >= 2 * sum(1 for o in ORGANISATIONS if not o[1]), done


def test_a_ragged_film():
    w, h = 67, 45
    want_rad, want_px = oracle_film("plain", 2, 0, None, w, h)
    assert np.isnan(want_rad).any()
    acc = G.Accel.from_scene(ML.limits_scene(G))  # (its own accel: a failure here leaves no form set on one that later cases share)
    own = owners(w, h)
    for org in organisations(acc):
        rad, px = render(acc, w, h)
        same_film((w, h, org), px, want_px, own=own)
        same_radiance((w, h, org), rad, want_rad, own=own)


@pytest.mark.parametrize("i", range(len(ML.NAMES)), ids=ML.NAMES)
def test_each_entry_alone(i):
    w, h = ML.ENTRY_W, ML.ENTRY_H
    want_rad, want_px = oracle_film("plain", 2, 0, i, w, h)
    floor_rad, _ = oracle_film("plain", 2, 0, -1, w, h)
    assert (bits(want_rad) != bits(floor_rad)).any(), (ML.NAMES[i], "the entry shows on this film")
    acc = G.Accel.from_scene(ML.limits_scene(G, only=i))
    for streaming in (1, 0):  # the organisation the library chooses, and the megakernel
        G.set_streaming(acc, streaming)
        rad, px = render(acc, w, h)
        d_px = int((px != want_px).any(axis=-1).sum())
        d_rad = int((bits(rad) != bits(want_rad)).any(axis=-1).sum())
        assert d_px == 0 and d_rad == 0, ("material %s" % ML.NAMES[i], "streaming", streaming, "film bytes differ in %d pixels, radiance in %d" % (d_px, d_rad))


# ---- the hits at which the shadow skip decides something ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sheet_oracle(lights, recursion):
    o = oracle()
    oacc = o.Accel(ML.sheet_scene(o, lights, recursion))
    o.set_trig_mode(1)
    try:
        film = o.Film(ML.SHEET_W, ML.SHEET_H)
        o.capture_subset_mt(0, 1, oacc, film, 8)
        return o.capture_radiance(oacc, ML.SHEET_W, ML.SHEET_H, nthreads=8), film.pixels().copy()
    finally:
        o.set_trig_mode(0)


@pytest.mark.parametrize("lights", LIT_CASES)
def test_the_backlit_sheet(lights):
    """material_limits.sheet_scene: every light unreflected at the sheet's hits and one of them visible -- under the NaN falloff the only
    hits at which a skipped shadow walk would lose the reference's NaN."""
    w, h = ML.SHEET_W, ML.SHEET_H
    want_rad, want_px = sheet_oracle(lights, 1)
    if lights == "falloff_nan":
        assert np.isnan(want_rad).all(axis=-1).sum() >= 250, "the sheet is NaN: the light in its plane is visible"
    acc = G.Accel.from_scene(ML.sheet_scene(G, lights))
    try:
        for org in organisations(acc):
            for skip in (True, False):
                G.set_shadow_skip(acc, skip)
                rad, px = render(acc, w, h)
                d_px, d_rad = int((px != want_px).any(axis=-1).sum()), int((bits(rad) != bits(want_rad)).any(axis=-1).sum())
                assert d_px == 0 and d_rad == 0, (lights, org, "skip", skip, "film bytes differ in %d pixels, radiance in %d" % (d_px, d_rad))
    finally:
        G.set_shadow_skip(acc, True)
    rays = G.camera_rays(acc, w, h)
    got = G.radiance(acc, rays)
    assert np.array_equal(bits(got), bits(want_rad.reshape(-1, 3))), (lights, "radiance")
    planes = G.radiance_groups(acc, rays, [la.LightGroup(0b11, ambient=True), la.LightGroup(0b10)])
    assert np.array_equal(bits(planes[0]), bits(got)), (lights, "radiance_groups")
    # lit scatter: the same lights passed with the call, on an accel without any
    bare = G.Accel.from_scene(ML.sheet_scene(G, lights, no_lights=True))
    table = ML.sheet_records(lights)
    full = G.scatter_lit(bare, rays, table, ML.AMBIENT)
    lean = G.scatter_lit(bare, rays, table, ML.AMBIENT, ("direct", "terms"))
    for p in ("direct", "terms"):
        assert np.array_equal(bits(lean[p]), bits(full[p])), (lights, p, "with and without visible")
    assert np.array_equal(bits((0.0 + full["direct"]) * 1.0), bits(sheet_oracle(lights, 0)[0].reshape(-1, 3))), (lights, "direct at depth 0")
    assert np.array_equal(bits(G.scatter(acc, rays, ("direct",))["direct"]), bits(full["direct"])), (lights, "lg_scatter's direct")


# ---- the radiance family, on the camera's own rays --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights,recursion", CASES, ids=CASE_IDS)
def test_radiance_is_the_oracles(lights, recursion):
    want, _ = oracle_film(lights, recursion)
    acc, rays = G.Accel.from_scene(ML.limits_scene(G, lights=lights, recursion=recursion)), camera_rays()  # (its own accel, as above)
    forms = set()
    try:
        for form in each_form(acc):
            for order in (0, 1):
                G.set_query_order(acc, order)
                same_radiance((lights, recursion, form, order), G.radiance(acc, rays), want)
            G.set_query_order(acc, 0)
            forms.add(form)
    finally:
        G.set_query_order(acc, 0)
    assert {"reference", "prune"} <= forms, forms


@pytest.mark.parametrize("lights,recursion", CASES, ids=CASE_IDS)
def test_radiance_groups_are_the_oracles_renders_of_the_light_subsets(lights, recursion):
    acc, rays = accel_of(lights, recursion), camera_rays()
    assert G.light_count(acc) == 2
    pairs = group_pairs(2)
    planes = G.radiance_groups(acc, rays, [la.LightGroup(m, ambient=a) for m, a in pairs])
    for g, (m, a) in enumerate(pairs):
        same_radiance((lights, recursion, "group", m, a), planes[g], oracle_film(lights, recursion, subset=(m, a))[0])
    full = pairs.index((0b11, True))
    same_radiance((lights, recursion, "all lights and ambient"), planes[full], G.radiance(acc, rays))
    if lights not in ("falloff_zero", "falloff_inf", "intensity_zero"):  # not vacuous: the case's own light shows (those three add nothing, or +-0)
        assert (bits(planes[pairs.index((0b10, False))]) != bits(planes[pairs.index((0, False))])).any()


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_the_scatter_composition_is_the_oracles_radiance(depth):
    want, _ = oracle_film("plain", depth)
    acc = accel_of()  # one accel, whatever depth is composed
    got = R.compose(lambda r: G.scatter(acc, r), camera_rays(), depth)
    same_radiance(("compose", depth), got, want)


def witness_children(pscene, rays):
    """Per ray, from the CPU witness (scatter_ref.witness_level's presence tests, with the weights beside them): flags, reflect_weight
    (n, 3), refract_weight (n, 5)."""
    n = len(rays)
    flags, rw, tw = np.zeros(n, dtype=np.uint32), np.zeros((n, 3)), np.zeros((n, 5))
    P = pyref
    for i, r in enumerate(rays):
        o, d = tuple(float(x) for x in r[:3]), tuple(float(x) for x in r[3:])
        hit = P.closest(pscene, o, d)
        if hit is None:
            continue
        flags[i] = R.HIT
        wo = P.neg(P.normalize(d))
        ng = P.normalize(P.cross(hit["g"][0], hit["g"][1]))
        if P.dot(ng, wo) < 0.0:
            ng = P.neg(ng)
        ns = P.normalize(hit["n"]) if hit["n"] is not None else P.normalize(P.cross(hit["s"][0], hit["s"][1]))
        bsdf = P.BSDF(ng, ns, P.normalize(hit["s"][0]), P.scattering(hit["mat"]))
        spectrum, wi, pdf = bsdf.sample_f(wo, P.TRANSMISSION | P.SPECULAR)
        if not (pdf <= 0.0 or spectrum == P.ZERO or abs(P.dot(wi, ns)) == 0.0):
            flags[i] |= R.REFRACT
            tw[i] = tuple(spectrum) + (abs(P.dot(wi, ns)), pdf)
        spectrum, wi, pdf = bsdf.sample_f(wo, P.REFLECTION | P.SPECULAR)
        if not (pdf <= 0.0 or spectrum == P.ZERO or P.dot(wi, ns) <= 0.0):
            flags[i] |= R.REFLECT
            rw[i] = spectrum
    return flags, rw, tw


def test_the_child_planes_of_the_specular_entries():
    rays, own = camera_rays(), owners()
    sel = np.isin(own, ML.SPECULAR)
    out = G.scatter(accel_of(), np.ascontiguousarray(rays[sel]))
    flags, rw, tw = witness_children(ML.limits_scene(pyref.Api), rays[sel])
    names = np.array(ML.NAMES)[own[sel]]
    for i in ML.SPECULAR:
        assert (own[sel] == i).sum() >= 50, (ML.NAMES[i], "rays on the entry")
    bad = out["flags"] != flags
    assert not bad.any(), ("presence and flags", sorted(set(names[bad])), int(bad.sum()))
    has_r, has_t = (flags & R.REFLECT) != 0, (flags & R.REFRACT) != 0
    for plane, absent in (("reflect", ~has_r), ("reflect_weight", ~has_r), ("refract", ~has_t), ("refract_weight", ~has_t)):
        zero = ~out[plane][absent].view(np.uint64).any(axis=1)
        assert zero.all(), (plane, "an absent child's elements are +0.0", sorted(set(names[absent][~zero])))
    # A cube's shading frame holds no trigonometry: its weights are the witness's, bit for bit.  A sphere's dpdu comes from sin / cos of phi,
    # glibc's in the witness and the portable ones on the device: the witness's own tolerance there, and exactness for what no ulp can move.
    cube = own[sel] % 3 == 2
    assert (cube & has_r).sum() >= 100 and (cube & has_t).sum() >= 100 and (~cube & has_r).sum() >= 100 and (~cube & has_t).sum() >= 100
    for plane, want in (("reflect_weight", rw), ("refract_weight", tw)):
        got = out[plane]
        bad = (bits(got) != bits(want)).any(axis=1) & cube
        assert not bad.any(), (plane, "cubes, bit for bit", sorted(set(names[bad])), int(bad.sum()))
        exact = (np.isnan(want) | (want == 0.0) | (want == 1.0) | np.isinf(want))  # NaN positions, zeros (signed), clamped ones, infinities: exactly
        bad = (bits(got) != bits(want)) & exact
        assert not bad.any(), (plane, "NaN, 0, 1 and inf", sorted(set(names[bad.any(axis=1)])))
        with np.errstate(invalid="ignore"):
            bad = ~(np.isclose(got, want, rtol=1e-12, atol=1e-15, equal_nan=True))
        assert not bad.any(), (plane, sorted(set(names[bad.any(axis=1)])))
        same = (bits(got) == bits(want)).all(axis=1)[~cube]
        assert same.sum() * 100 >= 99 * len(same), (plane, int((~same).sum()), len(same))
    # every class among what was pinned: children present and absent, a weight of exactly zero in a channel of a present child, clamped ones
    both, none_ = has_r & has_t, (flags == R.HIT)
    assert both.sum() >= 100 and none_.sum() >= 100 and (has_r & ~has_t).sum() >= 100 and (has_t & ~has_r).sum() >= 100, (both.sum(), none_.sum())
    assert (rw[has_r] == 0.0).any() and (rw[has_r] == 1.0).any() and (tw[has_t][:, :3] == 0.0).any()


@pytest.mark.parametrize("lights", LIT_CASES)
def test_scatter_lit_under_the_cases_lights(lights):
    rays = camera_rays()
    bare = accel_of(no_lights=True)
    table = ML.light_records(lights)
    full = G.scatter_lit(bare, rays, table, ML.AMBIENT)  # visible asked for: every pair is walked
    lean = G.scatter_lit(bare, rays, table, ML.AMBIENT, ("direct", "terms"))  # the skip decides which pairs are
    for p in ("direct", "terms"):
        differs = (bits(lean[p]) != bits(full[p])).reshape(len(rays), -1).any(axis=1)
        assert not differs.any(), (lights, p, "with and without visible", blame(differs))
    want = G.scatter(accel_of(lights, 1), rays, ("direct",))["direct"]
    same_radiance((lights, "direct is lg_scatter's on an accel built with the lights"), full["direct"], want)
    same_radiance((lights, "(0 + direct) * 1 is the oracle's radiance at depth 0"), (0.0 + full["direct"]) * 1.0, oracle_film(lights, 0)[0])
    hit = (full["flags"] & R.HIT) != 0
    assert hit.mean() >= 0.25 and (~hit).any() and full["terms"].shape == (len(rays), 2, 3)
    if lights == "falloff_zero":
        assert not full["terms"][:, 1].view(np.uint64).any(), "f_att == 0: never added"
    if lights == "falloff_nan":
        assert np.isnan(full["terms"][hit][:, 1]).any()


def test_capture_rays_capture_views_and_gathers_are_radiances_bytes():
    acc, rays = accel_of(), camera_rays()
    want_rad, want_px = oracle_film()
    rad = G.radiance(acc, rays)
    same_radiance("radiance", rad, want_rad)
    px, rgb = G.capture_rays(acc, rays, W, H, rgba=True, rgb=True)
    same_radiance("capture_rays", rgb, rad)
    same_film("capture_rays", px, want_px)
    px, rgb = G.capture_views(acc, [G.accel_view(acc)], W, H, rgba=True, rgb=True)
    same_radiance("capture_views", rgb[0], rad)
    same_film("capture_views", px[0], want_px)
    origin = rays[0, :3]
    assert (rays[:, :3].view(np.uint64) == origin.view(np.uint64)).all(), "a perspective camera: one origin"
    dirs = np.ascontiguousarray(rays[:, 3:])
    for lanes in ("direction", "pose"):
        got = G.radiance_gather(acc, np.stack([origin, origin]), dirs, planes=("radiance",), lanes=lanes)["radiance"]
        for pose in (0, 1):
            same_radiance(("radiance_gather", lanes, pose), got[pose], rad)


# ---- queries after shading --------------------------------------------------------------------------------------------------------------------
def test_intersect_on_the_same_accel_is_still_the_oracles():
    acc, rays = accel_of(), camera_rays()
    G.radiance(acc, rays)
    hits = G.intersect(acc, rays)
    o = oracle()
    o.set_trig_mode(1)
    try:
        want, wmat = o.intersect(o.Accel(ML.limits_scene(o)), rays)
    finally:
        o.set_trig_mode(0)
    for k in ("t", "p", "ng", "ns"):
        assert np.array_equal(bits(hits[k]), bits(want[k])), k
    for k in ("kind", "prim", "instance"):
        assert np.array_equal(hits[k], want[k]), k
    hit = want["kind"] != 0
    assert hit.mean() >= 0.25 and (~hit).any() and np.array_equal(hits["material"] == -1, ~hit)
    table = {int(m): G.accel_material(acc, int(m)) for m in np.unique(hits["material"][hit])}
    assert len(table) >= 2
    for i in np.where(hit)[0][::7]:
        m = table[int(hits["material"][i])]
        assert m["kind"] == wmat["kind"][i] and np.array(m["p"]).view(np.int64).tolist() == wmat["p"][i].view(np.int64).tolist(), (i, ML.NAMES[owners()[i]])
