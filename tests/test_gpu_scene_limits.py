"""Every entry point at the scene graph's limits (tests/limit_scenes.py): eight levels of nesting, 64 and 65 accels, and
per-lane stacks that need more than 64 KiB of dynamic LDS in the 256-lane kernels.

  1  the base calls -- render, capture_radiance, intersect, occluded, radiance -- against the CPU oracle (portable trig) per scene, in every
     organisation and traversal form the scene admits; the LDS fit each scene is meant to have is asserted;
  2  each derived family against its own contract on the same scenes, through the helpers of the family's own test file, in the accel's
     default form and in one forced form;
  3  the work counters of the unpruned reference walk equal the oracle's where no shadow ray is cast;
  4  the dynamic-LDS limit is monotone: a shallower accel built after a deeper one does not take the deeper one's launches away (a fresh
     process each, tests/scene_limits_child.py);
  5  a ninth level is refused, and the process renders eight levels correctly afterwards.
Nothing is tolerated: RGBA8 byte for byte, f64 bit for bit with any NaN equal to any NaN.  Before anything is compared, the ORACLE's answer is
asserted not to be vacuous: hits and misses, rays that end in the accels at the end of the longest chains, occluded and open segments.

Which side of the accel-record line (accel.cpp: accels <= 64) a scene is on in its 256-lane forms -- the image has no read-back, the device-free
test_limit_scenes_host.py restates the rule: chain8_shallow and accels64 carry the records in LDS (arec != nullptr in walk.h), accels65 reads
the DAccel table (65 accels), deep_a and deep_c read it too (their stacks leave no room: four workgroups a CU would not fit)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_rays as E
import lasgun_amd as la
import limit_scenes as L
import pyref
import test_gpu_directions as DI
import test_gpu_features as FE
import test_gpu_hit_layers as HL
import test_gpu_radiance_gather as GA
import test_gpu_range_scan as RS
import test_gpu_view_features as VF
import test_gpu_views as VW
import test_gpu_visibility as VI
from light_subsets import group_pairs, subset_scene
from oracle_lib import oracle
from query_witness import Witness
from test_gpu_level_door import Dark
from test_gpu_radiance_groups import lg
from test_gpu_radiance_query import bits, with_camera
from test_gpu_ray_query_edges import Expect, forms
from test_gpu_visibility import reset, set_form

pytestmark = pytest.mark.gpu
G = la.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = L.W, L.H
ERR = 2.220446049250313e-16 * 65536.0  # the shading offset (integrate.rs:40)
BASE_SCENES = ("chain8_shallow", "accels64", "accels65", "deep_a")
FAMILY_SCENES = ("chain8_shallow", "accels65", "deep_a")
DEEPEST = {"chain8_shallow": (7, 9), "accels64": (2, 4), "accels65": (2, 4), "deep_a": (7,), "deep_c": (7,)}  # the accels at the end of the longest chains
LDS_FITS = {"chain8_shallow": True, "accels64": True, "accels65": True, "deep_a": False, "deep_c": False}  # set_lds_scene's answer
FORCED = {"chain8_shallow": "reference", "accels64": "reference", "accels65": "reference", "deep_a": "prune"}  # the second form of a family case
SECOND = ("perspective", 70.0, (2.0, 1.5, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))  # another camera (test_gpu_radiance_query.with_camera)
DOORS = (3, 0)  # lg_accel_set_level_door: the default, and every level entered and left the long way (a lone mesh returns to its own group)
ORGS = [(org, streaming, prune) for org, streaming in (("megakernel", 0), ("levels", 2), ("queue", 3)) for prune in (False, True)]


def same_f64(got, want):
    """Bit for bit, any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))


def spread(total, n):
    return np.linspace(0, total - 1, n).round().astype(np.int64)


def pick(idx, n):
    return idx[spread(len(idx), min(n, len(idx)))]


def oracle_film(build, w, h):
    """(RGBA8, f64 radiance, counters) of the oracle's render in the trigonometry the device runs."""
    o = oracle()
    oacc = o.Accel(build(o))
    o.set_trig_mode(1)
    try:
        film = o.Film(w, h)
        o.stats_reset()
        o.capture_subset(0, 1, oacc, film)
        stats = o.stats_read()
        return film.pixels(), o.capture_radiance(oacc, w, h), stats
    finally:
        o.set_trig_mode(0)


class Case:
    """What the oracle says about one scene, and the inputs chosen on its answer: computed once, never changed."""

    def __init__(self, name):
        self.name, self.build = name, L.SCENES[name]
        o = oracle()
        self.oacc = o.Accel(self.build(o))
        pscene = self.build(pyref.Api)
        self.rgba, self.rad, self.stats = oracle_film(self.build, W, H)
        # not vacuous, the render: a picture, and rays that go all the way down the chain
        assert len(np.unique(self.rgba.reshape(-1, 4), axis=0)) > 50, name
        depth = 1 if name.startswith("accels") else 7
        assert self.stats["accel_entries"] >= depth * self.stats["primary_rays"] and self.stats["shadow_rays"] > 0, (name, self.stats)
        cam = np.array([[*od[0], *od[1]] for y in range(H) for x in range(W) for od in pscene.camera.sample(x, y, W, H)], dtype=np.float64)
        self.eye, self.light = cam[0, :3].copy(), np.array(pscene.lights[0][0])
        exp = Expect(self.oacc, cam, np.array(["camera"] * len(cam)))
        hit = exp.hits["kind"] != 0
        inner = hit & np.isin(exp.hits["instance"], DEEPEST[name])
        assert inner.sum() >= 8 and (hit & ~inner).sum() >= 15 and (~hit).sum() >= 15, (name, int(inner.sum()), int(hit.sum()))
        assert all((exp.hits["instance"][hit] == d).sum() >= 4 for d in DEEPEST[name]), (name, "every longest chain ends in a hit")
        chosen = np.concatenate([pick(np.flatnonzero(inner), 15), pick(np.flatnonzero(hit & ~inner), 15)])
        chosen = np.concatenate([chosen, pick(np.flatnonzero(~hit), 44 - len(chosen))])
        # shadow segments from the oracle's hit points towards the first light, half of them blocked
        h = exp.hits[hit]
        ng = np.where((np.einsum("ij,ij->i", h["ng"], -cam[hit, 3:]) < 0.0)[:, None], -h["ng"], h["ng"])
        p = h["p"] + ng * ERR
        seg = np.concatenate([p, self.light - p], axis=1)
        o.set_trig_mode(1)
        try:
            blocked = o.occluded(self.oacc, seg)
        finally:
            o.set_trig_mode(0)
        assert blocked.sum() >= 4 and (~blocked).sum() >= 4, (name, int(blocked.sum()), len(seg))
        shadow = np.concatenate([seg[pick(np.flatnonzero(blocked), 11)], seg[pick(np.flatnonzero(~blocked), 22)]])[:22]
        lo, hi, boxes = E.scene_geometry(Witness(pscene), pscene)
        edge, fam = E.edge_rays(lo, hi, boxes=boxes, seed=len(name), f1_tiles=1)
        f1, f2, f3 = (np.flatnonzero(fam == f) for f in ("F1", "F2", "F3"))
        poisoned = np.array([i for i in f2 if not (E.is_plain(edge[i]) and E.f64_plain_ray(edge[i]))])
        one_tile = np.concatenate([pick(f1, 24), pick(poisoned, 20), pick(f3, 20)])  # one tile of F1 - F3
        assert len(one_tile) == 64 and len(chosen) == 44 and len(shadow) == 22
        head = np.concatenate([cam[chosen], shadow])
        self.edge130 = np.ascontiguousarray(np.concatenate([head, edge[one_tile]]))
        self.plain130 = np.ascontiguousarray(np.concatenate([head, edge[pick(f1, 64)]]))  # finite rays with a direction, for the restatements
        self.edge65 = np.ascontiguousarray(self.edge130[np.random.default_rng(5).permutation(130)[:65]])
        fams = np.array(["camera"] * 44 + ["shadow"] * 22 + ["edge"] * 64)
        self.exp130, self.exp65 = Expect(self.oacc, self.edge130, fams), Expect(self.oacc, self.edge65, np.array(["mixed"] * 65))
        for e in (self.exp130, self.exp65):  # not vacuous, the batches
            k = e.hits["kind"] != 0
            assert k.any() and not k.all() and e.occ.any() and not e.occ.all() and all((e.hits["instance"][k] == d).any() for d in DEEPEST[name]), name
        # 65 points on the scene's surfaces with their normals, 9 points and 9 directions around them; 65 poses near the eye and 9 beams
        sel = pick(np.flatnonzero(hit), 65)
        hs = exp.hits[sel]
        nrm = np.where((np.einsum("ij,ij->i", hs["ng"], -cam[sel, 3:]) < 0.0)[:, None], -hs["ng"], hs["ng"])
        self.pts, self.nrm = np.ascontiguousarray(hs["p"] + nrm * ERR), np.ascontiguousarray(nrm)
        centre, reach = 0.5 * (p.min(axis=0) + p.max(axis=0)), 0.5 * float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
        self.to = np.ascontiguousarray(np.concatenate([VI.sphere_points(centre, reach, 8), self.light[None, :]]))
        self.dirs = np.ascontiguousarray(la.sphere_directions(9, reach))
        self.poses = np.ascontiguousarray(self.eye + 0.3 * VI.sphere_points(np.zeros(3), 1.0, 65))
        self.beams = np.ascontiguousarray(np.concatenate([cam[pick(np.flatnonzero(inner), 3), 3:], cam[pick(np.flatnonzero(hit & ~inner), 3), 3:],
                                                          cam[pick(np.flatnonzero(~hit), 3), 3:]]))
        assert self.pts.shape == (65, 3) and self.to.shape == (9, 3) and self.dirs.shape == (9, 3) and self.beams.shape == (9, 3)
        self.scan_rays = RS.explicit_rays(self.poses, None, self.beams)
        self.exp_scan = Expect(self.oacc, self.scan_rays, np.array(["scan"] * len(self.scan_rays)))
        self.exp_seg = Expect(self.oacc, VI.segments(self.pts, self.to), np.array(["segment"] * (65 * 9)))
        k = self.exp_scan.hits["kind"] != 0
        assert 0.1 <= k.mean() <= 0.9 and np.isin(self.exp_scan.hits["instance"][k], DEEPEST[name]).any(), (name, k.mean())
        assert 0.05 <= self.exp_seg.occ.mean() <= 0.95, (name, self.exp_seg.occ.mean())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


_accels = {}


def accel_of(name):
    """The scene's accel, shared by the tests of this file (every test leaves it in its default form)."""
    if name not in _accels:
        _accels[name] = G.Accel(L.SCENES[name](G))
    return _accels[name]


def query_forms(name, accel):
    """test_gpu_ray_query_edges.forms, with the LDS fit the scene is meant to have asserted."""
    fs = forms(accel)
    assert ("lds" in [f for f, _ in fs]) == LDS_FITS[name], (name, [f for f, _ in fs])
    return fs


# ---- 1: the base calls against the oracle -------------------------------------------------------------------------------------------------
def base_intersect_occluded(name, accel, c):
    for form, setup in query_forms(name, accel):
        setup()
        for door in DOORS:
            G.set_level_door(accel, door)
            for exp, rays in ((c.exp130, c.edge130), (c.exp65, c.edge65)):
                exp.check(accel, G.intersect(accel, rays), G.occluded(accel, rays), (name, form, door, len(rays)))


def base_radiance(name, accel, c):
    cam = G.camera_rays(accel, W, H)
    first = {}
    for form, setup in query_forms(name, accel):
        setup()
        assert same_f64(G.radiance(accel, cam).reshape(H, W, 3), c.rad), (name, form, "the camera's rays")
        # the oracle has no li() of a caller's ray: on the mixed batches every form gives the first form's bits (their hits are pinned by
        # the intersect case, the camera's radiance above, a second camera's in the views case)
        for rays in (c.edge130, c.edge65):
            got = G.radiance(accel, rays)
            assert same_f64(got, first.setdefault(len(rays), got)), (name, form, len(rays))


def base_render(name, accel, c, radiance):
    for lds in ((True, False) if LDS_FITS[name] else (False,)):
        assert G.set_lds_scene(accel, lds) == LDS_FITS[name], (name, "set_lds_scene says whether the scene fits")
        for (org, streaming, prune), door in [(o, d) for o in ORGS for d in DOORS]:
            G.set_streaming(accel, streaming)
            G.set_prune(accel, prune)
            G.set_level_door(accel, door)
            if radiance:
                rad = G.capture_radiance(accel, W, H)
                assert same_f64(rad, c.rad), (name, org, prune, lds, door, int((bits(rad) != bits(c.rad)).sum()))
            else:
                film = G.Film(W, H)
                G.capture_subset(0, 1, accel, film)
                assert np.array_equal(film.pixels(), c.rgba), (name, org, prune, lds, door, int((film.pixels() != c.rgba).sum()))
                assert G.last_organisation(accel).startswith({"megakernel": "megakernel", "levels": "wavefront", "queue": "queue"}[org]), (name, org)


BASE_CALLS = {"intersect": base_intersect_occluded, "radiance": base_radiance, "render": lambda n, a, c: base_render(n, a, c, False),
              "capture_radiance": lambda n, a, c: base_render(n, a, c, True)}


def restore(accel):
    reset(accel)
    G.set_streaming(accel, 1)
    G.set_level_door(accel, 3)


@pytest.mark.parametrize("call", list(BASE_CALLS))
@pytest.mark.parametrize("name", BASE_SCENES)
def test_base_calls_match_the_oracle_in_every_form(name, call):
    c, accel = case(name), accel_of(name)
    info = G.accel_info(accel)
    assert info["accels"] == {"chain8_shallow": 10, "accels64": 64, "accels65": 65, "deep_a": 8}[name]
    assert (L.lds_bytes_256(info["max_stack"]) > 64 * 1024) == (name == "deep_a"), info
    try:
        BASE_CALLS[call](name, accel, c)
    finally:
        restore(accel)


# ---- 2: the derived families against their own contracts ------------------------------------------------------------------------------------
def fam_visibility(name, accel, c):
    segs = VI.segments(c.pts, c.to)
    occ = G.occluded(accel, segs)
    c.exp_seg.check(accel, G.intersect(accel, segs), occ, (name, "segments"))
    bits_, blocked = G.visibility(accel, c.pts, c.to, counts=True)
    assert np.array_equal(bits_, VI.pack(occ, 65, 9)) and np.array_equal(blocked, occ.reshape(65, 9).sum(axis=1)), name


def fam_directions(name, accel, c):
    above, opened = DI.restate(lambda r: G.occluded(accel, r), c.pts, c.nrm, c.dirs)
    o_above, o_opened = DI.restate(lambda r: oracle_occluded(c, r), c.pts, c.nrm, c.dirs)
    assert np.array_equal(above, o_above) and np.array_equal(opened, o_opened) and opened.any() and (above & ~opened).any(), name
    DI.compare((name,), G.open_directions(accel, c.pts, c.dirs, c.nrm, counts=True), above, opened)


def oracle_occluded(c, rays):
    o = oracle()
    o.set_trig_mode(1)
    try:
        return o.occluded(c.oacc, rays)
    finally:
        o.set_trig_mode(0)


def fam_range_scan(name, accel, c):
    hits = G.intersect(accel, c.scan_rays)
    c.exp_scan.check(accel, hits, G.occluded(accel, c.scan_rays), (name, "scan rays"))
    RS.compare((name,), G.range_scan(accel, c.poses, c.beams, None, RS.PLANES, 0), RS.restate(hits, 65, 9))


def fam_hit_layers(name, accel, c):
    want = HL.chain(lambda r: G.intersect(accel, r), c.plain130, 3)
    assert (want["count"] == 0).any() and (want["count"] >= 2).any(), (name, np.bincount(want["count"]))
    got = G.hit_layers(accel, c.plain130, 3, HL.PLANES)
    HL.compare((name, 3), got, want)
    assert got["hits"][0].tobytes() == G.intersect(accel, c.plain130).tobytes(), "layer 0 is lg_intersect's array itself"


def fam_features(name, accel, c):
    hits = G.intersect(accel, G.camera_rays(accel, W, H))
    table = FE.random_table(accel)
    got = G.capture_features(accel, W, H, material_rgb=table, into=FE.prefill(W, H))
    FE.compare(got, FE.expected(hits, 1, FE.table_rgb(hits, table)), (0, 0, W, H), W, (name,))


def views_of(accel):
    return [G.accel_view(accel), VW.view_of(SECOND)]


def fam_view_features(name, accel, c):
    views, (w, h) = views_of(accel), (W // 2, H // 2)
    hits = VF.view_hits(accel, views, w, h)
    assert (hits["kind"] != 0).any() and (hits["kind"] == 0).any(), name
    table = VF.random_table(accel)
    VF.compare(G.capture_view_features(accel, views, w, h, material_rgb=table), VF.restate(hits, 1, FE.table_rgb(hits, table)), (name,))


def fam_gather(name, accel, c):
    L_ = G.radiance(accel, c.scan_rays).reshape(65, 9, 3)  # (poses x beams: the oracle's hits on these rays are mixed, Case.exp_scan)
    GA.check_gather((name,), accel, c.poses, c.beams, None, GA.WEIGHTS[:9], L_, lanes_set=(0,))


def fam_ray_film(name, accel, c):
    rgba, rgb = G.capture_rays(accel, G.camera_rays(accel, W, H), W, H, rgb=True)
    assert np.array_equal(rgba, c.rgba) and same_f64(rgb, c.rad), (name, int((rgba != c.rgba).sum()))


@functools.lru_cache(maxsize=None)
def second_film(name):
    return oracle_film(lambda api: with_camera(L.SCENES[name](api), SECOND), W, H)[:2]


def fam_views(name, accel, c):
    views = views_of(accel)
    rgba, rgb = G.capture_views(accel, views, W, H, rgb=True)
    for k, (want_rgba, want_rad) in enumerate(((c.rgba, c.rad), second_film(name))):
        assert np.array_equal(rgba[k], want_rgba) and same_f64(rgb[k], want_rad), (name, k, int((rgba[k] != want_rgba).sum()))
    by_rgba, by_rgb = VW.by_rays(accel, views, W, H)
    assert np.array_equal(rgba, by_rgba) and same_f64(rgb, by_rgb), name


def fam_light_groups(name, accel, c):
    pairs = group_pairs(G.light_count(accel))
    planes = G.radiance_groups(accel, c.plain130, lg(pairs))
    for g, (m, a) in enumerate(pairs):
        want = G.radiance(G.Accel(subset_scene(G, L.SCENES[name], m, a)), c.plain130)
        assert same_f64(planes[g], want), (name, g, m, a)
    assert not same_f64(planes[0], planes[pairs.index(((1 << G.light_count(accel)) - 1, True))]), (name, "the lights do not show")


FAMILIES = {"visibility": fam_visibility, "directions": fam_directions, "range_scan": fam_range_scan, "hit_layers": fam_hit_layers,
            "features": fam_features, "view_features": fam_view_features, "gather": fam_gather, "ray_film": fam_ray_film, "views": fam_views,
            "light_groups": fam_light_groups}
FAMILY_CASES = [(n, f) for n in FAMILY_SCENES for f in FAMILIES] + [("accels64", "visibility"), ("accels64", "range_scan")]


@pytest.mark.parametrize("name,family", FAMILY_CASES, ids=["%s-%s" % nf for nf in FAMILY_CASES])
def test_families_keep_their_contracts(name, family):
    c, accel = case(name), accel_of(name)
    try:
        for form in ("default", FORCED[name]):
            if form != "default":
                set_form(accel, form)
            FAMILIES[family](name, accel, c)
    finally:
        restore(accel)


# ---- 3: the work counters of the reference walk ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain8_shallow", "accels65"])
def test_counters_equal_the_oracles(name):
    """Without lights every traversal is a closest-hit walk, whose work the reference's counters state exactly (test_gpu_level_door.py)."""
    o = oracle()
    oacc = o.Accel(L.SCENES[name](Dark(o)))
    o.stats_reset()
    o.capture_subset(0, 1, oacc, o.Film(W, H))
    want = o.stats_read()
    assert want["shadow_rays"] == 0 and want["accel_entries"] >= (7 if name == "chain8_shallow" else 1) * want["primary_rays"], want
    assert want["spheres_tested"] > 0 and want["cuboids_tested"] > 0 and want["triangles_tested"] > 0 and want["secondary_rays"] > 0, want
    acc = G.Accel(L.SCENES[name](Dark(G)))
    G.set_prune(acc, False)
    for lds in (True, False):
        assert G.set_lds_scene(acc, lds)
        got = G.capture_stats(acc, W, H)
        assert got == want, (name, lds, got, want)


# ---- 4: the dynamic-LDS limit is monotone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("middle", ["deep_c", "readme"])
def test_a_shallower_accel_does_not_lower_the_lds_limit(middle):
    """hipFuncSetAttribute is process-wide: deep_a, then `middle` (deep_c: above 64 KiB and below deep_a; readme_scene: the control under
    64 KiB), then deep_a again -- every launch succeeds and matches the oracle."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scene_limits_child.py"), middle], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("done"), (middle, r.returncode, r.stdout[-2000:], r.stderr[-3000:])


# ---- 5: the refusal -------------------------------------------------------------------------------------------------------------------------
def test_a_ninth_level_is_refused_and_eight_render_afterwards():
    with pytest.raises(la.LasgunError, match="nested deeper than 8 levels"):
        G.Accel(L.chain9(G))
    c = case("chain8_shallow")
    acc = G.Accel(L.chain8_shallow(G))
    film = G.Film(W, H)
    G.capture_subset(0, 1, acc, film)
    assert np.array_equal(film.pixels(), c.rgba) and same_f64(G.capture_radiance(acc, W, H), c.rad)
