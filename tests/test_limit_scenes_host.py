"""The scenes of tests/limit_scenes.py are what they claim, without a device: the accel counts on either side of the line at which the accel
records leave LDS, eight levels and the refusal of a ninth, stacks past 64 KiB of dynamic LDS in the 256-lane forms -- and the constants the
committed search found are what the search finds.  (That the host builder's dump of each equals the oracle's bit for bit is
tests/test_host.py, BUILD_CASES; the oracle against the witness on them is tests/test_oracle_ray_query.py.)"""
import numpy as np
import pytest

import lasgun_amd as la
import limit_scenes as L
from oracle_lib import oracle

G = la.api
LDS_MAX = 160 * 1024  # one CU's LDS (accel.cpp)
ACCEL_RECORD = 16 * 16  # LDS_ACCEL_UNITS x 16 bytes (dscene.h)


def info(scene):
    return G.host_build_dump(scene)[2]


def accel_records_in_lds(i):
    """accel.cpp: the accel records ride behind the stacks of the 256-lane kernels for at most 64 accels, where four workgroups still fit a CU."""
    return i["accels"] <= 64 and (L.lds_bytes_256(i["max_stack"]) + i["accels"] * ACCEL_RECORD) * 4 <= LDS_MAX


def levels_of(scene):
    """The deepest nesting of a pyref scene: accels on the path root .. self, a mesh counted as the accel it becomes."""
    def depth(agg):
        return 1 + max([depth(n[1]) if n[0] == "group" else 1 for n in agg.contents if n[0] in ("group", "mesh")] + [0])
    return depth(scene.root)


@pytest.mark.parametrize("name,accels", [("accels64", 64), ("accels65", 65), ("chain8_shallow", 10), ("deep_a", 8), ("deep_c", 8)])
def test_accel_counts_and_levels(name, accels):
    import pyref
    i = info(L.SCENES[name](G))
    assert i["accels"] == accels, i
    want_levels = 3 if name.startswith("accels") else L.MAX_LEVELS
    assert levels_of(L.SCENES[name](pyref.Api)) == want_levels
    # the side of the accel-record line each scene is on
    assert accel_records_in_lds(i) == (name in ("accels64", "chain8_shallow")), (name, i)
    if name.startswith("accels"):
        assert i["triangles"] > 0 and i["spheres"] > 20 and i["cuboids"] > 10 and i["has_specular"] == 1


def test_the_two_accel_scenes_differ_by_one_group():
    a, b = info(L.accels64(G)), info(L.accels65(G))
    assert b["accels"] == a["accels"] + 1 and a["max_stack"] == b["max_stack"] and b["spheres"] + b["cuboids"] == a["spheres"] + a["cuboids"] + 1


def test_chain8_shallow_fits_the_lds_resident_form():
    scene = L.chain8_shallow(G)
    i = info(scene)
    for pairs in (False, True):
        img = G.scene_lds_image(scene, pairs)
        assert img is not None, "the scene tables fit beside 1024 stacks"
        assert (i["max_stack"] + 2) * 1024 * 4 + img[1]["units"] * 16 <= LDS_MAX, (i, img[1])
        assert img[1]["accels"] == 10
    assert L.lds_bytes_256(i["max_stack"]) <= 64 * 1024


def test_deep_scenes_pass_64_kib_and_deep_a_is_deeper():
    a, c = info(L.deep_a(G)), info(L.deep_c(G))
    assert a["max_stack"] == L.DEEP_A_MAX_STACK >= 65, a
    assert c["max_stack"] == L.DEEP_C_MAX_STACK and 63 <= c["max_stack"] < a["max_stack"], c
    assert L.lds_bytes_256(a["max_stack"]) > L.lds_bytes_256(c["max_stack"]) > 64 * 1024
    assert L.lds_bytes_256(a["max_stack"]) <= LDS_MAX  # (the product builds it: the refusal "BVH too deep" starts at 160 entries)
    for scene in (L.deep_a(G), L.deep_c(G)):
        assert G.scene_lds_image(scene, False) is None, "no LDS-resident form: 1024 stacks of this depth alone pass a CU's LDS"


@pytest.mark.parametrize("which", ["a", "c"])
def test_the_committed_seeds_are_what_the_search_finds(which):
    base, seeds, deepest = {"a": (L.DEEP_A_BASE, L.DEEP_A_SEEDS, L.DEEP_A_MAX_STACK), "c": (L.DEEP_C_BASE, L.DEEP_C_SEEDS, L.DEEP_C_MAX_STACK)}[which]
    assert L.deep_search(G, base=base) == (seeds, deepest)
    assert len(seeds) == L.MAX_LEVELS


def same_dump(builder):
    f, i, _ = G.host_build_dump(builder(G))
    of, oi = oracle().Accel(builder(oracle())).dump()
    return np.array_equal(i, oi) and np.array_equal(f.view(np.uint64), of.view(np.uint64))


def test_a_ninth_level_is_refused_and_the_next_build_is_whole():
    with pytest.raises(la.LasgunError, match="nested deeper than 8 levels"):
        G.host_build_dump(L.chain9(G))
    assert same_dump(L.chain8_shallow)  # the refused build left nothing behind in the builder's tables
    with pytest.raises(la.LasgunError, match="nested deeper than 8 levels"):
        G.host_build_dump(L.deep_scene(G, L.DEEP_A_SEEDS + (8000,)))
    assert info(L.deep_a(G))["max_stack"] == L.DEEP_A_MAX_STACK


def test_the_oracle_has_no_such_limit():
    """The reference nests as deep as the scene does; eight levels is the product's own limit.  Nine levels render, and
    rays get to the ninth: the mesh alone in the innermost group is hit."""
    o = oracle()
    acc = o.Accel(L.chain9(o))
    o.stats_reset()
    film = o.Film(L.W, L.H)
    o.capture_subset(0, 1, acc, film)
    stats = o.stats_read()
    assert stats["accel_entries"] >= 8 * stats["primary_rays"] and stats["triangles_tested"] > 0, stats
    assert len(np.unique(film.pixels().reshape(-1, 4), axis=0)) > 50, "a picture"
    rays = np.array([[*od[0], *od[1]] for y in range(12) for x in range(16) for od in L.chain9(__import__("pyref").Api).camera.sample(x, y, 16, 12)])
    hits, _ = o.intersect(acc, rays)
    assert ((hits["kind"] == 3) & (hits["instance"] == 8)).any() and (hits["instance"] == 10).any() and (hits["kind"] == 0).any()
