"""The hit-attribute tests are not vacuous, shown on the CPU: the reference evaluator (tests/attr_ref.py) over the CPU oracle's closest hits
of the test rays (tests/attr_cases.py).  The classes the contract distinguishes all occur -- triangles with real, default and degenerate
texture coordinates, smooth and flat normals, spheres hit from outside and from inside, all six faces of a box, a scaled, a rotated and a
swap_backface instance --, the films alone give the ones a camera outside the geometry can see, and the reference obeys the contract's own
closed forms (the barycentrics sum to one, they blend the vertices to the hit point, the local point goes to the world point) to within
rounding: the worst errors printed here are what tests/test_gpu_hit_attributes.py holds the device to, plus 4 ulps."""
import numpy as np
import pytest

import pyref

import attr_cases as C
import attr_ref as R
from oracle_lib import oracle


@pytest.fixture(scope="module")
def films():
    O = oracle()
    out = {}
    for name, builder, (w, h) in C.SCENES:
        pscene = builder(pyref.Api)
        accel = O.Accel.from_scene(builder(O))
        cat = R.Catalog(pscene)
        rays = C.film_rays(pscene, w, h)
        hits, _ = O.intersect(accel, rays)
        layers = [(rays, hits)]
        for _ in range(2):  # the two segments behind: lg_hit_layers' layers 1 and 2
            r = C.continuation(*layers[-1])
            layers.append((r, O.intersect(accel, r)[0]))
        out[name] = (cat, layers)
    return out


def test_the_films_hit_every_kind_and_the_classes_a_camera_can_see(films):
    seen = set()
    for name in C.FILMS:
        cat, layers = films[name]
        rays, hits = layers[0]
        assert len(rays) == C.W * C.H and (hits["kind"] == 0).any() and (hits["kind"] != 0).sum() > len(rays) // 3, name
        seen |= C.classes(cat, rays, hits)
    kinds = set(int(k) for name in C.FILMS for k in np.unique(films[name][1][0][1]["kind"]))
    assert kinds == {0, 1, 2, 3}
    assert {"uv_real", "uv_default", "smooth", "flat", "sphere_outside", "scaled", "rotated", "swap_backface"} <= seen, seen
    assert sum(1 for c in seen if c.startswith("box_face_")) >= 3, seen


def test_with_the_segments_behind_and_the_extra_scene_every_class_occurs(films):
    seen = set()
    for name, _, _ in C.SCENES:
        cat, layers = films[name]
        for rays, hits in layers:
            seen |= C.classes(cat, rays, hits)
    assert seen >= C.WANTED, sorted(C.WANTED - seen)
    front, behind = set(), set()
    for name in C.FILMS:  # the films' own continuation rays leave spheres from inside and boxes by their far faces
        cat, layers = films[name]
        front |= C.classes(cat, *layers[0])
        for rays, hits in layers[1:]:
            behind |= C.classes(cat, rays, hits)
    assert "sphere_inside" in behind and "sphere_inside" not in front, (sorted(front), sorted(behind))
    assert sum(1 for c in front | behind if c.startswith("box_face_")) == 6 and not behind <= front, (sorted(front), sorted(behind))
    extra = C.classes(films["extra"][0], *films["extra"][1][0])
    assert {"uv_degenerate", "uv_real", "uv_default", "sphere_inside", "swap_backface", "scaled", "rotated"} <= extra, sorted(extra)


def test_the_reference_obeys_the_closed_forms_and_flags_every_record(films):
    for name, _, _ in C.SCENES:
        cat, layers = films[name]
        rays, hits = layers[0]
        pl = R.planes(cat, rays, hits)
        hit = hits["kind"] != 0
        assert np.array_equal(pl["flags"], np.where(hit, R.HIT, 0)), name  # the oracle's own records are never NO_HIT or BAD_RECORD
        for key, _ in R.PLANES:
            assert not pl[key][~hit].any() and not np.signbit(pl[key][~hit]).any(), (name, key)
        tri = hits["kind"] == 3
        assert not pl["bary"][hit & ~tri].any() and (pl["bary"][tri] >= 0.0).all(), name
        worst = R.closed_forms(cat, hits, pl)
        print("witness closed forms, %s: %r" % (name, worst))
        scale = max(1.0, float(np.abs(hits["p"][hit]).max()))
        assert worst["bary_sum"] <= 8 * 2.0 ** -53 and worst["vertex_blend"] <= 64 * 2.0 ** -53 * scale and worst["local_to_world"] <= 64 * 2.0 ** -53 * scale, (name, worst)
        uv = pl["uv"][hit & (hits["kind"] != 3)]
        assert ((uv >= 0.0) & (uv <= 1.0) | np.isnan(uv)).all(), name  # a sphere's and a box face's parameter lies in the unit square


def test_a_wrong_ray_and_a_bad_record_are_told_apart(films):
    cat, layers = films["kitchen_sink"]
    rays, hits = layers[0]
    i = int(np.nonzero(hits["kind"] == 1)[0][0])
    k = int(np.nonzero(hits["kind"] == 3)[0][0])
    away = np.concatenate([rays[i, :3], -rays[i, 3:]])
    assert R.attributes(cat, away, 1, int(hits[i]["prim"]), int(hits[i]["instance"]))[0] in (R.NO_HIT, R.HIT)
    far = np.array([50.0, 50.0, 50.0, 0.0, 1.0, 0.0])
    for j in (i, k, int(np.nonzero(hits["kind"] == 2)[0][0])):
        assert R.attributes(cat, far, int(hits[j]["kind"]), int(hits[j]["prim"]), int(hits[j]["instance"]))[0] == R.NO_HIT
    assert R.attributes(cat, rays[i], 7, 0, 0)[0] == R.BAD_RECORD
    assert R.attributes(cat, rays[i], 1, len(cat.spheres), 0)[0] == R.BAD_RECORD
    assert R.attributes(cat, rays[i], 1, 0, len(cat.accels))[0] == R.BAD_RECORD
    assert R.attributes(cat, rays[k], 3, len(cat.accels[int(hits[k]["instance"])]["mesh"][0].polys), int(hits[k]["instance"]))[0] == R.BAD_RECORD
    wrong = next(a for a in range(len(cat.accels)) if a != cat.spheres[0][2])
    assert R.attributes(cat, rays[i], 1, 0, wrong)[0] == R.BAD_RECORD
    assert R.attributes(cat, rays[i], 0, 5, 5) == (0, None)
