"""The segment-proximity tests are not vacuous, shown on the brute force alone (tests/segment_ref.py over the segments of
tests/segment_cases.py, no device): every class the contract distinguishes is present with at least 20 segments a scene where the scene can
hold it -- each of the six triangle sub-candidates as the winner, the sphere's three cases, a segment wholly inside a box, a segment
parallel to an edge, the degenerate segment, an exact key tie, endpoints at 1e6, non-finite segments, segments at least as long as the
bounds' diagonal --, the radii of the GPU test exclude some segments and not all, and at least 200 segments a mesh scene have a ray form
whose first hit (tests/pyref.py through tests/query_witness.py) lies at t in [0.01, 0.99] with barycentrics of at least 0.01: the segments
that tests/test_gpu_closest_segments.py requires to answer distance == +0.0."""
import numpy as np
import pytest

import attr_ref
import closest_cases as C
import query_witness
import segment_cases as SC
import segment_ref as SR

FEW = 20


def winners(name):
    _, b, segs, want, diag = SC.case(name)
    w = want["winner"]
    kind = np.where(w >= 0, b.ids[np.maximum(w, 0), 1], 0).astype(np.int64)
    return b, segs, want, diag, kind


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_every_class_is_present(name):
    b, segs, want, diag, kind = winners(name)
    det = want["detail"].astype(np.int64)
    assert len(segs) == 4097
    sub = [int(((kind == 3) & (det == k)).sum()) for k in range(1, 7)]
    print("%s: a triangle wins by sub-candidate 1 .. 6: %s" % (name, sub))
    assert min(sub) >= FEW, sub
    if len(b.cw):
        cases = [int(((kind == 1) & (det == k)).sum()) for k in (SR.SPHERE_OUTSIDE, SR.SPHERE_INSIDE, SR.SPHERE_CROSSING)]
        print("%s: a sphere wins outside, inside, crossing: %s" % (name, cases))
        assert min(cases) >= FEW, cases
    if len(b.box):
        # wholly inside: both endpoints have coordinates in [0, 1] in the box's own frame (corner 0, edges to corners 1, 2, 4)
        inside = np.zeros(len(segs), dtype=bool)
        for w in b.box:
            basis = np.stack([w[1] - w[0], w[2] - w[0], w[4] - w[0]], axis=1)
            with np.errstate(invalid="ignore"):
                c0, c1 = np.linalg.solve(basis, (segs[:, :3] - w[0]).T).T, np.linalg.solve(basis, (segs[:, 3:] - w[0]).T).T
                inside |= ((c0 > 1e-9) & (c0 < 1 - 1e-9) & (c1 > 1e-9) & (c1 < 1 - 1e-9)).all(axis=1)
        inside &= (segs[:, :3] != segs[:, 3:]).any(axis=1)
        print("%s: %d segments wholly inside a box, %d of them answered by that box at a distance above zero" % (name, inside.sum(), (inside & (kind == 2) & (want["distance"] > 0)).sum()))
        assert (inside & (kind == 2) & (want["distance"] > 0.0)).sum() >= FEW, "a segment wholly inside a box gets the distance to its surface"
    # parallel to an edge of some triangle, to 1e-12 of the two lengths
    u = segs[:, 3:] - segs[:, :3]
    par = np.zeros(len(segs), dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        e = b.tri[:, j] - b.tri[:, i]
        for lo in range(0, len(e), 128):
            with np.errstate(invalid="ignore"):
                cr = np.cross(u[:, None, :], e[None, lo:lo + 128, :])
                par |= ((cr * cr).sum(axis=2) <= 1e-24 * (u * u).sum(axis=1)[:, None] * (e[lo:lo + 128] ** 2).sum(axis=1)[None]).any(axis=1)
    length = SC.lengths(segs)
    par &= length > 0.0
    deg = (segs[:, :3] == segs[:, 3:]).all(axis=1)
    far = np.isfinite(segs).all(axis=1) & (np.abs(segs).max(axis=1) >= 9e5)
    bad = ~np.isfinite(segs).all(axis=1)
    counts = {"parallel to an edge": int(par.sum()), "degenerate": int(deg.sum()), "an exact key tie": int(want["tie"].sum()), "endpoints at 1e6": int(far.sum()),
              "as long as the bounds' diagonal": int((length >= diag).sum())}
    print("%s: %s, non-finite %d" % (name, counts, bad.sum()))
    assert all(v >= FEW for v in counts.values()), counts
    assert bad.sum() >= 8 and (want["touch"][bad] == 0).all() and np.isinf(want["distance"][bad]).all(), "a non-finite segment is a miss"
    assert (want["touch"][far] == 1).all(), "a far segment still has a nearest primitive at radius +INF"
    assert (want["detail"][deg & (kind == 3)] == 0).all() and (want["param"][deg] == 0.0).all(), "the degenerate segment answers in the point form"
    ok = want["touch"] == 1
    assert (want["param"][ok] >= 0.0).all() and (want["param"][ok] <= 1.0).all() and not np.signbit(want["param"]).any()


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_the_radii_exclude_some_segments_and_not_all(name):
    _, _, segs, want, _ = SC.case(name)
    refs = SC.references(name)
    assert refs[0]["touch"].tobytes() == want["touch"].tobytes() and refs[0]["distance"].tobytes() == want["distance"].tobytes()
    for index, radius in enumerate(C.radii(want)):
        hits = int(refs[index]["touch"].sum())
        print("%s, radius %r: %d of %d segments touch" % (name, radius, hits, len(segs)))
        assert 0 < hits < len(segs) or index == 0
        assert ((refs[index]["touch"] == 1) == np.isfinite(refs[index]["distance"])).all()
    radii = SC.mixed_radii(name, 30)
    assert np.isnan(radii).sum() >= 10 and (radii == -1.0).sum() >= 10 and (np.signbit(radii) & (radii == 0.0)).sum() >= 10 and np.isinf(radii).sum() >= 10
    mixed = refs[4]
    dead = np.isnan(radii) | (radii < 0.0)
    assert (mixed["touch"][dead] == 0).all() and 0 < mixed["touch"].sum() < len(segs)
    zero = (radii == 0.0) & np.signbit(radii)
    assert mixed["touch"][zero].tobytes() == refs[1]["touch"][zero].tobytes(), "-0.0 is zero"


def pierced(name, limit=400):
    """Indices of segments whose ray form o = p0, d = p1 - p0 first hits a triangle at t in [0.01, 0.99] with barycentrics >= 0.01
    (pyref's walk and tests/attr_ref.py's barycentrics), among the first `limit` candidates the brute force answers with a triangle at
    distance zero."""
    pscene, b, segs, want, _ = SC.case(name)
    w = want["winner"]
    kind = np.where(w >= 0, b.ids[np.maximum(w, 0), 1], 0)
    cand = np.nonzero((want["distance"] == 0.0) & (kind == 3))[0][:limit]
    wit, cat = query_witness.Witness(pscene), attr_ref.Catalog(pscene)
    keep = []
    for i in cand:
        o, d = segs[i, :3], segs[i, 3:] - segs[i, :3]
        hit = wit.closest(o, d)
        if hit is None or hit["id"][0] != 3 or not 0.01 <= hit["t"] <= 0.99:
            continue
        flags, at = attr_ref.attributes(cat, np.concatenate([o, d]), *hit["id"])
        if flags == attr_ref.HIT and min(at["bary"]) >= 0.01:
            keep.append(int(i))
    return np.array(keep, dtype=np.int64)


@pytest.mark.parametrize("name", list(C.MESH_SCENES))
def test_at_least_200_segments_a_mesh_scene_pierce_a_triangle_well_inside(name):
    _, _, _, want, _ = SC.case(name)
    keep = pierced(name)
    print("%s: %d segments pass the ray-form filter" % (name, len(keep)))
    assert len(keep) >= 200
    assert (want["distance"][keep] == 0.0).all() and (want["touch"][keep] == 1).all() and not np.signbit(want["distance"][keep]).any()
