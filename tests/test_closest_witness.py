"""The witness of the closest-point tests, with tests/pyref.py and the brute force (tests/closest_ref.py) alone -- no library call, no GPU:
the scenes and points that tests/test_gpu_closest_points.py holds the kernel to (tests/closest_cases.py) contain every class the contract
distinguishes, so that a kernel that agrees with the brute force on them has been asked every question: winners of each kind, each triangle
region and each box face, points inside a sphere, at its centre, inside a box and on a surface (distance 0), exact ties between two
primitives decided by the key (at least one pair per mesh scene), a radius that excludes some winners and not all, misses, non-finite
points.  And the gate's verdicts, restated from the chains: a sphere under scale(1.2, 1.2, 1.2) plus rotations is admitted, under
scale(1.2, 0.8, 1.0) refused by instance; meshes and boxes are admitted under non-uniform scale."""
import numpy as np
import pytest

import closest_cases as C
import closest_ref as R
import pyref

INF = float("inf")


@pytest.mark.parametrize("name", list(C.SCENES))
def test_the_points_hold_every_class(name):
    _, b, pts, want = C.case(name)
    assert pts.shape == (C.N_POINTS, 3)
    kind, detail, d = want["id"][:, 0], want["detail"], want["distance"]
    present = {1: len(b.cw) > 0, 2: len(b.box) > 0, 3: len(b.tri) > 0}
    for k in (1, 2, 3):
        assert ((kind == k).sum() >= 50) == present[k], (name, k, int((kind == k).sum()))
    if present[3]:
        regions = np.bincount(detail[kind == 3], minlength=8)
        assert (regions[1:] >= 3).all(), (name, "each triangle region", regions)
    if present[2]:
        faces = np.bincount(detail[kind == 2] // 2, minlength=6)
        assert (faces >= 3).all(), (name, "each box face", faces)
    finite = np.isfinite(pts).all(axis=1)
    assert (~finite).sum() == 8 and (kind[~finite] == 0).all() and (d[~finite] == INF).all() and not want["point"][~finite].any(), (name, "non-finite points get the miss record")
    assert (kind[finite] != 0).all(), (name, "at radius +INF every finite point has a winner")
    assert (d == 0.0).sum() >= 50, (name, "points on a surface")
    assert (np.abs(pts[finite]).max(axis=1) > 1e5).sum() >= 60, (name, "points at 1e6")
    if present[1]:
        r = np.sqrt(R.dot(b.pw - b.cw, b.pw - b.cw))
        dist = np.sqrt(((pts[finite][:, None, :] - b.cw[None]) ** 2).sum(axis=2))
        assert (dist == 0.0).any() and ((dist > 0.0) & (dist < 0.9 * r[None])).any(), (name, "a sphere's centre, and points inside one")
    if present[2]:
        lo, hi = b.box.min(axis=1), b.box.max(axis=1)
        centre = (b.box[:, 0] + b.box[:, 7]) / 2.0
        assert any((np.abs(pts[finite] - c).max(axis=1) < 1e-12).any() for c in centre), (name, "a point inside a box (its centre)")
        assert (lo <= hi).all()
    # a radius that excludes some winners and not all; radius 0 and 2^-20 keep the surface points alone
    for radius in C.radii(want)[1:]:
        got = b.closest(pts, radius)
        hits = (got["id"][:, 0] != 0).sum()
        assert 0 < hits < finite.sum(), (name, radius, int(hits))
        within = d <= radius
        assert np.array_equal(got["id"][:, 0] != 0, within & finite), (name, radius, "exactly the winners within the radius stay")


@pytest.mark.parametrize("name", C.MESH_SCENES)
def test_exact_ties_between_two_primitives_are_decided_by_the_key(name):
    _, b, pts, want = C.case(name)
    finite = np.isfinite(pts).all(axis=1)
    q = pts[finite]
    ties, decided = 0, 0
    for lo in range(0, len(q), 512):
        _, d2, _ = b.candidates(q[lo:lo + 512])
        low = np.nanmin(np.where(np.isnan(d2), INF, d2), axis=1)
        tie = d2 == low[:, None]
        multi = tie.sum(axis=1) >= 2
        ties += int(multi.sum())
        w = want["winner"][finite][lo:lo + 512]
        for i in np.nonzero(multi)[0]:
            keys = b.key[tie[i]]
            assert b.key[w[i]] == keys.min(), (name, lo + i)
            decided += 1
    print("closest points witness, %s: %d points whose smallest d2 is shared by two or more primitives" % (name, ties))
    assert ties >= 10 and decided >= 10, (name, ties, decided)


def test_the_gates_verdicts():
    def scene(build):
        s = pyref.Api.Scene.new()
        s.set_perspective_camera(50.0)
        build(s, pyref.Api)
        return R.Brute(s).cat

    M = pyref.Api.Material.matte([0.5, 0.5, 0.5], 0.0)

    def uniform(s, api):
        g = api.Aggregate.new()
        g.scale(1.2, 1.2, 1.2); g.rotate_y(30.0); g.rotate(40.0, [0.6, 0.0, 0.8]); g.translate([0.5, 1.5, -1.0])
        g.add_sphere([0.1, 0.2, 0.3], 0.4, M)
        s.root.add_group(g)

    def squashed(s, api):
        s.root.add_sphere([0.0, 0.0, 0.0], 1.0, M)
        ok = api.Aggregate.new()
        ok.rotate_x(10.0)
        ok.add_sphere([0.0, 2.0, 0.0], 0.5, M)
        s.root.add_group(ok)
        g = api.Aggregate.new()
        g.scale(1.2, 0.8, 1.0)
        g.add_sphere([0.1, 0.2, 0.3], 0.4, M)
        s.root.add_group(g)

    def squashed_solids(s, api):
        mesh = s.parse_obj(C.TETRA_OBJ)
        g = api.Aggregate.new()
        g.scale(1.2, 0.8, 1.0); g.rotate_z(25.0)
        g.add_obj_of(mesh, M)
        g.add_cube([0.0, 0.0, 0.0], 1.0, M)
        s.root.add_group(g)
        s.root.add_sphere([3.0, 0.0, 0.0], 0.5, M)

    assert C.gate(scene(uniform)) == -1
    assert C.gate(scene(squashed)) == 2, "refused by instance: the third accel in scene-graph order"
    assert C.gate(scene(squashed_solids)) == -1
    assert C.gate(C.case("own")[1].cat) == -1 and C.gate(C.case("chain8_shallow")[1].cat) == 1
