"""The points of the proximity-query tests (tests/closest_cases.py: 4097 a scene, its four radii) hold every class of answer that
tests/test_gpu_nearest.py has to tell apart, by the brute force alone (tests/nearest_ref.py) and without a device: points with no
candidate within the radius, with fewer than k, with exactly k and with more than k; exact ties ACROSS the cut (the last slot and the first
candidate left out have equal d2, so the key alone decides which of them is in); lists that span more than one instance and more than
one kind; and, at radius 0 and 2^-20, rows with fewer than k admissible candidates.  The counts are printed; each class has to hold at
least 10 points per scene where the scene can hold it (torus has two instances and no box)."""
import numpy as np
import pytest

import closest_cases as C
import nearest_ref as N

K = N.MAX_K
ENOUGH = 10


def ties_across_the_cut(want8, k):
    """Points whose slot k - 1 and first candidate left out have equal d2 (k <= MAX_K, over the answer made at MAX_K)."""
    after = want8["next_d2"] if k == K else want8["d2"][k]
    return (want8["count"] > k) & (want8["d2"][k - 1] == after)


@pytest.mark.parametrize("name", list(C.SCENES))
def test_every_class_of_answer_is_present(name):
    want = N.reference(name, 2)  # the median radius
    count = want["count"].astype(np.int64)
    classes = {"count 0": int((count == 0).sum()), "count 1 .. k-1": int(((count > 0) & (count < K)).sum()), "count k": int((count == K).sum()),
               "count > k": int((count > K).sum())}
    print("nearest witness, %s, median radius, k = %d: %s" % (name, K, classes))
    assert count.sum() > 0 and (want["touch"] == (count > 0)).all()
    if name in ("own", "torus"):
        assert all(v >= ENOUGH for v in classes.values()), (name, classes)
    assert classes["count 0"] >= ENOUGH and classes["count 1 .. k-1"] >= ENOUGH, (name, classes)
    # the order: ascending d2 down the slots, ascending key within a tie; empty slots behind the filled ones
    d2, win = want["d2"], want["winner"]
    _, b, _, _ = C.case(name)
    for j in range(1, K):
        both = win[j] >= 0
        assert (win[j - 1][both] >= 0).all()
        assert (d2[j - 1][both] <= d2[j][both]).all()
        tie = both & (d2[j - 1] == d2[j])
        assert (b.key[win[j - 1][tie]] < b.key[win[j][tie]]).all()
    assert ((win >= 0).sum(axis=0) == np.minimum(count, K)).all()


@pytest.mark.parametrize("name,k", [("own", 8), ("torus", 8), ("cornell", 3)])
def test_exact_ties_across_the_cut(name, k):
    at_median = int(ties_across_the_cut(N.reference(name, 2), k).sum())
    at_inf = int(ties_across_the_cut(N.reference(name, 0), k).sum())
    print("nearest witness, %s, k = %d: %d points tie across the cut at the median radius, %d at +INF" % (name, k, at_median, at_inf))
    assert at_median >= ENOUGH and at_inf >= 100, (name, k, at_median, at_inf)


def test_lists_span_instances_and_kinds():
    want = N.reference("own", 2)
    ids, filled = want["id"], want["winner"] >= 0
    inst = np.where(filled, ids[:, :, 2].astype(np.int64), -1)
    kind = np.where(filled, ids[:, :, 0].astype(np.int64), -1)
    spans = lambda a: np.array([len(set(col[col >= 0].tolist())) > 1 for col in a.T])  # noqa: E731
    instances, kinds = int(spans(inst).sum()), int(spans(kind).sum())
    print("nearest witness, own, median radius, k = %d: %d lists span more than one instance, %d more than one kind" % (K, instances, kinds))
    assert instances >= ENOUGH and kinds >= ENOUGH


@pytest.mark.parametrize("name", list(C.SCENES))
def test_small_radii_leave_rows_with_fewer_than_k(name):
    for index in (1, 3):  # radius 0 and 2^-20
        count = N.reference(name, index)["count"]
        some = int(((count > 0) & (count < K)).sum())
        print("nearest witness, %s, radius %r: %d points with 1 .. k-1 admissible candidates, %d with none" % (name, C.radii(C.case(name)[3])[index], some, int((count == 0).sum())))
        assert some >= ENOUGH, (name, index, some)
