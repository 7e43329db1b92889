"""The brute force of the proximity-query tests (include/lasgun_hip.h: lg_nearest*), over tests/closest_ref.py's Brute.candidates() -- every
candidate of every point, no tree, no visit order: the header's admissibility (d2 <= r_i*r_i && d2 < +INF, a point with a non-finite
coordinate or a NaN / negative radius of its own has none), numpy's lexsort by (d2, key), the first k, the count.  Imports neither the HIP
library nor anything that needs a GPU."""
import functools

import numpy as np

import closest_cases as C
import closest_ref as R

INF = float("inf")
MAX_K = 8
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
PLANES = ("touch", "count", "distance", "point", "id")
SLOT_PLANES = PLANES[2:]


def nearest(b, points, radii=None, radius=INF, k=MAX_K, chunk=256):
    """The header's answer for every point: {"touch" (n,) uint8, "count" (n,) uint32, "distance" (k, n), "point" (k, n, 3), "id" (k, n, 4)
    uint32 with material left 0xFFFFFFFF (a table index is the library's own: the Material of slot j is b.materials[winner[j]]), "winner"
    (k, n) the candidate's index or -1, "next_d2" (n,): the d2 of the first admissible candidate left out (+INF: none), "d2" (k, n)}."""
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    r = np.full(n, radius, dtype=np.float64) if radii is None else np.ascontiguousarray(radii, dtype=np.float64)
    assert r.shape == (n,)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = r * r                                                   # one f64 product
        valid = (r >= 0.0) & np.isfinite(pts).all(axis=1)            # (-0.0 >= 0; a NaN is not)
    out = {"touch": np.zeros(n, dtype=np.uint8), "count": np.zeros(n, dtype=np.uint32), "distance": np.full((k, n), INF), "point": np.zeros((k, n, 3)),
           "id": np.tile(np.array(R.MISS_ID, dtype=np.uint32), (k, n, 1)), "winner": np.full((k, n), -1, dtype=np.int64), "next_d2": np.full(n, INF),
           "d2": np.full((k, n), INF)}
    for lo in range(0, n, chunk):
        q = pts[lo:lo + chunk]
        sel = slice(lo, lo + len(q))
        x, d2, _ = b.candidates(q)
        if d2.shape[1] == 0:
            continue
        with np.errstate(invalid="ignore"):
            ok = (d2 <= r2[sel, None]) & (d2 < INF) & valid[sel, None]
        count = ok.sum(axis=1)
        d2m = np.where(ok, d2, INF)
        keym = np.where(ok, b.key[None], NO_KEY)
        order = np.lexsort((keym, d2m), axis=1)                      # ascending d2, an exact tie by ascending key; the inadmissible last
        rows = np.arange(len(q))
        out["count"][sel] = count
        out["touch"][sel] = count > 0
        for j in range(min(k, d2.shape[1])):
            w = order[:, j]
            have = j < count
            out["distance"][j, sel] = np.where(have, np.sqrt(np.where(have, d2[rows, w], 0.0)), INF)
            out["d2"][j, sel] = np.where(have, d2[rows, w], INF)
            out["point"][j, sel] = np.where(have[:, None], x[rows, w], 0.0)
            ids = b.ids[w]
            full = np.stack([ids[:, 1], ids[:, 2], ids[:, 0], np.full(len(q), 0xFFFFFFFF, dtype=np.uint64)], axis=1).astype(np.uint32)
            out["id"][j, sel] = np.where(have[:, None], full, np.array(R.MISS_ID, dtype=np.uint32)[None])
            out["winner"][j, sel] = np.where(have, w, -1)
        if d2.shape[1] > k:
            w = order[:, k]
            out["next_d2"][sel] = np.where(count > k, d2[rows, w], INF)
    return out


def first(want, k):
    """The answer at k <= the k it was made for: the first k slots (touch and count do not depend on k)."""
    return {p: (want[p][:k] if p in SLOT_PLANES + ("winner", "d2") else want[p]) for p in want}


@functools.lru_cache(maxsize=None)
def reference(name, radius_index):
    """The brute force's answer at k = MAX_K for a scene of tests/closest_cases.py under one of its four shared radii, once."""
    _, b, pts, want = C.case(name)
    return nearest(b, pts, radius=C.radii(want)[radius_index], k=MAX_K)


def mixed_radii(name, seed):
    """A radius per point: a seeded mix of +INF, 0, -0.0, the median, 2^-20, NaN, -1 and random values between 0 and twice the median."""
    _, _, pts, want = C.case(name)
    med = C.radii(want)[2]
    rng = np.random.default_rng(seed)
    fixed = np.array([INF, 0.0, -0.0, med, 2.0 ** -20, float("nan"), -1.0])
    pick = rng.integers(0, len(fixed) + 3, len(pts))
    return np.where(pick < len(fixed), fixed[np.minimum(pick, len(fixed) - 1)], rng.uniform(0.0, 2.0 * med, len(pts)))
