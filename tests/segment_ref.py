"""The brute force of the segment-proximity tests (include/lasgun_hip.h: lg_closest_segments*): lasgun_amd/csrc/segment_prim.h restated in
vectorised numpy, word for word, over ALL primitives of a tests/pyref.py scene -- no tree, no visit order.  The primitives in world space,
their keys and materials are tests/closest_ref.py's Brute.  All float64, nothing fused (numpy never fuses), dot and cross in the project's
operation order.  Imports neither the HIP library nor anything that needs a GPU."""
import numpy as np

import closest_ref as R
from closest_ref import dot

INF = float("inf")
PLANES = ("touch", "distance", "param", "point", "id")
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
# `detail` of a candidate: a triangle's sub-candidate 1 .. 6 (0: the point form, -1: all NaN); a box's 8 * triangle + sub-candidate; a
# sphere's 11 outside, 12 inside, 13 crossing by a root, 14 crossing by the fallback (10: the point form, -1: NaN)
SPHERE_POINT, SPHERE_OUTSIDE, SPHERE_INSIDE, SPHERE_CROSSING, SPHERE_FALLBACK = 10, 11, 12, 13, 14


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def clamp01(x):
    return np.where(x <= 0.0, 0.0, np.where(x >= 1.0, 1.0, x))


def col(s):
    return s[..., None]


def seg_edge(p0, p1, e0, e1):
    """(x, s, d2): Ericson 5.1.9 with EPSILON = 0 in the header's operation order."""
    d1, d2, r = p1 - p0, e1 - e0, p0 - e0
    a, e, f = dot(d1, d1), dot(d2, d2), dot(d2, r)
    c, b = dot(d1, r), dot(d1, d2)
    denom = a * e - b * b
    s_gen = np.where(denom != 0.0, clamp01((b * f - c * e) / denom), 0.0)
    t_gen = (b * s_gen + f) / e
    s_lo, s_hi = clamp01(-c / a), clamp01((b - c) / a)
    s_g = np.where(t_gen < 0.0, s_lo, np.where(t_gen > 1.0, s_hi, s_gen))
    t_g = np.where(t_gen < 0.0, 0.0, np.where(t_gen > 1.0, 1.0, t_gen))
    a0, e0z = a <= 0.0, e <= 0.0
    s = np.where(a0, 0.0, np.where(e0z, s_lo, s_g))
    t = np.where(a0 & e0z, 0.0, np.where(a0, clamp01(f / e), np.where(e0z, 0.0, t_g)))
    c1, c2 = p0 + d1 * col(s), e0 + d2 * col(t)
    w = c1 - c2
    shape = np.broadcast(s, s).shape
    return np.broadcast_to(c2, shape + (3,)), s, dot(w, w)


def seg_pierce(p0, p1, a, b, c):
    """(crosses, x, s): Ericson 5.3.6 made two-sided, confirmed on formed points."""
    ab, ac, qp = b - a, c - a, p0 - p1
    n = cross(ab, ac)
    d = dot(qp, n)
    ap = p0 - a
    t = dot(ap, n)
    e = cross(qp, ap)
    v, w = dot(ac, e), -dot(ab, e)
    neg = d < 0.0
    d, t, v, w = np.where(neg, -d, d), np.where(neg, -t, t), np.where(neg, -v, v), np.where(neg, -w, w)
    hit = (d > 0.0) & (d < INF) & (t >= 0.0) & (t <= d) & (v >= 0.0) & (w >= 0.0) & ((v + w) <= d)
    s = clamp01(t / d)
    y = p0 + (p1 - p0) * col(s)
    inf3 = lambda p: np.fmax(np.abs(p[..., 0]), np.fmax(np.abs(p[..., 1]), np.abs(p[..., 2])))  # noqa: E731
    g = 2.0 ** -46 * np.fmax(np.fmax(inf3(y), inf3(a)), np.fmax(inf3(b), inf3(c)))
    confirmed = R.closest_triangle(y, a, b, c)[1] <= g * g
    return hit & confirmed, y, s


def seg_triangle(p0, p1, a, b, c):
    """(x, s, d2, which)."""
    with np.errstate(all="ignore"):
        shape = np.broadcast(p0[..., 0], a[..., 0]).shape
        best_x, best_s = np.zeros(shape + (3,)), np.zeros(shape)
        best_d2, have, which = np.full(shape, np.nan), np.zeros(shape, dtype=bool), np.full(shape, -1, dtype=np.int16)

        def take(ok, x, s, d2, tag):
            nonlocal best_x, best_s, best_d2, have, which
            t = ok & ~np.isnan(d2) & (~have | (d2 < best_d2))
            best_x, best_s, best_d2 = np.where(col(t), x, best_x), np.where(t, s, best_s), np.where(t, d2, best_d2)
            have, which = have | t, np.where(t, tag, which)
        hit, x, s = seg_pierce(p0, p1, a, b, c)
        take(hit, x, s, np.zeros(shape), 1)
        everything = np.ones(shape, dtype=bool)
        x0, d20, _ = R.closest_triangle(p0, a, b, c)
        take(everything, x0, np.zeros(shape), d20, 2)
        x1, d21, _ = R.closest_triangle(p1, a, b, c)
        take(everything, x1, np.ones(shape), d21, 3)
        for j, (e0, e1) in enumerate(((a, b), (b, c), (c, a))):
            x, s, d2 = seg_edge(p0, p1, e0, e1)
            take(everything, x, s, d2, 4 + j)
        deg = np.broadcast_to((p0 == p1).all(axis=-1), shape)
        return np.where(col(deg), x0, best_x), np.where(deg, 0.0, best_s), np.where(deg, d20, best_d2), np.where(deg, 0, which)


def seg_box(p0, p1, corners):
    """corners: (..., 8, 3), world space.  (x, s, d2, 8 * triangle + which; -1: all NaN)."""
    best = None
    for t, (i, j, k) in enumerate(R.BOX_TRIANGLES):
        x, s, d2, which = seg_triangle(p0, p1, corners[..., i, :], corners[..., j, :], corners[..., k, :])
        tag = 8 * t + which
        if best is None:
            have = ~np.isnan(d2)
            best = [np.where(col(have), x, 0.0), np.where(have, s, 0.0), np.where(have, d2, np.nan), np.where(have, tag, -1), have]
            continue
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(d2) & (~best[4] | (d2 < best[2]))
        best = [np.where(col(take), x, best[0]), np.where(take, s, best[1]), np.where(take, d2, best[2]), np.where(take, tag, best[3]), best[4] | take]
    return best[0], best[1], best[2], best[3].astype(np.int16)


def seg_sphere(p0, p1, cw, pw):
    """(x, s, d2, case)."""
    with np.errstate(all="ignore"):
        pc = pw - cw
        rw = np.sqrt(dot(pc, pc))
        u = p1 - p0
        uu = dot(u, u)
        v0, v1 = p0 - cw, p1 - cw
        tt = dot(cw - p0, u)
        sstar = np.where(uu > 0.0, clamp01(tt / uu), 0.0)
        m = p0 + u * col(sstar)
        vm = m - cw
        lmin = np.sqrt(dot(vm, vm))
        l0, l1 = np.sqrt(dot(v0, v0)), np.sqrt(dot(v1, v1))
        far1 = l1 > l0
        lmax = np.where(far1, l1, l0)
        vf = np.where(col(far1), v1, v0)
        shape = lmin.shape
        # outside
        d = lmin - rw
        x_out, d2_out = cw + vm * col(rw / lmin), d * d
        # inside
        d = rw - lmax
        x_in = np.where(col(lmax == 0.0), np.broadcast_to(pw, shape + (3,)), cw + vf * col(rw / lmax))
        s_in, d2_in = np.where(far1, 1.0, 0.0), d * d
        # crossing
        B, C = dot(v0, u), dot(v0, v0) - rw * rw
        disc = B * B - uu * C
        q = np.sqrt(disc)
        s1, s2 = (-B - q) / uu, (-B + q) / uu
        ok1, ok2 = (s1 >= 0.0) & (s1 <= 1.0), (s2 >= 0.0) & (s2 <= 1.0)
        s_root = np.where(ok1, clamp01(s1), clamp01(s2))
        root = ok1 | ok2
        s_cross = np.where(root, s_root, sstar)
        x_cross = np.where(col(root), p0 + u * col(s_root), m)
        outside, inside = lmin > rw, ~(lmin > rw) & (lmax < rw)
        crossing = ~outside & ~inside & (lmin <= rw) & (lmax >= rw) & (lmax < INF)
        x = np.where(col(outside), x_out, np.where(col(inside), x_in, np.where(col(crossing), x_cross, 0.0)))
        s = np.where(outside, sstar, np.where(inside, s_in, np.where(crossing, s_cross, 0.0)))
        d2 = np.where(outside, d2_out, np.where(inside, d2_in, np.where(crossing, 0.0, np.nan)))
        case = np.where(outside, SPHERE_OUTSIDE, np.where(inside, SPHERE_INSIDE, np.where(crossing, np.where(root, SPHERE_CROSSING, SPHERE_FALLBACK), -1)))
        deg = np.broadcast_to((p0 == p1).all(axis=-1), shape)
        xp, d2p = R.closest_sphere(p0, cw, pw)
        return np.where(col(deg), xp, x), np.where(deg, 0.0, s), np.where(deg, d2p, d2), np.where(deg, SPHERE_POINT, case).astype(np.int16)


def candidates(b, segments):
    """(x (n, C, 3), s (n, C), d2 (n, C), detail (n, C)) of every candidate of R.Brute b, in its candidates' order: spheres, boxes, triangles."""
    seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 1, 6)
    p0, p1 = seg[..., :3], seg[..., 3:]
    n = len(seg)
    parts = []
    if len(b.cw):
        parts.append(seg_sphere(p0, p1, b.cw[None], b.pw[None]))
    if len(b.box):
        parts.append(seg_box(p0, p1, b.box[None]))
    if len(b.tri):
        parts.append(seg_triangle(p0, p1, b.tri[None, :, 0], b.tri[None, :, 1], b.tri[None, :, 2]))
    if not parts:
        return np.zeros((n, 0, 3)), np.zeros((n, 0)), np.zeros((n, 0)), np.zeros((n, 0), dtype=np.int16)
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(4))


def closest_segments(b, segments, radii_sets, chunk=128):
    """The header's answer for every segment under each of `radii_sets` (each an (n,) array or one number), the candidates formed once:
    a list of {"touch" (n,) uint8, "distance" (n,), "param" (n,), "point" (n, 3), "id" (n, 4) uint32 with material left 0xFFFFFFFF,
    "detail" (n,), "winner" (n,) the candidate's index or -1, "tie" (n,) bool: another admissible candidate has the winner's d2}."""
    seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 6)
    n = len(seg)
    sets = [np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64), (n,))) for r in radii_sets]
    outs = [{"touch": np.zeros(n, dtype=np.uint8), "distance": np.full(n, INF), "param": np.zeros(n), "point": np.zeros((n, 3)),
             "id": np.tile(np.array(R.MISS_ID, dtype=np.uint32), (n, 1)), "detail": np.zeros(n, dtype=np.int16), "winner": np.full(n, -1, dtype=np.int64),
             "tie": np.zeros(n, dtype=bool)} for _ in sets]
    finite = np.isfinite(seg).all(axis=1)
    for lo in range(0, n, chunk):
        q = seg[lo:lo + chunk]
        sel = slice(lo, lo + len(q))
        x, s, d2, det = candidates(b, q)
        if d2.shape[1] == 0:
            continue
        rows = np.arange(len(q))
        for r, out in zip(sets, outs):
            with np.errstate(invalid="ignore", over="ignore"):
                r2 = r[sel] * r[sel]
                valid = (r[sel] >= 0.0) & finite[sel]
                ok = (d2 <= r2[:, None]) & (d2 < INF) & valid[:, None]
            d2m = np.where(ok, d2, INF)
            low = d2m.min(axis=1)
            tie = ok & (d2m == low[:, None])
            w = np.where(tie, b.key[None], NO_KEY).argmin(axis=1)
            hit = tie.any(axis=1)
            out["touch"][sel] = hit
            out["distance"][sel] = np.where(hit, np.sqrt(np.where(hit, low, 0.0)), INF)
            out["param"][sel] = np.where(hit, s[rows, w], 0.0)
            out["point"][sel] = np.where(hit[:, None], x[rows, w], 0.0)
            ids = b.ids[w]
            full = np.stack([ids[:, 1], ids[:, 2], ids[:, 0], np.full(len(q), 0xFFFFFFFF, dtype=np.uint64)], axis=1).astype(np.uint32)
            out["id"][sel] = np.where(hit[:, None], full, np.array(R.MISS_ID, dtype=np.uint32)[None])
            out["detail"][sel] = np.where(hit, det[rows, w], 0)
            out["winner"][sel] = np.where(hit, w, -1)
            out["tie"][sel] = hit & (tie.sum(axis=1) > 1)
    return outs
