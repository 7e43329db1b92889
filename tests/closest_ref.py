"""The brute force of the closest-point tests (include/lasgun_hip.h: lg_closest_points*): the header's arithmetic restated in vectorised
numpy, word for word, over ALL primitives of a tests/pyref.py scene -- no tree, no visit order.  Chains, meshes, spheres, boxes and lg_hit's
numbering come from tests/attr_ref.py's Catalog.  All float64, nothing fused (numpy never fuses), dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
Imports neither the HIP library nor anything that needs a GPU."""
import numpy as np

import attr_ref

INF = float("inf")
MISS_ID = (0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
# the twelve triangles of a box, as corners (bit 0 / 1 / 2 of a corner's number: the box's max on x / y / z): -x, +x, -y, +y, -z, +z, each
# face cut by the diagonal from its lowest corner to its highest
BOX_TRIANGLES = ((0, 2, 6), (0, 6, 4), (1, 3, 7), (1, 7, 5), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (0, 1, 3), (0, 3, 2), (4, 5, 7), (4, 7, 6))


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def xf_point(m, p):
    """The library's transform of a point by a pyref matrix (m[column][row]): ((c0*x + c1*y) + c2*z) + c3*1.0 per component; every
    component NaN where a coordinate is not finite."""
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = np.stack([((m[0][r] * x + m[1][r] * y) + m[2][r] * z) + m[3][r] * 1.0 for r in range(3)], axis=-1)
    out[~np.isfinite(p).all(axis=-1)] = np.nan
    return out


def to_world(chain, p):
    """W_A: the accel's own transform, then its parent's, up to the root's."""
    for m, _, _ in reversed(chain):
        p = xf_point(m, p)
    return p


def closest_on_triangle(q, a, b, c):
    """(x, region): Ericson 5.1.5 in the header's operation order; region 1 .. 7 is the step that answered."""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, q - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = q - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = q - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den = 1.0 / ((va + vb) + vc)
        col = lambda s: s[..., None]  # noqa: E731
        x7 = (a + ab * col(vb * den)) + ac * col(vc * den)
        x6 = b + (c - b) * col((d4 - d3) / ((d4 - d3) + (d5 - d6)))
        x5 = a + ac * col(d2 / (d2 - d6))
        x3 = a + ab * col(d1 / (d1 - d3))
        tests = [((d1 <= 0.0) & (d2 <= 0.0), a), ((d3 >= 0.0) & (d4 <= d3), b), ((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), x3),
                 ((d6 >= 0.0) & (d5 <= d6), c), ((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), x5),
                 ((va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0), x6)]
        shape = np.broadcast(d1, d1).shape
        x = np.broadcast_to(x7, shape + (3,)).copy()
        region = np.full(shape, 7, dtype=np.int8)
        for k in range(5, -1, -1):  # the first test that holds wins: applied last
            hold, xk = tests[k]
            x = np.where(col(hold), np.broadcast_to(xk, shape + (3,)), x)
            region = np.where(hold, k + 1, region)
    return x, region


def closest_triangle(q, a, b, c):
    x, region = closest_on_triangle(q, a, b, c)
    with np.errstate(all="ignore"):
        e = q - x
        return x, dot(e, e), region


def closest_box(q, corners):
    """corners: (..., 8, 3), world space.  (x, d2, triangle): the lowest d2 of the twelve, the first on a tie; a NaN never replaces anything;
    all twelve NaN: d2 = NaN, triangle -1."""
    best_x = best_d2 = best_t = None
    for t, (i, j, k) in enumerate(BOX_TRIANGLES):
        x, d2, _ = closest_triangle(q, corners[..., i, :], corners[..., j, :], corners[..., k, :])
        if best_x is None:
            have = ~np.isnan(d2)
            best_x, best_d2, best_t = np.where(have[..., None], x, 0.0), np.where(have, d2, np.nan), np.where(have, t, -1)
            continue
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(d2) & (np.isnan(best_d2) | (d2 < best_d2))
        best_x, best_d2, best_t = np.where(take[..., None], x, best_x), np.where(take, d2, best_d2), np.where(take, t, best_t)
    return best_x, best_d2, best_t


def closest_sphere(q, cw, pw):
    with np.errstate(all="ignore"):
        pc = pw - cw
        rw = np.sqrt(dot(pc, pc))
        v = q - cw
        l = np.sqrt(dot(v, v))  # noqa: E741
        d = np.abs(l - rw)
        x = cw + v * (rw / l)[..., None]
        x = np.where((l == 0.0)[..., None], np.broadcast_to(pw, x.shape), x)
        return x, d * d


class Brute:
    """Every primitive of a pyref scene in world space, in lg_hit's numbering: candidates() and closest() over all of them."""

    def __init__(self, pscene):
        self.cat = cat = attr_ref.Catalog(pscene)
        # the material lg_intersect reports for a hit on each primitive, as the pyref Material (None: the default material): a sphere's or a
        # box's own; a triangle's is its mesh instance's, the only accel on its chain that can carry one
        sphere_mat, box_mat = [], []

        def collect(agg):  # (the Catalog's own order: depth first, insertion order)
            for node in agg.contents:
                if node[0] == "sphere":
                    sphere_mat.append(node[3])
                elif node[0] == "cuboid":
                    box_mat.append(node[3])
                elif node[0] == "group":
                    collect(node[1])
        collect(pscene.root)
        assert len(sphere_mat) == len(cat.spheres) and len(box_mat) == len(cat.cuboids)
        tri, tri_id = [], []
        for inst, acc in enumerate(cat.accels):
            if acc["mesh"] is None:
                continue
            obj = acc["mesh"][0]
            pos = np.array(obj.position, dtype=np.float64).reshape(-1, 3)
            faces = np.array([[poly[0][0], poly[1][0], poly[2][0]] for poly in obj.polys], dtype=np.int64).reshape(-1, 3)
            world = to_world(acc["chain"], pos)
            tri.append(world[faces])
            tri_id += [(inst, 3, f) for f in range(len(faces))]
        self.tri = np.concatenate(tri) if tri else np.zeros((0, 3, 3))
        box, box_id = [], []
        for prim, (mn, mx, inst) in enumerate(cat.cuboids):
            corners = np.array([[(mx if k & 1 else mn)[0], (mx if k & 2 else mn)[1], (mx if k & 4 else mn)[2]] for k in range(8)], dtype=np.float64)
            box.append(to_world(cat.accels[inst]["chain"], corners))
            box_id.append((inst, 2, prim))
        self.box = np.array(box).reshape(-1, 8, 3)
        cw, pw, sph_id = [], [], []
        for prim, (cen, rad, inst) in enumerate(cat.spheres):
            c = np.array(cen, dtype=np.float64)
            chain = cat.accels[inst]["chain"]
            cw.append(to_world(chain, c))
            pw.append(to_world(chain, c + np.array([float(rad), 0.0, 0.0])))
            sph_id.append((inst, 1, prim))
        self.cw, self.pw = np.array(cw).reshape(-1, 3), np.array(pw).reshape(-1, 3)
        ids = np.array(sph_id + box_id + tri_id, dtype=np.uint64).reshape(-1, 3)  # candidates in this order: spheres, boxes, triangles
        self.ids = ids
        self.materials = sphere_mat + box_mat + [cat.accels[int(inst)]["mesh"][1] for inst, _, _ in tri_id]  # per candidate, in the candidates' order
        self.key = (ids[:, 0] << np.uint64(34)) | (ids[:, 1] << np.uint64(32)) | ids[:, 2]
        self.count = len(ids)

    def candidates(self, points):
        """(x (n, C, 3), d2 (n, C), detail (n, C)) of every candidate: detail = the triangle's region 1 .. 7, the box's triangle 0 .. 11 (-1:
        all NaN), 0 for a sphere."""
        q = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 1, 3)
        n = len(q)
        xs, d2s, det = [], [], []
        if len(self.cw):
            x, d2 = closest_sphere(q, self.cw[None], self.pw[None])
            xs.append(x), d2s.append(d2), det.append(np.zeros(d2.shape, dtype=np.int8))
        if len(self.box):
            x, d2, t = closest_box(q, self.box[None])
            xs.append(x), d2s.append(d2), det.append(t.astype(np.int8))
        if len(self.tri):
            x, d2, region = closest_triangle(q, self.tri[None, :, 0], self.tri[None, :, 1], self.tri[None, :, 2])
            xs.append(x), d2s.append(d2), det.append(region)
        if not xs:
            return np.zeros((n, 0, 3)), np.zeros((n, 0)), np.zeros((n, 0), dtype=np.int8)
        return np.concatenate(xs, axis=1), np.concatenate(d2s, axis=1), np.concatenate(det, axis=1)

    def closest(self, points, radius=INF, chunk=256):
        """The header's answer for every point: {"distance" (n,), "point" (n, 3), "id" (n, 4) uint32 with material left 0xFFFFFFFF
        (a table index is the library's own: the winner's Material is self.materials[winner]), "detail" (n,) int8, "winner" (n,) the
        candidate's index or -1}."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = len(pts)
        out = {"distance": np.full(n, INF), "point": np.zeros((n, 3)), "id": np.tile(np.array(MISS_ID, dtype=np.uint32), (n, 1)),
               "detail": np.zeros(n, dtype=np.int8), "winner": np.full(n, -1, dtype=np.int64)}
        r2 = np.float64(radius) * np.float64(radius)
        for lo in range(0, n, chunk):
            q = pts[lo:lo + chunk]
            x, d2, det = self.candidates(q)
            if d2.shape[1] == 0:
                continue
            with np.errstate(invalid="ignore"):
                ok = (d2 <= r2) & (d2 < INF) & np.isfinite(q).all(axis=1)[:, None]
            d2m = np.where(ok, d2, INF)
            low = d2m.min(axis=1)
            tie = ok & (d2m == low[:, None])
            key = np.where(tie, self.key[None], np.uint64(0xFFFFFFFFFFFFFFFF))
            w = key.argmin(axis=1)
            hit = tie.any(axis=1)
            rows = np.arange(len(q))
            sel = slice(lo, lo + len(q))
            out["distance"][sel] = np.where(hit, np.sqrt(np.where(hit, low, 0.0)), INF)
            out["point"][sel] = np.where(hit[:, None], x[rows, w], 0.0)
            ids = self.ids[w]
            full = np.stack([ids[:, 1], ids[:, 2], ids[:, 0], np.full(len(q), 0xFFFFFFFF, dtype=np.uint64)], axis=1).astype(np.uint32)
            out["id"][sel] = np.where(hit[:, None], full, np.array(MISS_ID, dtype=np.uint32)[None])
            out["detail"][sel] = np.where(hit, det[rows, w], 0)
            out["winner"][sel] = np.where(hit, w, -1)
        return out


def same_bits(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes()
