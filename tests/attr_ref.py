"""The reference of the hit-attribute tests (include/lasgun_hip.h: lg_hit_attributes*, lg_hit_attributes_of*): the attributes of ONE named
primitive for ONE ray, restating the header's contract through tests/pyref.py -- the local ray by the chain's inverse transforms, the
primitive's own intersector, local / bary / uv from its intermediate values, then transform_ray_intersection and the backface swap of every
accel on the way up, then the BSDF's tangents.  The numbering is lg_hit's (tests/query_witness.py says the same): spheres and boxes counted
in scene-graph order (depth first, insertion order), accels in the same order with the root 0, a triangle by its face number in its OBJ.
atan2 / acos / sin / cos come from pyref.math and pyref.sincos, so under trig(api) -- or query_witness.portable_trig() -- they are the
library's portable ones (math_eval ops 2-5), and glibc's otherwise.  Imports neither the HIP library nor anything that needs a GPU."""
import contextlib
import math

import numpy as np

import pyref

INF = float("inf")
HIT, NO_HIT, BAD_RECORD = 1, 2, 4  # LG_ATTR_*
PLANES = (("bary", 3), ("uv", 2), ("local", 3), ("frame", 6), ("dp", 6))  # lg_attr_out's double planes, in its order


class _Trig:
    """`math` for pyref with sin / atan2 / acos through `api.math_eval` (ops 2, 4, 5; cos is op 3)."""

    def __init__(self, api):
        self._api = api

    def _op(self, op, a, b=0.0):
        return float(self._api.math_eval(op, np.array([a]), np.array([b]))[0])

    def sin(self, x): return self._op(2, x)
    def atan2(self, y, x): return self._op(4, y, x)
    def acos(self, x): return self._op(5, x)
    def __getattr__(self, name): return getattr(math, name)


@contextlib.contextmanager
def trig(api):
    """pyref's trigonometry taken from api.math_eval (the device's, or the oracle's portable mode: the same algorithm) within the block."""
    t = _Trig(api)
    saved = pyref.math, pyref.sincos
    pyref.math, pyref.sincos = t, (lambda x: (t.sin(x), t._op(3, x)))
    try:
        yield
    finally:
        pyref.math, pyref.sincos = saved


class Catalog:
    """What (kind, prim, instance) names in a pyref scene.  accels[i] = {"chain": [(m, minv, swap), ...] root .. self, "mesh": (obj, mat) or
    None}; spheres[i] = (centre, radius, accel); cuboids[i] = (min, max, accel)."""

    def __init__(self, scene):
        self.accels, self.spheres, self.cuboids = [], [], []
        self._group(scene.root, [])

    def _group(self, agg, chain):
        chain = chain + [(agg.transform.m, agg.transform.minv, agg.swap)]
        me = len(self.accels)
        self.accels.append({"chain": chain, "mesh": None})
        for node in agg.contents:
            if node[0] == "sphere":
                self.spheres.append((node[1], node[2], me))
            elif node[0] == "cuboid":
                self.cuboids.append((node[1], node[2], me))
            elif node[0] == "mesh":  # BVHAccel::from_mesh (bvh.rs:141-147): an accel of its own with the identity transform
                ident = pyref.mat_identity()
                self.accels.append({"chain": chain + [(ident, ident, False)], "mesh": (node[1], node[2])})
            else:
                self._group(node[1], chain)

    def record_ok(self, kind, prim, instance):
        """The header's rule for a record that names something (kind 0 is answered before it)."""
        if kind < 1 or kind > 3 or instance >= len(self.accels):
            return False
        if kind == 3:
            mesh = self.accels[instance]["mesh"]
            return mesh is not None and prim < len(mesh[0].polys)
        table = self.spheres if kind == 1 else self.cuboids
        return prim < len(table) and table[prim][2] == instance


def _axis(v):
    return 0 if v[0] == 1.0 else (1 if v[1] == 1.0 else 2)


def _triangle_bary(obj, poly, o, d):
    """Triangle::intersect up to t (triangle.rs:161-251): (t, b0, b1, b2) or None."""
    p0, p1, p2 = obj.position[poly[0][0]], obj.position[poly[1][0]], obj.position[poly[2][0]]
    p0t, p1t, p2t = pyref.sub(p0, o), pyref.sub(p1, o), pyref.sub(p2, o)
    kz = pyref.max_dimension((abs(d[0]), abs(d[1]), abs(d[2])))
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dd = (d[kx], d[ky], d[kz])
    p0t, p1t, p2t = [p0t[kx], p0t[ky], p0t[kz]], [p1t[kx], p1t[ky], p1t[kz]], [p2t[kx], p2t[ky], p2t[kz]]
    sx, sy, sz = pyref._div(-dd[0], dd[2]), pyref._div(-dd[1], dd[2]), pyref._div(1.0, dd[2])
    for q in (p0t, p1t, p2t):
        q[0] += sx * q[2]
        q[1] += sy * q[2]
    e0 = p1t[0] * p2t[1] - p1t[1] * p2t[0]
    e1 = p2t[0] * p0t[1] - p2t[1] * p0t[0]
    e2 = p0t[0] * p1t[1] - p0t[1] * p1t[0]
    if (e0 < 0.0 or e1 < 0.0 or e2 < 0.0) and (e0 > 0.0 or e1 > 0.0 or e2 > 0.0):
        return None
    det = e0 + e1 + e2
    if det == 0.0:
        return None
    p0t[2] *= sz
    p1t[2] *= sz
    p2t[2] *= sz
    tscaled = e0 * p0t[2] + e1 * p1t[2] + e2 * p2t[2]
    if (det < 0.0 and tscaled >= 0.0) or (det > 0.0 and tscaled <= 0.0):
        return None
    invdet = 1.0 / det
    return tscaled * invdet, e0 * invdet, e1 * invdet, e2 * invdet


def attributes(cat, ray, kind, prim, instance):
    """(flags, {"bary", "uv", "local", "frame", "dp"} as tuples) of the record (kind, prim, instance) for `ray` (6 floats); the dict is
    None unless flags == HIT."""
    if kind == 0:
        return 0, None
    if not cat.record_ok(kind, prim, instance):
        return BAD_RECORD, None
    o, d = tuple(float(v) for v in ray[:3]), tuple(float(v) for v in ray[3:])
    chain = cat.accels[instance]["chain"]
    for _, minv, _ in chain:  # inverse_transform_ray of every accel root .. instance (bvh.rs:462)
        o, d = pyref.transform_point(minv, o), pyref.transform_vector(minv, d)
    bary = (0.0, 0.0, 0.0)
    if kind == 1:
        cen, rad, _ = cat.spheres[prim]
        t, inside = pyref.sphere_t(o, d, cen, rad)
        if t < 0.0:
            return NO_HIT, None
        local = pyref.add(o, pyref.mul(d, t))
        p = pyref.sub(local, cen)
        if p[0] == 0.0 and p[1] == 0.0:
            p = (1e-5 * rad, p[1], p[2])
        phi = pyref.math.atan2(p[1], p[0])
        if phi < 0.0:
            phi += 2.0 * pyref.PI
        theta = pyref.math.acos(pyref.fmin(pyref.fmax(pyref._div(p[2], rad), -1.0), 1.0))
        uv = (phi / (2.0 * pyref.PI), theta / pyref.PI)
        g = pyref.sphere_isect(o, d, cen, rad, t, inside)
        s, n = g, None
    elif kind == 2:
        mn, mx, _ = cat.cuboids[prim]
        dinv = (pyref._div(1.0, d[0]), pyref._div(1.0, d[1]), pyref._div(1.0, d[2]))
        r = pyref.cuboid_isect(o, d, dinv, mn, mx, INF)
        if r is None:
            return NO_HIT, None
        t, dp0, dp1, n = r
        local = pyref.add(o, pyref.mul(d, t))
        j, k = _axis(dp0), _axis(dp1)
        uv = (pyref._div(local[j] - mn[j], mx[j] - mn[j]), pyref._div(local[k] - mn[k], mx[k] - mn[k]))
        g = s = (dp0, dp1)
    else:
        obj, _ = cat.accels[instance]["mesh"]
        poly = obj.polys[prim]
        tb = _triangle_bary(obj, poly, o, d)
        if tb is None:
            return NO_HIT, None
        t, b0, b1, b2 = tb
        bary = (b0, b1, b2)
        tex = [obj.texture[poly[i][1]] for i in range(3)] if obj.texture else [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]
        uv = ((b0 * tex[0][0] + b1 * tex[1][0]) + b2 * tex[2][0], (b0 * tex[0][1] + b1 * tex[1][1]) + b2 * tex[2][1])
        local = pyref.add(o, pyref.mul(d, t))
        _, g, s, n = pyref.triangle_isect(obj, poly, o, d, float("nan"))  # (`t >= NaN` never cuts)
    for m, minv, swap in reversed(chain):  # transform_ray_intersection (transform.rs:243-264), then swap_backface (surface.rs:87-99)
        g2 = (pyref.transform_vector(m, g[0]), pyref.transform_vector(m, g[1]))
        s = (pyref.transform_vector(m, s[0]), pyref.transform_vector(m, s[1])) if g != s else g2
        g = g2
        n = None if n is None else pyref.transform_normal(minv, n)
        if swap:
            g, s = (g[1], g[0]), (s[1], s[0])
            n = None if n is None else pyref.neg(n)
    ns = pyref.normalize(n) if n is not None else pyref.normalize(pyref.cross(s[0], s[1]))
    ss = pyref.normalize(s[0])
    ts = pyref.cross(ns, ss)
    return HIT, {"bary": bary, "uv": uv, "local": local, "frame": ss + ts, "dp": g[0] + g[1]}


def planes(cat, rays, hits):
    """attributes() of every (ray, record) as the library's planes: {"flags": uint32 (n,), "bary": float64 (n, 3), ...}; +0.0 where the
    flags are not HIT."""
    n = len(rays)
    out = {"flags": np.zeros(n, dtype=np.uint32)}
    for name, width in PLANES:
        out[name] = np.zeros((n, width), dtype=np.float64)
    for i in range(n):
        h = hits[i]
        flags, at = attributes(cat, rays[i], int(h["kind"]), int(h["prim"]), int(h["instance"]))
        out["flags"][i] = flags
        if at is not None:
            for name, _ in PLANES:
                out[name][i] = at[name]
    return out


def same_planes(got, want):
    """Bit for bit, except that where `want` is NaN `got` is SOME NaN (the header's NaN rule)."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.dtype != np.float64:
        return np.array_equal(g, w)
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.int64), w[~nan].view(np.int64))


# ---- the three closed forms (what a caller does with the planes), as worst absolute errors over the hits
def closed_forms(cat, hits, pl):
    """{"bary_sum": max |b0+b1+b2 - 1| over triangle hits, "vertex_blend": max |sum b_k P_k - p| over them (P_k the face's vertices taken
    to world space through the chain's transforms, p the record's point), "local_to_world": max |M local - p| over all hits, M the chain's
    transforms applied innermost first}: each the largest component's error; NaN and infinite rows are left out."""
    def to_world(inst, q):
        for m, _, _ in reversed(cat.accels[inst]["chain"]):
            q = pyref.transform_point(m, q)
        return q

    def keep(worst, key, e):
        if e == e and e != INF:
            worst[key] = max(worst[key], e)

    worst = {"bary_sum": 0.0, "vertex_blend": 0.0, "local_to_world": 0.0}
    for i in np.nonzero(pl["flags"] == HIT)[0]:
        h = hits[i]
        kind, prim, inst = int(h["kind"]), int(h["prim"]), int(h["instance"])
        p = [float(v) for v in h["p"]]
        if kind == 3:
            b = [float(v) for v in pl["bary"][i]]
            obj, _ = cat.accels[inst]["mesh"]
            P = [to_world(inst, obj.position[v[0]]) for v in obj.polys[prim]]
            keep(worst, "bary_sum", abs((b[0] + b[1] + b[2]) - 1.0))
            for c in range(3):
                keep(worst, "vertex_blend", abs(((b[0] * P[0][c] + b[1] * P[1][c]) + b[2] * P[2][c]) - p[c]))
        w = to_world(inst, tuple(float(v) for v in pl["local"][i]))
        for c in range(3):
            keep(worst, "local_to_world", abs(w[c] - p[c]))
    return worst
