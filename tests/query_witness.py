"""The identity-tracking witness of the ray-query tests: tests/pyref.py walking the reference's BVH (tests/pyref_bvh.py), wrapped so that
it also says WHICH primitive won -- (kind, prim, instance) in the numbering of lg_hit -- and, under portable_trig(), with the sphere's
trigonometry taken from the oracle's portable functions (orc_math_eval ops 2-5, the algorithms the device runs).  Imports neither the
HIP library nor anything that needs a GPU."""
import contextlib
import math
import struct

import numpy as np

import pyref
import pyref_bvh

INF = float("inf")


# ---- the witness with primitive identity --------------------------------------------------------------------------------------------
class _TracedAccel(pyref_bvh.Accel):
    """pyref_bvh.Accel whose hit dict also carries "id" = (kind, prim, instance) of the winning primitive: the primitives' intersectors
    below note the last one that returned a hit (the reference's winner is the last accepted one of its walk, bvh.rs:481-488)."""

    def intersect(self, o, d, best_t):
        self.last = None
        r = super().intersect(o, d, best_t)
        if r is not None:
            r["id"] = self.last
        return r


def _tagged(prim, holder, ident):
    inner = prim["isect"]

    def isect(o, d, dinv, best_t):
        r = inner(o, d, dinv, best_t)
        if r is not None:
            holder[0].last = r.get("id", ident)  # a nested accel's hit brings its own identity
        return r
    prim["isect"] = isect
    return prim


class Witness:
    """pyref_bvh.build with the numbering of lg_hit: spheres and boxes counted in scene-graph order (depth first, insertion order),
    accels in the same order with the root 0, a triangle by its face number in its OBJ."""

    def __init__(self, scene):
        self.scene = scene
        self.count = {"sphere": 0, "cuboid": 0, "accel": 0}
        self.root = self._group(scene.root)

    def _next(self, what):
        i = self.count[what]
        self.count[what] += 1
        return i

    def _group(self, agg):
        me, holder, prims = self._next("accel"), [None], []
        for node in agg.contents:
            if node[0] == "sphere":
                prims.append(_tagged(pyref_bvh._sphere_prim(node[1], node[2], node[3]), holder, (1, self._next("sphere"), me)))
            elif node[0] == "cuboid":
                prims.append(_tagged(pyref_bvh._cuboid_prim(node[1], node[2], node[3]), holder, (2, self._next("cuboid"), me)))
            elif node[0] == "mesh":
                prims.append(_tagged(pyref_bvh._accel_prim(self._mesh(node[1], node[2])), holder, None))
            else:
                prims.append(_tagged(pyref_bvh._accel_prim(self._group(node[1])), holder, None))
        acc = _TracedAccel(prims, agg.transform.m, agg.transform.minv, None, agg.swap)
        holder[0] = acc
        return acc

    def _mesh(self, obj, mat):  # BVHAccel::from_mesh (bvh.rs:141-147)
        me, holder = self._next("accel"), [None]
        tris = [_tagged(pyref_bvh._triangle_prim(obj, poly), holder, (3, f, me)) for f, poly in enumerate(obj.polys)]
        acc = _TracedAccel(tris, pyref.mat_identity(), pyref.mat_identity(), mat, False)
        holder[0] = acc
        return acc

    def closest(self, o, d):
        """None, or {"t", "id", "mat", "p", "ng", "ns"}: the hit resolved as shading sees it (surface.rs:158-183, integrate.rs:29-40)."""
        o, d = tuple(float(v) for v in o), tuple(float(v) for v in d)  # (plain Python floats, as pyref computes with)
        r = self.root.intersect(o, d, INF)
        if r is None:
            return None
        wo = pyref.neg(pyref.normalize(d))
        ng = pyref.normalize(pyref.cross(r["g"][0], r["g"][1]))
        if pyref.dot(ng, wo) < 0.0:
            ng = pyref.neg(ng)
        ns = pyref.normalize(r["n"]) if r["n"] is not None else pyref.normalize(pyref.cross(r["s"][0], r["s"][1]))
        return {"t": r["t"], "id": r["id"], "mat": r["own"] if r["own"] is not None else r["mat"],
                "p": pyref.add(o, pyref.mul(d, r["t"])), "ng": ng, "ns": ns}


class _PortableMath:
    """`math` for pyref.sphere_isect with atan2 / acos / sin from the oracle's portable trigonometry (what the device computes)."""

    def __init__(self, o):
        self._o = o

    def _op(self, op, a, b=0.0):
        return float(self._o.math_eval(op, np.array([a]), np.array([b]))[0])

    def sin(self, x): return self._op(2, x)
    def atan2(self, y, x): return self._op(4, y, x)
    def acos(self, x): return self._op(5, x)
    def __getattr__(self, name): return getattr(math, name)


@contextlib.contextmanager
def portable_trig():
    from oracle_lib import oracle
    pm = _PortableMath(oracle())
    saved = pyref.math, pyref.sincos
    pyref.math, pyref.sincos = pm, (lambda x: (pm.sin(x), pm._op(3, x)))
    try:
        yield
    finally:
        pyref.math, pyref.sincos = saved


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def same(a, b):
    """Bit for bit, except that any NaN equals any NaN (a NaN's sign and payload are not part of the reference's semantics: a ray with a
    NaN direction component can be 'hit' at t = NaN, and x86 and the GPU generate different default NaNs)."""
    return bits(a) == bits(b) or (a != a and b != b)


def pod(m):
    """pyref.Material -> (kind, flat parameters) in lg_material's order (include/lasgun_hip.h)."""
    kinds = {"matte": 0, "plastic": 1, "metal": 2, "glass": 3, "mirror": 4}
    flat = []
    for v in m.p:
        flat.extend(v if isinstance(v, tuple) else (v,))
    return kinds[m.kind], [bits(v) for v in flat]
