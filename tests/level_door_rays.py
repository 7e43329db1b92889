"""Shared by the level-door tests and tools/level_door_share.py -- TEST INFRASTRUCTURE.  The doors of a scene as the witness builds them
(tests/pyref_bvh.py: every nested BVHAccel with its inverse transform, its node-0 box and the chain of transforms that leads to it), the
probe of walk.h's ST_ENTER block restated twice -- on Python floats with the witness's own helpers, and in numpy -- the reference's node-0
test, the lone-mesh rule, and the edge-case rays of the issue, placed from the doors' own numbers."""
import math
import struct

import numpy as np

import pyref
import pyref_bvh
from pyref import INF, _div, transform_point, transform_vector

NAN = float("nan")


class Door:
    """One nested accel: `accel` (pyref_bvh.Accel), `chain` = the accels from the root down to its PARENT (their minv, in order, take a world
    ray into the space the door is reached in), `k` = the thinnest axis of its node-0 box, `lone` = the rule of DESIGN.md 3.1."""

    def __init__(self, accel, chain, is_mesh):
        self.accel, self.chain, self.is_mesh = accel, chain, is_mesh
        lo, hi = accel.nodes[0][0]
        ext = [hi[i] - lo[i] for i in range(3)]
        k = 0
        for i in (1, 2):
            if ext[i] < ext[k]:
                k = i
        self.k, self.lo, self.hi = k, lo[k], hi[k]
        self.row = tuple(accel.minv[c][k] for c in range(4))
        self.lone = False


def _bits(x):
    return struct.pack("<d", x)


def lone_rule(group, is_mesh_of):
    """the group holds exactly one primitive, a mesh accel with the identity as its inverse transform, node 0 of the group is a
    leaf, and the two node-0 boxes are the same 48 bytes."""
    if len(group.prims) != 1 or not group.nodes[0][1]:
        return False
    child = group.prims[0].get("accel")
    if child is None or not is_mesh_of(child):
        return False
    ident = pyref.mat_identity()
    if any(_bits(child.minv[c][r]) != _bits(ident[c][r]) for c in range(4) for r in range(3)):
        return False
    (glo, ghi), (mlo, mhi) = group.nodes[0][0], child.nodes[0][0]
    return all(_bits(glo[i]) == _bits(mlo[i]) and _bits(ghi[i]) == _bits(mhi[i]) for i in range(3))


def doors(pscene):
    """(root accel, [Door]) of a pyref scene, in the walk's pre-order."""
    root = pyref_bvh.build(pscene.root)
    meshes = set()

    def mark(agg, acc):  # which witness accels are meshes: pyref_bvh.build keeps the aggregate's order
        for node, prim in zip(agg.contents, acc.prims):
            if node[0] == "mesh":
                meshes.add(id(prim["accel"]))
            elif node[0] not in ("sphere", "cuboid"):
                mark(node[1], prim["accel"])
    mark(pscene.root, root)
    out = []

    def walk(acc, chain):
        for prim in acc.prims:
            child = prim.get("accel")
            if child is not None:
                out.append(Door(child, chain + [acc], id(child) in meshes))
                walk(child, chain + [acc])
    walk(root, [])
    for d in out:
        d.lone = (not d.is_mesh) and lone_rule(d.accel, lambda a: id(a) in meshes)
    return root, out


def parent_ray(door, o, d):
    """The world ray in the space the door is reached in: the minv of every accel on the chain, in order (bvh.rs:462)."""
    for acc in door.chain:
        o, d = transform_point(acc.minv, o), transform_vector(acc.minv, d)
    return o, d


def probe(door, o, d):
    """walk.h's probe on Python floats: component k of the local ray by the expressions of transform_point / transform_vector, the two plane
    parameters of that axis, m = fmax(t1, t2); True = "the lane does not enter"."""
    a0, a1, a2, a3 = door.row
    if not (math.isfinite(o[0]) and math.isfinite(o[1]) and math.isfinite(o[2])):
        return False  # (transform_point: 0 * inf in w makes every component NaN)
    ok = ((a0 * o[0] + a1 * o[1]) + a2 * o[2]) + a3 * 1.0
    dk = ((a0 * d[0] + a1 * d[1]) + a2 * d[2]) + a3 * 0.0
    inv = _div(1.0, dk)
    m = pyref.fmax((door.lo - ok) * inv, (door.hi - ok) * inv)
    return m <= 0.0


def node0_hit(door, o, d):
    """The reference's own decision at the door: the whole local ray, Bounds::intersects on node 0."""
    ol, dl = transform_point(door.accel.minv, o), transform_vector(door.accel.minv, d)
    dinv = (_div(1.0, dl[0]), _div(1.0, dl[1]), _div(1.0, dl[2]))
    return pyref_bvh.slab_intersects(door.accel.nodes[0][0], ol, dinv)


def probe_numpy(door, o, d):
    """The probe again on (n, 3) float64 arrays; the same verdicts as probe() ray for ray."""
    a0, a1, a2, a3 = door.row
    with np.errstate(all="ignore"):
        fin = np.isfinite(o).all(axis=1)
        ok = ((a0 * o[:, 0] + a1 * o[:, 1]) + a2 * o[:, 2]) + a3 * 1.0
        dk = ((a0 * d[:, 0] + a1 * d[:, 1]) + a2 * d[:, 2]) + a3 * 0.0
        inv = 1.0 / dk
        m = np.fmax((door.lo - ok) * inv, (door.hi - ok) * inv)
        return fin & (m <= 0.0)


def edge_rays(pscene, seed=1):
    """World rays (n, 6) and a family name per ray, placed from the doors of `pscene`.  Doors reached through an identity chain (the space they
    are reached in is the world) get the exact cases -- the others see the same rays as a general sample:
      face      origin exactly on one of the door's two planes (t = 0 on the probe's axis), directions towards, away and along
      dzero     d'_k = +0 and -0 with the origin inside, below and above the slab (inf, 0 * inf)
      negzero   directions with -0 components on the other axes, into the door (a lone-mesh group then takes both levels)
      nonfinite NaN and infinite components in origin and direction
      random    origins around the scene, directions anywhere"""
    rng = np.random.default_rng(seed)
    _, ds = doors(pscene)
    rays, fam = [], []

    def put(f, o, d):
        rays.append([*o, *d]); fam.append(f)
    ident = pyref.mat_identity()
    for dr in ds:
        if any(acc.minv != ident for acc in dr.chain):
            continue
        lo, hi = dr.accel.nodes[0][0]
        cen_l = [0.5 * lo[i] + 0.5 * hi[i] for i in range(3)]
        # rows of minv that are +-unit vectors plus a translation let a world origin land on the plane exactly; otherwise the family is a near miss
        m = dr.accel.m
        for plane in (dr.lo, dr.hi):
            pl = list(cen_l); pl[dr.k] = plane
            ow = transform_point(m, pl)
            for _ in range(6):
                d = rng.normal(size=3)
                put("face", ow, d); put("face", ow, -d)
            for axis in range(3):
                e = [0.0, 0.0, 0.0]; e[axis] = 1.0
                put("face", ow, e); put("face", ow, [-v for v in e])
        for off in (0.5, -0.25, 1.5):  # inside, below, above the slab (a slab without thickness: on it, below, above)
            pl = list(cen_l); pl[dr.k] = dr.lo + (dr.hi - dr.lo) * off + (0.0 if dr.hi > dr.lo else (off - 0.5))
            ow = transform_point(m, pl)
            for z in (0.0, -0.0):
                for _ in range(3):
                    dl = list(rng.normal(size=3)); dl[dr.k] = z
                    put("dzero", ow, transform_vector(m, dl) if dr.accel.minv != ident else dl)
        for _ in range(12):
            o = rng.uniform(-3.0, 3.0, size=3)
            to = np.array(transform_point(m, cen_l)) - o
            j = int(rng.integers(3))
            to[j] = -0.0
            if rng.integers(2):
                to[(j + 1) % 3] = -0.0
            put("negzero", o, to)
        cw = transform_point(m, cen_l)
        for bad in (NAN, INF, -INF):
            for j in range(3):
                o = list(rng.uniform(-3.0, 3.0, size=3)); d = [cw[i] - o[i] for i in range(3)]
                ob = list(o); ob[j] = bad
                put("nonfinite", ob, d)
                db = list(d); db[j] = bad
                put("nonfinite", o, db)
    for i in range(512):
        o = rng.uniform(-3.5, 3.5, size=3)
        if i % 3 == 1:  # aimed at the middle of the scene, where its primitives are: hits
            d = (rng.uniform(-1.2, 1.2, size=3) - o) * float(rng.choice([0.3, 1.0, 7.0]))
        elif i % 3 == 2:  # leaving the middle: doors behind the ray, other primitives ahead
            o = rng.uniform(-1.0, 1.0, size=3)
            d = rng.uniform(-1.6, 1.6, size=3) - o
        else:
            d = rng.normal(size=3) * float(rng.choice([0.3, 1.0, 7.0]))
        put("random", o, d)
    return np.array(rays, dtype=np.float64), np.array(fam)


def walk_entries(root, ds, o, d, out):
    """Walk one world ray through the witness (BVHAccel::intersect, no early exit) and append to `out`, for every nested accel it ENTERS, the
    tuple (door, origin, direction) of the ray as the accel receives it (in its parent's space)."""
    by_id = {id(dr.accel): dr for dr in ds}
    orig = pyref_bvh.Accel.intersect

    def spy(self, o_, d_, best_t):
        dr = by_id.get(id(self))
        if dr is not None:
            out.append((dr, o_, d_))
        return orig(self, o_, d_, best_t)
    pyref_bvh.Accel.intersect = spy
    try:
        return root.intersect(o, d, INF)
    finally:
        pyref_bvh.Accel.intersect = orig


def tally(entries):
    """Counts over walked entries: all, misses at node 0, misses the probe proves; the implication is asserted on every one."""
    n = miss0 = shut = 0
    for dr, o, d in entries:
        n += 1
        hit0 = node0_hit(dr, o, d)
        s = probe(dr, o, d)
        assert not (s and hit0), (dr.row, dr.lo, dr.hi, o, d)
        miss0 += not hit0
        shut += s
    return n, miss0, shut
