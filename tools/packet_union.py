#!/usr/bin/env python3
"""How much of the tree the 64 rays of an 8 x 8 pixel tile share on the headline frame (4096^2, the Cornell shell + 1024 spheres), without a
device and without the built library: the reference's own tree (tests/pyref_bvh.py), the reference's camera (tests/pyref.py).  For every
sampled tile the 64 primary rays, and the 64 shadow rays from their hits to the light, are put to the root accel's box tests -- no node is
culled by t, so the nodes a ray hits are those whose ancestors it hits -- and the tool writes, per tile and kind of ray, the interior nodes
and leaves hit per lane (average, maximum), their union over the tile (what a walk with one cursor per wave visits) and the number of
distinct sign triples of the directions ("octants") and of (sign triple, plain or not) pairs ("groups": what such a walk takes one after the other).  The shadow rays are walked to the
end (no early exit): the figure is the tree's, not the any-hit walk's.

usage: python tools/packet_union.py [--tiles 200] [--seed 1] > profiles/packet_union.jsonl      (a summary goes to stderr)"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyref  # noqa: E402
import pyref_bvh  # noqa: E402

SIDE = 4096


def scenes_module():
    """lasgun_amd/scenes.py by its path: importing the package would load the built library."""
    spec = importlib.util.spec_from_file_location("lasgun_scenes", os.path.join(ROOT, "lasgun_amd", "scenes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def slab(box, o, dinv):  # Bounds::intersects (cuboid.rs:104-121) for 64 rays: fmin / fmax ignore a NaN operand
    with np.errstate(all="ignore"):
        t1, t2 = (np.asarray(box[0]) - o) * dinv, (np.asarray(box[1]) - o) * dinv
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
        tnear = np.fmax(np.fmax(np.fmax(-np.inf, lo[:, 0]), lo[:, 1]), lo[:, 2])
        tfar = np.fmin(np.fmin(np.fmin(np.inf, hi[:, 0]), hi[:, 1]), hi[:, 2])
        return (tnear <= tfar) & (tfar > 0.0)


def shared(nodes, o, d):
    """Per-lane and union counts of the interior nodes and leaves of `nodes` that the 64 rays (o, d) hit."""
    with np.errstate(all="ignore"):
        dinv = 1.0 / d
    inner, leaves = np.zeros(len(o), dtype=np.int64), np.zeros(len(o), dtype=np.int64)
    union_inner = union_leaves = 0
    todo = [(0, np.ones(len(o), dtype=bool))]
    while todo:
        cur, mask = todo.pop()
        bounds, leaf, a, b = nodes[cur]
        hit = slab(bounds, o, dinv) & mask
        if not hit.any():
            continue
        if leaf:
            leaves += hit
            union_leaves += 1
        else:
            inner += hit
            union_inner += 1
            todo += [(b, hit), (cur + 1, hit)]
    signs = dinv < 0.0
    key = signs[:, 0] * 1 + signs[:, 1] * 2 + signs[:, 2] * 4
    octants = len(np.unique(key))
    plain = np.isfinite(dinv).all(axis=1) & (dinv != 0.0).all(axis=1) & np.isfinite(o).all(axis=1)  # (walk.h, neg_mask_x: a ray that is not plain is walked in a group of its own)
    groups = len(np.unique(key + np.where(plain, 0, 8)))
    return {"inner_avg": float(inner.mean()), "inner_max": int(inner.max()), "inner_union": union_inner, "leaves_avg": float(leaves.mean()),
            "leaves_max": int(leaves.max()), "leaves_union": union_leaves, "octants": octants, "groups": groups, "rays": int(len(o))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    scene = scenes_module().spheres_scene(pyref.Api, nspheres=1024)
    root = pyref_bvh.build(scene.root)
    light = scene.lights[0]
    light_pos = np.asarray(light[0] if isinstance(light, (tuple, list)) else light.position, dtype=np.float64)
    rng = np.random.default_rng(args.seed)
    n_tiles = SIDE // 8
    centre = [(n_tiles // 2 - k % 2, int(x)) for k, x in enumerate(rng.integers(0, n_tiles, size=max(args.tiles // 10, 2)))]  # the two centre rows
    centre += [(int(y), n_tiles // 2 - k % 2) for k, y in enumerate(rng.integers(0, n_tiles, size=max(args.tiles // 10, 2)))]  # ... and columns
    tiles = centre + [(int(y), int(x)) for y, x in rng.integers(0, n_tiles, size=(max(args.tiles - len(centre), 0), 2))]
    totals = {"primary": [], "shadow": []}
    for ty, tx in tiles:
        rays = [scene.camera.sample(tx * 8 + i, ty * 8 + j, SIDE, SIDE)[0] for j in range(8) for i in range(8)]
        o = np.asarray([r[0] for r in rays], dtype=np.float64)
        d = np.asarray([r[1] for r in rays], dtype=np.float64)
        rec = {"tile": [ty, tx], "primary": shared(root.nodes, o, d)}
        hits = [root.intersect(r[0], r[1], float("inf")) for r in rays]
        keep = [k for k, h in enumerate(hits) if h is not None]
        if keep:
            p = np.asarray([pyref.add(rays[k][0], pyref.mul(rays[k][1], hits[k]["t"])) for k in keep], dtype=np.float64)
            rec["shadow"] = shared(root.nodes, p, light_pos - p)
        totals["primary"].append(rec["primary"])
        if "shadow" in rec:
            totals["shadow"].append(rec["shadow"])
        print(json.dumps(rec))
    for kind, rows in totals.items():
        if rows:
            mean = lambda k: sum(r[k] for r in rows) / len(rows)  # noqa: E731
            print("%-8s %4d tiles: interior per lane %.2f / max %.2f, union %.2f; leaves per lane %.2f / max %.2f, union %.2f; octants %.2f, groups %.2f (most %d); nodes in the tree %d"
                  % (kind, len(rows), mean("inner_avg"), mean("inner_max"), mean("inner_union"), mean("leaves_avg"), mean("leaves_max"), mean("leaves_union"),
                     mean("octants"), mean("groups"), max(r["groups"] for r in rows), len(root.nodes)), file=sys.stderr)


if __name__ == "__main__":
    main()
