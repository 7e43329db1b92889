#!/usr/bin/env python3
"""What a scene's rays do where they reach a nested accel, counted on the CPU with the witness (tests/pyref.py,
tests/pyref_bvh.py): entries per ray, the share of them that end in a miss at node 0, the share of THOSE that one axis already proves --
the thinnest of the node-0 box, fmax(t1, t2) <= 0, the walk's probe -- and that any of the three axes would, the share of (8 x 8 tile,
accel) pairs in which every entering lane is such a miss, and the entries of lone meshes.  Primary rays of randomly chosen 8 x 8 tiles of the
film and the shadow rays of their hits; the walks are the reference's (closest hit, no early exit).  The implication "one-axis miss => node-0
miss" is asserted on every entry.  CPU only: scenes.py is loaded by path (the package needs the built library).
usage: python tools/level_door_share.py [scene[:size[:tiles]] ...] >> profiles/level_door_share.jsonl     (default: spheres_scene:4096:3000)"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import pyref  # noqa: E402
import level_door_rays as R  # noqa: E402
from pyref import add, cross, dot, mul, neg, normalize, sub, _div, transform_point, transform_vector  # noqa: E402

_spec = importlib.util.spec_from_file_location("lasgun_scenes", os.path.join(ROOT, "lasgun_amd", "scenes.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)
if not hasattr(pyref.Camera, "set_aperture_radius"):
    pyref.Camera.set_aperture_radius = lambda self, radius: self
ERR = 2.220446049250313e-16 * 2.0 ** 16


def any_axis(door, o, d):
    """fmax(t1, t2) <= 0 on ANY axis of the whole local ray (what a three-axis probe would prove)."""
    ol, dl = transform_point(door.accel.minv, o), transform_vector(door.accel.minv, d)
    lo, hi = door.accel.nodes[0][0]
    for i in range(3):
        inv = _div(1.0, dl[i])
        if pyref.fmax((lo[i] - ol[i]) * inv, (hi[i] - ol[i]) * inv) <= 0.0:
            return True
    return False


def share(scene_name, size, tiles, seed=1):
    pscene = getattr(S, scene_name)(pyref.Api)
    root, ds = R.doors(pscene)
    lone_group = {id(g.accel) for g in ds if g.lone}
    rng = np.random.default_rng(seed)
    t = size // 8
    chosen = rng.choice(t * t, size=min(tiles, t * t), replace=False)
    kinds = {"primary": dict(rays=0, entries=0, miss0=0, one_axis=0, any_axis=0, pairs=0, pairs_all_shut=0, mesh_entries=0, lone_entries=0),
             "shadow": dict(rays=0, entries=0, miss0=0, one_axis=0, any_axis=0, pairs=0, pairs_all_shut=0, mesh_entries=0, lone_entries=0)}

    def account(kind, tile_entries):
        """tile_entries: per lane, the entries of its walk"""
        c = kinds[kind]
        pair = {}
        for lane in tile_entries:
            c["rays"] += 1
            for dr, o, d in lane:
                if dr.is_mesh:
                    c["mesh_entries"] += 1
                    c["lone_entries"] += id(dr.chain[-1]) in lone_group
                    continue
                hit0 = R.node0_hit(dr, o, d)
                s = R.probe(dr, o, d)
                assert not (s and hit0), (dr.row, dr.lo, dr.hi, o, d)
                c["entries"] += 1
                c["miss0"] += not hit0
                c["one_axis"] += s
                c["any_axis"] += (not hit0) and any_axis(dr, o, d)
                pair.setdefault(id(dr), []).append(s)
        c["pairs"] += len(pair)
        c["pairs_all_shut"] += sum(all(v) for v in pair.values())

    for tile in chosen.tolist():
        ty, tx = divmod(tile, t)
        prim, shad = [], []
        for y in range(8 * ty, 8 * ty + 8):
            for x in range(8 * tx, 8 * tx + 8):
                for o, d in pscene.camera.sample(x, y, size, size)[:1]:
                    lane = []
                    hit = R.walk_entries(root, ds, o, d, lane)
                    prim.append(lane)
                    if hit is None:
                        continue
                    ng = normalize(cross(hit["g"][0], hit["g"][1]))
                    if dot(ng, neg(normalize(d))) < 0.0:
                        ng = neg(ng)
                    p = add(add(o, mul(d, hit["t"])), mul(ng, ERR))
                    for lpos, _, _ in pscene.lights:
                        lane = []
                        R.walk_entries(root, ds, p, sub(lpos, p), lane)
                        shad.append(lane)
        account("primary", prim)
        account("shadow", shad)
    out = {"scene": scene_name, "size": size, "tiles": int(len(chosen)), "seed": seed, "source": "witness walks (tests/pyref_bvh.py), closest hit, no early exit",
           "doors": len(ds), "lone_groups": sum(d.lone for d in ds)}
    for kind, c in kinds.items():
        e, m = max(c["entries"], 1), max(c["miss0"], 1)
        out[kind] = dict(c, group_entries_per_ray=c["entries"] / max(c["rays"], 1), miss_at_node0=c["miss0"] / e, one_axis_miss=c["one_axis"] / e,
                         one_axis_of_misses=c["one_axis"] / m, any_axis_miss=c["any_axis"] / e, pairs_all_one_axis_miss=c["pairs_all_shut"] / max(c["pairs"], 1),
                         mesh_entries_per_ray=c["mesh_entries"] / max(c["rays"], 1))
    return out


if __name__ == "__main__":
    for arg in sys.argv[1:] or ["spheres_scene:4096:3000"]:
        parts = arg.split(":")
        print(json.dumps(share(parts[0], int(parts[1]) if len(parts) > 1 else 4096, int(parts[2]) if len(parts) > 2 else 3000)), flush=True)
