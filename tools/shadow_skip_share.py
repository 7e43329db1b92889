#!/usr/bin/env python3
"""How much of a frame the shadow skip applies to, counted on the CPU: the share of primary hits at which every light
fails BSDF::f's `reflect` test, and the share of 8 x 8 level-0 tiles (of those with a hit at all, and of all) in which every hit does.
Primary rays from pyref's camera, hits from the CPU oracle; the predicate in numpy from the hit records (a count, not a bit-exact film).
With --gpu the rays are the product's own camera rays and the hits its ray queries' (lg_camera_rays, lg_intersect: the render's walk on the
device), in bands of 256 rows -- how a whole 4096^2 film is counted.
usage: python tools/shadow_skip_share.py [--gpu] [size | size:crop ...] >> profiles/shadow_skip_share.jsonl"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pyref  # noqa: E402
from lasgun_amd import scenes as S  # noqa: E402
from oracle_lib import oracle  # noqa: E402

ERR = 2.220446049250313e-16 * 65536.0


def predicate(rays, hits, lights):
    """(hit, skippable) per ray"""
    hit = hits["kind"] != 0
    d = rays[:, 3:]
    wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
    ng = hits["ng"]
    ng = np.where((np.einsum("ij,ij->i", ng, wo) < 0.0)[:, None], -ng, ng)  # face-forwarded, as the shading frame holds it
    p = hits["p"] + ng * ERR
    skip = np.ones(len(rays), dtype=bool)
    for pos, _, _ in lights:
        wi = np.asarray(pos) - p
        skip &= ~(np.einsum("ij,ij->i", wi, ng) * np.einsum("ij,ij->i", wo, ng) > 0.0)
    return hit, skip & hit


def tiles_row(film, window, source, hit, skip):
    size = hit.shape[0]
    t = size // 8
    tile_hits = hit.reshape(t, 8, t, 8).sum(axis=(1, 3))
    tile_skip = skip.reshape(t, 8, t, 8).sum(axis=(1, 3))
    whole = (tile_hits > 0) & (tile_skip == tile_hits)
    return {"scene": "spheres_scene (Cornell shell + 1024 plastic spheres, one point light)", "size": film, "window": window, "source": source,
            "hits": int(hit.sum()), "hits_skippable": int(skip.sum()), "share_of_hits": float(skip.sum() / hit.sum()),
            "tiles": int(t * t), "tiles_wholly_skippable": int(whole.sum()), "share_of_tiles": float(whole.sum() / (t * t)),
            "hits_in_wholly_skippable_tiles": int(tile_hits[whole].sum()), "tiles_partly_skippable": int(((tile_skip > 0) & ~whole).sum())}


def share_gpu(size):
    import lasgun_amd as la
    G = la.api
    acc = G.Accel(S.spheres_scene(G))
    lights = S.spheres_scene(pyref.Api).lights
    hit, skip = [], []
    for y0 in range(0, size, 256):
        rays = G.camera_rays(acc, size, size, 0, y0, size, min(y0 + 256, size))
        a, b = predicate(rays, G.intersect(acc, rays), lights)
        hit.append(a); skip.append(b)
    return tiles_row(size, [0, 0, size, size], "device ray queries (lg_camera_rays + lg_intersect), numpy predicate",
                     np.concatenate(hit).reshape(size, size), np.concatenate(skip).reshape(size, size))


def share(size, crop=None):  # crop: only the central crop x crop window of the size x size film (a 4096^2 film is too many rays for the Python camera)
    o = oracle()
    cam = S.spheres_scene(pyref.Api).camera
    lights = S.spheres_scene(pyref.Api).lights
    film, off = size, 0 if crop is None else (size - crop) // 2
    size = crop or size
    rays = np.array([[*od[0], *od[1]] for y in range(off, off + size) for x in range(off, off + size) for od in cam.sample(x, y, film, film)], dtype=np.float64)
    hits, _ = o.intersect(o.Accel(S.spheres_scene(o)), rays, nthreads=16)
    hit, skip = predicate(rays, hits, lights)
    return tiles_row(film, [off, off, off + size, off + size], "CPU oracle hits, numpy predicate", hit.reshape(size, size), skip.reshape(size, size))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--gpu"]:
        for arg in sys.argv[2:] or ["1024", "4096"]:
            print(json.dumps(share_gpu(int(arg))), flush=True)
    else:
        for arg in sys.argv[1:] or ["512", "1024", "4096:1024"]:  # size, or size:crop
            print(json.dumps(share(*[int(v) for v in arg.split(":")])), flush=True)
