#!/usr/bin/env python3
"""Ray-query throughput (include/lasgun_hip.h, lg_intersect_device / lg_occluded_device) on three scenes: the headline (configs[2], 1024
spheres, LDS-resident), config 4 (the glass torus mesh, pruned walk) and config 5 (mixed).  Per scene three rows:
  (a) closest hits of the camera's 4096^2 primary rays (lg_camera_rays_device),
  (b) the same rays in a seeded random order (incoherent),
  (c) occlusion of the shadow segments to light 0 from (a)'s hits (the render's shadow origin: p + ng * 2^-36),
and, as diagnostics, (a) and (c) with the rays in the render's own order (8 x 8 pixel tiles, rows a8 / c8) and (c) in a seeded random order (cs).
--order 1 walks those rows' rays in the sorted order (lg_accel_set_query_order(1)); without it every row is measured as given (order 0) and
then again sorted (rows "... [order 1]", the key and the sort inside the timed call), and one more row times the key and the sort alone
(lg_query_order_device on (b)'s rays).
Radiance queries (lg_radiance_device) -- rows r / rs / r8: the radiance of (a)'s rays as given, in a seeded random order, and in 8 x 8 pixel
tiles, under --order 0|1 (both without it) -- beside the row they are measured against, "frame": lg_capture_rows_device of the same film at
one sample per pixel with lg_accel_set_streaming(2), the same rays through the same passes, and "hbm": lg_probe_rate(0) in GB/s.
--rows radiance measures these rows alone, --rows frame the frame row alone (any build of the library has it).
Ray films (lg_capture_rays_device) -- rows f8 / fr: the film of (a)'s rays into RGBA8, in 8 x 8 pixel tiles with their offsets and in row-major
order without, beside r8 and frame; and f9: a 1024^2 film of 9 samples per pixel (the camera's rays at supersampling 2), with the share of the
call that lg_profile_read_kinds credits to kind 1 (the combine passes and the resolve pass).  --rows film measures frame, hbm and these;
--rows takes a comma-separated list (--rows radiance,film).
Visibility matrices (lg_visibility_device) -- --rows visibility: 4096 from points (the first hits of a camera grid, in 8 x 8 tiles of the grid,
pushed out along ng by the shading offset) against 4096 to points (64 rings of 64 points on the sphere around the bounds of what the camera
sees), 16.7 M segments.  Row x8: lg_occluded_device on those segments written out as 48-byte rays in the matrix's 8 x 8 block order (the
yardstick: this row needs nothing the parent commit's library does not have, so the same file measures it there); row v8: the bit matrix
from the two point sets; row v8c: the bit matrix and the row counts.  Where both run, v8's bits are checked against x8's bytes.
Each row: rays, ms per call (device events, mean over >= 20 timed calls after warm-up), Mrays/s, device_source_sha16; --repeats R measures
everything R times (rows carry "repeat").
Feature buffers (lg_capture_features_device) -- --rows features, on the film of --size: row g8, all five planes (at most 48 bytes a pixel); row
g8d, depth + id alone (20 bytes); beside them, in the same session, the route to the same information without them: row x8c,
lg_camera_rays_device + lg_intersect_device on preallocated buffers (144 bytes a ray written, the per-pixel reduction still to do), and
the closest-hit query alone on those rays in camera order (a) and in 8 x 8 pixel tiles (a8).  With one sample a pixel g8's depth and ids
are checked against the hits.
Direction sets (lg_open_directions_device) -- --rows directions (not part of "all"): the first hits of a 1024^2 camera frame in 8 x 8 tile
order, pushed out along ng, normals ng, against 64 Fibonacci directions of length a quarter of the hit bounds' diagonal.  Row o64: the bit
matrix and both counts from the N + 64 vectors; row ox: lg_occluded_device (the parent commit's library has it) on the explicit rays of the
ABOVE pairs only, ordered as the kernel walks them (per block of 64 points, direction-major) -- the best the two-call route can do, the
rays' construction not timed; row op: the same rays point-major.  o64's bits and counts are checked against op's bytes.
Range scans (lg_range_scan_device) -- --rows scan (not part of "all"), two shapes a scene, each in both lane forms.  Shape a: the first hits
of a 1024^2 camera frame in 8 x 8 tile order, pushed out along ng, as poses without frames x 64 unit Fibonacci beams.  Shape b: 1024 poses
along the camera's view axis, each with a rotation frame (the sensor yawed about the camera's up by a full turn over the poses) x the
64 rings x 1024 azimuths of spinning_lidar_beams(-25 .. 15 degrees).  Rows s1 / s2: range, hits and nearest in beam lanes / pose lanes; rows
s1a / s2a: all six outputs.  Beside them lg_intersect_device (the parent commit's library has it) on the explicit rays of the same pairs,
their construction not timed: row sx1, pose-major, which is beam lanes' own order and the caller's natural one; row sx2, per block of 64
poses beam-major, pose lanes' own order.  Every scan's range, hits and nearest are checked against sx1's records.
Radiance gathers (lg_radiance_gather_device) -- --rows gather (not part of "all"), two shapes a scene, each in both lane forms, sums alone (li
parked).  Shape a: the first hits of a 1024^2 camera frame in 8 x 8 tile order, pushed out along ng, as poses with frames_from_normals(ng) x
the 64 cosine_directions, one weight column of 1 / 64 (a lightmap's irradiance / pi).  Shape b: 4096 probes, a 16^3 grid in the hits' bounds,
without frames x the 6144 sphere_directions with sh_weights (9 columns: an SH9 probe grid).  Rows g1 / g2: direction lanes / pose lanes.
Beside them lg_radiance_device (the parent commit's library has it) on the explicit rays of the same pairs, their construction not timed: row
gx1, pose-major, which is direction lanes' own order and the caller's natural one; row gx2, per block of 64 poses direction-major, pose
lanes' own order.  Every gather's sums are checked against the sequential sum of gx1's radiance (torch: a product and a sum a step).  Each row
carries kind1_ms, what lg_profile_read_kinds credits to kind 1 in one profiled call (the level combine passes, and for g1 / g2 the resolve);
resolve_ms = a g row's kind1_ms minus its yardstick's is the resolve's own time.  These rows time --calls calls as given (at least 3), not 20.
View batches (lg_capture_views_device) -- --rows views (not part of "all"), two shapes a scene, RGBA8 films.  Shape A: 64 orbit_views of 128 x 128
at one sample -- the scene's own eye and 63 more on the circle through it about the camera's up, looking at the camera's look point with its
field of view.  Shape B: the scene's own view at 4096 x 4096.  Row v: the batch, one call.  Beside it, both the parent commit's own
capabilities: row vk, lg_capture_subset_device(0, 1, ..) on K accels rebuilt per camera, K render chains on one stream (the K scene + accel
builds are timed apart, host wall clock: build_ms); row vx8, lg_capture_rays_device on the views' rays written out in 8 x 8-tile order through
pixel_offsets (the rays' construction not timed).  Every row's films are checked against row v's bytes.
View features (lg_capture_view_features_device) -- --rows viewfeatures (not part of "all"), two shapes a scene.  Shape A: the 64 orbit views of
--rows views at 128 x 128, one sample, depth + normal + id + point.  Row f: one call.  Beside it, the two routes the parent commit offers for the
same planes: row fi, lg_view_rays_device + lg_intersect_device per view (48 bytes a ray out, 96 bytes a hit back, no reduction counted); row fk,
lg_capture_features_device on K accels rebuilt per camera (builds timed apart, host wall clock: build_ms; there is no point there).  Every row's
planes are checked against row f's bytes where they coincide.  Shape B: the scene's own view at 4096 x 4096, all six planes (row f) against
lg_capture_features_device with the same camera (row g8, five planes), measured in alternation, `round` 0 and 1.
Hit layers (lg_hit_layers_device) -- --rows layers (not part of "all"): the camera's rays of a --size^2 film, 8 layers.  Row L8: one call, along +
id + count; row LX: the same call with inside alone (the x-ray image, 8 bytes out a ray).  Beside them the route the parent commit offers: rows
Y8 / YX, 8 rounds of lg_intersect_device with the planes pre-filled, the next origins computed and the live rays compacted by torch on the
same stream (the compaction's size comes back to the host every round: the route needs it).  Timed L8, Y8, LX, YX, so --repeats alternates
them; Y's planes are checked against L's bytes.  These rows time --calls calls as given (at least 4; the Y rows half as many), not 20.
Ray paths (lg_trace_paths_device) -- --rows paths (not part of "all"): the camera's rays of a --size^2 film, 8 bounces, glass refracts and
everything else reflects.  Row P8: one call, point + id + count + end.  Row Z8: the route without it -- 8 rounds of lg_intersect_device with
the next rays formed and the live rays compacted by torch on the same stream -- into the same planes, checked against P8's bytes.
Surface scatter (lg_scatter_device) -- --rows scatter (not part of "all"): the camera's rays of a --size^2 film.  Row R0: lg_radiance_device on the
scene rebuilt at depth 0, the floor (the same closest and shadow passes, 24 bytes a ray).  Rows S2 / S7: direct + flags / all seven planes, with
what they cost over the floor in ms and per byte written.  Row CD: li() composed to the scene's own depth over the device form with torch, against
row RD, one lg_radiance_device call (measure_scatter).
Lit scatter (lg_scatter_lit_device) -- --rows lit (not part of "all"): the camera's rays of a --size^2 film.  Row F, the floor: lg_scatter_device,
direct + flags, on the scene rebuilt with four lights.  Row L4: lg_scatter_lit_device with those four lights shared, on the scene without lights
(same_bytes: its planes against F's).  Row L64: 64 shared lights.  Rows P1 / P16: 1 and 16 lights per ray, and P1t / P16t with terms.  Row L64v:
L64 with visible asked for (every pair walked: the skip's yardstick inside one process; LASGUN_LIT_SKIP=0 turns the skip off for a whole run).
Rows M64 / MR: one light at 64 positions by 64 calls on ONE accel against 64 rebuilt accels + lg_scatter_device, on a film of at most 1024^2
(64 launch contexts of a 4096^2 chain would not fit), the rebuilds timed apart (build_ms) (measure_lit).
Hit attributes (lg_hit_attributes_device, lg_hit_attributes_of_device) -- --rows attributes (not part of "all"): the camera's rays of a --size^2 film.
Row I, the floor: lg_intersect_device.  Rows A2 / A7: the walking form with uv + bary alone / with all seven planes.  Rows O / W: the _of form on a
compacted tenth of the hits against re-walking that tenth.
Closest points (lg_closest_points_device) -- --rows closest (not part of "all"): 2^20 points of a 128 x 128 x 64 grid over 1.2 x the scene's
bounds (the root box through the root's transform), in grid order.  Row C: all three planes, radius +INF; row Cr: radius 5 % of the bounds'
diagonal.  Timed C, Cr, so --repeats alternates them.
Proximity queries (lg_nearest_device) -- --rows nearest (not part of "all"): the same 2^20 grid points.  Rows N1 / N4 / N8: k = 1, 4, 8 with
distance + id at radius 5 % of the bounds' diagonal and at +INF, each beside row F, lg_closest_points_device with distance + id at that radius
(the floor for k = 1; over_closest_points: the ratio).  Row T: touch alone at 5 %, beside row Fd, lg_closest_points_device with distance
alone; row Q: count alone at 5 %.  --calls at most 4.
Segment proximity (lg_closest_segments_device) -- --rows segments (not part of "all"): 2^20 segments (--segments N: fewer) centred on the grid
points of --rows closest, lengths 1 % and 100 % of the bounds' diagonal, radius +INF and 5 % of it.  Rows S: distance + id; St: touch alone;
N: lg_nearest_device, k = 1, on the midpoints, the yardstick.  What stage 2 of the pruning buys: build a second library in a copy of the tree with
`make -C lasgun_amd/csrc EXTRA_DEVFLAGS=-DLG_SEGMENTS_NO_STAGE2`, name it in LASGUN_HIP_LIB and run --long-only --label "stage 2 compiled out".
Light groups (lg_radiance_groups_device) -- --rows groups (not part of "all"): the camera's rays of a --size^2 film on each scene given four
point lights (the builder's one and three more, positions in the rows), G = 6 groups: base, ambient, the four lights.  Row G6: one call.
Beside it: row GK, G calls of lg_radiance_device on G accels rebuilt per group (builds timed apart: build_ms; planes compared: same_bytes);
row R1, one lg_radiance_device call on the full scene, the floor.  Timed G6, GK, R1, so --repeats alternates them; --calls calls as given (at least 3).
usage: python tools/query_rate.py [--calls 20] [--size 4096] [--repeats 1] [--order 0|1] [--rows all|queries|radiance|frame|film|visibility|features|directions|scan|gather|views|viewfeatures|layers|groups|paths|scatter|lit|attributes|nearest|closest|segments[,...]] [--segments N] [--long-only] [--label TEXT] [--out profiles/r08_query_order.jsonl]
       python tools/query_rate.py --once     (one headline frame rendered, then (a), (c) and (r8) once: for rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lasgun_amd as la  # noqa: E402
import pyref  # noqa: E402  (the scenes' light positions, built through the same scene functions)
from lasgun_amd import scenes as S  # noqa: E402

G = la.api
SCENES = [("configs[2] spheres (LDS-resident)", lambda api: S.spheres_scene(api)),
          ("config 4 glass torus (pruned walk)", lambda api: S.mesh_scene(api)),
          ("config 5 mixed", lambda api: S.mixed_scene(api))]
ERR = 2.220446049250313e-16 * 65536.0  # the shading offset (integrate.rs:40)


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def shadow_segments(hits, light):
    """(c)'s rays from (a)'s hits: origin p + ng * 2^-36 (what the shadow passes leave from, point.rs:43-44), direction light - origin."""
    f = hits.view(torch.float64).view(-1, 12)
    kind = hits.view(torch.int32).view(-1, 24)[:, 20]
    f = f[kind != 0]
    o = f[:, 1:4] + f[:, 4:7] * ERR
    d = torch.tensor(light, dtype=torch.float64, device=o.device) - o
    return torch.cat([o, d], dim=1).contiguous()


def measure(name, builder, size, calls, seed, order=None):
    scene = builder(G)
    accel = G.Accel.from_scene(scene)
    light = builder(pyref.Api).lights[0][0]
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    n = size * size * G.camera_samples(accel)
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    hits = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    shuffled = rays[torch.randperm(n, device="cuda", generator=gen)].contiguous()
    hits_b = torch.empty_like(hits)
    rows = []
    pix = torch.arange(size * size, device="cuda")
    key = ((pix // size // 8) * (size // 8) + (pix % size) // 8) * 64 + ((pix // size) % 8) * 8 + (pix % size) % 8
    tile_order = torch.argsort(key)
    del pix, key
    G.set_query_order(accel, 0)
    G.intersect_device(accel, n, rays.data_ptr(), hits.data_ptr(), stream=s)
    segs = shadow_segments(hits, light)
    occ = torch.empty((segs.shape[0],), dtype=torch.uint8, device="cuda")
    for mode in ((0, 1) if order is None else (order,)):
        G.set_query_order(accel, mode)
        tag = " [order 1]" if mode == 1 and order is None else ""
        ms = timed(lambda: G.intersect_device(accel, n, rays.data_ptr(), hits.data_ptr(), stream=s), calls)
        rows.append(("a: closest, camera order" + tag, n, ms, mode))
        ms = timed(lambda: G.intersect_device(accel, n, shuffled.data_ptr(), hits_b.data_ptr(), stream=s), calls)
        rows.append(("b: closest, random order" + tag, n, ms, mode))
        ms = timed(lambda: G.occluded_device(accel, segs.shape[0], segs.data_ptr(), occ.data_ptr(), stream=s), calls)
        rows.append(("c: occluded, shadow segments to light 0" + tag, segs.shape[0], ms, mode))
        occluded_fraction = round(float(occ.float().mean()), 4)
        segs_s = segs[torch.randperm(segs.shape[0], device="cuda", generator=gen)].contiguous()
        ms = timed(lambda: G.occluded_device(accel, segs_s.shape[0], segs_s.data_ptr(), occ.data_ptr(), stream=s), calls)
        rows.append(("cs: occluded, shadow segments in random order" + tag, segs_s.shape[0], ms, mode))
        del segs_s
        # the same rays and segments in the render's own order -- 8 x 8 pixel tiles, a tile per wave -- instead of row-major (diagnostic rows)
        if n == size * size:
            tiled = rays[tile_order].contiguous()
            ms = timed(lambda: G.intersect_device(accel, n, tiled.data_ptr(), hits_b.data_ptr(), stream=s), calls)
            rows.append(("a8: closest, 8x8 pixel tiles" + tag, n, ms, mode))
            del tiled
            segs8 = shadow_segments(hits.view(-1, 96)[tile_order].contiguous().view(-1), light)
            ms = timed(lambda: G.occluded_device(accel, segs8.shape[0], segs8.data_ptr(), occ.data_ptr(), stream=s), calls)
            rows.append(("c8: occluded, shadow segments in 8x8 pixel tiles" + tag, segs8.shape[0], ms, mode))
            del segs8
    if order is None and n < (1 << 32):
        perm = torch.empty((n,), dtype=torch.int32, device="cuda")
        ms = timed(lambda: G.query_order_device(accel, n, shuffled.data_ptr(), perm.data_ptr(), None, stream=s), calls)
        rows.append(("sort: key and sort alone, (b)'s rays", n, ms, 1))
    G.set_query_order(accel, 0)
    out = []
    for row, nr, ms, mode in rows:
        out.append({"scene": name, "row": row, "order": mode, "film": [size, size], "rays": int(nr), "ms": round(ms, 4), "mrays_per_s": round(nr / ms / 1e3, 1),
                    "calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel),
                    "occluded_fraction": occluded_fraction if row.startswith("c:") else None,
                    "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)})
    return out


def measure_radiance(name, builder, size, calls, seed, order=None, frame_only=False, film_rows=False, radiance_rows=True):
    """Rows frame / hbm / r / rs / r8 of one scene (module docstring)."""
    scene = builder(G)
    accel = G.Accel.from_scene(scene)
    s = torch.cuda.current_stream().cuda_stream
    rows = []
    G.set_streaming(accel, 2)  # the level-by-level pipeline: what a radiance query always runs as
    film = torch.empty((size * size * 4,), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: G.capture_rows_device(accel, size, size, 0, size, film.data_ptr(), stream=s), calls)
    rows.append(("frame: capture_rows_device, streaming 2", size * size, ms, 0))
    rows.append(("hbm: lg_probe_rate(0), GB/s", 0, G.probe_rate("hbm_copy"), 0))
    del film
    if not frame_only:
        assert G.camera_samples(accel) == 1
        n = size * size
        rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
        G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
        out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(seed)
        pix = torch.arange(n, device="cuda")
        key = ((pix // size // 8) * (size // 8) + (pix % size) // 8) * 64 + ((pix // size) % 8) * 8 + (pix % size) % 8
        tile_order = torch.argsort(key)
        del pix, key
        if film_rows:
            rgba = torch.empty((n * 4,), dtype=torch.uint8, device="cuda")
            for mode in ((0, 1) if order is None else (order,)):
                G.set_query_order(accel, mode)
                other = rays[tile_order].contiguous()
                ms = timed(lambda: G.capture_rays_device(accel, n, other.data_ptr(), size, size, offsets_ptr=tile_order.data_ptr(), rgba_ptr=rgba.data_ptr(), stream=s), calls)
                rows.append(("f8: ray film RGBA8, 8x8 pixel tiles with offsets", n, ms, mode))
                del other
                ms = timed(lambda: G.capture_rays_device(accel, n, rays.data_ptr(), size, size, rgba_ptr=rgba.data_ptr(), stream=s), calls)
                rows.append(("fr: ray film RGBA8, row-major", n, ms, mode))
            G.set_query_order(accel, 0)
            del rgba
            rows += film_nine_samples(builder, calls, s)
        for mode in ((0, 1) if order is None else (order,)) if radiance_rows else ():
            G.set_query_order(accel, mode)
            ms = timed(lambda: G.radiance_device(accel, n, rays.data_ptr(), out.data_ptr(), stream=s), calls)
            rows.append(("r: radiance, camera order", n, ms, mode))
            other = rays[tile_order].contiguous()
            ms = timed(lambda: G.radiance_device(accel, n, other.data_ptr(), out.data_ptr(), stream=s), calls)
            rows.append(("r8: radiance, 8x8 pixel tiles", n, ms, mode))
            other = rays[torch.randperm(n, device="cuda", generator=gen)].contiguous()
            ms = timed(lambda: G.radiance_device(accel, n, other.data_ptr(), out.data_ptr(), stream=s), calls)
            rows.append(("rs: radiance, random order", n, ms, mode))
            del other
        G.set_query_order(accel, 0)
    return [{"scene": name, "row": row, "order": mode, "film": [size, size], "rays": int(nr), "ms": round(ms, 4) if nr else None,
             "mrays_per_s": round(nr / ms / 1e3, 1) if nr else None, "gbps": None if nr else round(ms, 1), "calls": calls,
             "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)} for row, nr, ms, mode in rows]


def film_nine_samples(builder, calls, s, size=1024):
    """Row f9: a size^2 film of 9 samples per pixel, and the share of its kernels' time in kind 1 (combine + resolve passes)."""
    scene = builder(G)
    scene.camera.set_supersampling(2)
    accel = G.Accel.from_scene(scene)
    n = size * size
    rays = torch.empty((n * 9, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    rgba = torch.empty((n * 4,), dtype=torch.uint8, device="cuda")
    call = lambda: G.capture_rays_device(accel, n, rays.data_ptr(), size, size, samples=9, rgba_ptr=rgba.data_ptr(), stream=s)  # noqa: E731
    ms = timed(call, calls)
    G.profile_enable(accel, True)
    call()
    kinds = G.profile_read_kinds(accel)
    G.profile_enable(accel, False)
    total = sum(ms_k for ms_k, _ in kinds.values())
    share = kinds["combine"][0] / total if total > 0 else None
    return [("f9: ray film RGBA8, %d^2 x 9 samples (kind-1 share %s)" % (size, "%.3f" % share if share is not None else "n/a"), n * 9, ms, 0)]


def visibility_points(accel, s, n=4096):
    """(from, to): n first hits of a camera grid in 8 x 8 tiles of the grid (the grid grown from 64 x 64 until it has n hits), pushed out along
    ng; n points on the sphere around the hits' bounds, 64 equal-area rings of n / 64 points, neighbours in the array neighbours on a ring."""
    g = 64
    while True:
        rays = torch.empty((g * g, 6), dtype=torch.float64, device="cuda")
        G.camera_rays_device(accel, g, g, 0, 0, g, g, rays.data_ptr(), stream=s)
        hits = torch.empty((g * g * 96,), dtype=torch.uint8, device="cuda")
        G.intersect_device(accel, g * g, rays.data_ptr(), hits.data_ptr(), stream=s)
        pix = torch.arange(g * g, device="cuda")
        key = ((pix // g // 8) * (g // 8) + (pix % g) // 8) * 64 + ((pix // g) % 8) * 8 + (pix % g) % 8
        tiled = hits.view(-1, 96)[torch.argsort(key)].contiguous()
        f = tiled.view(torch.float64).view(-1, 12)
        f = f[tiled.view(torch.int32).view(-1, 24)[:, 20] != 0]
        if f.shape[0] >= n:
            break
        g += 8
    p = f[:, 1:4]
    lo, hi = p.min(dim=0).values, p.max(dim=0).values
    frm = (p[:n] + f[:n, 4:7] * ERR).contiguous()
    rings = 64
    k = torch.arange(n, device="cuda")
    z = 1.0 - 2.0 * ((k // (n // rings)).double() + 0.5) / rings
    phi = 2.0 * torch.pi * ((k % (n // rings)).double() + 0.5) / (n // rings)
    r = torch.sqrt(1.0 - z * z)
    to = (0.5 * (lo + hi) + 0.5 * torch.linalg.norm(hi - lo) * torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], dim=1)).contiguous()
    return frm, to, g


def measure_visibility(name, builder, calls, n=4096):
    """Rows x8 / v8 / v8c of one scene (module docstring)."""
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    frm, to, grid = visibility_points(accel, s, n)
    b = n // 8
    o = frm.view(b, 1, 8, 1, 3).expand(b, b, 8, 8, 3)
    segs = torch.cat([o, to.view(1, b, 1, 8, 3).expand(b, b, 8, 8, 3) - o], dim=4).contiguous().view(-1, 6)  # block (ti, tj), then row, then column
    del o
    occ = torch.empty((n * n,), dtype=torch.uint8, device="cuda")
    rows = []
    ms = timed(lambda: G.occluded_device(accel, n * n, segs.data_ptr(), occ.data_ptr(), stream=s), calls)
    rows.append(("x8: occluded, the matrix's segments as rays in 8x8 block order", ms, 48.0 + 1.0))
    fraction = round(float(occ.float().mean()), 4)
    del segs
    if hasattr(G, "visibility_device"):
        bits = torch.empty((n, n // 8), dtype=torch.uint8, device="cuda")
        blocked = torch.empty((n,), dtype=torch.int32, device="cuda")
        ms = timed(lambda: G.visibility_device(accel, n, frm.data_ptr(), n, to.data_ptr(), bits.data_ptr(), n // 8, None, stream=s), calls)
        rows.append(("v8: visibility, bit matrix of %d x %d points" % (n, n), ms, 2.0 * n * 24.0 / (n * n) + 0.125))
        ms = timed(lambda: G.visibility_device(accel, n, frm.data_ptr(), n, to.data_ptr(), bits.data_ptr(), n // 8, blocked.data_ptr(), stream=s), calls)
        rows.append(("v8c: visibility, bit matrix and row counts", ms, 2.0 * n * 24.0 / (n * n) + 0.125 + 4.0 / n))
        torch.cuda.synchronize()
        want = occ.view(b, b, 8, 8).permute(0, 2, 1, 3).reshape(n, b, 8).int()  # [row][byte][bit]
        want = (want << torch.arange(8, device="cuda", dtype=torch.int32)).sum(dim=2).to(torch.uint8)
        assert torch.equal(bits, want), "v8's bits are not x8's bytes"
        assert torch.equal(blocked, occ.view(b, b, 8, 8).permute(0, 2, 1, 3).reshape(n, n).sum(dim=1).int())
    return [{"scene": name, "row": row, "from": n, "to": n, "rays": n * n, "camera_grid": grid, "ms": round(ms, 4), "mrays_per_s": round(n * n / ms / 1e3, 1),
             "bytes_per_segment": round(bps, 4), "occluded_fraction": fraction, "calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2",
             "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)} for row, ms, bps in rows]


def measure_directions(name, builder, calls, size=1024, k=64):
    """Rows o64 / ox / op of one scene (module docstring)."""
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    assert G.camera_samples(accel) == 1 and size % 8 == 0
    rays = torch.empty((size * size, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    rays = rays.view(size // 8, 8, size // 8, 8, 6).permute(0, 2, 1, 3, 4).contiguous().view(-1, 6)  # 8 x 8 pixel tiles
    hits = torch.empty((size * size * 96,), dtype=torch.uint8, device="cuda")
    G.intersect_device(accel, size * size, rays.data_ptr(), hits.data_ptr(), stream=s)
    f = hits.view(torch.float64).view(-1, 12)
    f = f[hits.view(torch.int32).view(-1, 24)[:, 20] != 0]
    del rays, hits
    n = f.shape[0]
    pts, nrm = (f[:, 1:4] + f[:, 4:7] * ERR).contiguous(), f[:, 4:7].contiguous()
    lo, hi = f[:, 1:4].min(dim=0).values, f[:, 1:4].max(dim=0).values
    dirs = torch.from_numpy(la.sphere_directions(k, 0.25 * float(torch.linalg.norm(hi - lo)))).cuda()
    above = (nrm[:, None, 0] * dirs[None, :, 0] + nrm[:, None, 1] * dirs[None, :, 1]) + nrm[:, None, 2] * dirs[None, :, 2] > 0.0  # [n][k], the header's order
    nb = (n + 63) // 64
    padded = torch.zeros((nb * 64, k), dtype=torch.bool, device="cuda")
    padded[:n] = above
    b, j, l = padded.view(nb, 64, k).permute(0, 2, 1).nonzero(as_tuple=True)  # per block of 64 points, direction-major: the kernel's order
    walked = torch.cat([pts[b * 64 + l], dirs[j]], dim=1).contiguous()
    del padded, b, j, l
    i, j = above.nonzero(as_tuple=True)
    by_point = torch.cat([pts[i], dirs[j]], dim=1).contiguous()
    m = walked.shape[0]
    assert by_point.shape[0] == m
    occ = torch.empty((m,), dtype=torch.uint8, device="cuda")
    rows = []
    ms = timed(lambda: G.occluded_device(accel, m, walked.data_ptr(), occ.data_ptr(), stream=s), calls)
    rows.append(("ox: occluded, the above pairs as rays, per 64-point block direction-major", ms, m, 48.0 + 1.0))
    del walked
    ms = timed(lambda: G.occluded_device(accel, m, by_point.data_ptr(), occ.data_ptr(), stream=s), calls)
    rows.append(("op: occluded, the above pairs as rays, point-major", ms, m, 48.0 + 1.0))
    fraction = round(float(occ.float().mean()), 4)
    del by_point
    if hasattr(G, "open_directions_device"):
        bits = torch.empty((n, k // 8), dtype=torch.uint8, device="cuda")
        nopen, nabove = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
        ms = timed(lambda: G.open_directions_device(accel, n, pts.data_ptr(), nrm.data_ptr(), k, dirs.data_ptr(), bits.data_ptr(), k // 8, nopen.data_ptr(),
                                                    nabove.data_ptr(), stream=s), calls)
        rows.append(("o64: open directions, bit matrix and both counts of %d points x %d directions" % (n, k), ms, m, (2.0 * n * 24.0 + k * 24.0) / m + (k / 8 + 8.0) * n / m))
        torch.cuda.synchronize()
        opened = torch.zeros((n, k), dtype=torch.bool, device="cuda")
        opened[i, j] = occ == 0
        want = (opened.view(n, k // 8, 8).int() << torch.arange(8, device="cuda", dtype=torch.int32)).sum(dim=2).to(torch.uint8)
        assert torch.equal(bits, want), "o64's bits are not op's bytes"
        assert torch.equal(nopen, opened.sum(dim=1).int()) and torch.equal(nabove, above.sum(dim=1).int())
    return [{"scene": name, "row": row, "points": n, "dirs": k, "pairs": n * k, "rays": walked_rays, "ms": round(ms, 4), "mrays_per_s": round(walked_rays / ms / 1e3, 1),
             "bytes_per_walked_ray": round(bpr, 4), "above_fraction": round(m / (n * k), 4), "occluded_fraction_of_above": fraction, "calls": calls,
             "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
             "gpu": torch.cuda.get_device_name(0)} for row, ms, walked_rays, bpr in rows]


def scan_shapes(accel, builder, s, size=1024, k=64):
    """[(shape, poses, frames or None, beams)] of one scene, device tensors (module docstring)."""
    assert G.camera_samples(accel) == 1 and size % 8 == 0
    rays = torch.empty((size * size, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    rays = rays.view(size // 8, 8, size // 8, 8, 6).permute(0, 2, 1, 3, 4).contiguous().view(-1, 6)  # 8 x 8 pixel tiles
    hits = torch.empty((size * size * 96,), dtype=torch.uint8, device="cuda")
    G.intersect_device(accel, size * size, rays.data_ptr(), hits.data_ptr(), stream=s)
    f = hits.view(torch.float64).view(-1, 12)
    f = f[hits.view(torch.int32).view(-1, 24)[:, 20] != 0]
    shape_a = ("a", (f[:, 1:4] + f[:, 4:7] * ERR).contiguous(), None, torch.from_numpy(la.sphere_directions(k, 1.0)).cuda())
    del rays, hits, f
    cam = builder(pyref.Api).camera
    eye, view, up, aux = (torch.tensor(v, dtype=torch.float64, device="cuda") for v in (cam.origin, cam.view, cam.up, cam.aux))
    n = 1024
    poses = (eye[None, :] + torch.linspace(0.0, 1.0, n, dtype=torch.float64, device="cuda")[:, None] * view[None, :]).contiguous()
    yaw = torch.arange(n, dtype=torch.float64, device="cuda") * (2.0 * torch.pi / n)
    fwd, left = view / torch.linalg.norm(view), -aux
    x = torch.cos(yaw)[:, None] * fwd + torch.sin(yaw)[:, None] * left   # the sensor's axes in world space: the columns of M
    y = -torch.sin(yaw)[:, None] * fwd + torch.cos(yaw)[:, None] * left
    frames = torch.stack([x, y, up[None, :].expand(n, 3)], dim=2).contiguous().view(n, 9)  # row-major: M[c][axis]
    return [shape_a, ("b", poses, frames, torch.from_numpy(la.spinning_lidar_beams(64, 1024, -25.0, 15.0)).cuda())]


def measure_scan(name, builder, calls):
    """Rows sx1 / sx2 / s1 / s2 / s1a / s2a of one scene, per shape (module docstring)."""
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    out = []
    for shape, poses, frames, beams in scan_shapes(accel, builder, s):
        n, k = poses.shape[0], beams.shape[0]
        if frames is None:
            d = beams[None, :, :].expand(n, k, 3)
        else:  # the header's expression: three products, two sums in the stated order (separate kernels: nothing fused)
            M = frames.view(n, 1, 9)
            d = torch.stack([(M[..., 3 * c] * beams[None, :, 0] + M[..., 3 * c + 1] * beams[None, :, 1]) + M[..., 3 * c + 2] * beams[None, :, 2] for c in range(3)], dim=2)
        by_pose = torch.cat([poses[:, None, :].expand(n, k, 3), d], dim=2).contiguous().view(-1, 6)
        del d
        nb = (n + 63) // 64
        pi = (torch.arange(nb, device="cuda")[:, None, None] * 64 + torch.arange(64, device="cuda")[None, None, :]).expand(nb, k, 64)
        valid = pi < n
        src = (pi * k + torch.arange(k, device="cuda")[None, :, None])[valid]  # per block of 64 poses, beam-major: pose lanes' own order
        by_block = by_pose[src].contiguous()
        del pi, valid, src
        m = n * k
        hits = torch.empty((m * 96,), dtype=torch.uint8, device="cuda")
        rows = []
        ms = timed(lambda: G.intersect_device(accel, m, by_block.data_ptr(), hits.data_ptr(), stream=s), calls)
        rows.append(("sx2: closest, the pairs as rays, per 64-pose block beam-major (pose lanes' own order)", ms, 144.0))
        del by_block
        ms = timed(lambda: G.intersect_device(accel, m, by_pose.data_ptr(), hits.data_ptr(), stream=s), calls)
        rows.append(("sx1: closest, the pairs as rays, pose-major (beam lanes' own order)", ms, 144.0))
        del by_pose
        torch.cuda.synchronize()
        kind = hits.view(torch.int32).view(-1, 24)[:, 20].view(n, k)
        want_range = hits.view(torch.float64).view(-1, 12)[:, 0].float().view(n, k)
        want_hits = (kind != 0).sum(dim=1).int()
        bits = want_range.view(torch.int32)
        want_nearest = torch.where((kind != 0) & (bits >= 0), bits, torch.full_like(bits, 0x7F800000)).min(dim=1).values.clamp(max=0x7F800000)  # (a NaN range never wins)
        fraction = round(float((kind != 0).float().mean()), 4)
        del hits
        if hasattr(G, "range_scan_device"):
            rng = torch.empty((n, k), dtype=torch.float32, device="cuda")
            nhit, near = torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.float32, device="cuda")
            point, normal = (torch.empty((n, k, 3), dtype=torch.float32, device="cuda") for _ in range(2))
            ident = torch.empty((n, k, 4), dtype=torch.int32, device="cuda")
            fp = frames.data_ptr() if frames is not None else None
            inputs = (n * (24.0 + (72.0 if frames is not None else 0.0)) + k * 24.0) / m
            for lanes in (1, 2):
                form = "beam lanes" if lanes == 1 else "pose lanes"
                ms = timed(lambda: G.range_scan_device(accel, n, poses.data_ptr(), fp, k, beams.data_ptr(), range_ptr=rng.data_ptr(), hits_ptr=nhit.data_ptr(),
                                                       nearest_ptr=near.data_ptr(), lanes=lanes, stream=s), calls)
                rows.append(("s%d: range scan, %s, range + hits + nearest" % (lanes, form), ms, inputs + 4.0 + 8.0 / k))
                torch.cuda.synchronize()
                assert torch.equal(rng.view(torch.int32), bits), "the scan's range is not sx1's t"
                assert torch.equal(nhit, want_hits) and torch.equal(near.view(torch.int32), want_nearest), "the scan's reductions are not sx1's"
                ms = timed(lambda: G.range_scan_device(accel, n, poses.data_ptr(), fp, k, beams.data_ptr(), rng.data_ptr(), point.data_ptr(), normal.data_ptr(),
                                                       ident.data_ptr(), nhit.data_ptr(), near.data_ptr(), lanes=lanes, stream=s), calls)
                rows.append(("s%da: range scan, %s, all six outputs" % (lanes, form), ms, inputs + 44.0 + 8.0 / k))
                torch.cuda.synchronize()
                assert torch.equal(ident[..., 0], kind), "the scan's ids are not sx1's"
            del rng, point, normal, ident
        out += [{"scene": name, "shape": shape, "row": row, "poses": n, "beams": k, "frames": frames is not None, "rays": m, "ms": round(ms, 4),
                 "mrays_per_s": round(m / ms / 1e3, 1), "bytes_per_pair": round(bpp, 4), "hit_fraction": fraction,
                 "auto_lanes": G.range_scan_lanes(n, k) if hasattr(G, "range_scan_lanes") else None, "calls": calls,
                 "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
                 "gpu": torch.cuda.get_device_name(0)} for row, ms, bpp in rows]
        del want_range, bits, kind
    return out


def gather_shapes(accel, s, size=1024):
    """[(shape, poses, frames or None, dirs, weights)] of one scene, device tensors (module docstring)."""
    assert G.camera_samples(accel) == 1 and size % 8 == 0
    rays = torch.empty((size * size, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    rays = rays.view(size // 8, 8, size // 8, 8, 6).permute(0, 2, 1, 3, 4).contiguous().view(-1, 6)  # 8 x 8 pixel tiles
    hits = torch.empty((size * size * 96,), dtype=torch.uint8, device="cuda")
    G.intersect_device(accel, size * size, rays.data_ptr(), hits.data_ptr(), stream=s)
    f = hits.view(torch.float64).view(-1, 12)
    f = f[hits.view(torch.int32).view(-1, 24)[:, 20] != 0]
    p, ng = f[:, 1:4], f[:, 4:7]
    lo, hi = p.min(dim=0).values, p.max(dim=0).values
    frames = torch.from_numpy(la.frames_from_normals(ng.cpu().numpy())).cuda().view(-1, 9).contiguous()
    shape_a = ("a", (p + ng * ERR).contiguous(), frames, torch.from_numpy(la.cosine_directions(64)).cuda(), torch.full((64, 1), 1.0 / 64.0, dtype=torch.float64, device="cuda"))
    t = (torch.arange(16, dtype=torch.float64, device="cuda") + 0.5) / 16.0
    grid = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), dim=3).view(-1, 3)
    dirs = la.sphere_directions(6144)
    shape_b = ("b", (lo + grid * (hi - lo)).contiguous(), None, torch.from_numpy(dirs).cuda(), torch.from_numpy(la.sh_weights(dirs)).cuda())
    return [shape_a, shape_b]


def measure_gather(name, builder, calls):
    """Rows gx1 / gx2 / g1 / g2 of one scene, per shape (module docstring)."""
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    calls = max(calls, 3)

    def kind1(fn):
        G.profile_enable(accel, True)
        fn()
        torch.cuda.synchronize()
        kinds = G.profile_read_kinds(accel)
        G.profile_enable(accel, False)
        return kinds["combine"][0]

    out = []
    for shape, poses, frames, dirs, weights in gather_shapes(accel, s):
        n, k, c = poses.shape[0], dirs.shape[0], weights.shape[1]
        if frames is None:
            d = dirs[None, :, :].expand(n, k, 3)
        else:  # the header's expression: three products, two sums in the stated order (separate kernels: nothing fused)
            M = frames.view(n, 1, 9)
            d = torch.stack([(M[..., 3 * a] * dirs[None, :, 0] + M[..., 3 * a + 1] * dirs[None, :, 1]) + M[..., 3 * a + 2] * dirs[None, :, 2] for a in range(3)], dim=2)
        by_pose = torch.cat([poses[:, None, :].expand(n, k, 3), d], dim=2).contiguous().view(-1, 6)
        del d
        nb = (n + 63) // 64
        pi = (torch.arange(nb, device="cuda")[:, None, None] * 64 + torch.arange(64, device="cuda")[None, None, :]).expand(nb, k, 64)
        src = (pi * k + torch.arange(k, device="cuda")[None, :, None])[pi < n]  # per block of 64 poses, direction-major: pose lanes' own order
        by_block = by_pose[src].contiguous()
        del pi, src
        m = n * k
        rad = torch.empty((m, 3), dtype=torch.float64, device="cuda")
        rows = []
        call = lambda: G.radiance_device(accel, m, by_block.data_ptr(), rad.data_ptr(), stream=s)  # noqa: E731
        rows.append(("gx2: radiance, the pairs as rays, per 64-pose block direction-major (pose lanes' own order)", timed(call, calls, 2), kind1(call), 72.0))
        del by_block
        call = lambda: G.radiance_device(accel, m, by_pose.data_ptr(), rad.data_ptr(), stream=s)  # noqa: E731
        rows.append(("gx1: radiance, the pairs as rays, pose-major (direction lanes' own order)", timed(call, calls, 2), kind1(call), 72.0))
        del by_pose
        torch.cuda.synchronize()
        L = rad.view(n, k, 3)
        want = torch.zeros((n, c, 3), dtype=torch.float64, device="cuda")
        for j in range(k):  # the contract's sum: one product, one sum a step, in order
            want = want + L[:, j, None, :] * weights[j, :, None]
        del rad, L
        if hasattr(G, "radiance_gather_device"):
            sums = torch.empty((n, c, 3), dtype=torch.float64, device="cuda")
            fp = frames.data_ptr() if frames is not None else None
            bpp = (n * (24.0 + (72.0 if frames is not None else 0.0)) + k * 24.0 + k * c * 8.0 + n * c * 24.0) / m
            for lanes in (1, 2):
                call = lambda: G.radiance_gather_device(accel, n, poses.data_ptr(), fp, k, dirs.data_ptr(), weights.data_ptr(), c, sums_ptr=sums.data_ptr(),  # noqa: E731
                                                        lanes=lanes, stream=s)
                sums.fill_(float("nan"))
                ms = timed(call, calls, 2)
                rows.append(("g%d: radiance gather, %s, sums" % (lanes, "direction lanes" if lanes == 1 else "pose lanes"), ms, kind1(call), bpp))
                torch.cuda.synchronize()
                assert torch.equal(sums.view(torch.int64), want.view(torch.int64)), "the gather's sums are not the sequential sum of gx1's radiance"
            del sums
        yard = {"g1": rows[1][2], "g2": rows[0][2]}
        out += [{"scene": name, "shape": shape, "row": row, "poses": n, "dirs": k, "weights": c, "frames": frames is not None, "rays": m, "ms": round(ms, 4),
                 "mrays_per_s": round(m / ms / 1e3, 1), "bytes_per_pair": round(bpp, 4), "kind1_ms": round(k1, 4),
                 "resolve_ms": round(k1 - yard[row[:2]], 4) if row[:2] in yard else None,
                 "auto_lanes": G.radiance_gather_lanes(n, k) if hasattr(G, "radiance_gather_lanes") else None, "calls": calls,
                 "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
                 "gpu": torch.cuda.get_device_name(0)} for row, ms, k1, bpp in rows]
        del want
    return out


_VIEW_ACCELS = {}  # scene name -> (the K rebuilt accels of shape A, their build's wall-clock ms): built once, whatever --repeats says


def measure_views(name, builder, calls):
    """Rows v / vk / vx8 of one scene in both shapes (module docstring)."""
    import math
    import numpy as np
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    own = G.accel_view(accel)
    eye, view, up = (np.array(v[:]) for v in (own.origin, own.view, own.up))
    center, radius = eye + view, float(np.linalg.norm(view))
    fov = math.degrees(2.0 * math.atan(own.image_plane_height / (2.0 * radius)))
    K = 64
    orbit = [la.view_look_at(eye, center, up, fov=fov)] + la.orbit_views(center, radius, 0.0, K, fov, up=up)[1:]
    if name not in _VIEW_ACCELS:
        t0 = time.time()
        accels = []
        for v in orbit:
            scene = builder(G)
            scene.set_perspective_camera(fov).look_at(list(v.origin[:]), list(center), list(up))
            accels.append(G.Accel.from_scene(scene))
        _VIEW_ACCELS[name] = (accels, (time.time() - t0) * 1e3)
    rebuilt, build_ms = _VIEW_ACCELS[name]
    out = []
    for shape, views, w, h, chain in (("A: 64 orbit views x 128 x 128", orbit, 128, 128, rebuilt), ("B: 1 view x 4096 x 4096", [own], 4096, 4096, [accel])):
        k, npix = len(views), w * h
        S_ = int(views[0].samples_root) ** 2
        films = torch.zeros((k * npix * 4,), dtype=torch.uint8, device="cuda")
        rows = []
        call = lambda: G.capture_views_device(accel, views, w, h, rgba_ptr=films.data_ptr(), stream=s)  # noqa: E731
        rows.append(("v: view batch, one call", timed(call, calls, 2), None))
        torch.cuda.synchronize()
        want = films.clone()
        # K render chains on K accels rebuilt per camera (the organisation each accel's own choice picks)
        call = lambda: [G.capture_subset_device(0, 1, a, w, h, films.data_ptr() + 4 * npix * i, stream=s) for i, a in enumerate(chain)]  # noqa: E731
        films.zero_()
        ms = timed(call, calls, 8)
        torch.cuda.synchronize()
        same = bool(torch.equal(films, want))
        orgs = sorted({str(G.last_organisation(a)) for a in chain})
        rows.append(("vk: lg_capture_subset_device on K rebuilt accels, K render chains", ms, {"build_ms": round(build_ms, 1) if k > 1 else None, "organisations": orgs,
                                                                                           "same_bytes": same}))
        # the views' rays written out in 8 x 8-tile order, one ray film over the K films stacked
        n = k * npix * S_
        rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
        for i, v in enumerate(views):
            G.view_rays_device(accel, v, w, h, 0, 0, w, h, rays.data_ptr() + 48 * npix * S_ * i, stream=s)
        tiles = torch.from_numpy(la.tile_order_offsets(w, h).view(np.int64)).cuda()
        offs = (torch.arange(k, device="cuda")[:, None] * npix + tiles[None, :]).contiguous().view(-1)
        tiled = rays.view(k * npix, S_, 6)[offs].contiguous().view(n, 6)
        del rays
        films.zero_()
        call = lambda: G.capture_rays_device(accel, k * npix, tiled.data_ptr(), w, h * k, samples=S_, offsets_ptr=offs.data_ptr(), rgba_ptr=films.data_ptr(), stream=s)  # noqa: E731
        ms = timed(call, calls, 2)
        torch.cuda.synchronize()
        rows.append(("vx8: lg_capture_rays_device on the views' rays in 8x8-tile order with pixel_offsets", ms, {"same_bytes": bool(torch.equal(films, want))}))
        del tiled, offs, films, want
        out += [{"scene": name, "shape": shape, "row": row, "views": k, "film": [w, h], "samples": S_, "rays": n, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1),
                 **(extra or {}), "calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel),
                 "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)} for row, ms, extra in rows]
    return out


def measure_view_features(name, builder, calls):
    """Rows f / fi / fk of shape A and f / g8 of shape B for one scene (module docstring)."""
    import math
    import numpy as np
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    own = G.accel_view(accel)
    assert own.samples_root == 1, "the shapes are one sample a pixel"
    eye, view, up = (np.array(v[:]) for v in (own.origin, own.view, own.up))
    center, radius = eye + view, float(np.linalg.norm(view))
    fov = math.degrees(2.0 * math.atan(own.image_plane_height / (2.0 * radius)))
    K = 64
    orbit = [la.view_look_at(eye, center, up, fov=fov)] + la.orbit_views(center, radius, 0.0, K, fov, up=up)[1:]
    if name not in _VIEW_ACCELS:
        t0 = time.time()
        accels = []
        for v in orbit:
            scene = builder(G)
            scene.set_perspective_camera(fov).look_at(list(v.origin[:]), list(center), list(up))
            accels.append(G.Accel.from_scene(scene))
        _VIEW_ACCELS[name] = (accels, (time.time() - t0) * 1e3)
    rebuilt, build_ms = _VIEW_ACCELS[name]
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    common = {"calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
              "gpu": torch.cuda.get_device_name(0)}
    out = []
    # ---- shape A
    w = h = 128
    npix, n = w * h, K * w * h
    depth, normal, point, ident = f32(n), f32(n, 3), f32(n, 3), torch.empty((n, 4), dtype=torch.int32, device="cuda")
    call = lambda: G.capture_view_features_device(accel, orbit, w, h, depth_ptr=depth.data_ptr(), normal_ptr=normal.data_ptr(), id_ptr=ident.data_ptr(),  # noqa: E731
                                                  point_ptr=point.data_ptr(), stream=s)
    rows = [("f: view features, depth + normal + id + point, one call", timed(call, calls, 2), 44.0, None)]
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    hits = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
    call = lambda: [(G.view_rays_device(accel, v, w, h, 0, 0, w, h, rays.data_ptr() + 48 * npix * i, stream=s),  # noqa: E731
                     G.intersect_device(accel, npix, rays.data_ptr() + 48 * npix * i, hits.data_ptr() + 96 * npix * i, stream=s)) for i, v in enumerate(orbit)]
    ms = timed(call, calls, 2)
    torch.cuda.synchronize()
    hf, hi = hits.view(torch.float64).view(-1, 12), hits.view(torch.int32).view(-1, 24)
    hit = hi[:, 20] != 0
    same = bool(torch.equal(ident, hi[:, 20:24])) and bool(torch.equal(depth, hf[:, 0].float())) and bool(torch.equal(normal, hf[:, 7:10].float())) \
        and bool(torch.equal(point, torch.where(hit[:, None], hf[:, 1:4].float(), torch.zeros_like(point))))
    rows.append(("fi: lg_view_rays_device + lg_intersect_device per view (no reduction)", ms, 144.0, {"same_bytes": same, "hit_share": round(float(hit.float().mean()), 4)}))
    del rays, hits, hf, hi
    depth2, normal2, ident2 = torch.empty_like(depth), torch.empty_like(normal), torch.empty_like(ident)
    call = lambda: [G.capture_features_device(a, w, h, None, depth_ptr=depth2.data_ptr() + 4 * npix * i, normal_ptr=normal2.data_ptr() + 12 * npix * i,  # noqa: E731
                                              id_ptr=ident2.data_ptr() + 16 * npix * i, stream=s) for i, a in enumerate(rebuilt)]
    ms = timed(call, calls, 2)
    torch.cuda.synchronize()
    same = bool(torch.equal(depth, depth2)) and bool(torch.equal(normal, normal2)) and bool(torch.equal(ident, ident2))
    rows.append(("fk: lg_capture_features_device on K rebuilt accels (depth + normal + id: no point there)", ms, 32.0, {"build_ms": round(build_ms, 1), "same_bytes": same}))
    out += [{"scene": name, "shape": "A: 64 orbit views x 128 x 128", "row": row, "views": K, "film": [w, h], "samples": 1, "rays": n, "ms": round(ms, 4),
             "mrays_per_s": round(n / ms / 1e3, 1), "bytes_per_pixel": bpp, **(extra or {}), **common} for row, ms, bpp, extra in rows]
    del depth, normal, point, ident, depth2, normal2, ident2
    # ---- shape B: the same camera through both entry points, in alternation
    w = h = 4096
    n = w * h
    table = torch.from_numpy(G.default_albedo_table(accel)).cuda()
    a, b = [(f32(n), f32(n, 3), f32(n, 3), f32(n), torch.empty((n, 4), dtype=torch.int32, device="cuda")) for _ in range(2)]
    point = f32(n, 3)
    views_call = lambda: G.capture_view_features_device(accel, [own], w, h, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(),  # noqa: E731
                                                        point.data_ptr(), table.data_ptr(), stream=s)
    own_call = lambda: G.capture_features_device(accel, w, h, None, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr(),  # noqa: E731
                                                 table.data_ptr(), stream=s)
    rows = []
    for rnd in range(2):
        rows.append(("f: view features, all six planes", timed(views_call, calls, 2), 60.0, rnd))
        rows.append(("g8: lg_capture_features_device, all five planes", timed(own_call, calls, 2), 48.0, rnd))
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
    out += [{"scene": name, "shape": "B: 1 view x 4096 x 4096", "row": row, "views": 1, "film": [w, h], "samples": 1, "rays": n, "ms": round(ms, 4),
             "mrays_per_s": round(n / ms / 1e3, 1), "bytes_per_pixel": bpp, "round": rnd, "same_bytes": same, **common} for row, ms, bpp, rnd in rows]
    return out


def measure_features(name, builder, size, calls):
    """Rows a / a8 / x8c / g8 / g8d of one scene (module docstring)."""
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    S_ = G.camera_samples(accel)
    npix = size * size
    n = npix * S_
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    hits = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
    rows = []
    ms = timed(lambda: (G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s),
                        G.intersect_device(accel, n, rays.data_ptr(), hits.data_ptr(), stream=s)), calls)
    rows.append(("x8c: camera rays + closest on preallocated buffers (the two-call route, no reduction)", ms, 144.0 * S_))
    ms = timed(lambda: G.intersect_device(accel, n, rays.data_ptr(), hits.data_ptr(), stream=s), calls)
    rows.append(("a: closest, camera order", ms, 144.0 * S_))
    if S_ == 1 and size % 8 == 0:
        tiled = rays.view(size // 8, 8, size // 8, 8, 6).permute(0, 2, 1, 3, 4).contiguous().view(n, 6)
        hits_b = torch.empty_like(hits)
        ms = timed(lambda: G.intersect_device(accel, n, tiled.data_ptr(), hits_b.data_ptr(), stream=s), calls)
        rows.append(("a8: closest, 8x8 pixel tiles", ms, 144.0 * S_))
        del tiled, hits_b
    if hasattr(G, "capture_features_device"):
        depth, coverage = (torch.empty((npix,), dtype=torch.float32, device="cuda") for _ in range(2))
        normal, albedo = (torch.empty((npix, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        ident = torch.empty((npix, 4), dtype=torch.int32, device="cuda")
        table = torch.from_numpy(G.default_albedo_table(accel)).cuda()
        ms = timed(lambda: G.capture_features_device(accel, size, size, None, depth.data_ptr(), normal.data_ptr(), albedo.data_ptr(), coverage.data_ptr(),
                                                     ident.data_ptr(), table.data_ptr(), stream=s), calls)
        rows.append(("g8: features, all five planes", ms, 48.0))
        depth2, ident2 = torch.empty_like(depth), torch.empty_like(ident)
        ms = timed(lambda: G.capture_features_device(accel, size, size, None, depth_ptr=depth2.data_ptr(), id_ptr=ident2.data_ptr(), stream=s), calls)
        rows.append(("g8d: features, depth + id", ms, 20.0))
        torch.cuda.synchronize()
        assert torch.equal(depth, depth2) and torch.equal(ident, ident2), "g8d's planes are not g8's"
        if S_ == 1:  # one sample: depth is (float)t and id the hit's last 16 bytes
            assert torch.equal(ident, hits.view(torch.int32).view(-1, 24)[:, 20:24]), "g8's ids are not lg_intersect's"
            assert torch.equal(depth, hits.view(torch.float64).view(-1, 12)[:, 0].float()), "g8's depth is not lg_intersect's t"
    return [{"scene": name, "row": row, "film": [size, size], "samples": S_, "rays": n, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1),
             "bytes_per_pixel": bpp, "calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel),
             "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)} for row, ms, bpp in rows]


def measure_layers(name, builder, size, calls, K=8):
    """Hit layers on the camera's rays of a size^2 film, K layers.  Row L8: one lg_hit_layers_device call, along + id + count; row LX: the same
    call with inside alone.  Rows Y8 / YX: the route without it -- K rounds of lg_intersect_device, the planes pre-filled, the next origins
    (p - ng * 2^-36) computed and the live rays compacted by torch on the same stream -- into the same planes.  L8 / Y8 / LX / YX are timed
    in that order, so a repeat alternates them; Y's planes are checked against L's bytes."""
    if not hasattr(G, "hit_layers_device"):
        return []
    scene = builder(G)
    accel = G.Accel.from_scene(scene)
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    n = size * size * G.camera_samples(accel)
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    inf = float("inf")
    miss = torch.tensor([0, -1, -1, -1], dtype=torch.int32, device="cuda")

    def planes():
        return (torch.empty((K, n), dtype=torch.float64, device="cuda"), torch.empty((K, n, 4), dtype=torch.int32, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.float64, device="cuda"))

    along, ident, count, inside = planes()
    y_along, y_ident, y_count, y_inside = planes()
    hits = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
    rounds = []

    def loop(xray):
        """The caller's own loop: lg_intersect_device, read the records, move the origins, compact; K times over."""
        if xray:
            y_inside.zero_()
        else:
            y_along.fill_(inf)
            y_ident[:] = miss
            y_count.zero_()
        cur, live, T = rays, None, None
        rounds.clear()
        for j in range(K):
            m = cur.shape[0]
            if m == 0:
                break
            rounds.append(m)
            G.intersect_device(accel, m, cur.data_ptr(), hits.data_ptr(), stream=s)
            h64, h32 = hits.view(torch.float64)[:m * 12].view(m, 12), hits.view(torch.int32)[:m * 24].view(m, 24)
            hit = h32[:, 20] != 0
            on = hit.nonzero().squeeze(1)  # (the compaction: its size comes back to the host)
            idx = on if live is None else live[on]
            t = h64[on, 0]
            if xray:
                if j & 1:
                    y_inside[idx] += t
            else:
                T = t if T is None else T[on] + t
                y_along[j, idx] = T
                y_ident[j, idx] = h32[on, 20:24]
                y_count[idx] += 1
            nxt = cur[on]
            nxt[:, :3] = h64[on, 1:4] - h64[on, 4:7] * ERR
            cur, live = nxt, idx

    rows = []
    ms = timed(lambda: G.hit_layers_device(accel, n, rays.data_ptr(), K, along_ptr=along.data_ptr(), id_ptr=ident.data_ptr(), count_ptr=count.data_ptr(), stream=s), calls, warmup=1)
    rows.append(("L8: hit layers, one call, along + id + count", ms, K * 24.0 + 4.0, None))
    ms = timed(lambda: loop(False), max(calls // 2, 2), warmup=1)
    rows.append(("Y8: K rounds of lg_intersect_device + torch moves and compaction, along + id + count", ms, K * 24.0 + 4.0, list(rounds)))
    torch.cuda.synchronize()
    assert torch.equal(along.view(torch.int64), y_along.view(torch.int64)) and torch.equal(ident, y_ident) and torch.equal(count, y_count), "Y8's planes are not L8's"
    ms = timed(lambda: G.hit_layers_device(accel, n, rays.data_ptr(), K, inside_ptr=inside.data_ptr(), stream=s), calls, warmup=1)
    rows.append(("LX: hit layers, one call, inside alone", ms, 8.0, None))
    ms = timed(lambda: loop(True), max(calls // 2, 2), warmup=1)
    rows.append(("YX: K rounds of lg_intersect_device + torch moves and compaction, inside alone", ms, 8.0, list(rounds)))
    torch.cuda.synchronize()
    assert torch.equal(inside.view(torch.int64), y_inside.view(torch.int64)), "YX's inside is not LX's"
    cnt = count.cpu()
    return [{"scene": name, "row": row, "film": [size, size], "rays": n, "max_layers": K, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1),
             "bytes_out_per_ray": bpr, "rounds": rnd, "count_hist": torch.bincount(cnt, minlength=K + 1).tolist(), "calls": calls,
             "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
             "gpu": torch.cuda.get_device_name(0)} for row, ms, bpr, rnd in rows]


def measure_paths(name, builder, size, calls, K=8):
    """Ray paths on the camera's rays of a size^2 film, K bounces, the table "glass refracts, everything else reflects", the geometric
    normal.  Row P8: one lg_trace_paths_device call, point + id + count + end.  Row Z8: the route without it -- K rounds of
    lg_intersect_device, the planes pre-filled, the next rays formed (the header's arithmetic, one torch operation per f64 operation) and
    the live rays compacted by torch on the same stream -- into the same planes.  P8 / Z8 are timed in that order, so a repeat alternates
    them; Z's planes are checked against P's bytes."""
    if not hasattr(G, "trace_paths_device"):
        return []
    scene = builder(G)
    accel = G.Accel.from_scene(scene)
    s = torch.cuda.current_stream().cuda_stream
    G.set_query_order(accel, 0)
    n = size * size * G.camera_samples(accel)
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    rules = la.path_rules(accel, default=la.PATH_REFLECT)
    t_refract = torch.from_numpy((rules["action"] == la.PATH_REFRACT)).cuda()
    t_ior = torch.from_numpy(rules["ior"].copy()).cuda()
    miss = torch.tensor([0, -1, -1, -1], dtype=torch.int32, device="cuda")

    def planes():
        return (torch.empty((K, n, 3), dtype=torch.float64, device="cuda"), torch.empty((K, n, 4), dtype=torch.int32, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda"))

    point, ident, count, end = planes()
    z_point, z_ident, z_count, z_end = planes()
    hits = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
    medium = torch.empty((n,), dtype=torch.bool, device="cuda")
    rounds = []
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # noqa: E731
    col = lambda v: v[:, None]  # noqa: E731

    def loop():
        """The caller's own loop: lg_intersect_device, read the records, reflect or refract, compact; K times over."""
        z_point.zero_()
        z_ident[:] = miss
        z_count.zero_()
        z_end.zero_()  # LG_PATH_END_CUT: what a ray alive after K rounds keeps
        medium.zero_()
        cur, live = rays, None
        rounds.clear()
        for j in range(K):
            m = cur.shape[0]
            if m == 0:
                break
            rounds.append(m)
            G.intersect_device(accel, m, cur.data_ptr(), hits.data_ptr(), stream=s)
            h64, h32 = hits.view(torch.float64)[:m * 12].view(m, 12), hits.view(torch.int32)[:m * 24].view(m, 24)
            hit = h32[:, 20] != 0
            on = hit.nonzero().squeeze(1)  # (the compaction: its size comes back to the host)
            off = (~hit).nonzero().squeeze(1)
            idx = on if live is None else live[on]
            z_end[off if live is None else live[off]] = 1  # LG_PATH_END_ESCAPED
            p, ng, d = h64[on, 1:4], h64[on, 4:7], cur[on, 3:]
            z_point[j, idx] = p
            z_ident[j, idx] = h32[on, 20:24]
            z_count[idx] += 1
            mat = h32[on, 23].long()
            sdn = dot(d, ng)
            flip = sdn > 0.0
            N, sdn = torch.where(col(flip), -ng, ng), torch.where(flip, -sdn, sdn)
            step = ng * ERR
            mirrored = d - col(2.0 * sdn) * N
            L = torch.sqrt(dot(d, d))
            u = d * col(1.0 / L)
            ci = -dot(u, N)
            med = medium[idx]
            eta = torch.where(med, t_ior[mat], 1.0 / t_ior[mat])
            sin2 = (eta * eta) * torch.fmax(1.0 - ci * ci, torch.zeros_like(ci))
            refracts = t_refract[mat] & ~(sin2 >= 1.0)
            a = eta * ci - torch.sqrt(1.0 - sin2)
            refracted = (col(eta) * u + col(a) * N) * col(L)
            nxt = torch.cat([torch.where(col(refracts), p - step, p + step), torch.where(col(refracts), refracted, mirrored)], dim=1)
            medium[idx] = med ^ refracts
            fin = torch.isfinite(nxt).all(dim=1)
            z_end[idx[~fin]] = 3  # LG_PATH_END_DEGENERATE
            keep = fin.nonzero().squeeze(1)
            cur, live = nxt[keep], idx[keep]

    rows = []
    ms = timed(lambda: G.trace_paths_device(accel, n, rays.data_ptr(), K, rules, 0, point_ptr=point.data_ptr(), id_ptr=ident.data_ptr(), count_ptr=count.data_ptr(),
                                            end_ptr=end.data_ptr(), stream=s), calls, warmup=1)
    rows.append(("P8: ray paths, one call, point + id + count + end", ms, None))
    ms = timed(loop, max(calls // 2, 2), warmup=1)
    rows.append(("Z8: K rounds of lg_intersect_device + torch bounces and compaction, point + id + count + end", ms, list(rounds)))
    torch.cuda.synchronize()
    same = {"point": torch.equal(point.view(torch.int64), z_point.view(torch.int64)), "id": torch.equal(ident, z_ident), "count": torch.equal(count, z_count),
            "end": torch.equal(end, z_end)}
    assert all(same.values()), ("Z8's planes are not P8's", same)
    return [{"scene": name, "row": row, "film": [size, size], "rays": n, "max_bounces": K, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1),
             "bytes_out_per_ray": K * 40.0 + 8.0, "rounds": rnd, "count_hist": torch.bincount(count.cpu(), minlength=K + 1).tolist(),
             "end_hist": torch.bincount(end.cpu(), minlength=4).tolist(), "calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2",
             "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)} for row, ms, rnd in rows]


GROUP_LIGHTS = 4  # the builder's one light and three more (measure_groups)
_GROUP_ACCELS = {}  # scene name -> (the accels rebuilt per group, their build's wall-clock ms): built once, whatever --repeats says


def measure_groups(name, builder, size, calls):
    """Light groups on the camera's rays of a size^2 film, the scene with FOUR point lights: the builder's own at L = (x, y, z) and three more
    at L + (0.8, -0.25, 0.8), L + (-0.8, -0.25, 0.8) and L + (0, -0.25, -0.8) (the three scenes share one Cornell shell with L under its ceiling) with intensities (0.5, 0.4, 0.3), (0.3, 0.4, 0.5), (0.4, 0.5, 0.3) and falloff (1, 0, 0).  G = 6:
    per_light_groups(4) -- base, ambient, the four lights.  Row G6: one lg_radiance_groups_device call.  Beside it, in the same session: row
    GK, G calls of lg_radiance_device on G accels rebuilt per group (tests/light_subsets.py; the builds timed apart, host wall clock:
    build_ms), and row R1, ONE lg_radiance_device call on the full scene -- the floor: the difference to G6 is what G planes cost.  Timed
    G6, GK, R1, so --repeats alternates them; GK's planes are compared with G6's bytes (same_bytes)."""
    if not hasattr(G, "radiance_groups_device"):
        return []
    from light_subsets import subset_scene
    x, y, z = builder(pyref.Api).lights[0][0]
    extra = [((x + 0.8, y - 0.25, z + 0.8), (0.5, 0.4, 0.3)), ((x - 0.8, y - 0.25, z + 0.8), (0.3, 0.4, 0.5)), ((x, y - 0.25, z - 0.8), (0.4, 0.5, 0.3))]

    def four(api):
        scene = builder(api)
        for pos, col in extra:
            scene.add_point_light(list(pos), list(col), [1.0, 0.0, 0.0])
        return scene

    accel = G.Accel.from_scene(four(G))
    assert G.light_count(accel) == GROUP_LIGHTS
    groups = la.per_light_groups(GROUP_LIGHTS)
    k = len(groups)
    if name not in _GROUP_ACCELS:
        t0 = time.time()
        rebuilt = [G.Accel.from_scene(subset_scene(G, four, g.lights, bool(g.flags & la.GROUP_AMBIENT))) for g in groups]
        _GROUP_ACCELS[name] = (rebuilt, (time.time() - t0) * 1e3)
    rebuilt, build_ms = _GROUP_ACCELS[name]
    s = torch.cuda.current_stream().cuda_stream
    for a in [accel] + rebuilt:
        G.set_query_order(a, 0)
    assert G.camera_samples(accel) == 1
    n = size * size
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    planes = torch.empty((k, n, 3), dtype=torch.float64, device="cuda")
    other = torch.empty((k, n, 3), dtype=torch.float64, device="cuda")
    rows = []
    ms = timed(lambda: G.radiance_groups_device(accel, n, rays.data_ptr(), groups, planes.data_ptr(), stream=s), calls, warmup=1)
    rows.append(("G6: radiance groups, one call, base + ambient + %d lights" % GROUP_LIGHTS, ms, k, None))
    ms = timed(lambda: [G.radiance_device(a, n, rays.data_ptr(), other.data_ptr() + 24 * n * i, stream=s) for i, a in enumerate(rebuilt)], calls, warmup=1)
    torch.cuda.synchronize()
    rows.append(("GK: lg_radiance_device on G accels rebuilt per group, G calls", ms, k, {"build_ms": round(build_ms, 1), "same_bytes": bool(torch.equal(planes.view(torch.int64), other.view(torch.int64)))}))
    ms = timed(lambda: G.radiance_device(accel, n, rays.data_ptr(), other.data_ptr(), stream=s), calls, warmup=1)
    rows.append(("R1: lg_radiance_device, the full scene, one call (the floor)", ms, 1, None))
    return [{"scene": name, "row": row, "film": [size, size], "rays": n, "lights": GROUP_LIGHTS, "planes": p, "light_positions": [[x, y, z]] + [list(e[0]) for e in extra],
             "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1), **(x_ or {}), "calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2",
             "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)} for row, ms, p, x_ in rows]


def measure_scatter(name, builder, size, calls):
    """Surface scatter on the camera's rays of a size^2 film.  Row R0, the yardstick: lg_radiance_device on the same scene rebuilt at depth
    0 -- the same closest and shadow passes, 24 bytes written a ray.  Row S2: lg_scatter_device, direct + flags (28 bytes a ray).  Row S7: all
    seven planes (284 bytes a ray).  over_floor_ms = the row's ms minus R0's of the same repeat, ns_per_byte_over_floor = that over the bytes
    the row writes beyond R0's 24 a ray.  Then the price of opening the tree: row CD, the composition to the scene's own depth D through the
    device form with torch on the same stream (mask, compact, multiply, add per level), against row RD, ONE lg_radiance_device call on the scene
    as it is; CD's value is compared with RD's bytes (same_bytes).  Timed R0, S2, S7, CD, RD, so --repeats alternates them."""
    if not hasattr(G, "scatter_device"):
        return []
    accel = G.Accel.from_scene(builder(G))
    flat_scene = builder(G)
    flat_scene.set_max_recursion_depth(0)
    flat = G.Accel.from_scene(flat_scene)
    depth = int(builder(pyref.Api).recursion)
    for a in (accel, flat):
        G.set_query_order(a, 0)
    assert G.camera_samples(accel) == 1
    s = torch.cuda.current_stream().cuda_stream
    n = size * size
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    rad, hits, direct, flags = f64(n, 3), torch.empty((n * 24,), dtype=torch.int32, device="cuda"), f64(n, 3), torch.empty((n,), dtype=torch.int32, device="cuda")
    reflect, rw, refract, tw = f64(n, 6), f64(n, 3), f64(n, 6), f64(n, 5)

    def L(r, d):
        m = r.shape[0]
        di, fl = f64(m, 3), torch.empty((m,), dtype=torch.int32, device="cuda")
        if d == depth:
            G.scatter_device(accel, m, r, direct_ptr=di, flags_ptr=fl, stream=s)
            return torch.where(((fl & 1) != 0)[:, None], (di + 0.0) + 0.0, di)
        cr, wr, ct, wt = f64(m, 6), f64(m, 3), f64(m, 6), f64(m, 5)
        G.scatter_device(accel, m, r, direct_ptr=di, flags_ptr=fl, reflect_ptr=cr, reflect_weight_ptr=wr, refract_ptr=ct, refract_weight_ptr=wt, stream=s)
        hit, has_r, has_t = (fl & 1) != 0, (fl & 2) != 0, (fl & 4) != 0
        R, T = torch.zeros_like(di), torch.zeros_like(di)
        ir, it = has_r.nonzero().squeeze(1), has_t.nonzero().squeeze(1)
        if ir.numel():
            R[ir] = wr[ir] * L(cr[ir].contiguous(), d + 1)
        if it.numel():
            w = wt[it]
            T[it] = ((w[:, :3] * L(ct[it].contiguous(), d + 1)) * w[:, 3:4]) / w[:, 4:5]
        return torch.where(hit[:, None], (di + R) + T, di)

    composed = [None]

    def compose():
        composed[0] = (0.0 + L(rays, 0)) * 1.0

    rows = []
    ms = timed(lambda: G.radiance_device(flat, n, rays.data_ptr(), rad.data_ptr(), stream=s), calls, warmup=1)
    floor = ms
    rows.append(("R0: lg_radiance_device, the scene rebuilt at depth 0 (the floor)", ms, 24, None))
    ms = timed(lambda: G.scatter_device(accel, n, rays, direct_ptr=direct, flags_ptr=flags, stream=s), calls, warmup=1)
    rows.append(("S2: lg_scatter_device, direct + flags", ms, 28, None))
    ms = timed(lambda: G.scatter_device(accel, n, rays, hits_ptr=hits, direct_ptr=direct, flags_ptr=flags, reflect_ptr=reflect, reflect_weight_ptr=rw, refract_ptr=refract,
                                        refract_weight_ptr=tw, stream=s), calls, warmup=1)
    rows.append(("S7: lg_scatter_device, all seven planes", ms, 284, None))
    ms = timed(compose, max(calls // 4, 2), warmup=1)
    got = composed[0]
    ms_rd = timed(lambda: G.radiance_device(accel, n, rays.data_ptr(), rad.data_ptr(), stream=s), calls, warmup=1)
    torch.cuda.synchronize()
    rows.append(("CD: li() composed to depth %d over lg_scatter_device with torch" % depth, ms, None, {"depth": depth, "same_bytes": bool(torch.equal(got.view(torch.int64), rad.view(torch.int64)))}))
    rows.append(("RD: lg_radiance_device, the scene as it is, one call", ms_rd, 24, {"depth": depth}))
    out = []
    for row, ms, nbytes, x_ in rows:
        r = {"scene": name, "row": row, "film": [size, size], "rays": n, "ms": round(ms, 4), "mrays_per_s": round(n / ms / 1e3, 1), **(x_ or {})}
        if nbytes is not None:
            r["bytes_per_ray"] = nbytes
        if row[:2] in ("S2", "S7"):
            r["over_floor_ms"] = round(ms - floor, 4)
            r["ns_per_byte_over_floor"] = round((ms - floor) * 1e6 / ((nbytes - 24) * n), 5)
        r.update({"calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
                  "gpu": torch.cuda.get_device_name(0)})
        out.append(r)
    return out


def measure_attributes(name, builder, size, calls):
    """Hit attributes on the camera's rays of a size^2 film.  Row I, the floor: lg_intersect_device (96 bytes written a ray).  Row A2: the
    walking form, uv + bary alone (40 bytes a ray).  Row A7: all seven planes (244 bytes a ray).  over_floor_ms = the row's ms minus I's of the
    same repeat.  Then the _of form on a compacted tenth of the hits (every tenth hit, rays and records gathered with torch outside the timed
    call): row O, lg_hit_attributes_of_device, all six planes; row W, the route without it, the walking form on that tenth.  O's planes are
    compared with W's bytes (same_bytes).  Timed I, A2, A7, O, W, so --repeats alternates them."""
    if not hasattr(G, "hit_attributes_device"):
        return []
    accel = G.Accel.from_scene(builder(G))
    G.set_query_order(accel, 0)
    assert G.camera_samples(accel) == 1
    s = torch.cuda.current_stream().cuda_stream
    n = size * size
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    u32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    hits, flags, bary, uv, local, frame, dp = u32(n, 24), u32(n), f64(n, 3), f64(n, 2), f64(n, 3), f64(n, 6), f64(n, 6)
    rows = []
    ms = timed(lambda: G.intersect_device(accel, n, rays.data_ptr(), hits.data_ptr(), stream=s), calls, warmup=1)
    floor = ms
    rows.append(("I: lg_intersect_device (the floor)", n, ms, 96, None))
    ms = timed(lambda: G.hit_attributes_device(accel, n, rays, uv_ptr=uv, bary_ptr=bary, stream=s), calls, warmup=1)
    rows.append(("A2: lg_hit_attributes_device, uv + bary", n, ms, 40, None))
    ms = timed(lambda: G.hit_attributes_device(accel, n, rays, hits_ptr=hits, flags_ptr=flags, bary_ptr=bary, uv_ptr=uv, local_ptr=local, frame_ptr=frame, dp_ptr=dp, stream=s),
               calls, warmup=1)
    rows.append(("A7: lg_hit_attributes_device, all seven planes", n, ms, 244, None))
    torch.cuda.synchronize()
    tenth = (hits[:, 20] != 0).nonzero().squeeze(1)[::10]
    m = int(tenth.numel())
    if m:
        r10, h10 = rays[tenth].contiguous(), hits[tenth].contiguous()
        of = [u32(m), f64(m, 3), f64(m, 2), f64(m, 3), f64(m, 6), f64(m, 6)]
        wk = [u32(m), f64(m, 3), f64(m, 2), f64(m, 3), f64(m, 6), f64(m, 6)]
        names = ("flags_ptr", "bary_ptr", "uv_ptr", "local_ptr", "frame_ptr", "dp_ptr")
        ms_o = timed(lambda: G.hit_attributes_of_device(accel, m, r10, h10, stream=s, **dict(zip(names, of))), calls, warmup=1)
        ms_w = timed(lambda: G.hit_attributes_device(accel, m, r10, stream=s, **dict(zip(names, wk))), calls, warmup=1)
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(of, wk))
        rows.append(("O: lg_hit_attributes_of_device, a compacted tenth of the hits, six planes", m, ms_o, 148, {"same_bytes": bool(same)}))
        rows.append(("W: lg_hit_attributes_device on that tenth (re-walking it), six planes", m, ms_w, 148, None))
    out = []
    for row, nr, ms, nbytes, x_ in rows:
        r = {"scene": name, "row": row, "film": [size, size], "rays": nr, "ms": round(ms, 4), "mrays_per_s": round(nr / ms / 1e3, 1), "bytes_per_ray": nbytes, **(x_ or {})}
        if row[:2] in ("A2", "A7"):
            r["over_floor_ms"] = round(ms - floor, 4)
        r.update({"calls": calls, "traversal": "lds" if G.set_lds_scene(accel, True) else "l2", "prune": G.get_prune(accel), "device_source_sha16": la.device_source_sha16(),
                  "gpu": torch.cuda.get_device_name(0)})
        out.append(r)
    return out


def measure_closest(name, builder, calls):
    """Closest points on 2^20 grid points (128 x 128 x 64, grid order) over 1.2 x the scene's bounds, all three planes (48 bytes written a
    point).  Row C: radius +INF; row Cr: radius 5 % of the bounds' diagonal."""
    if not hasattr(G, "closest_points_device"):
        return []
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    probe = G.intersect(accel, G.camera_rays(accel, 64, 64))
    p = probe["p"][probe["kind"] != 0]
    lo, hi = p.min(axis=0), p.max(axis=0)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0 * 1.2
    ax = [mid[k] + half[k] * np.linspace(-1.0, 1.0, m) for k, m in enumerate((128, 128, 64))]
    grid = np.ascontiguousarray(np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3))
    n = len(grid)
    pts = torch.from_numpy(grid).cuda()
    dist, point, ids = torch.empty((n,), dtype=torch.float64, device="cuda"), torch.empty((n, 3), dtype=torch.float64, device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda")
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    out = []
    for row, radius in (("C: lg_closest_points_device, three planes, radius +INF", float("inf")), ("Cr: the same, radius 5 % of the bounds' diagonal", 0.05 * diag)):
        ms = timed(lambda: G.closest_points_device(accel, n, pts, radius, distance_ptr=dist, point_ptr=point, id_ptr=ids, stream=s), calls, warmup=1)
        found = int((ids[:, 0] != 0).sum())
        out.append({"scene": name, "row": row, "points": n, "radius": radius, "ms": round(ms, 4), "mpoints_per_s": round(n / ms / 1e3, 2), "bytes_per_point": 48, "within_radius": found,
                    "calls": calls, "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)})
    return out


def measure_nearest(name, builder, calls):
    """Proximity queries (lg_nearest_device) on measure_closest's 2^20 grid points, beside lg_closest_points_device on the same points in the
    same session.  Rows N1 / N4 / N8: k = 1, 4, 8 with distance + id (24 bytes a slot and point), at radius 5 % of the bounds' diagonal and at
    +INF, each with its ratio to row F, lg_closest_points_device with distance + id at that radius -- the floor for k = 1.  Row T: the
    touch-only form at 5 %, beside row Fd, lg_closest_points_device with distance alone.  Row Q: count alone at 5 %."""
    if not hasattr(G, "nearest_device"):
        return []
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    probe = G.intersect(accel, G.camera_rays(accel, 64, 64))
    p = probe["p"][probe["kind"] != 0]
    lo, hi = p.min(axis=0), p.max(axis=0)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0 * 1.2
    ax = [mid[k] + half[k] * np.linspace(-1.0, 1.0, m) for k, m in enumerate((128, 128, 64))]
    grid = np.ascontiguousarray(np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3))
    n = len(grid)
    pts = torch.from_numpy(grid).cuda()
    dist, ids = torch.empty((8, n), dtype=torch.float64, device="cuda"), torch.empty((8, n, 4), dtype=torch.int32, device="cuda")
    touch, count = torch.empty((n,), dtype=torch.uint8, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda")
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    out = []

    def row(label, radius, ms, nbytes, floor=None, **more):
        r = {"scene": name, "row": label, "points": n, "radius": radius, "ms": round(ms, 4), "mpoints_per_s": round(n / ms / 1e3, 2), "bytes_per_point": nbytes, **more,
             "calls": calls, "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)}
        if floor is not None:
            r["over_closest_points"] = round(ms / floor, 3)
        out.append(r)

    for tag, radius in (("radius 5 % of the bounds' diagonal", 0.05 * diag), ("radius +INF", float("inf"))):
        floor = timed(lambda: G.closest_points_device(accel, n, pts, radius, distance_ptr=dist, id_ptr=ids, stream=s), calls, warmup=1)
        row("F: lg_closest_points_device, distance + id, " + tag, radius, floor, 24, within_radius=int((ids[0, :, 0] != 0).sum()))
        for k in (1, 4, 8):
            ms = timed(lambda: G.nearest_device(accel, n, pts, None, radius, k, distance_ptr=dist, id_ptr=ids, stream=s), calls, warmup=1)
            row("N%d: lg_nearest_device, k = %d, distance + id, %s" % (k, k, tag), radius, ms, 24 * k, floor, filled_slots=int((ids[:k, :, 0] != 0).sum()))
    radius = 0.05 * diag
    floor = timed(lambda: G.closest_points_device(accel, n, pts, radius, distance_ptr=dist, stream=s), calls, warmup=1)
    row("Fd: lg_closest_points_device, distance alone, radius 5 % of the bounds' diagonal", radius, floor, 8)
    ms = timed(lambda: G.nearest_device(accel, n, pts, None, radius, 0, touch_ptr=touch, stream=s), calls, warmup=1)
    row("T: lg_nearest_device, touch alone (leaves at the first contact), radius 5 % of the bounds' diagonal", radius, ms, 1, floor, touching=int(touch.sum()))
    ms = timed(lambda: G.nearest_device(accel, n, pts, None, radius, 0, count_ptr=count, stream=s), calls, warmup=1)
    row("Q: lg_nearest_device, count alone (meets every primitive within the radius), radius 5 % of the bounds' diagonal", radius, ms, 4, floor,
        largest_count=int(count.max()), mean_count=round(float(count.double().mean()), 3))
    return out


def measure_segments(name, builder, calls, count=1 << 20, long_only=False, label=None):
    """Segment proximity (lg_closest_segments_device) on `count` segments (2^20 by default) whose midpoints are measure_closest's grid
    points (the first `count` of a seeded shuffle), directions seeded, lengths 1 % and 100 % of the bounds' diagonal, at radius +INF and at
    5 % of the diagonal.  Rows S: distance + id (the best form); rows St: touch alone (leaves at the first contact; at radius 5 % only --
    at +INF the first candidate ends every walk).  Beside them the yardstick, row N: lg_nearest_device, k = 1, distance + id on the
    segments' midpoints at that radius (`over_nearest_midpoints`: the ratio).  long_only: the 100 % rows alone -- what a library built with
    -DLG_SEGMENTS_NO_STAGE2 (LASGUN_HIP_LIB names it; `label` says so in the rows) is measured on, to show what stage 2 of the pruning buys."""
    if not hasattr(G, "closest_segments_device"):
        return []
    accel = G.Accel.from_scene(builder(G))
    s = torch.cuda.current_stream().cuda_stream
    probe = G.intersect(accel, G.camera_rays(accel, 64, 64))
    p = probe["p"][probe["kind"] != 0]
    lo, hi = p.min(axis=0), p.max(axis=0)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0 * 1.2
    ax = [mid[k] + half[k] * np.linspace(-1.0, 1.0, m) for k, m in enumerate((128, 128, 64))]
    grid = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(30)
    n = min(int(count), len(grid))
    centre = np.ascontiguousarray(grid if n == len(grid) else grid[np.sort(rng.permutation(len(grid))[:n])])
    d = rng.normal(0.0, 1.0, (n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    pts = torch.from_numpy(centre).cuda()
    dist, ids = torch.empty((n,), dtype=torch.float64, device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda")
    touch = torch.empty((n,), dtype=torch.uint8, device="cuda")
    out = []

    def row(tag, radius, length, ms, nbytes, floor=None, **more):
        r = {"scene": name, "row": tag, "segments": n, "radius": radius, "length": length, "ms": round(ms, 4), "msegments_per_s": round(n / ms / 1e3, 2), "bytes_per_segment": nbytes,
             **more, "calls": calls, "build": label or "product", "device_source_sha16": la.device_source_sha16(), "gpu": torch.cuda.get_device_name(0)}
        if floor is not None:
            r["over_nearest_midpoints"] = round(ms / floor, 3)
        out.append(r)

    for rtag, radius in (("radius +INF", float("inf")), ("radius 5 % of the bounds' diagonal", 0.05 * diag)):
        floor = timed(lambda: G.nearest_device(accel, n, pts, None, radius, 1, distance_ptr=dist, id_ptr=ids, stream=s), calls, warmup=1)
        row("N: lg_nearest_device, k = 1, distance + id, the segments' midpoints, " + rtag, radius, 0.0, floor, 24, within_radius=int((ids[:, 0] != 0).sum()))
        for ltag, frac in (("length 1 %", 0.01), ("length 100 %", 1.0)):
            if long_only and frac != 1.0:
                continue
            length = frac * diag
            segs = torch.from_numpy(np.ascontiguousarray(np.concatenate([centre - d * (0.5 * length), centre + d * (0.5 * length)], axis=1))).cuda()
            ms = timed(lambda: G.closest_segments_device(accel, n, segs, None, radius, distance_ptr=dist, id_ptr=ids, stream=s), calls, warmup=1)
            row("S: lg_closest_segments_device, distance + id, %s, %s" % (ltag, rtag), radius, length, ms, 24, floor, within_radius=int((ids[:, 0] != 0).sum()),
                at_zero=int((dist == 0.0).sum()))
            if radius != float("inf"):
                ms = timed(lambda: G.closest_segments_device(accel, n, segs, None, radius, touch_ptr=touch, stream=s), calls, warmup=1)
                row("St: lg_closest_segments_device, touch alone (leaves at the first contact), %s, %s" % (ltag, rtag), radius, length, ms, 1, floor, touching=int(touch.sum()))
            del segs
    return out


def once(size):
    """The headline frame rendered once, then its rays queried once (closest, then the shadow segments to light 0)."""
    scene = S.spheres_scene(G)
    accel = G.Accel.from_scene(scene)
    s = torch.cuda.current_stream().cuda_stream
    film = torch.empty((size * size * 4,), dtype=torch.uint8, device="cuda")
    G.capture_rows_device(accel, size, size, 0, size, film.data_ptr(), stream=s)
    n = size * size
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(accel, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    hits = torch.empty((n * 96,), dtype=torch.uint8, device="cuda")
    G.intersect_device(accel, n, rays.data_ptr(), hits.data_ptr(), stream=s)
    segs = shadow_segments(hits, S.spheres_scene(pyref.Api).lights[0][0])
    occ = torch.empty((segs.shape[0],), dtype=torch.uint8, device="cuda")
    G.occluded_device(accel, segs.shape[0], segs.data_ptr(), occ.data_ptr(), stream=s)
    tiled = rays.view(size // 8, 8, size // 8, 8, 6).permute(0, 2, 1, 3, 4).contiguous().view(n, 6)  # 8 x 8 pixel tiles: row r8
    rad = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    G.radiance_device(accel, n, tiled.data_ptr(), rad.data_ptr(), stream=s)
    torch.cuda.synchronize()
    print(json.dumps({"once": True, "rays": n, "shadow_segments": int(segs.shape[0])}))


_LIT_ACCELS = {}


def measure_lit(name, builder, size, calls):
    """Lit scatter on the camera's rays of a size^2 film (the rows: the module's docstring).  The four lights are measure_groups': the
    builder's own at L and three more around it under the shell's ceiling; the other lights are drawn with a fixed seed from the box
    L + [-0.8, 0.8] x [-0.5, 0] x [-0.8, 0.8] with intensities in [0.02, 0.2] and falloff (1, 0, 0).  Timed F, L4, L64, L64v, P1, P1t, P16, P16t,
    M64, MR, so --repeats alternates them."""
    if not hasattr(G, "scatter_lit_device"):
        return []
    from light_subsets import subset_scene
    pscene = builder(pyref.Api)
    (x, y, z), col0, fall0 = pscene.lights[0][0], pscene.lights[0][1], pscene.lights[0][2]
    four = la.lights_array([la.Light((x, y, z), col0, fall0), la.Light((x + 0.8, y - 0.25, z + 0.8), (0.5, 0.4, 0.3)),
                            la.Light((x - 0.8, y - 0.25, z + 0.8), (0.3, 0.4, 0.5)), la.Light((x, y - 0.25, z - 0.8), (0.4, 0.5, 0.3))])
    ambient = tuple(float(c) for c in pscene.ambient)
    rng = np.random.default_rng(23)
    pool = np.zeros(64, dtype=la.LIGHT_DTYPE)
    pool["position"] = np.array([x, y, z]) + rng.uniform([-0.8, -0.5, -0.8], [0.8, 0.0, 0.8], (64, 3))
    pool["intensity"] = rng.uniform(0.02, 0.2, (64, 3))
    pool["falloff"] = (1.0, 0.0, 0.0)

    def relit(lights):
        def scene_of(api):
            scene = subset_scene(api, builder, 0, False)
            for rec in lights:
                scene.add_point_light(rec["position"].tolist(), rec["intensity"].tolist(), rec["falloff"].tolist())
            scene.set_ambient_light(list(ambient))
            return scene
        return scene_of

    small = min(size, 1024)
    if name not in _LIT_ACCELS:
        bare, lit4 = G.Accel.from_scene(relit(pool[:0])(G)), G.Accel.from_scene(relit(four)(G))
        t0 = time.time()
        moved = [G.Accel.from_scene(relit(pool[i:i + 1])(G)) for i in range(64)]
        _LIT_ACCELS[name] = (bare, lit4, moved, (time.time() - t0) * 1e3)
    bare, lit4, moved, build_ms = _LIT_ACCELS[name]
    for a in [bare, lit4] + moved:
        G.set_query_order(a, 0)
    s = torch.cuda.current_stream().cuda_stream
    n, ns = size * size, small * small
    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(bare, size, size, 0, 0, size, size, rays.data_ptr(), stream=s)
    rays_s = torch.empty((ns, 6), dtype=torch.float64, device="cuda")
    G.camera_rays_device(bare, small, small, 0, 0, small, small, rays_s.data_ptr(), stream=s)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    direct, flags, direct2, flags2, vis = f64(n, 3), i32(n), f64(n, 3), i32(n), i32(n, 2)
    idx = torch.from_numpy(rng.integers(0, 64, (n, 16))).cuda()
    tab = torch.from_numpy(pool.view(np.float64).reshape(64, 9).copy()).cuda()
    tab16 = tab[idx].contiguous()            # (n, 16, 9): ray i's lights
    tab1 = tab16[:, 0, :].contiguous()       # (n, 9)
    del idx
    terms = f64(n, 16, 3)
    skip = os.environ.get("LASGUN_LIT_SKIP", "1") != "0"
    rows = []

    def row(tag, fn, k, nbytes, rays_n=n, c=calls, **extra):
        ms = timed(fn, c, warmup=1)
        rows.append((tag, ms, k, nbytes, rays_n, extra))
        return ms

    row("F: lg_scatter_device, direct + flags, the scene rebuilt with four lights (the floor)", lambda: G.scatter_device(lit4, n, rays, direct_ptr=direct, flags_ptr=flags, stream=s), 4, 28)
    row("L4: lg_scatter_lit_device, the same four lights shared, direct + flags", lambda: G.scatter_lit_device(bare, n, rays, lights=four, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, stream=s), 4, 28)
    torch.cuda.synchronize()
    rows[-1][5]["same_bytes"] = bool(torch.equal(direct.view(torch.int64), direct2.view(torch.int64)) and torch.equal(flags, flags2))
    row("L64: 64 shared lights, direct + flags", lambda: G.scatter_lit_device(bare, n, rays, lights=pool, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, stream=s), 64, 28)
    kept = direct2.clone()
    row("L64v: 64 shared lights, direct + flags + visible (every pair walked)", lambda: G.scatter_lit_device(bare, n, rays, lights=pool, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, visible_ptr=vis, stream=s), 64, 36)
    torch.cuda.synchronize()
    rows[-1][5]["same_bytes"] = bool(torch.equal(kept.view(torch.int64), direct2.view(torch.int64)))  # the skip changes no bit of direct
    del kept
    row("P1: one light per ray, direct + flags", lambda: G.scatter_lit_device(bare, n, rays, per_ray_lights_ptr=tab1, count=1, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, stream=s), 1, 28)
    row("P1t: one light per ray, direct + flags + terms", lambda: G.scatter_lit_device(bare, n, rays, per_ray_lights_ptr=tab1, count=1, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, terms_ptr=terms, stream=s), 1, 52)
    row("P16: 16 lights per ray, direct + flags", lambda: G.scatter_lit_device(bare, n, rays, per_ray_lights_ptr=tab16, count=16, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, stream=s), 16, 28)
    row("P16t: 16 lights per ray, direct + flags + terms", lambda: G.scatter_lit_device(bare, n, rays, per_ray_lights_ptr=tab16, count=16, ambient=ambient, direct_ptr=direct2, flags_ptr=flags2, terms_ptr=terms, stream=s), 16, 28 + 16 * 24)
    del tab16, tab1, terms
    many, other = f64(64, ns, 3), f64(64, ns, 3)
    row("M64: one light at 64 positions, 64 lg_scatter_lit_device calls on one accel, direct", lambda: [G.scatter_lit_device(bare, ns, rays_s, lights=pool[i:i + 1], ambient=ambient, direct_ptr=many.data_ptr() + 24 * ns * i, stream=s) for i in range(64)],
        1, 24, rays_n=64 * ns, c=max(calls // 2, 2), film=[small, small])
    row("MR: the same by 64 rebuilt accels + lg_scatter_device, direct (the rebuilds timed apart)", lambda: [G.scatter_device(a, ns, rays_s, direct_ptr=other.data_ptr() + 24 * ns * i, stream=s) for i, a in enumerate(moved)],
        1, 24, rays_n=64 * ns, c=max(calls // 2, 2), film=[small, small], build_ms=round(build_ms, 1))
    torch.cuda.synchronize()
    rows[-2][5]["same_bytes"] = bool(torch.equal(many.view(torch.int64), other.view(torch.int64)))
    out = []
    for tag, ms, k, nbytes, rays_n, extra in rows:
        r = {"scene": name, "row": tag, "film": [size, size], "rays": rays_n, "lights": k, "ms": round(ms, 4), "mrays_per_s": round(rays_n / ms / 1e3, 1), "bytes_per_ray": nbytes, "skip": skip}
        r.update(extra)
        r.update({"calls": calls, "traversal": "lds" if G.set_lds_scene(bare, True) else "l2", "prune": G.get_prune(bare), "device_source_sha16": la.device_source_sha16(),
                  "gpu": torch.cuda.get_device_name(0)})
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--order", type=int, choices=(0, 1), default=None)
    ap.add_argument("--rows", default="all", help="comma-separated: all, queries, radiance, frame, film, visibility, features, directions, scan, gather, views, viewfeatures, layers, groups, paths, scatter, lit, attributes, closest, nearest, segments")
    ap.add_argument("--out", default=None)
    ap.add_argument("--segments", type=int, default=1 << 20, help="--rows segments: how many segments (at most the grid's 2^20)")
    ap.add_argument("--long-only", action="store_true", help="--rows segments: the rows of full-length segments alone")
    ap.add_argument("--label", default=None, help="--rows segments: the rows' `build` (default: product), for a library named by LASGUN_HIP_LIB")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    G.set_device(0)
    if args.once:
        once(args.size)
        return
    want = set(args.rows.split(","))
    if not want or want - {"all", "queries", "radiance", "frame", "film", "visibility", "features", "directions", "scan", "gather", "views", "viewfeatures", "layers", "groups", "paths", "scatter", "lit", "attributes", "closest", "nearest", "segments"}:
        ap.error("--rows: all, queries, radiance, frame, film, visibility, features, directions, scan, gather, views, viewfeatures, layers, groups, paths, scatter, lit, attributes, closest, nearest, segments")
    t0 = time.time()
    rows = []
    for repeat in range(max(args.repeats, 1)):
        for name, builder in SCENES:
            got = measure(name, builder, args.size, max(args.calls, 20), args.seed, args.order) if want & {"all", "queries"} else []
            if want & {"all", "visibility"}:
                got += measure_visibility(name, builder, max(args.calls, 20))
            if want & {"all", "features"}:
                got += measure_features(name, builder, args.size, max(args.calls, 20))
            if "directions" in want:
                got += measure_directions(name, builder, max(args.calls, 20))
            if "scan" in want:
                got += measure_scan(name, builder, max(args.calls, 20))
            if "gather" in want:
                got += measure_gather(name, builder, args.calls)
            if "views" in want:
                got += measure_views(name, builder, max(args.calls, 3))
            if "viewfeatures" in want:
                got += measure_view_features(name, builder, max(args.calls, 3))
            if "layers" in want:
                got += measure_layers(name, builder, args.size, max(args.calls, 4))
            if "groups" in want:
                got += measure_groups(name, builder, args.size, max(args.calls, 3))
            if "paths" in want:
                got += measure_paths(name, builder, args.size, max(args.calls, 4))
            if "scatter" in want:
                got += measure_scatter(name, builder, args.size, max(args.calls, 4))
            if "lit" in want:
                got += measure_lit(name, builder, args.size, max(args.calls, 3))
            if "attributes" in want:
                got += measure_attributes(name, builder, args.size, max(args.calls, 4))
            if "closest" in want:
                got += measure_closest(name, builder, max(args.calls, 4))
            if "nearest" in want:
                got += measure_nearest(name, builder, min(max(args.calls, 2), 4))
            if "segments" in want:
                got += measure_segments(name, builder, min(max(args.calls, 2), 4), args.segments, args.long_only, args.label)
            if want - {"queries", "visibility", "features", "directions", "scan", "gather", "views", "viewfeatures", "layers", "groups", "paths", "scatter", "lit", "attributes", "closest", "nearest", "segments"}:
                got += measure_radiance(name, builder, args.size, max(args.calls, 20), args.seed, args.order, frame_only=want == {"frame"},
                                        film_rows=bool(want & {"all", "film"}), radiance_rows=bool(want & {"all", "radiance"}))
            for r in got:
                r["repeat"] = repeat
                print(json.dumps(r), flush=True)
                rows.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("# %.1f s" % (time.time() - t0), file=sys.stderr)


if __name__ == "__main__":
    main()
