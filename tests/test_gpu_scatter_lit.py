"""Lit scatter (include/lasgun_hip.h: lg_scatter_lit, lg_scatter_lit_device): surface scatter under lights that come with the call.  Pinned
bit for bit with what the project already has: an accel REBUILT with the same lights must give the same bytes through lg_scatter,
lg_radiance_groups and lg_occluded.

  0  not vacuous, on the CPU oracle's `occluded` first: between 5 % and 95 % of the (hit, light) pairs are occluded;
  1  shared K in {1, 4, 32}: the seven scatter planes on an accel without lights equal lg_scatter's on an accel rebuilt with those lights
     and that ambient; the scene's own lights, or 40 of them, change nothing;
  2  (0 + direct) * 1.0 is the CPU oracle's radiance of the scene built at depth 0 with pool[0:8];
  3  K in {0, 31, 32, 33, 64, 65, 70}: terms are the single-light planes of lg_radiance_groups on rebuilt accels, visible is !lg_occluded
     of the segments restated in numpy, direct is the sequential sum of terms plus the K = 0 call's direct;
  4  per ray, K in {1, 3, 33}: the shared call's columns; a per-ray table of equal rows gives the shared call's bytes;
  5  sizes, both modes, both orders, every traversal form, more tiles than twice the grid's waves;
  6  plane subsets over garbage (direct and terms the same bytes with and without visible: the skip's proof), the device form on a second
     stream between guard words, K = 65 in three chunks and more in a fresh process;
  7  edge rays; every error of the contract, nothing launched, no output touched.
Compared as bit patterns; nothing is tolerated except lg_scatter's NaN rule (scatter_ref.bits)."""
import functools
import hashlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import edge_rays as E
import lasgun_amd as la
import lit_ref as L
import scatter_ref as R
from lasgun_amd import scenes as S
from oracle_lib import oracle
from test_gpu_hit_layers import odd_rays
from test_gpu_radiance_query import each_form, oracle_radiance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
W, H = 96, 64
PLANES = la.LIT_PLANES
SCATTER = la.SCATTER_PLANES
bits = R.bits
POOL = L.pool()
AMB = L.AMBIENT

BUILDERS = {
    "kitchen_sink": lambda api: S.kitchen_sink_scene(api, supersampling=0),
    "cornell_glass": lambda api: S.cornell_scene(api, "glass"),
    "spooky": lambda api: S.spooky_scene(api, supersampling=0),
    "f3": E.f3_scene,
}


@functools.lru_cache(maxsize=None)
def bare(name):
    """The scene with NO lights and zero ambient: nothing the call could lean on."""
    return G.Accel.from_scene(L.relit(BUILDERS[name], POOL[:0], (0.0, 0.0, 0.0))(G))


@functools.lru_cache(maxsize=None)
def rebuilt(name, lo, hi, depth=None):
    return G.Accel.from_scene(L.relit(BUILDERS[name], POOL[lo:hi], AMB, depth)(G))


@functools.lru_cache(maxsize=None)
def film(name):
    rays = G.camera_rays(bare(name), W, H)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def shared(name, k):
    """ONE reference per (scene, K): all nine planes of the shared call on the bare accel; left unchanged."""
    out = G.scatter_lit(bare(name), film(name), POOL[:k], AMB)
    for a in out.values():
        a.setflags(write=False)
    return out


def same(ctx, got, want, planes):
    for p in planes:
        assert got[p].shape == want[p].shape and got[p].tobytes() == want[p].tobytes(), (ctx, p, "bytes differ")


def take(out, idx):
    return {p: np.ascontiguousarray(out[p][idx]) for p in out}


# ---- 0: not vacuous ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass"])
def test_the_pool_is_partly_occluded_on_the_cpu_oracle(name):
    o = oracle()
    oacc = o.Accel(L.relit(BUILDERS[name], POOL[:0], (0.0, 0.0, 0.0))(o))
    rays = film(name)
    hits, _ = o.intersect(oacc, rays)
    hit = hits["kind"] != 0
    assert 0.05 <= hit.mean() <= 0.95, (name, hit.mean(), "the rays are neither all hits nor all misses")
    seg = L.shadow_segments(hits[hit][::4], POOL["position"]).reshape(-1, 6)
    occ = o.occluded(oacc, np.ascontiguousarray(seg)).mean()
    print("%s: %.1f %% of (hit, light) pairs occluded, %.1f %% of rays hit" % (name, 100 * occ, 100 * hit.mean()))
    assert 0.05 <= occ <= 0.95, (name, occ)


# ---- 1: against a rebuilt accel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 32])
@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass", "spooky"])
def test_the_scatter_planes_are_lg_scatters_on_an_accel_rebuilt_with_the_lights(name, k):
    rays = film(name)
    want = G.scatter(rebuilt(name, 0, k), rays)
    hit = (want["flags"] & R.HIT) != 0
    assert hit.any() and (~hit).any() and (want["direct"][hit] != 0.0).any()
    got = shared(name, k)
    same((name, k, "no lights in the scene"), got, want, SCATTER)
    own = G.Accel.from_scene(BUILDERS[name](G))  # the scene's own lights and ambient play no part
    assert G.light_count(own) >= 1
    same((name, k, "the scene's own lights"), G.scatter_lit(own, rays, POOL[:k], AMB, SCATTER), want, SCATTER)
    if k == 4:  # a scene of 40 lights is accepted, and they play no part
        forty = G.Accel.from_scene(L.relit(BUILDERS[name], POOL[10:50], (0.9, 0.9, 0.9))(G))
        assert G.light_count(forty) == 40
        same((name, k, "40 lights in the scene"), G.scatter_lit(forty, rays, POOL[:k], AMB, SCATTER), want, SCATTER)
        # not vacuous: other lights give other bytes
        assert G.scatter_lit(bare(name), rays, POOL[4:8], AMB, ("direct",))["direct"].tobytes() != want["direct"].tobytes()


# ---- 2: against the CPU oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass"])
def test_direct_is_the_cpu_oracles_radiance_at_depth_0(name):
    want = oracle_radiance(L.relit(BUILDERS[name], POOL[:8], AMB, depth=0), W, H).reshape(-1, 3)
    assert not np.isnan(want).any()
    got = (0.0 + shared(name, 8)["direct"]) * 1.0
    assert got.tobytes() == want.tobytes(), (name, int((got.view(np.int64) != want.view(np.int64)).any(axis=1).sum()))


# ---- 3: terms, visibility and the sum --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_terms(name):
    """(n, 70, 3): light k's single-light plane of lg_radiance_groups on depth-0 accels rebuilt with pool[0:32], [32:64], [64:70]."""
    rays = film(name)
    cols = []
    for lo, hi in ((0, 32), (32, 64), (64, 70)):
        planes = G.radiance_groups(rebuilt(name, lo, hi, 0), rays, [la.LightGroup(1 << l) for l in range(hi - lo)])
        cols.append(np.transpose(planes, (1, 0, 2)))
    out = np.ascontiguousarray(np.concatenate(cols, axis=1))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def open_lights(name):
    """(n, 70) bool: !lg_occluded of the hits' shadow segments, restated in numpy from lg_intersect's hits; False at a miss."""
    acc = bare(name)
    hits = G.intersect(acc, film(name))
    hit = hits["kind"] != 0
    seg = L.shadow_segments(hits[hit], POOL["position"])
    vis = np.zeros((len(hits), L.POOL_N), dtype=bool)
    vis[hit] = ~G.occluded(acc, np.ascontiguousarray(seg.reshape(-1, 6))).reshape(seg.shape[:2])
    vis.setflags(write=False)
    return vis


@pytest.mark.parametrize("k", [0, 31, 32, 33, 64, 65, 70])
@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass"])
def test_terms_visibility_and_the_sum(name, k):
    out = shared(name, k)
    n = len(film(name))
    hit = (out["flags"] & R.HIT) != 0
    assert out["terms"].shape == (n, k, 3) and out["visible"].shape == (n, (k + 31) // 32)
    want_terms, want_vis = group_terms(name)[:, :k], open_lights(name)[:, :k]
    assert out["terms"][hit].tobytes() == np.ascontiguousarray(want_terms[hit]).tobytes(), (name, k, "a hit's terms are the single-light groups' planes")
    assert not out["terms"][~hit].view(np.uint64).any(), (name, k, "a miss's terms are +0.0")
    assert out["visible"].tobytes() == L.pack_bits(want_vis).tobytes(), (name, k, "visible is !lg_occluded; a miss's words and the bits at or above K are 0")
    base = shared(name, 0)["direct"]
    want_direct = L.sequential_sum(out["terms"], base)
    assert out["direct"][hit].tobytes() == np.ascontiguousarray(want_direct[hit]).tobytes(), (name, k, "direct is the sequential sum + the ambient term")
    assert out["direct"][~hit].tobytes() == base[~hit].tobytes(), (name, k, "a miss's direct is the background")
    if k == 70:  # not vacuous: lit and unlit terms, open and blocked lights, the light without attenuation
        lit = (out["terms"][hit] != 0.0).any(axis=2)
        assert 0.05 <= lit.mean() <= 0.95 and 0.05 <= want_vis[hit].mean() <= 0.95, (lit.mean(), want_vis[hit].mean())
        z = L.ZERO_FALLOFF
        assert want_vis[hit][:, z].any() and not lit[:, z].any(), "f_att == 0: visible by its own test, never added"
        assert (lit & ~want_vis[hit]).sum() == 0


# ---- 4: per ray ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 33])
def test_per_ray_lights_are_the_shared_calls_columns(k):
    name = "cornell_glass"
    rays, ref = film(name), shared(name, 70)
    n = len(rays)
    idx = np.random.default_rng(40 + k).integers(0, L.POOL_N, (n, k))
    got = G.scatter_lit(bare(name), rays, POOL[idx], AMB)
    rows = np.arange(n)[:, None]
    assert got["terms"].tobytes() == np.ascontiguousarray(ref["terms"][rows, idx]).tobytes(), (k, "terms")
    vis70 = L.unpack_bits(ref["visible"], L.POOL_N)
    assert got["visible"].tobytes() == L.pack_bits(vis70[rows, idx]).tobytes(), (k, "visible")
    hit = (got["flags"] & R.HIT) != 0
    want = L.sequential_sum(got["terms"], shared(name, 0)["direct"])
    assert got["direct"][hit].tobytes() == np.ascontiguousarray(want[hit]).tobytes(), (k, "direct")
    same((k, "the planes that do not depend on the lights"), got, ref, ("hits", "flags", "reflect", "reflect_weight", "refract", "refract_weight"))
    assert (got["direct"][hit] != ref["direct"][hit]).any()
    # a per-ray table whose rows all equal a shared table: the shared call's bytes
    rows_equal = np.ascontiguousarray(np.broadcast_to(POOL[:k], (n, k)))
    same((k, "equal rows"), G.scatter_lit(bare(name), rays, rows_equal, AMB), shared(name, k), PLANES)


# ---- 5: shapes and forms -----------------------------------------------------------------------------------------------------------------------
def mode_lights(mode, k, idx):
    return POOL[:k] if mode == "shared" else POOL[idx[:, :k]]


@pytest.mark.parametrize("mode", ["shared", "per_ray"])
def test_sizes_and_orders(mode):
    acc = bare("cornell_glass")
    rays = np.concatenate([film("cornell_glass")[::2], G.camera_rays(acc, 40, 30)])[:4097]
    assert len(rays) == 4097
    k = 33
    idx = np.random.default_rng(9).integers(0, L.POOL_N, (4097, k))
    ref = G.scatter_lit(acc, rays, mode_lights(mode, k, idx), AMB)
    hit = (ref["flags"] & R.HIT) != 0
    assert hit.sum() >= 100 and (~hit).sum() >= 100 and (ref["visible"][hit, 1] != 0).any()
    try:
        for order in (0, 1):
            G.set_query_order(acc, order)
            for n in (0, 1, 63, 64, 65, 129, 4097):
                got = G.scatter_lit(acc, rays[:n], mode_lights(mode, k, idx[:n]) if mode == "per_ray" else POOL[:k], AMB)
                assert all(got[p].shape[0] == n for p in PLANES)
                same((mode, order, n), got, take(ref, slice(0, n)), PLANES)
    finally:
        G.set_query_order(acc, 0)
    assert la.api.call("scatter_lit", acc.h, None, 0, None, None) == 0  # n == 0: a no-op whatever the pointers
    assert la.api.call("scatter_lit_device", None, None, 0, None, None, None) == 0
    got = acc.scatter_lit(rays[:65], POOL[:k], AMB, planes=("direct", "visible"))
    assert list(got) == ["direct", "visible"]
    if mode == "shared":
        same("accel.scatter_lit", got, take(ref, slice(0, 65)), ("direct", "visible"))


@pytest.mark.parametrize("name", ["cornell_glass", "mesh_glass"])
def test_every_form_gives_identical_bytes(name):
    acc = bare(name) if name != "mesh_glass" else G.Accel.from_scene(S.mesh_scene(G, nu=48, nv=48, material="glass"))
    rays = G.camera_rays(acc, W, H)[: 64 * 60 + 5]
    n, k = len(rays), 35
    pool = POOL.copy()
    if name == "mesh_glass":  # the mesh scene is of another size: the pool's box around ITS hits
        p = G.intersect(acc, rays)
        p = p["p"][p["kind"] != 0]
        pool["position"] = p.mean(axis=0) + (POOL["position"] - POOL["position"].mean(axis=0)) * (np.ptp(p, axis=0).max() / 5.0)
    idx = np.random.default_rng(11).integers(0, L.POOL_N, (n, k))
    ref, checked = {}, set()
    try:
        for form in each_form(acc):
            for order in (0, 1):
                G.set_query_order(acc, order)
                for mode in ("shared", "per_ray"):
                    got = G.scatter_lit(acc, rays, pool[:k] if mode == "shared" else pool[idx], AMB)
                    if mode not in ref:
                        ref[mode] = got
                        hit = (got["flags"] & R.HIT) != 0
                        v = L.unpack_bits(got["visible"], k)[hit]
                        assert hit.any() and (~hit).any() and v.any() and not v.all(), (name, mode, v.mean())
                    same((name, form, order, mode), got, ref[mode], PLANES)
            G.set_query_order(acc, 0)
            checked.add(form)
    finally:
        G.set_query_order(acc, 0)
    need = {"reference", "prune", "lds", "lds+prune"} if name != "mesh_glass" else {"reference", "prune", "fast"}
    assert need <= checked, (name, checked)


def test_more_tiles_than_twice_the_grids_waves():
    """LDS form: one 1024-lane workgroup per CU, 16 waves each; the set repeated until its 64-ray tiles pass 2 x 16 x CUs."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    name = "cornell_glass"
    full = film(name)
    reps = 1
    while (reps * len(full) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    planes = ("direct", "visible")  # (terms of half a million rays x 33 lights are 400 MB of host arrays: sizes_and_orders pins that plane)
    once = shared(name, 33)
    got = G.scatter_lit(bare(name), np.ascontiguousarray(np.tile(full, (reps, 1))), POOL[:33], AMB, planes)
    assert (got["direct"].shape[0] + 63) // 64 > 2 * 16 * cus
    same(reps, got, take({p: once[p] for p in planes}, np.tile(np.arange(len(full)), reps)), planes)


# ---- 6: planes, streams and chunks -------------------------------------------------------------------------------------------------------------
SUBSETS = [(p,) for p in PLANES] + [("direct", "terms"), ("terms", "visible"), ("direct", "flags"), ("hits", "visible", "refract"), ("direct", "terms", "reflect_weight")]
GUARD, FILL = 64, 0x25A5A5A5


def plane_words(k):
    return {"hits": 24, "direct": 6, "flags": 1, "reflect": 12, "reflect_weight": 6, "refract": 12, "refract_weight": 10, "terms": 6 * k, "visible": (k + 31) // 32}


@pytest.mark.parametrize("mode", ["shared", "per_ray"])
def test_plane_subsets_over_garbage_and_the_skip(mode):
    name, k = "cornell_glass", 40
    acc = bare(name)
    rays = film(name)[: 64 * 30 + 9]
    n = len(rays)
    idx = np.random.default_rng(12).integers(0, L.POOL_N, (n, k))
    lights = mode_lights(mode, k, idx)
    ref = G.scatter_lit(acc, rays, lights, AMB)  # (visible asked for: every pair is walked)
    hit = (ref["flags"] & R.HIT) != 0
    blocked = ~L.unpack_bits(ref["visible"], k)[hit]
    assert 0.05 <= blocked.mean() <= 0.95
    rng = np.random.default_rng(5)
    for planes in SUBSETS:
        bufs = {p: rng.integers(1, 2 ** 32, ref[p].size * ref[p].dtype.itemsize // 4, dtype=np.uint64).astype(np.uint32).view(ref[p].dtype).reshape(ref[p].shape)
                for p in PLANES}
        kept = {p: bufs[p].tobytes() for p in PLANES if p not in planes}
        for _ in range(2):
            got = G.scatter_lit(acc, rays, lights, AMB, planes, into={p: bufs[p] for p in planes})
            assert all(got[p] is bufs[p] for p in planes)
            same((mode, "host", planes), got, ref, planes)  # direct and terms: the same bytes with and without visible
        assert all(bufs[p].tobytes() == kept[p] for p in kept), ("planes not asked for are untouched", planes)


def test_the_device_form_on_a_second_stream_between_guard_words():
    torch = pytest.importorskip("torch")
    name, k = "cornell_glass", 33
    acc = bare(name)
    rays = film(name)[: 64 * 30 + 9]
    n = len(rays)
    words = plane_words(k)
    idx = np.random.default_rng(13).integers(0, L.POOL_N, (n, k))
    drays = torch.from_numpy(rays.copy()).cuda()
    dtab = torch.from_numpy(np.ascontiguousarray(POOL[idx]).view(np.float64).reshape(n, k * 9).copy()).cuda()
    stream = torch.cuda.Stream()
    for mode in ("shared", "per_ray"):
        ref = G.scatter_lit(acc, rays, mode_lights(mode, k, idx), AMB)
        for order in (0, 1):
            G.set_query_order(acc, order)
            try:
                for planes in (PLANES, ("direct", "terms"), ("hits", "visible", "refract")):
                    dev = {p: torch.full((GUARD + n * words[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
                    torch.cuda.synchronize()
                    with torch.cuda.stream(stream):
                        s = torch.cuda.current_stream().cuda_stream
                        assert s != 0
                        kw = {p + "_ptr": dev[p].data_ptr() + 4 * GUARD for p in planes}
                        if mode == "shared":
                            table = POOL[:k].copy()
                            G.scatter_lit_device(acc, n, drays, lights=table, ambient=AMB, stream=s, **kw)
                            table["position"] = 1e30  # the host table may be overwritten on return: it was staged
                            del table
                        else:
                            G.scatter_lit_device(acc, n, drays, per_ray_lights_ptr=dtab, count=k, ambient=AMB, stream=s, **kw)
                    stream.synchronize()
                    for p in PLANES:
                        back = dev[p].cpu().numpy().view(np.uint32)
                        assert (back[:GUARD] == FILL).all() and (back[-GUARD:] == FILL).all(), (mode, order, planes, p, "the guard words")
                        if p in planes:
                            assert back[GUARD:-GUARD].tobytes() == ref[p].tobytes(), (mode, order, planes, p)
                        else:
                            assert (back == FILL).all(), (mode, order, planes, p, "not asked for")
            finally:
                G.set_query_order(acc, 0)


CHUNK_K = 65
CHUNK_PLANES = ("direct", "flags", "visible")  # (terms of 2^20 rays x 65 lights would be 1.6 GB: the plane is indexed by the ray like direct)


def chunk_rays(accel):
    """2^20 rays in no order: at the least budget (64 MiB) a chunk of a one-level chain with three visibility words a hit holds about
    320 thousand of them."""
    rays = G.camera_rays(accel, 1024, 1024)
    return np.ascontiguousarray(rays[np.random.default_rng(4).permutation(len(rays))])


def digests(out):
    return [hashlib.sha256(out[p].tobytes()).hexdigest() for p in CHUNK_PLANES]


def chunk_scene(api):
    return L.relit(BUILDERS["cornell_glass"], POOL[:0], (0.0, 0.0, 0.0))(api)


def test_many_chunks_give_the_bytes_of_one():
    acc = bare("cornell_glass")
    want = digests(G.scatter_lit(acc, chunk_rays(acc), POOL[:CHUNK_K], AMB, CHUNK_PLANES))
    with tempfile.TemporaryDirectory() as tmp:
        op = os.path.join(tmp, "out.txt")
        env = dict(os.environ)
        env.update({"LASGUN_DEBUG": "1", "LASGUN_WF_BUDGET_MB": "64"})
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lit_child.py"), op], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        m = re.findall(r"lit scatter: levels (\d+), (\d+) tiles in chunks of (\d+) \([^)]*\), (sorted order|as given), 65 shared lights", p.stderr)
        assert [x[3] for x in m] == ["as given", "sorted order"], p.stderr[-3000:]
        for levels, tiles, chunk, _ in m:
            assert int(levels) == 1 and (int(tiles) + int(chunk) - 1) // int(chunk) >= 3, m
        lines = [line.split() for line in open(op).read().splitlines()]
        assert [line[0] for line in lines] == ["0", "1"]
        for line in lines:
            assert line[1:] == want, ("order", line[0])


# ---- 7: edge rays and errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell_glass", "f3"])
def test_edge_rays_are_lg_scatters_on_the_rebuilt_accel(case):
    k = 5
    if case == "f3":
        rays = np.ascontiguousarray(E.edge_rays(*E.F3_BOUNDS, boxes=E.F3_BOXES, seed=3)[0])
    else:
        rays = odd_rays(film(case)[: 64 * 40 + 17])
    lights = POOL[:k].copy()
    if case == "f3":  # the scene's own place: the pool's box moved over its bounds
        lo, hi = np.array(E.F3_BOUNDS[0], dtype=np.float64), np.array(E.F3_BOUNDS[1], dtype=np.float64)
        lights["position"] = lo + (hi - lo) * np.random.default_rng(3).uniform(-0.25, 1.25, (k, 3))
    acc = bare(case)
    want = G.scatter(G.Accel.from_scene(L.relit(BUILDERS[case], lights, AMB)(G)), rays)
    got = G.scatter_lit(acc, rays, lights, AMB)
    hit = (want["flags"] & R.HIT) != 0
    assert hit.any() and (~hit).any() and not np.isfinite(rays).all(), (case, "hits, misses and rays that are not finite")
    for f in ("t", "p", "ng", "ns"):
        assert np.array_equal(bits(got["hits"][f]), bits(want["hits"][f])), (case, f)
    for f in ("kind", "prim", "instance", "material"):
        assert np.array_equal(got["hits"][f], want["hits"][f]), (case, f)
    assert np.array_equal(got["flags"], want["flags"]), case
    for p in ("direct", "reflect", "reflect_weight", "refract", "refract_weight"):
        assert np.array_equal(np.isnan(got[p]), np.isnan(want[p])), (case, p, "NaN where lg_scatter is NaN, and nowhere else")
        assert np.array_equal(bits(got[p]), bits(want[p])), (case, p, int((bits(got[p]) != bits(want[p])).any(axis=1).sum()))
    assert not got["terms"][~hit].view(np.uint64).any() and not got["visible"][~hit].any()
    # the skip changes no bit on these rays either
    lean = G.scatter_lit(acc, rays, lights, AMB, ("direct", "terms"))
    for p in ("direct", "terms"):
        assert np.array_equal(bits(lean[p]), bits(got[p])), (case, p, "with and without visible")


def test_errors_are_refused_before_any_launch():
    torch = pytest.importorskip("torch")
    import ctypes as C
    acc = bare("cornell_glass")
    n, k = 100, 33
    words = plane_words(k)
    rays = film("cornell_glass")[: n + 1].copy()
    drays = torch.from_numpy(rays.copy()).cuda()
    dev = {p: torch.full((n * words[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
    ptrs = {p + "_ptr": dev[p].data_ptr() for p in PLANES}
    host = {p: np.full(n * words[p], FILL, dtype=np.uint32) for p in PLANES}
    dtab = torch.zeros((n * k * 9 + 1,), dtype=torch.float64, device="cuda")
    htab = np.ascontiguousarray(np.broadcast_to(POOL[:k], (n, k)))
    torch.cuda.empty_cache()
    # "ends beyond its allocation": the buffer has to BE an allocation (tests/test_gpu_scatter.py): 2^17 rows of four lights' terms are
    # 12 MiB, 2^17 rows of two lights' records 18 MiB, each a block of its own, and the call asks for one row more
    many = 1 << 17
    short_terms = torch.full((many * 4 * 6,), FILL, dtype=torch.int32, device="cuda")
    short_tab = torch.zeros((many * 2 * 9,), dtype=torch.float64, device="cuda")
    long_rays = torch.zeros((many + 1, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def raw(accel, rays_p, count, ls, out):
        return la.api.call("scatter_lit_device", accel, rays_p, count, C.addressof(ls) if ls is not None else None, C.addressof(out) if out is not None else None, None)

    amb = (C.c_double * 3)(*AMB)
    table = POOL[:k].copy()
    good_ls = la.CLightSet(table.ctypes.data, k, 0, amb)
    good_out = la.CLitOut(la.CScatterOut(*[dev[p].data_ptr() for p in SCATTER]), dev["terms"].data_ptr(), dev["visible"].data_ptr())
    rp = C.c_void_p(drays.data_ptr())
    refused = [
        raw(acc.h, rp, n, None, good_out),                                                               # a NULL lights
        raw(acc.h, rp, n, la.CLightSet(table.ctypes.data, la.MAX_CALL_LIGHTS + 1, 0, amb), good_out),    # count > LG_MAX_CALL_LIGHTS
        raw(acc.h, rp, n, la.CLightSet(table.ctypes.data, k, 2, amb), good_out),                         # per_ray not 0 or 1
        raw(acc.h, rp, n, la.CLightSet(None, k, 0, amb), good_out),                                      # count > 0 with a NULL table
        raw(acc.h, rp, n, la.CLightSet(None, k, 1, amb), good_out),
        raw(acc.h, rp, n, good_ls, la.CLitOut()),                                                        # all nine planes NULL
        raw(acc.h, rp, n, good_ls, None), raw(None, rp, n, good_ls, good_out), raw(acc.h, None, n, good_ls, good_out),
        raw(acc.h, rp, 0xFFFFFFFF * 64 + 1, good_ls, good_out),                                          # lg_scatter's own limit
        raw(acc.h, rp, 1 << 58, la.CLightSet(table.ctypes.data, 1024, 0, amb), good_out),                # n * K * 72 does not fit size_t
        raw(acc.h, rp, (1 << 64) // 24 // 1024 + 1, la.CLightSet(table.ctypes.data, 1024, 0, amb), good_out),  # n * K * 24
        raw(acc.h, rp, n, la.CLightSet(htab.ctypes.data, k, 1, amb), good_out),                          # a per-ray table in host memory
        raw(acc.h, rp, n, la.CLightSet(dtab.data_ptr() + 4, k, 1, amb), good_out),                       # ... misaligned
        raw(acc.h, rp, many + 1, la.CLightSet(short_tab.data_ptr(), 2, 1, amb), la.CLitOut(la.CScatterOut(), short_terms.data_ptr(), None)),  # ... ends beyond its allocation
    ]
    assert all(r != 0 for r in refused), refused
    call = lambda **kw: G.scatter_lit_device(acc, n, drays, lights=table, ambient=AMB, stream=0, **dict(ptrs, **kw))  # noqa: E731
    bad = [lambda: G.scatter_lit_device(acc, many + 1, long_rays, lights=POOL[:4], terms_ptr=short_terms, stream=0)]  # terms ends beyond its allocation
    for p in PLANES:
        align = 16 if p == "hits" else 4 if p in ("flags", "visible") else 8
        bad.append(lambda p=p, align=align: call(**{p + "_ptr": dev[p].data_ptr() + align // 2}))   # misaligned
        bad.append(lambda p=p: call(**{p + "_ptr": host[p].ctypes.data}))                             # a host pointer
    for j, f in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            f()
        assert str(e.value), j
        print("refused %d: %s" % (j, e.value))
    with pytest.raises(la.LasgunError) as e:
        bad[0]()
    assert "terms ends beyond its allocation" in str(e.value)
    # the host form
    hout = la.CLitOut(la.CScatterOut(*[host[p].ctypes.data for p in SCATTER]), host["terms"].ctypes.data, host["visible"].ctypes.data)
    none = la.CLitOut()
    for args in ((None, rays.ctypes.data, n, C.addressof(good_ls), C.addressof(hout)), (acc.h, None, n, C.addressof(good_ls), C.addressof(hout)),
                 (acc.h, rays.ctypes.data, n, None, C.addressof(hout)), (acc.h, rays.ctypes.data, n, C.addressof(good_ls), None),
                 (acc.h, rays.ctypes.data, n, C.addressof(good_ls), C.addressof(none))):
        assert la.api.call("scatter_lit", *args) != 0 and G.last_error()
    with pytest.raises(ValueError):
        G.scatter_lit(acc, rays[:n], POOL[:k].reshape(1, k))  # a per-ray table of another n
    torch.cuda.synchronize()
    for p in PLANES:
        assert (dev[p].cpu().numpy().view(np.uint32) == FILL).all() and (host[p] == FILL).all(), (p, "no output is touched")
    assert bool((short_terms == FILL).all())
    call()  # ... and served afterwards
    torch.cuda.synchronize()
    want = G.scatter_lit(acc, rays[:n], table, AMB)
    for p in PLANES:
        back = dev[p].cpu().numpy().view(np.uint32)
        assert back[: n * words[p]].tobytes() == want[p].tobytes() and (back[n * words[p]:] == FILL).all(), p
