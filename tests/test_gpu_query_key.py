"""The sorted ray order of ray queries against things that are not the library (k_sort.hip, raykey.h, query.cpp: world_key_bounds):
  1. the key: what the device returns for a ray is, bit for bit, what the numpy restatement of the documented layout gives
     (tests/raykey_ref.py, itself held to raykey.h on the CPU by tests/test_raykey_host.py), on rays that sit on every border of the
     layout (tests/raykey_cases.py), in scenes whose bounds come from the independent witness -- one of them with a rotated, unevenly
     scaled root, where the corners of the world bounds matter; and the layout's own promises, asked of the device's keys directly;
  2. the sort at the sizes where its launch shape changes (k_sort.hip: sort_items, sort_blocks, the scan's 128 tiles), random keys and
     three keys in long runs;
  3. a walk through a permutation of that size: the same bytes as the walk in the caller's order."""
import numpy as np
import pytest

import pyref

import edge_rays as E
import lasgun_amd as la
import raykey_cases as C
import raykey_ref as R
from lasgun_amd import scenes as S
from query_witness import Witness
from test_gpu_ray_query_order import scene_box, traversal_forms

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = la.api
FILL = 0xA5A5A5A5


def words(n):
    return torch.full((n,), FILL - (1 << 32), dtype=torch.int32, device="cuda")


def device_order(accel, n, rays_dev, perm_dev, keys_dev):
    """(perm, keys) of the first n rays of rays_dev through lg_query_order_device; perm_dev and keys_dev are refilled with 0xA5 first
    and nothing past their n-th word may change."""
    perm_dev.fill_(FILL - (1 << 32))
    keys_dev.fill_(FILL - (1 << 32))
    torch.cuda.synchronize()
    G.query_order_device(accel, n, rays_dev.data_ptr(), perm_dev.data_ptr(), keys_dev.data_ptr(), stream=0)
    torch.cuda.synchronize()
    perm, keys = perm_dev.cpu().numpy().view(np.uint32), keys_dev.cpu().numpy().view(np.uint32)
    assert (perm[n:] == FILL).all() and (keys[n:] == FILL).all(), "words past the n-th were written"
    return perm[:n], keys[:n]


def first_difference(got, want, rays=None):
    bad = np.nonzero(got != want)[0]
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return (len(bad), i, None if rays is None else rays[i].tolist(), hex(int(got[i])), hex(int(want[i])))


# ---- 1: the key ---------------------------------------------------------------------------------------------------------------------
KEY_SCENES = [("grid", E.grid_scene), ("instanced", S.instanced_scene), ("rotated_root", C.rotated_root_scene)]


@pytest.mark.parametrize("name,builder", KEY_SCENES, ids=[s[0] for s in KEY_SCENES])
def test_device_keys_are_the_restated_keys(name, builder):
    wit = Witness(builder(pyref.Api))
    box, m = wit.root.nodes[0][0], wit.root.m
    lo, hi = R.world_bounds(box[0], box[1], m)
    if name == "rotated_root":  # (on the CPU: the corners matter here)
        two = np.array([pyref.transform_point(m, box[0]), pyref.transform_point(m, box[1])])
        assert not np.array_equal(lo, two.min(axis=0)) and not np.array_equal(hi, two.max(axis=0))
    else:
        assert m == pyref.mat_identity()
    bounds = R.key_bounds(lo, hi)
    rays = C.key_ray_set(lo, hi, seed=len(name))
    assert 150000 <= len(rays) <= 250000
    C.check_reach(rays, bounds)
    want = R.ray_key(rays, bounds)
    assert want.dtype == np.uint32

    accel = G.Accel.from_scene(builder(G))
    perm, keys = G.query_order(accel, rays)
    assert first_difference(keys, want, rays) is None
    assert np.array_equal(perm, np.argsort(want, kind="stable").astype(np.uint32))
    n = len(rays)
    dr = torch.from_numpy(rays).cuda()
    dperm, dkeys = device_order(accel, n, dr, words(n + 64), words(n + 64))
    assert first_difference(dkeys, want, rays) is None
    assert np.array_equal(dperm, perm)
    # the layout, asked of the device's keys without the restatement
    C.check_layout(lambda r: G.query_order(accel, r)[1], lo, hi)


# ---- 2: the sort at its sizing limits -----------------------------------------------------------------------------------------------
# k_sort.hip: a pass cuts n elements into nblocks chunks of SORT_BLOCK * items elements, a workgroup each, walked in `items` rounds of
# SORT_BLOCK; the counts (SORT_DIGITS per chunk) are scanned in tiles of SCAN_TILE.
SORT_BLOCK, SORT_MAX_BLOCKS, SORT_MIN_ITEMS, SORT_DIGITS, SCAN_TILE = 256, 2048, 4, 256, 4096


def sort_shape(n):
    """(items, nblocks, scan tiles, elements in the last chunk, rounds of the last chunk that are wholly past n): sort_items, sort_blocks
    and launch_query_order restated."""
    items = max(SORT_MIN_ITEMS, -(-n // (SORT_BLOCK * SORT_MAX_BLOCKS)))
    nblocks = -(-n // (SORT_BLOCK * items))
    last = n - (nblocks - 1) * SORT_BLOCK * items
    return items, nblocks, -(-SORT_DIGITS * nblocks // SCAN_TILE), last, items - -(-last // SORT_BLOCK)


FULL = SORT_BLOCK * SORT_MAX_BLOCKS * SORT_MIN_ITEMS  # 2^21: the most elements at the smallest chunk size
STEP = SORT_BLOCK * SORT_MAX_BLOCKS                   # 2^19: every further STEP elements are one more round per chunk
# n -> the shape it must have (a change of the constants above fails here first, and shows which sizes to move)
SORT_SIZES = {
    FULL - 1: (4, 2048, 128, 1023, 0),            # every chunk and every scan tile in use, the last round one lane short
    FULL: (4, 2048, 128, 1024, 0),                # ... exactly full: 2^19 counts, all 128 lanes of the scan's tile sums live
    FULL + 1: (5, 1639, 103, 513, 2),             # the first items = 5; the last chunk ends two rounds early
    5 * STEP: (5, 2048, 128, 1280, 0),            # items = 5, 2048 full chunks
    5 * STEP + 1: (6, 1707, 107, 1025, 1),        # the first items = 6; a round of one element, then an empty one
    6 * SORT_BLOCK * 1707 + 1: (6, 1708, 107, 1, 5),  # a last chunk of one element and five empty rounds
    3000003: (6, 1954, 123, 195, 5),              # a ragged tail
}
RUNS = (1, 63, 64, 65, 255, 257, 1279, 1281)  # run lengths of equal keys: either side of a wave, a round and a chunk of 5 rounds


def test_the_sort_sizes_reach_the_regimes_they_name():
    assert (FULL, STEP) == (1 << 21, 1 << 19)
    for n, shape in SORT_SIZES.items():
        assert sort_shape(n) == shape, (n, sort_shape(n))
    assert sort_shape(1150037)[:3] == (4, 1124, 71)  # (the largest sort of tests/test_gpu_ray_query_order.py)
    assert max(s[2] for s in SORT_SIZES.values()) == SORT_DIGITS * SORT_MAX_BLOCKS // SCAN_TILE == 128


@pytest.fixture(scope="module")
def sort_inputs():
    """One accel, one device copy of each ray set at the largest size (every n takes a prefix) and their restated keys."""
    nmax = max(SORT_SIZES)
    wit = Witness(S.spheres_scene(pyref.Api))
    box = wit.root.nodes[0][0]
    lo, hi = R.world_bounds(box[0], box[1], wit.root.m)
    bounds = R.key_bounds(lo, hi)
    rng = np.random.default_rng(21)
    random = np.concatenate([rng.uniform(lo, hi, (nmax, 3)), rng.normal(0.0, 1.0, (nmax, 3))], axis=1)
    want_random = R.ray_key(random, bounds)
    # three rays in runs: the later ray has the smaller key somewhere, so that no pass is the identity
    three = np.array([tuple(hi - 0.01 * (hi - lo)) + (0.3, -0.2, -1.0), tuple(lo + 0.01 * (hi - lo)) + (-0.5, 0.4, 0.7),
                      tuple(0.5 * (lo + hi)) + (0.9, 0.1, -0.05)])
    key3 = R.ray_key(three, bounds)
    assert len(set(key3.tolist())) == 3 and key3[0] > key3[1]
    which = np.repeat(np.arange(-(-nmax // sum(RUNS)) * len(RUNS)) % 3, np.tile(RUNS, -(-nmax // sum(RUNS))))[:nmax]
    assert len(which) == nmax
    accel = G.Accel.from_scene(S.spheres_scene(G))
    data = {"accel": accel, "perm": words(nmax + 64), "keys": words(nmax + 64),
            "random": (torch.from_numpy(random).cuda(), want_random), "runs": (torch.from_numpy(np.ascontiguousarray(three[which])).cuda(), key3[which])}
    yield data
    data.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", sorted(SORT_SIZES), ids=["n=%d" % n for n in sorted(SORT_SIZES)])
def test_the_sort_at_its_sizing_limits(sort_inputs, n):
    items = sort_shape(n)[0]
    for which in ("random", "runs"):
        rays_dev, want = sort_inputs[which]
        want = want[:n]
        if which == "random":  # every pass has something to do in every digit
            for byte in range(4):
                assert len(np.unique((want >> np.uint32(8 * byte)) & np.uint32(0xFF))) >= 200, byte
        perm, keys = device_order(sort_inputs["accel"], n, rays_dev, sort_inputs["perm"], sort_inputs["keys"])
        assert first_difference(keys, want) is None, which
        bad = first_difference(perm, np.argsort(want, kind="stable").astype(np.uint32))
        if bad is not None:
            slot = bad[1]
            chunk, rest = divmod(slot, SORT_BLOCK * items)
            pytest.fail("%s, n = %d: %d slots differ, the first is slot %d (chunk %d of the output, round %d, wave %d, lane %d): perm %s, want %s"
                        % (which, n, bad[0], slot, chunk, rest // SORT_BLOCK, rest % SORT_BLOCK // 64, rest % 64, bad[3], bad[4]))


# ---- 3: a walk through a permutation of that size -----------------------------------------------------------------------------------
WALKS = [("spheres", lambda: S.spheres_scene(G), "lds"), ("mixed", lambda: S.mixed_scene(G, nspheres=256, nu=64, nv=64), "prune")]


@pytest.mark.parametrize("name,builder,form", WALKS, ids=[w[0] for w in WALKS])
def test_a_sorted_walk_of_two_million_rays_gives_identical_bytes(name, builder, form):
    n = FULL + 1
    accel = G.Accel.from_scene(builder())
    setup = dict(traversal_forms(accel))
    assert form in setup, (name, sorted(setup))
    rng = np.random.default_rng(31 + len(name))
    lo, hi = scene_box(accel)
    cam = G.camera_rays(accel, 448, 448)
    cam = cam[rng.permutation(len(cam))]
    cam[:, 3:] *= rng.uniform(0.05, 4.0, (len(cam), 1))  # (t < 1 and t >= 1 both occur)
    copies = 8
    tiled = np.tile(cam, (copies, 1))
    tiled[:, :3] += np.repeat(rng.normal(0.0, 0.05, (copies, 3)), len(cam), axis=0)  # (each copy from its own eye)
    k = n - len(tiled)
    assert k > n // 8
    o = rng.uniform(lo - (hi - lo), hi + (hi - lo), (k, 3))
    d = (rng.uniform(lo, hi, (k, 3)) - o) * rng.uniform(0.3, 3.0, (k, 1))
    rays = np.concatenate([tiled, np.concatenate([o, d], axis=1)])
    rays = np.ascontiguousarray(rays[rng.permutation(n)])
    assert len(rays) == n

    dr = torch.from_numpy(rays).cuda()
    out = []
    for order in (0, 1):
        setup[form]()
        G.set_query_order(accel, order)
        dh = torch.full((n * 96,), 0xA5, dtype=torch.uint8, device="cuda")
        do = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        G.intersect_device(accel, n, dr.data_ptr(), dh.data_ptr(), stream=0)
        G.occluded_device(accel, n, dr.data_ptr(), do.data_ptr(), stream=0)
        torch.cuda.synchronize()
        out.append((dh, do))
    G.set_query_order(accel, 0)
    (h0, o0), (h1, o1) = out
    if not torch.equal(h0, h1):
        rec = (h0.view(n, 96) != h1.view(n, 96)).any(dim=1).nonzero().flatten()
        pytest.fail("%s, %s: closest hits differ in %d rays, the first is ray %d" % (name, form, len(rec), int(rec[0])))
    if not torch.equal(o0, o1):
        rec = (o0 != o1).nonzero().flatten()
        pytest.fail("%s, %s: occlusion bytes differ in %d rays, the first is ray %d" % (name, form, len(rec), int(rec[0])))
    occ = o0.cpu().numpy()
    assert set(np.unique(occ).tolist()) == {0, 1}, "some segments are blocked and some are not"
    kind = h0.view(n, 96)[:, 80:84].cpu().numpy().copy().view(np.uint32).ravel()  # (lg_hit.kind, offset 80)
    assert (kind != 0).sum() > n // 16, ((kind != 0).sum(), n)
