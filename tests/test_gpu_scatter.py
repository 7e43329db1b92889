"""Surface scatter (include/lasgun_hip.h: lg_scatter, lg_scatter_device): one level of li()'s tree, opened.  The header's composition rule
(tests/scatter_ref.py, compose) over lg_scatter alone must be lg_radiance's value, bit for bit, to any depth.

  1  the composition to depth D on ONE accel equals lg_radiance on an accel built at depth D: three scenes x D in 0 .. 3;
  2  the composition equals the CPU oracle's radiance directly (cornell glass, D = 2);
  3  not vacuous: over the loop's levels a miss, a hit with no child, reflection only, refraction only, both children and a total
     internal reflection inside a solid all occur -- on the CPU witness first, then in the planes;
  4  plane pins: hits, a miss's direct, the reflected child and the transmitted origin restated in numpy, the transmitted direction's two
     closed forms, absent children, flags, two depths;
  5  shapes, traversal forms, both orders, more tiles than twice the grid's waves, plane subsets over garbage, the device form on a
     second stream between guard words, three chunks and more in a fresh process;
  6  32 lights and none;
  7  edge rays: everything that is not NaN bit for bit, NaN where the reference is NaN;
  8  every error of the contract, nothing launched, no output touched.
Compared as bit patterns with every NaN canonicalised (scatter_ref.bits)."""
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
import pyref
import scatter_ref as R
from lasgun_amd import scenes as S
from test_gpu_hit_layers import odd_rays
from test_gpu_radiance_query import each_form, many_lights_scene, oracle_radiance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
W, H = 96, 64
PLANES = la.SCATTER_PLANES
bits = R.bits
if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference accepts it and never reads it)
    pyref.Camera.set_aperture_radius = lambda self, radius: self

SCENES = {
    "kitchen_sink": lambda api: S.kitchen_sink_scene(api, supersampling=0),
    "cornell_glass": lambda api: S.cornell_scene(api, "glass"),
    "spooky": lambda api: S.spooky_scene(api, supersampling=0),
}
BUBBLE_C, BUBBLE_R = (0.0, 0.7, 1.5), 0.5


def classes_scene(api):
    """Cornell glass and three spheres more, so that the reference alone produces every class of ray within two levels: a glass without
    a reflective part (refraction only), a mirror (reflection only), and a glass of eta 0.5 -- the reference's normals always face the
    ray, so a hit is always 'entering', and total internal reflection happens where the medium entered is the thinner one: a ray that
    has entered this sphere meets its surface again from inside and, past 30 degrees, is reflected with no transmitted child."""
    scene = S.cornell_scene(api, "glass")
    M = api.Material
    scene.root.add_sphere([-1.0, 1.0, 0.5], 0.6, M.glass([0.0, 0.0, 0.0], [0.9, 0.9, 0.9], 1.5))
    scene.root.add_sphere(list(BUBBLE_C), BUBBLE_R, M.glass([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], 0.5))
    scene.root.add_sphere([1.0, 1.0, -0.5], 0.6, M.mirror([0.9, 0.9, 0.9]))
    return scene


SCENES["classes"] = classes_scene


def at_depth(name, depth):
    def scene_of(api):
        scene = SCENES[name](api)
        scene.set_max_recursion_depth(depth)
        return scene
    return scene_of


@functools.lru_cache(maxsize=None)
def accel_at(name, depth):
    return G.Accel.from_scene(at_depth(name, depth)(G))


def scatter(accel, planes=PLANES):
    return lambda rays: G.scatter(accel, rays, planes)


def same(ctx, got, want, planes=PLANES):
    for p in planes:
        assert got[p].tobytes() == want[p].tobytes(), (ctx, p, "bytes differ")


def material_table(accel):
    """kind and p[6] (a glass's eta) of every material of the accel, indexable by lg_hit::material (-1: the last row, kind -1)."""
    mats = [G.accel_material(accel, i) for i in range(G.material_count(accel))]
    return np.array([m["kind"] for m in mats] + [-1]), np.array([m["p"][6] for m in mats] + [np.nan])


def in_bubble(rays):
    return np.linalg.norm(rays[:, :3] - np.array(BUBBLE_C), axis=1) < BUBBLE_R


# ---- 1: the composition is lg_radiance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["kitchen_sink", "cornell_glass", "spooky"])
def test_the_composition_to_depth_d_is_lg_radiance_at_depth_d(name, depth):
    built = accel_at(name, depth)
    rays = G.camera_rays(built, W, H)
    want = G.radiance(built, rays)
    assert not np.isnan(want).any(), "the comparison is of numbers"
    one = accel_at(name, 3)  # ONE accel, whatever depth is composed: its own depth plays no part
    got = R.compose(scatter(one), rays, depth)
    assert got.tobytes() == want.tobytes(), (name, depth, int((got.view(np.int64) != want.view(np.int64)).any(axis=1).sum()))
    if depth >= 1:  # the children carry something: the value differs from depth 0's
        assert (got != R.compose(scatter(one), rays, 0)).any(axis=1).mean() >= 0.02, (name, depth)


# ---- 2: ... and the CPU oracle's -----------------------------------------------------------------------------------------------------------
def test_the_composition_is_the_cpu_oracles_radiance():
    want = oracle_radiance(at_depth("cornell_glass", 2), W, H).reshape(-1, 3)
    accel = accel_at("cornell_glass", 0)
    got = R.compose(scatter(accel), G.camera_rays(accel, W, H), 2)
    assert not np.isnan(want).any()
    assert got.tobytes() == want.tobytes(), int((got.view(np.int64) != want.view(np.int64)).any(axis=1).sum())


# ---- 3: not vacuous ------------------------------------------------------------------------------------------------------------------------
CLASSES = ("miss", "no_child", "reflect_only", "refract_only", "both", "tir")


def test_every_class_of_ray_occurs_in_the_loop():
    pscene = classes_scene(pyref.Api)
    accel = accel_at("classes", 2)
    rays = G.camera_rays(accel, W, H)
    # the CPU witness first: the reference alone produces every class (no GPU result is looked at)
    seen = dict.fromkeys(CLASSES, 0)
    for r, lv in R.witness_levels(pscene, rays, 2):
        for k, v in R.classes(lv["flags"], in_bubble(r)).items():
            seen[k] += v
    assert all(seen[k] >= 1 for k in CLASSES), ("the witness", seen)
    # ... then the planes of the loop's levels, and the loop's value
    levels = []
    got = R.compose(scatter(accel), rays, 2, levels)
    assert {d for d, _, _ in levels} == {0, 1, 2}
    seen = dict.fromkeys(CLASSES, 0)
    kinds, _ = material_table(accel)
    for _, r, out in levels:
        glass = kinds[out["hits"]["material"]] == 3
        for k, v in R.classes(out["flags"], in_bubble(r) & glass).items():
            seen[k] += v
    assert all(seen[k] >= 1 for k in CLASSES), ("the planes", seen)
    want = G.radiance(accel, rays)
    assert not np.isnan(want).any() and got.tobytes() == want.tobytes()


# ---- 4: plane pins -------------------------------------------------------------------------------------------------------------------------
# The transmitted direction's closed forms.  Measured on the CPU witness's own transmitted directions (tests/pyref.py, the reference's
# arithmetic in Python) over the three levels of the classes scene's 96 x 64 film: | |wi| - 1 | is at worst 7 * 2^-52 and the Snell
# residual | sin(theta_t) - ratio * sin(theta_i) | at worst 2 * 2^-52 (cornell glass alone: 2 and 2).  The tolerance is that worst case
# and a margin of 4 ulps of 1.0 for the device's rays, which are its own children and not the witness's.
WITNESS_UNIT_ULPS, WITNESS_SNELL_ULPS, MARGIN_ULPS = 7.0, 2.0, 4.0
ULP = 2.0 ** -52


def test_the_planes_are_what_the_header_says():
    accel, shallow = accel_at("classes", 2), accel_at("classes", 0)
    rays = G.camera_rays(accel, W, H)
    # the tolerance, measured here on the witness before the device's directions are looked at
    pscene = classes_scene(pyref.Api)
    unit = snell = 0.0
    for r, lv in R.witness_levels(pscene, rays, 2):
        t = (lv["flags"] & R.REFRACT) != 0
        wi = lv["refract"][t][:, 3:]
        unit, snell = max(unit, R.unit_error(wi).max()), max(snell, R.snell_error(r[t], lv["ns"][t], wi, lv["eta"][t]).max())
    print("witness: unit %.1f ulps, snell %.1f ulps" % (unit / ULP, snell / ULP))
    assert unit <= WITNESS_UNIT_ULPS * ULP and snell <= WITNESS_SNELL_ULPS * ULP, (unit / ULP, snell / ULP, "the figures the tolerance was taken from")
    levels = []
    R.compose(scatter(accel), rays, 2, levels)
    _, etas = material_table(accel)
    counted = np.zeros(4, dtype=np.int64)
    for d, r, out in levels:
        flags, hits = out["flags"], out["hits"]
        hit, has_r, has_t = (flags & R.HIT) != 0, (flags & R.REFLECT) != 0, (flags & R.REFRACT) != 0
        counted += [hit.sum(), (~hit).sum(), has_r.sum(), has_t.sum()]
        assert hits.tobytes() == G.intersect(accel, r).tobytes(), (d, "hits is lg_intersect's record")
        assert np.array_equal(hit, hits["kind"] != 0) and not (flags & ~np.uint32(7)).any() and not ((has_r | has_t) & ~hit).any(), (d, "flags")
        assert out["direct"][~hit].tobytes() == G.radiance(shallow, r)[~hit].tobytes(), (d, "a miss's direct is li()'s background")
        assert np.array_equal(bits(out["reflect"][has_r]), bits(R.reflect_child(r, hits)[has_r])), (d, "the reflected child")
        assert np.array_equal(bits(out["refract"][has_t][:, :3]), bits(R.refract_origin(hits)[has_t])), (d, "the transmitted origin")
        for plane, absent in (("reflect", ~has_r), ("reflect_weight", ~has_r), ("refract", ~has_t), ("refract_weight", ~has_t)):
            assert not out[plane][absent].view(np.uint64).any(), (d, plane, "an absent child's elements are +0.0")
        assert (out["reflect"][has_r][:, 3:] != 0.0).any(axis=1).all() and (out["refract"][has_t][:, 3:] != 0.0).any(axis=1).all(), (d, "a present child has a direction")
        w = out["refract_weight"][has_t]
        assert (w[:, 4] > 0.0).all() and (w[:, 3] > 0.0).all() and (w[:, :3] != 0.0).any(axis=1).all(), (d, "a present child's weights")
        same(("two depths", d), G.scatter(shallow, r), out)
        if not has_t.any():
            continue
        wi = out["refract"][has_t][:, 3:]
        u, s = R.unit_error(wi).max(), R.snell_error(r[has_t], np.ascontiguousarray(hits["ns"])[has_t], wi, etas[hits["material"][has_t]]).max()
        print("level %d: unit %.1f ulps, snell %.1f ulps" % (d, u / ULP, s / ULP))
        assert u <= (WITNESS_UNIT_ULPS + MARGIN_ULPS) * ULP and s <= (WITNESS_SNELL_ULPS + MARGIN_ULPS) * ULP, (d, u / ULP, s / ULP)
    assert (counted >= 100).all(), (counted, "hits, misses and both kinds of children among what was pinned")


# ---- 5: shapes, forms, orders, streams, chunks -----------------------------------------------------------------------------------------------
def take(out, idx):
    return {p: np.ascontiguousarray(out[p][idx]) for p in out}


def test_sizes_and_orders():
    accel = accel_at("classes", 2)
    rays = np.concatenate([G.camera_rays(accel, W, H)[::2], G.camera_rays(accel, 40, 30)])[:4097]
    assert len(rays) == 4097
    ref = G.scatter(accel, rays)
    assert R.classes(ref["flags"])["both"] >= 100 and R.classes(ref["flags"])["miss"] >= 100
    try:
        for order in (0, 1):
            G.set_query_order(accel, order)
            for n in (0, 1, 63, 64, 65, 129, 4097):
                got = G.scatter(accel, rays[:n])
                assert all(got[p].shape[0] == n for p in PLANES)
                same((order, n), got, take(ref, slice(0, n)))
    finally:
        G.set_query_order(accel, 0)
    assert la.api.call("scatter", accel.h, None, 0, None) == 0  # n == 0: a no-op whatever the pointers
    assert la.api.call("scatter_device", None, None, 0, None, None) == 0
    got = accel.scatter(rays[:65], planes=("direct", "flags"))
    assert list(got) == ["direct", "flags"]
    same("accel.scatter", got, take(ref, slice(0, 65)), ("direct", "flags"))


@pytest.mark.parametrize("name", ["classes", "mesh_glass"])
def test_every_form_gives_identical_bytes(name):
    accel = accel_at("classes", 2) if name == "classes" else G.Accel.from_scene(S.mesh_scene(G, nu=48, nv=48, material="glass"))
    rays = G.camera_rays(accel, W, H)[: 64 * 60 + 5]
    ref, checked = None, set()
    try:
        for form in each_form(accel):
            for order in (0, 1):
                G.set_query_order(accel, order)
                got = G.scatter(accel, rays)
                if ref is None:
                    ref = got
                    c = R.classes(ref["flags"])
                    assert c["miss"] and c["both"] + c["reflect_only"] + c["refract_only"] and c["no_child"], c
                    want = G.radiance(accel_at("classes", 1), rays) if name == "classes" else None
                    if want is not None:
                        assert R.compose(scatter(accel), rays, 1).tobytes() == want.tobytes()
                same((name, form, order), got, ref)
            G.set_query_order(accel, 0)
            checked.add(form)
    finally:
        G.set_query_order(accel, 0)
    need = {"reference", "prune", "lds", "lds+prune"} if name == "classes" else {"reference", "prune", "fast"}
    assert need <= checked, (name, checked)


def test_more_tiles_than_twice_the_grids_waves():
    """LDS form: one 1024-lane workgroup per CU, 16 waves each; the set repeated until its 64-ray tiles pass 2 x 16 x CUs."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    accel = accel_at("classes", 2)
    full = G.camera_rays(accel, W, H)
    reps = 1
    while (reps * len(full) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    planes = ("direct", "flags", "refract_weight")
    once = G.scatter(accel, full, planes)
    got = G.scatter(accel, np.ascontiguousarray(np.tile(full, (reps, 1))), planes)
    assert (got["flags"].shape[0] + 63) // 64 > 2 * 16 * cus
    same(reps, got, take(once, np.tile(np.arange(len(full)), reps)), planes)


SUBSETS = [(p,) for p in PLANES] + [("direct", "flags"), ("hits", "reflect", "refract"), ("reflect_weight", "refract_weight", "flags")]
PLANE_WORDS = {"hits": 24, "direct": 6, "flags": 1, "reflect": 12, "reflect_weight": 6, "refract": 12, "refract_weight": 10}  # uint32 words a ray
GUARD, FILL = 64, 0x25A5A5A5


def test_plane_subsets_over_garbage_between_guard_words_on_a_second_stream():
    torch = pytest.importorskip("torch")
    accel = accel_at("classes", 2)
    rays = G.camera_rays(accel, W, H)[: 64 * 30 + 9]
    n = len(rays)
    ref = G.scatter(accel, rays)
    # the host form: the planes asked for over garbage, twice; the others untouched
    rng = np.random.default_rng(5)
    for planes in SUBSETS:
        bufs = {p: rng.integers(1, 2 ** 32, ref[p].size * ref[p].dtype.itemsize // 4, dtype=np.uint64).astype(np.uint32).view(ref[p].dtype).reshape(ref[p].shape)
                for p in PLANES}
        kept = {p: bufs[p].tobytes() for p in PLANES if p not in planes}
        for _ in range(2):
            got = G.scatter(accel, rays, planes, into={p: bufs[p] for p in planes})
            assert all(got[p] is bufs[p] for p in planes)
            same(("host", planes), got, ref, planes)
        assert all(bufs[p].tobytes() == kept[p] for p in kept), ("planes not asked for are untouched", planes)
    # the device form on a second stream: guard words on both sides of every plane
    drays = torch.from_numpy(rays.copy()).cuda()
    stream = torch.cuda.Stream()
    for order in (0, 1):
        G.set_query_order(accel, order)
        try:
            for planes in (PLANES,) + tuple(SUBSETS[7:]):
                dev = {p: torch.full((GUARD + n * PLANE_WORDS[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    s = torch.cuda.current_stream().cuda_stream
                    assert s != 0
                    G.scatter_device(accel, n, drays, stream=s, **{p + "_ptr": dev[p].data_ptr() + 4 * GUARD for p in planes})
                stream.synchronize()
                for p in PLANES:
                    back = dev[p].cpu().numpy().view(np.uint32)
                    assert (back[:GUARD] == FILL).all() and (back[-GUARD:] == FILL).all(), (order, planes, p, "the guard words")
                    if p in planes:
                        assert back[GUARD:-GUARD].tobytes() == ref[p].tobytes(), (order, planes, p)
                    else:
                        assert (back == FILL).all(), (order, planes, p, "not asked for")
        finally:
            G.set_query_order(accel, 0)


CHUNK_PLANES = ("direct", "flags", "refract", "refract_weight")


def chunk_rays(accel):
    """2^20 rays in no order: at the least budget (64 MiB) a chunk of a one-level chain holds about a third of them."""
    rays = G.camera_rays(accel, 1024, 1024)
    return np.ascontiguousarray(rays[np.random.default_rng(4).permutation(len(rays))])


def digests(out):
    return [hashlib.sha256(out[p].tobytes()).hexdigest() for p in CHUNK_PLANES]


def test_many_chunks_give_the_bytes_of_one():
    accel = accel_at("classes", 2)
    want = digests(G.scatter(accel, chunk_rays(accel), CHUNK_PLANES))
    with tempfile.TemporaryDirectory() as tmp:
        op = os.path.join(tmp, "out.txt")
        env = dict(os.environ)
        env.update({"LASGUN_DEBUG": "1", "LASGUN_WF_BUDGET_MB": "64"})
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scatter_child.py"), op], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
        m = re.findall(r"surface scatter: levels (\d+), (\d+) tiles in chunks of (\d+) \([^)]*\), (sorted order|as given)", p.stderr)
        assert [x[3] for x in m] == ["as given", "sorted order"], p.stderr[-3000:]
        for levels, tiles, chunk, _ in m:
            assert int(levels) == 1 and (int(tiles) + int(chunk) - 1) // int(chunk) >= 3, m
        lines = [line.split() for line in open(op).read().splitlines()]
        assert [line[0] for line in lines] == ["0", "1"]
        for line in lines:
            assert line[1:] == want, ("order", line[0])


# ---- 6: lights --------------------------------------------------------------------------------------------------------------------------------
def test_thirty_two_lights_and_none():
    for nlights in (32, 0):
        accel = G.Accel.from_scene(many_lights_scene(G, nlights))
        assert G.light_count(accel) == nlights
        rays = G.camera_rays(accel, 32, 32)
        out = G.scatter(accel, rays)
        hit = (out["flags"] & R.HIT) != 0
        assert hit.any() and (~hit).any() and not (out["flags"] & 6).any()
        want = G.radiance(accel, rays)
        assert R.compose(scatter(accel), rays, 3).tobytes() == want.tobytes(), nlights
        assert out["hits"].tobytes() == G.intersect(accel, rays).tobytes()
        lit = (out["direct"][hit] != 0.0).any(axis=1)
        assert lit.any() if nlights else not lit.any(), (nlights, "a matte sphere with no ambient term: the lights are all there is")


# ---- 7: edge rays -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["classes", "f3", "f7"])
def test_edge_rays_are_bit_for_bit_where_the_reference_is_a_number(case):
    if case == "classes":
        accel, depth = accel_at("classes", 2), 2
        rays = odd_rays(G.camera_rays(accel, W, H)[: 64 * 40 + 17])
    elif case == "f3":
        accel, depth = G.Accel.from_scene(E.f3_scene(G)), 1
        rays = np.ascontiguousarray(E.edge_rays(*E.F3_BOUNDS, boxes=E.F3_BOXES, seed=3)[0])
    else:
        accel, depth = G.Accel.from_scene(E.f7_scene(G)), 1
        rays = np.ascontiguousarray(E.edge_rays(*E.F7_BOUNDS, boxes=E.F7_BOXES, huge=True, seed=7)[0])
    built = accel
    if case != "classes":
        scene = (E.f3_scene if case == "f3" else E.f7_scene)(G)
        scene.set_max_recursion_depth(depth)
        built = G.Accel.from_scene(scene)
    want = G.radiance(built, rays)
    out = G.scatter(accel, rays)
    hits = G.intersect(accel, rays)
    assert (hits["kind"] != 0).any() and (hits["kind"] == 0).any() and not np.isfinite(rays).all(), (case, "hits, misses and rays that are not finite")
    for f in ("t", "p", "ng", "ns"):
        assert np.array_equal(bits(out["hits"][f]), bits(hits[f])), (case, f)
    for f in ("kind", "prim", "instance", "material"):
        assert np.array_equal(out["hits"][f], hits[f]), (case, f)
    got = R.compose(scatter(accel), rays, depth)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (case, "NaN where the reference is NaN, and nowhere else")
    assert np.array_equal(bits(got), bits(want)), (case, int((bits(got) != bits(want)).any(axis=1).sum()))
    if case == "classes":
        assert np.isnan(want).any() and np.isfinite(want).all(axis=1).mean() >= 0.5


# ---- 8: errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch():
    torch = pytest.importorskip("torch")
    import ctypes as C
    accel = accel_at("cornell_glass", 3)
    n = 100
    rays = G.camera_rays(accel, 16, 16)[: n + 1]
    drays = torch.from_numpy(rays.copy()).cuda()
    dev = {p: torch.full((n * PLANE_WORDS[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
    ptrs = {p + "_ptr": dev[p].data_ptr() for p in PLANES}
    host = {p: np.full(n * PLANE_WORDS[p], FILL, dtype=np.uint32) for p in PLANES}
    # For "a buffer that ends beyond its allocation" the buffer has to BE an allocation: torch hands small tensors out of 2 MiB blocks of
    # its own, and the library can only see where a block ends (hipMemGetAddressRange).  2^17 records are 12 MiB, a block of their own
    # (tests/test_gpu_views.py does the same), and the call asks for one record more.
    torch.cuda.empty_cache()
    many = 1 << 17
    short = torch.full((many * 24,), FILL, dtype=torch.int32, device="cuda")
    long_rays = torch.zeros((many + 1, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    call = lambda rp, count=n, acc=accel, **kw: G.scatter_device(acc, count, rp, stream=0, **dict(ptrs, **kw))  # noqa: E731
    bad = [lambda: call(None),
           lambda: G.scatter_device(accel, n, drays, stream=0),                                     # all seven planes NULL
           lambda: call(drays.data_ptr() + 4),                                                      # rays: 8 bytes
           lambda: call(rays.ctypes.data),                                                          # a host pointer
           lambda: call(drays, count=0xFFFFFFFF * 64 + 1),                                          # n > (2^32 - 1) * 64
           lambda: call(drays, count=1 << 62),                                                      # a plane's bytes do not fit size_t
           lambda: G.scatter_device(accel, many + 1, long_rays, hits_ptr=short, stream=0)]         # a buffer that ends beyond its allocation
    for p in PLANES:
        align = 16 if p == "hits" else 4 if p == "flags" else 8
        bad.append(lambda p=p, align=align: call(drays, **{p + "_ptr": dev[p].data_ptr() + align // 2}))   # misaligned
        bad.append(lambda p=p: call(drays, **{p + "_ptr": host[p].ctypes.data}))                             # a host pointer
    for k, f in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            f()
        assert str(e.value), k
        print("refused %d: %s" % (k, e.value))
    with pytest.raises(la.LasgunError) as e:  # ... and that it is refused for the stated reason, with the plane's name
        G.scatter_device(accel, many + 1, long_rays, hits_ptr=short, stream=0)
    assert "hits ends beyond its allocation" in str(e.value)
    torch.cuda.synchronize()
    assert bool((short == FILL).all())
    # the host form: NULL accel, rays, out; all planes NULL
    table = la.CScatterOut(*[host[p].ctypes.data for p in PLANES])
    none = la.CScatterOut()
    for args in ((None, rays.ctypes.data, n, C.addressof(table)), (accel.h, None, n, C.addressof(table)), (accel.h, rays.ctypes.data, n, None),
                 (accel.h, rays.ctypes.data, n, C.addressof(none)), (accel.h, rays.ctypes.data, 0xFFFFFFFF * 64 + 1, C.addressof(table))):
        assert la.api.call("scatter", *args) != 0 and G.last_error()
    # the sorted order's indices are 32-bit
    G.set_query_order(accel, 1)
    try:
        with pytest.raises(la.LasgunError) as e:
            call(drays, count=1 << 32)
        assert "2^32" in str(e.value)
    finally:
        G.set_query_order(accel, 0)
    # 33 lights: lg_radiance's refusal; a recursion depth of 20 is no reason to refuse
    acc33 = G.Accel.from_scene(many_lights_scene(G, 33))
    with pytest.raises(la.LasgunError) as e:
        call(drays, acc=acc33)
    assert "33 lights" in str(e.value)
    assert la.api.call("scatter", acc33.h, rays.ctypes.data, n, C.addressof(table)) != 0
    torch.cuda.synchronize()
    for p in PLANES:
        assert (dev[p].cpu().numpy().view(np.uint32) == FILL).all() and (host[p] == FILL).all(), (p, "no output is touched")
    deep = SCENES["cornell_glass"](G)
    deep.set_max_recursion_depth(20)
    call(drays, acc=G.Accel.from_scene(deep))
    torch.cuda.synchronize()
    want = G.scatter(accel, rays[:n])
    for p in PLANES:
        back = dev[p].cpu().numpy().view(np.uint32)
        assert back[: n * PLANE_WORDS[p]].tobytes() == want[p].tobytes() and (back[n * PLANE_WORDS[p]:] == FILL).all(), (p, "served afterwards, at any depth")
