"""Light groups (include/lasgun_hip.h: lg_radiance_groups, lg_radiance_groups_device): li() of each ray split by subsets of the scene's
lights, G planes from one chain of walks.  Plane g must be lg_radiance's value on an accel rebuilt from 'the same scene with the lights
of groups[g] alone' (tests/light_subsets.py), bit for bit.

  1  every plane against the oracle's capture_radiance (portable trig) of the subset scene, all groups in ONE call on the camera's rays;
     the all-lights-with-ambient plane is lg_radiance's very bytes;
  2  the deepest-level trap: a miss at the deepest level of a recursive scene lives in plane 0 alone until it is spread -- pinned with the
     base group at an index other than 0, and shown from the planes to be exercised;
  3  GPU against GPU on rays that are not the camera's: each plane against lg_radiance on the rebuilt accel;
  4  shapes: n, G (64 with repeated and empty groups), both orders, 32 lights, no lights;
  5  every traversal form, organisation and order gives identical bytes;
  6  many chunks (a fresh process under LASGUN_WF_BUDGET_MB=64) against one, both orders;
  7  the device form on a second stream, guard doubles around the block;
  8  every error of the contract, the output untouched.
Compared as bit patterns with every NaN canonicalised (tests/test_gpu_radiance_query.py, bits)."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import lasgun_amd as la
from lasgun_amd import scenes as S
from light_subsets import light_count, subset_scene, group_pairs
from test_gpu_radiance_query import L0_CASES, L0_FORMS, L0_IDS, TWO_TILES, bits, each_form, l0_scene, many_lights_scene, mixed_rays, oracle_radiance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
W, H = 96, 64

SCENES = {
    "kitchen_r0": lambda api: S.kitchen_sink_scene(api, recursion=0, supersampling=0),
    "kitchen_r1": lambda api: S.kitchen_sink_scene(api, recursion=1, supersampling=0),
    "kitchen_r2": lambda api: S.kitchen_sink_scene(api, recursion=2, supersampling=0),
    "spooky": lambda api: S.spooky_scene(api, supersampling=0),
    "exotic_obj": lambda api: S.exotic_obj_scene(api),
    "cornell_glass": lambda api: S.cornell_scene(api, "glass"),
    "mesh_glass": lambda api: S.mesh_scene(api, nu=48, nv=48, material="glass"),
}


def lg(pairs):
    return [la.LightGroup(m, ambient=a) for m, a in pairs]


@functools.lru_cache(maxsize=None)
def oracle_plane(name, lights, ambient):
    """The oracle's radiance of the subset scene on its own camera's W x H film (the camera is no light: the rays are the full scene's)."""
    want = oracle_radiance(lambda api: subset_scene(api, SCENES[name], lights, ambient), W, H).reshape(-1, 3)
    want.setflags(write=False)
    return want


def differ(a, b):
    """The share of pixels in which two planes differ in any bit."""
    return float((bits(a) != bits(b)).any(axis=1).mean())


# ---- 1: the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitchen_r0", "kitchen_r1", "kitchen_r2", "spooky", "exotic_obj", "cornell_glass"])
def test_every_plane_is_the_oracles_render_of_the_subset_scene(name):
    accel = G.Accel.from_scene(SCENES[name](G))
    nl = G.light_count(accel)
    assert nl == light_count(G, SCENES[name]) and nl >= 1
    pairs = group_pairs(nl)
    rays = G.camera_rays(accel, W, H)
    planes = G.radiance_groups(accel, rays, lg(pairs))  # ONE call
    assert planes.shape == (len(pairs), W * H, 3) and planes.dtype == np.float64
    for g, (m, a) in enumerate(pairs):
        want = oracle_plane(name, m, a)
        assert np.array_equal(bits(planes[g]), bits(want)), (name, g, m, a, int((bits(planes[g]) != bits(want)).any(axis=1).sum()))
    full = pairs.index(((1 << nl) - 1, True))
    assert np.array_equal(planes[full].view(np.int64), G.radiance(accel, rays).view(np.int64)), name  # the very bytes
    if nl >= 2:  # not vacuous: the lights show, and differently
        base, l0, l1 = planes[0], planes[2], planes[3]
        assert differ(l0, base) >= 0.25 and differ(l1, base) >= 0.25 and differ(l0, l1) >= 0.25, (name, differ(l0, base), differ(l1, base), differ(l0, l1))


def test_a_light_whose_attenuation_is_zero_gives_the_base_plane():
    accel = G.Accel.from_scene(SCENES["kitchen_r2"](G))
    rays = G.camera_rays(accel, W, H)
    planes = G.radiance_groups(accel, rays, lg([(0, False), (0b100, False)]))  # kitchen_sink's third light: f_att == 0
    assert planes[0].tobytes() == planes[1].tobytes()


# ---- 2: the deepest-level trap ------------------------------------------------------------------------------------------------------------
TRAP = [(0, True), (0, False), (0b01, False), (0b10, False), (0b111, True)]  # G = 5; the base group is NOT plane 0


def test_a_miss_at_the_deepest_level_reaches_every_plane():
    flat = G.Accel.from_scene(SCENES["kitchen_r0"](G))
    rays = G.camera_rays(flat, W, H)
    base0 = G.radiance_groups(flat, rays, lg(TRAP))[1]
    for name in ("kitchen_r1", "kitchen_r2"):
        accel = G.Accel.from_scene(SCENES[name](G))
        assert np.array_equal(G.camera_rays(accel, W, H), rays)
        planes = G.radiance_groups(accel, rays, lg(TRAP))
        if name == "kitchen_r1":
            # exercised: black without recursion (a hit, no light, no ambient), lit by the background alone one level down -- a specular
            # hit whose child missed at the deepest level
            carried = (base0 == 0.0).all(axis=1) & (planes[1] != 0.0).any(axis=1)
            assert carried.sum() >= 100, int(carried.sum())
        for g, (m, a) in enumerate(TRAP):
            want = oracle_plane(name, m, a)
            assert np.array_equal(bits(planes[g]), bits(want)), (name, g, int((bits(planes[g]) != bits(want)).any(axis=1).sum()))


# ---- 3: GPU against GPU on rays that are not the camera's ---------------------------------------------------------------------------------
def small_batch(accel, n, seed):
    """test_gpu_radiance_query.batch's kind: the camera's rays of a small film, then random rays from around the camera; n in all."""
    rng = np.random.default_rng(seed)
    cam = G.camera_rays(accel, 64, 32)
    extra = n - cam.shape[0]
    o = cam[0, :3] + rng.normal(0.0, 0.5, (extra, 3))
    d = rng.normal(0.0, 1.0, (extra, 3))
    return np.concatenate([cam, np.concatenate([o, d], axis=1)])


@pytest.mark.parametrize("name", ["kitchen_r2", "cornell_glass"])
def test_every_plane_is_lg_radiance_on_the_rebuilt_accel(name):
    accel = G.Accel.from_scene(SCENES[name](G))
    pairs = group_pairs(G.light_count(accel))
    rays = small_batch(accel, 4097, 17)
    planes = G.radiance_groups(accel, rays, lg(pairs))
    for g, (m, a) in enumerate(pairs):
        want = G.radiance(G.Accel.from_scene(subset_scene(G, SCENES[name], m, a)), rays)
        assert np.array_equal(bits(planes[g]), bits(want)), (name, g, m, a, int((bits(planes[g]) != bits(want)).any(axis=1).sum()))
    assert differ(planes[0], planes[pairs.index(((1 << G.light_count(accel)) - 1, True))]) >= 0.05


# ---- 4: shapes ---------------------------------------------------------------------------------------------------------------------------
FIVE = [(0b01, True), (0, False), (0b10, False), (0b111, True), (0, True)]


def test_sizes_group_counts_and_orders():
    accel = G.Accel.from_scene(SCENES["kitchen_r2"](G))
    rays = small_batch(accel, 4097, 5)
    ref = G.radiance_groups(accel, rays, lg(FIVE))
    assert len({ref[g].tobytes() for g in range(5)}) == 5
    sixty_four = [FIVE[i % 5] for i in range(40)] + [(0, False)] * 24  # repeated and empty groups
    tables = {1: [FIVE[3]], 2: FIVE[:2], 5: FIVE, 64: sixty_four}
    for order in (0, 1):
        G.set_query_order(accel, order)
        for n in (0, 1, 63, 64, 65, 129, 4097):
            for k, pairs in tables.items():
                got = G.radiance_groups(accel, rays[:n], lg(pairs))
                assert got.shape == (k, n, 3)
                for g, pair in enumerate(pairs):  # equal groups give equal bytes, wherever they stand in the table
                    assert got[g].tobytes() == ref[FIVE.index(pair), :n].tobytes(), (order, n, k, g)
    G.set_query_order(accel, 0)
    assert la.api.call("radiance_groups", accel.h, None, 0, None, 0, None) == 0  # n == 0: a no-op whatever the pointers
    assert la.api.call("radiance_groups_device", None, None, 0, None, 99, None, None) == 0


def test_thirty_two_lights_and_none():
    builder = lambda api: many_lights_scene(api, 32)  # noqa: E731
    accel = G.Accel.from_scene(builder(G))
    assert G.light_count(accel) == 32
    rays = G.camera_rays(accel, 32, 32)
    pairs = [(1 << 31, False), (1 | 1 << 31, False), (0xFFFFFFFF, True), (0, False)]
    planes = G.radiance_groups(accel, rays, lg(pairs))
    for g, (m, a) in enumerate(pairs):
        want = G.radiance(G.Accel.from_scene(subset_scene(G, builder, m, a)), rays)
        assert np.array_equal(bits(planes[g]), bits(want)), (g, hex(m))
    assert planes[2].tobytes() == G.radiance(accel, rays).tobytes()
    assert len({planes[g].tobytes() for g in range(4)}) == 4
    dark = G.Accel.from_scene(many_lights_scene(G, 0))
    assert G.light_count(dark) == 0
    planes = G.radiance_groups(dark, rays, lg([(0, False), (0, True)]))
    want = G.radiance(dark, rays)
    assert planes[0].tobytes() == want.tobytes() and planes[1].tobytes() == want.tobytes()
    with pytest.raises(la.LasgunError):
        G.radiance_groups(dark, rays, lg([(1, False)]))


# ---- 5: every traversal form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_glass", "mesh_glass"])
def test_every_form_gives_identical_bytes(name):
    accel = G.Accel.from_scene(SCENES[name](G))
    pairs = group_pairs(G.light_count(accel))
    groups = lg(pairs)
    rays = np.concatenate([G.camera_rays(accel, W, H), small_batch(accel, 4097, 13)[2048:]])
    G.set_prune(accel, False)
    fits = G.set_lds_scene(accel, False)
    ref = G.radiance_groups(accel, rays, groups)
    ref_bytes = ref.tobytes()
    assert len(np.unique(ref[-1, :, 0])) > 500 and len({ref[g].tobytes() for g in range(len(pairs))}) >= 4
    checked = []

    def check(form):
        assert G.radiance_groups(accel, rays, groups).tobytes() == ref_bytes, (name, form)
        checked.append(form)

    G.set_prune(accel, True); check("prune")
    if name == "cornell_glass":
        assert fits, "a scene of a few dozen triangles fits the LDS"
    if fits:
        G.set_prune(accel, False); G.set_lds_scene(accel, True); check("lds")
        G.set_prune(accel, True); check("lds+prune")
    G.set_prune(accel, None)
    try:
        G.set_mode(accel, True)
    except la.LasgunError:
        assert name != "mesh_glass", "the small torus scene admits the fast mode"
    else:
        check("fast")
        G.set_mode(accel, False)
    for org in (0, 3, 1):
        G.set_streaming(accel, org)
        check("streaming %d" % org)
    G.set_query_order(accel, 1)
    check("order 1")
    G.set_lds_scene(accel, False); check("order 1, tables in L2"); G.set_lds_scene(accel, True)
    G.set_query_order(accel, 0)
    G.set_lds_scene(accel, False); check("tables in L2")
    assert {"prune", "order 1", "tables in L2"} <= set(checked)


# ---- 6: chunks -----------------------------------------------------------------------------------------------------------------------------
EIGHT = [(0, False), (0, True), (1, False), (1, True), (0, False), (1, False), (0, True), (1, True)]


def test_many_chunks_give_the_bytes_of_one():
    accel = G.Accel.from_scene(SCENES["cornell_glass"](G))
    n = 1 << 17
    rays = G.camera_rays(accel, 512, 256)
    assert rays.shape[0] == n
    rays = rays[np.random.default_rng(4).permutation(n)]
    ref = G.radiance_groups(accel, rays, lg(EIGHT))
    assert ref[0].tobytes() != ref[3].tobytes()
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.npy"), os.path.join(tmp, "out.npy")
        np.save(rp, rays)
        for order in (0, 1):
            env = dict(os.environ)
            env.update({"LASGUN_DEBUG": "1", "LASGUN_WF_BUDGET_MB": "64"})
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "radiance_groups_child.py"), "cornell_glass", rp, op, str(order)], capture_output=True,
                               text=True, timeout=600, env=env)
            assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
            m = re.findall(r"radiance groups: levels \d+, (\d+) tiles in chunks of (\d+) \([^)]*\), (sorted order|as given), 8 groups", p.stderr)
            assert m and m[-1][2] == ("sorted order" if order else "as given"), p.stderr[-3000:]
            assert (int(m[-1][0]) + int(m[-1][1]) - 1) // int(m[-1][1]) >= 3, m[-1]
            assert np.load(op).tobytes() == ref.tobytes(), order


# ---- 7: the device form ----------------------------------------------------------------------------------------------------------------------
def test_the_device_form_on_a_second_stream_writes_its_block_alone():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(SCENES["kitchen_r2"](G))
    rays = small_batch(accel, 4097, 9)
    n, k, guard = rays.shape[0], len(FIVE), 64
    ref = G.radiance_groups(accel, rays, lg(FIVE))
    stream = torch.cuda.Stream()
    dr = torch.from_numpy(rays.copy()).cuda()
    for order in (1, 0):
        G.set_query_order(accel, order)
        buf = torch.full((guard + k * n * 3 + guard,), -7.5, dtype=torch.float64, device="cuda")
        buf[guard:-guard] = float("nan")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            G.radiance_groups_device(accel, n, dr, lg(FIVE), buf.data_ptr() + 8 * guard, stream=torch.cuda.current_stream().cuda_stream)
        stream.synchronize()
        got = buf.cpu().numpy()
        assert (got[:guard] == -7.5).all() and (got[-guard:] == -7.5).all(), order
        assert got[guard:-guard].tobytes() == ref.tobytes(), order


# ---- 8: errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_reported_and_nothing_is_launched():
    torch = pytest.importorskip("torch")
    accel = G.Accel.from_scene(SCENES["cornell_glass"](G))  # one light
    assert G.light_count(accel) == 1
    n = 100
    rays = G.camera_rays(accel, 16, 16)[: n + 1]
    dr = torch.from_numpy(rays.copy()).cuda()
    do = torch.full((2 * (n + 1) * 3,), float("nan"), dtype=torch.float64, device="cuda")
    host_out = np.full((2, n, 3), np.nan)
    two = lg([(0, False), (1, True)])
    torch.cuda.synchronize()
    dev = lambda rp, groups, op, count=n: G.radiance_groups_device(accel, count, rp, groups, op, stream=0)  # noqa: E731
    bad = [lambda: dev(None, two, do.data_ptr()),
           lambda: dev(dr.data_ptr(), two, None),
           lambda: dev(dr.data_ptr() + 4, two, do.data_ptr()),
           lambda: dev(dr.data_ptr(), two, do.data_ptr() + 4),
           lambda: dev(rays.ctypes.data, two, do.data_ptr()),        # host pointers
           lambda: dev(dr.data_ptr(), two, host_out.ctypes.data),
           lambda: dev(dr.data_ptr(), [], do.data_ptr()),                                        # n_groups == 0
           lambda: dev(dr.data_ptr(), lg([(0, False)] * 65), do.data_ptr()),                     # > LG_MAX_LIGHT_GROUPS
           lambda: dev(dr.data_ptr(), lg([(0, False), (0b10, False)]), do.data_ptr()),           # a light the scene does not have
           lambda: dev(dr.data_ptr(), [la.LightGroup(1, flags=2)], do.data_ptr()),               # an unknown flag
           lambda: dev(dr.data_ptr(), two, do.data_ptr(), count=(0xFFFFFFFF * 64) + 1),         # n > MAX_RAYS
           lambda: dev(dr.data_ptr(), lg([(0, False)] * 64), do.data_ptr(), count=1 << 60)]      # n * n_groups * 24 overflows
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    host_bad = [lambda: G.radiance_groups(accel, rays[:n], [], into=None),
                lambda: G.radiance_groups(accel, rays[:n], lg([(0, False)] * 65)),
                lambda: G.radiance_groups(accel, rays[:n], lg([(0b10, False)])),
                lambda: G.radiance_groups(accel, rays[:n], [la.LightGroup(0, flags=0x80000000)])]
    for k, call in enumerate(host_bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    table = (la.CLightGroup * 2)(*two)
    import ctypes as C
    tp = C.addressof(table)
    for args in ((accel.h, None, n, tp, 2, host_out.ctypes.data), (accel.h, rays.ctypes.data, n, None, 2, host_out.ctypes.data),
                 (accel.h, rays.ctypes.data, n, tp, 2, None), (None, rays.ctypes.data, n, tp, 2, host_out.ctypes.data),
                 (accel.h, rays.ctypes.data, n, tp, 0, host_out.ctypes.data), (accel.h, rays.ctypes.data, n, tp, 65, host_out.ctypes.data)):
        assert la.api.call("radiance_groups", *args) != 0 and G.last_error()
    assert np.isnan(host_out).all()
    # the sorted order's indices are 32-bit
    G.set_query_order(accel, 1)
    with pytest.raises(la.LasgunError) as e:
        dev(dr.data_ptr(), two, do.data_ptr(), count=1 << 32)
    assert "2^32" in str(e.value)
    G.set_query_order(accel, 0)
    # 33 lights and recursion 20: lg_radiance's two refusals
    acc33 = G.Accel.from_scene(many_lights_scene(G, 33))
    with pytest.raises(la.LasgunError) as e:
        G.radiance_groups_device(acc33, n, dr.data_ptr(), lg([(0, False)]), do.data_ptr(), stream=0)
    assert "33 lights" in str(e.value)
    deep = many_lights_scene(G, 1)
    deep.set_max_recursion_depth(20)
    with pytest.raises(la.LasgunError) as e:
        G.radiance_groups_device(G.Accel.from_scene(deep), n, dr.data_ptr(), lg([(0, False)]), do.data_ptr(), stream=0)
    assert "recursion" in str(e.value)
    torch.cuda.synchronize()
    assert np.isnan(do.cpu().numpy()).all()
    # ... and the call is served afterwards
    dev(dr.data_ptr(), two, do.data_ptr())
    torch.cuda.synchronize()
    assert do.cpu().numpy()[: 2 * n * 3].tobytes() == G.radiance_groups(accel, rays[:n], two).tobytes()


# ---- level 0's shared bodies: two tiles, the last one partial, in every form, KIND and order (test_gpu_radiance_query.py, section 6) -----
@pytest.mark.parametrize("name,builder,kind", L0_CASES, ids=L0_IDS)
def test_two_tiles_in_every_form_and_order_give_the_oracles_planes(name, builder, kind):
    scene_of = l0_scene(builder, kind)
    accel = G.Accel.from_scene(scene_of(G))
    pairs = group_pairs(G.light_count(accel))
    checked = set()
    for w, h in TWO_TILES:
        rays = G.camera_rays(accel, w, h)
        mixed_rays(accel, rays, (name, kind, w, h))
        want = [bits(oracle_radiance(lambda api: subset_scene(api, scene_of, m, a), w, h).reshape(-1, 3)) for m, a in pairs]
        for form in each_form(accel):
            for order in (0, 1):
                G.set_query_order(accel, order)
                planes = G.radiance_groups(accel, rays, lg(pairs))
                for g in range(len(pairs)):
                    assert np.array_equal(bits(planes[g]), want[g]), (name, kind, form, order, w * h, g, pairs[g])
            G.set_query_order(accel, 0)
            checked.add(form)
    assert L0_FORMS[name] <= checked, (name, checked)
