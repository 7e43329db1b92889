"""Hit layers (include/lasgun_hip.h: lg_hit_layers, lg_hit_layers_device): the first K surfaces along each ray in one launch, the next
segment started in the kernel at the hit's p - ng * 2^-36, the answer as layer-major planes.

The reference is the contract restated in numpy over lg_intersect (`chain`): a loop of K calls, o' = p - ng * 2.0**-36 (one product, one
subtraction per component), the direction's bits kept, the rays compacted between the calls, the planes assembled layer-major, T and inside
added sequentially in f64 (a NaN stays, as the header says: numpy alone does not say which of two NaNs a sum returns).  NOTHING is tolerated: every plane is compared as uint32 words, NaNs included.

  1  every traversal form, all five planes, K in {1, 2, 3, 8} on the subset (65 poses x 129 beams of the range-scan inputs made explicit,
     pose-major: 131 full tiles and a partial one), and runs of 1, 63, 64, 65 and 129 rays taken from it -- the single ray once with count 0
     and once with count >= 3; for K = 1, hits[0] is lg_intersect's array itself and along[0] its t;
  2  the accel's default form against the same loop over the CPU oracle's intersect, K = 8, the full 257 x 1031 set: count, along and inside
     bit for bit, kind / prim / instance equal, a material exactly where there is a hit;
  3  lg_accel_set_query_order(1) on the shuffled subset: the bytes of order 0;
  4  (LDS form) more tiles than twice the grid's waves: the tile claim's other path;
  5  outputs: every plane alone and three subsets over garbage, the same call twice; the device form on a stream that is not the default
     one over a 0x25A5A5A5 prefill with guard words behind every buffer, planes not asked for untouched;
  6  edge inputs against the restatement: NaN, +-inf, -0.0 and zero directions, origins at 1e300, the edge-case rays of tests/edge_rays.py;
  7  every error of the contract refused with every output at its prefill; n == 0 a no-op even with NULL everything.
No vacuous comparison, asserted on the reference's answer before anything is compared: on the subset at least 15 % of the rays have count 0,
15 % count >= 1 and 3 % count >= 3; at least half of the full tiles hold both a lane with count 0 and a lane with count >= 3 (the
wave-divergent ending); at K = 2 and K = 3 at least 3 % of the rays reach K; at K = 8 a ray of `instanced` and of `mesh_glass` has count >= 5."""
import ctypes

import numpy as np
import pytest

import edge_rays as E
import lasgun_amd as la
from lasgun_amd import _capi
from oracle_lib import oracle
from test_gpu_visibility import SCENES, FORMS, set_form, reset
from test_gpu_range_scan import scan_inputs, explicit_rays

pytestmark = pytest.mark.gpu

G = la.api
PLANES = la.LAYER_PLANES
KS = (1, 2, 3, 8)
STEP = 2.0 ** -36
MISS = np.zeros(1, dtype=la.HIT_DTYPE)
MISS["t"], MISS["prim"], MISS["instance"], MISS["material"] = np.inf, 0xFFFFFFFF, 0xFFFFFFFF, -1
MISS_ID = np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)


def id_words(h):
    return np.stack([h["kind"], h["prim"], h["instance"], h["material"].view(np.uint32)], axis=1).astype(np.uint32)


def keep_nan(a, b):
    """b, but a where a is NaN: the contract's 'a NaN stays' (which of two NaNs numpy's own sum returns depends on the length of the array)."""
    return np.where(np.isnan(a), a, b)


def chain(intersect, rays, K):
    """The contract restated: the five planes of K layers of `rays` from K calls of `intersect` (an (m, 6) array -> m lg_hit records)."""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = len(rays)
    hits = np.repeat(MISS, K * n).reshape(K, n)
    along = np.full((K, n), np.inf)
    ident = np.tile(MISS_ID, (K, n, 1))
    count, inside, T = np.zeros(n, dtype=np.uint32), np.zeros(n), np.zeros(n)
    live, cur = np.arange(n), rays.copy()
    for j in range(K):
        if len(live) == 0:
            break
        h = intersect(cur)
        hit = h["kind"] != 0
        hits[j, live], ident[j, live] = h, id_words(h)
        on, t = live[hit], h["t"][hit]
        with np.errstate(invalid="ignore", over="ignore"):
            T[on] = t if j == 0 else keep_nan(T[on], T[on] + t)
            along[j, on] = T[on]
            if j & 1:
                inside[on] = keep_nan(inside[on], inside[on] + t)
            count[on] += 1
            nxt = cur[hit].copy()
            nxt[:, :3] = keep_nan(h["p"][hit], h["p"][hit] - h["ng"][hit] * STEP)
        live, cur = on, np.ascontiguousarray(nxt)
    out = {"hits": hits, "along": along, "id": ident, "count": count, "inside": inside}
    for v in out.values():
        v.setflags(write=False)
    return out


def take(want, idx):
    """The planes of the rays `idx` of a reference (per ray: a layer of a ray depends on that ray alone)."""
    return {p: np.ascontiguousarray(want[p][:, idx] if p in ("hits", "along", "id") else want[p][idx]) for p in PLANES}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare(ctx, got, want, planes=PLANES):
    assert set(got) == set(planes), (ctx, sorted(got))
    for p in planes:
        g, w = got[p], want[p]
        assert g.shape == w.shape and g.dtype == w.dtype, (ctx, p, g.shape, w.shape, g.dtype, w.dtype)
        diff = words(g).reshape(-1) != words(w).reshape(-1)
        assert not diff.any(), (ctx, p, int(diff.sum()), "words differ; first at word", int(np.argmax(diff)), "of", diff.size)


_setup = {}


def setup(name):
    """(accel, subset rays, full rays) of a scene, built once: poses[::4] x beams[::8] and poses x beams, pose-major."""
    if name not in _setup:
        poses, beams = scan_inputs(name)
        sub = explicit_rays(np.ascontiguousarray(poses[::4]), None, np.ascontiguousarray(beams[::8]))
        assert sub.shape == (65 * 129, 6) == (8385, 6) and len(sub) // 64 == 131 and len(sub) % 64 == 1
        _setup[name] = (G.Accel.from_scene(SCENES[name](G)), sub, explicit_rays(poses, None, beams))
    return _setup[name]


_ref = {}


def reference(name, form, accel, K):
    """The subset's planes by the loop over lg_intersect in the accel's current form; computed once per (scene, form, K), never changed."""
    if (name, form, K) not in _ref:
        _ref[name, form, K] = chain(lambda r: G.intersect(accel, r), setup(name)[1], K)
    return _ref[name, form, K]


def mixed_tiles(count):
    """Per full 64-ray tile: it holds a lane with count 0 and a lane with count >= 3."""
    c = count[:len(count) // 64 * 64].reshape(-1, 64)
    return (c == 0).any(axis=1) & (c >= 3).any(axis=1)


def not_vacuous(name, form, accel):
    w8 = reference(name, form, accel, 8)
    c = w8["count"]
    assert (c == 0).mean() >= 0.15 and (c >= 1).mean() >= 0.15 and (c >= 3).mean() >= 0.03, (name, form, (c == 0).mean(), (c >= 1).mean(), (c >= 3).mean())
    m = mixed_tiles(c)
    assert 2 * int(m.sum()) >= len(m) == 131, (name, form, "tiles mixing a lane with count 0 and a lane with count >= 3", int(m.sum()), len(m))
    for K in (2, 3):
        assert (reference(name, form, accel, K)["count"] == K).mean() >= 0.03, (name, form, K, "rays that reach K")
    if name in ("instanced", "mesh_glass"):
        assert (c >= 5).any(), (name, form, "a ray with count >= 5")


def layers(accel, rays, K, planes=PLANES):
    return G.hit_layers(accel, rays, K, planes)


# ---- 1: bit for bit against the restatement, every form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_planes_equal_the_restatement(name, form):
    accel, sub, _ = setup(name)
    set_form(accel, form)
    try:
        not_vacuous(name, form, accel)
        c8 = reference(name, form, accel, 8)["count"]
        start = 64 * int(np.argmax(mixed_tiles(c8)))  # the first tile with the wave-divergent ending
        ones = [int(np.argmax(c8 == 0)), int(np.argmax(c8 >= 3))]
        assert c8[ones[0]] == 0 and c8[ones[1]] >= 3
        first = G.intersect(accel, sub)
        for K in KS:
            want = reference(name, form, accel, K)
            got = layers(accel, sub, K)
            compare((name, form, K, "subset"), got, want)
            if K == 1:
                assert got["hits"][0].tobytes() == first.tobytes(), "for K = 1, hits[0] is lg_intersect's array itself"
                assert got["along"][0].tobytes() == first["t"].tobytes(), "... and along[0] its t"
            for n in (63, 64, 65, 129):
                idx = np.arange(start, start + n)
                part = take(want, idx)
                if n >= 64:  # (the whole mixed tile is in)
                    assert (part["count"] == 0).any() and (part["count"] >= min(K, 3)).any(), (name, form, K, n)
                compare((name, form, K, n), layers(accel, np.ascontiguousarray(sub[idx]), K), part)
            for i in ones:  # n = 1: once a ray with count 0, once a ray with count >= 3
                part = take(want, np.array([i]))
                assert int(part["count"][0]) == min(int(c8[i]), K)
                compare((name, form, K, "one ray", i), accel.hit_layers(sub[i:i + 1].copy(), K, PLANES), part)
    finally:
        reset(accel)


# ---- 2: against the CPU oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_glass", "instanced", "mesh_glass"])
def test_count_along_inside_and_ids_equal_the_cpu_oracles_chain(name):
    accel, _, full = setup(name)
    assert len(full) == 257 * 1031
    o = oracle()
    oaccel = o.Accel(SCENES[name](o))
    o.set_trig_mode(True)
    try:
        want = chain(lambda r: o.intersect(oaccel, r, 16)[0], full, 8)
    finally:
        o.set_trig_mode(False)
    c = want["count"]
    assert (c == 0).mean() >= 0.15 and (c >= 1).mean() >= 0.15 and (c >= 3).mean() >= 0.03, (name, "oracle")
    got = layers(accel, full, 8, ("along", "id", "count", "inside"))
    compare((name, "oracle"), {p: got[p] for p in ("count", "along", "inside")}, want, ("count", "along", "inside"))
    assert np.array_equal(got["id"][..., :3], want["id"][..., :3]), (name, "kind, prim, instance")
    assert np.array_equal(got["id"][..., 3] == 0xFFFFFFFF, want["id"][..., 0] == 0), (name, "a material exactly where there is a hit")


# ---- 3: query order 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "prune")])
def test_the_sorted_order_gives_the_bytes_of_the_given_order(name, form):
    accel, sub, _ = setup(name)
    shuffle = np.random.default_rng(19).permutation(len(sub))
    rays = np.ascontiguousarray(sub[shuffle])
    set_form(accel, form)
    try:
        for K in (1, 3, 8):
            want = take(reference(name, form, accel, K), shuffle)
            as_given = layers(accel, rays, K)
            compare((name, form, K, "order 0"), as_given, want)
            G.set_query_order(accel, 1)
            try:
                assert G.get_query_order(accel) == 1
                compare((name, form, K, "order 1"), layers(accel, rays, K), as_given)
            finally:
                G.set_query_order(accel, 0)
    finally:
        G.set_query_order(accel, 0)
        reset(accel)


# ---- 4: the tile claim's other path ------------------------------------------------------------------------------------------------------
def test_more_tiles_than_twice_the_grids_waves():
    """LDS form: one 1024-lane workgroup per CU, 16 waves each; the full set repeated until its 64-ray tiles pass 2 x 16 x CUs."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    accel, _, full = setup("cornell_glass")
    reps = 1
    while (reps * len(full) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    set_form(accel, "lds")
    try:
        once = chain(lambda r: G.intersect(accel, r), full, 2)
        assert (once["count"] == 0).mean() >= 0.15 and (once["count"] == 2).mean() >= 0.03
        rays = np.ascontiguousarray(np.tile(full, (reps, 1)))
        assert (len(rays) + 63) // 64 > 2 * 16 * cus
        want = take(once, np.tile(np.arange(len(full)), reps))
        compare(("lds", "more tiles than twice the grid's waves", reps), layers(accel, rays, 2), want)
    finally:
        reset(accel)


# ---- 5: outputs --------------------------------------------------------------------------------------------------------------------------
SUBSETS = [(p,) for p in PLANES] + [("along", "id", "count"), ("hits", "inside"), ("count", "inside")]


def test_outputs_alone_in_subsets_over_garbage_and_twice():
    name, form, K = "instanced", "reference", 3
    accel, sub, _ = setup(name)
    rays = np.ascontiguousarray(sub[:64 * 20 + 9])
    want = take(reference(name, form, accel, K), np.arange(len(rays)))
    assert (want["count"] == 0).any() and (want["count"] == K).any()
    rng = np.random.default_rng(5)
    for planes in SUBSETS:
        bufs = {p: rng.integers(1, 2 ** 32, want[p].size * want[p].dtype.itemsize // 4, dtype=np.uint64).astype(np.uint32).view(want[p].dtype).reshape(want[p].shape)
                for p in PLANES}
        for p in PLANES:
            if p not in planes:
                words(bufs[p])[...] = 0xA5A5A5A5
        for _ in range(2):  # the same call twice: the same bytes
            got = G.hit_layers(accel, rays, K, planes, into={p: bufs[p] for p in planes})
            assert all(got[p] is bufs[p] for p in planes)
            compare(("outputs", planes), got, want, planes)
        assert all((words(bufs[p]) == 0xA5A5A5A5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", planes)
    got = accel.hit_layers(rays, K)
    assert list(got) == ["along", "id", "count"]
    compare("the default planes", got, want, ("along", "id", "count"))


PLANE_WORDS = {"hits": 24, "along": 2, "id": 4, "count": 1, "inside": 2}  # uint32 words an element
GUARD = 64                                                               # guard words behind every device buffer
FILL = 0x25A5A5A5


@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference"), ("mesh_glass", "fast")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel, sub, _ = setup(name)
    K, n = 3, len(sub)
    set_form(accel, form)
    try:
        want = reference(name, form, accel, K)
        host = layers(accel, sub, K)
        compare(("host form", name, form), host, want)
        elems = {p: (K * n if p in ("hits", "along", "id") else n) * PLANE_WORDS[p] for p in PLANES}
        drays = torch.from_numpy(sub).cuda()
        stream = torch.cuda.Stream()
        for planes in (PLANES, ("along", "count"), ("inside",)):
            dev = {p: torch.full((elems[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                s = torch.cuda.current_stream().cuda_stream
                assert s != 0
                for _ in range(2):  # the second call runs over the first one's results
                    G.hit_layers_device(accel, n, drays.data_ptr(), K, stream=s, **{p + "_ptr": dev[p].data_ptr() for p in planes})
            stream.synchronize()
            for p in PLANES:
                back = dev[p].cpu().numpy().view(np.uint32)
                assert (back[elems[p]:] == FILL).all(), (name, form, p, "nothing is written past the plane's elements")
                if p in planes:
                    assert back[:elems[p]].tobytes() == host[p].tobytes(), (name, form, planes, p)
                else:
                    assert (back == FILL).all(), (name, form, planes, p, "not asked for")
    finally:
        reset(accel)


# ---- 6: edge inputs ----------------------------------------------------------------------------------------------------------------------
def odd_rays(rays):
    """Copies of plain rays with NaN, +-inf, -0.0 and zero directions and with origins at 1e300, a few lanes of every tile."""
    r = rays.copy()
    inf, nan = np.inf, np.nan
    poisons = [(3, nan), (4, inf), (5, -inf), (3, -0.0), (4, 0.0), (0, nan), (1, inf), (2, -0.0), (0, 1e300), (2, -1e300)]
    for k, (col, v) in enumerate(poisons):
        r[7 * k + 3::97, col] = v
    r[11::131, 3:] = 0.0    # zero directions
    r[12::131, 3:] = -0.0
    r[13::131, :3] = 1e300  # origins at 1e300, looking back and away
    r[14::131, :3] = 1e300
    r[14::131, 3:] = -1.0
    return np.ascontiguousarray(r)


@pytest.mark.parametrize("case,form", [("subset", "lds"), ("subset", "reference"), ("f3", "reference"), ("f7", "reference"), ("mesh", "prune"), ("mesh", "fast")])
def test_edge_inputs_equal_the_restatement(case, form):
    if case == "subset":
        accel, sub, _ = setup("cornell_glass")
        rays = odd_rays(sub[:64 * 40 + 17])
    elif case == "mesh":
        accel, sub, _ = setup("mesh_glass")
        rays = odd_rays(sub[64 * 50:64 * 90 + 5])
    elif case == "f3":
        accel = G.Accel.from_scene(E.f3_scene(G))
        rays = E.edge_rays(*E.F3_BOUNDS, boxes=E.F3_BOXES, seed=3)[0]
    else:
        accel = G.Accel.from_scene(E.f7_scene(G))
        rays = E.edge_rays(*E.F7_BOUNDS, boxes=E.F7_BOXES, huge=True, seed=7)[0]
    rays = np.ascontiguousarray(rays)
    set_form(accel, form)
    try:
        for K in (1, 2, 8):
            want = chain(lambda r: G.intersect(accel, r), rays, K)
            if K == 8:
                assert (want["count"] == 0).any() and (want["count"] >= 2).any(), (case, form, "hits and misses among the edge rays")
            compare((case, form, K), layers(accel, rays, K), want)
    finally:
        reset(accel)


# ---- 7: errors and the empty set ---------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_an_empty_set_is_a_no_op():
    torch = pytest.importorskip("torch")
    accel, sub, _ = setup("cornell_glass")
    n, K = 70, 3
    rays = np.ascontiguousarray(sub[:n + 1])
    drays = torch.from_numpy(rays).cuda()
    sizes = {p: (K * n if p in ("hits", "along", "id") else n) * PLANE_WORDS[p] for p in PLANES}
    dev = {p: torch.full((sizes[p],), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for p in PLANES}
    hst = {p: np.full(sizes[p], 0x5A5A5A5A, dtype=np.uint32) for p in PLANES}
    torch.cuda.synchronize()
    R = drays.data_ptr()
    D = {p: dev[p].data_ptr() for p in PLANES}
    H = {p: hst[p].ctypes.data for p in PLANES}

    def V(n_, rays_, k_, **out):
        ptrs = dict(D)
        ptrs.update(out)
        G.hit_layers_device(accel, n_, rays_, k_, stream=0, **{p + "_ptr": ptrs[p] for p in PLANES})

    bad = [lambda: V(n, rays.ctypes.data, K)]                             # host pointers
    bad += [lambda p=p: V(n, R, K, **{p: H[p]}) for p in PLANES]
    bad += [lambda: V(n, R + 4, K)]                                       # misaligned
    bad += [lambda p=p: V(n, R, K, **{p: D[p] + 2}) for p in PLANES]
    bad += [lambda: V(n, R, K, hits=D["hits"] + 8),                       # hits and id are 16-byte aligned
            lambda: V(n, R, K, id=D["id"] + 8),
            lambda: V(n, R, K, along=D["along"] + 4),                     # along and inside 8
            lambda: V(n, R, K, inside=D["inside"] + 4),
            lambda: V(n, R, K, **{p: None for p in PLANES}),              # all five planes NULL
            lambda: V(n, None, K),                                        # NULL rays
            lambda: V(n, R, 0),                                           # max_layers == 0
            lambda: V(1 << 38, R, 1),                                     # n > (2^32 - 1) * 64
            lambda: V(1 << 37, R, 1 << 31),                               # n * max_layers beyond size_t
            lambda: V(1 << 30, R, 1 << 28),                               # ... fits, its bytes do not
            lambda: V(1 << 24, R, 1, **{p: None for p in PLANES if p != "count"})]  # 768 MiB of rays: the buffer ends long before
    for k, call in enumerate(bad):
        with pytest.raises(la.LasgunError) as e:
            call()
        assert str(e.value), k
    G.set_query_order(accel, 1)
    try:
        with pytest.raises(la.LasgunError):  # the sorted order's own limit
            V(1 << 32, R, 1)
        assert G.call("hit_layers", accel.h, rays.ctypes.data, 1 << 32, 1, ctypes.addressof(_capi.CLayersOut(*[H[p] for p in PLANES]))) != 0
    finally:
        G.set_query_order(accel, 0)
    hr = rays.ctypes.data
    full = _capi.CLayersOut(*[H[p] for p in PLANES])
    none = _capi.CLayersOut()
    A = ctypes.addressof
    host = [(accel.h, hr, n, K, A(none)),
            (accel.h, hr, n, K, None),
            (accel.h, None, n, K, A(full)),
            (None, hr, n, K, A(full)),
            (accel.h, hr, n, 0, A(full)),
            (accel.h, hr, 1 << 38, 1, A(full)),
            (accel.h, hr, 1 << 37, 1 << 31, A(full)),
            (accel.h, hr, 1 << 30, 1 << 28, A(full))]
    for k, args in enumerate(host):
        assert G.call("hit_layers", *args) != 0 and G.last_error(), k
    # the empty set: success, nothing written (whatever the pointers, whatever max_layers)
    V(0, R, K)
    V(0, R, 0)
    assert G.call("hit_layers", accel.h, hr, 0, K, A(full)) == 0 and G.call("hit_layers", accel.h, hr, 0, 0, A(none)) == 0
    assert G.call("hit_layers", None, None, 0, 0, None) == 0 and G.call("hit_layers_device", None, None, 0, 0, None, None) == 0
    empty = layers(accel, np.zeros((0, 6)), K)
    assert empty["hits"].shape == (K, 0) and empty["id"].shape == (K, 0, 4) and empty["count"].shape == (0,)
    torch.cuda.synchronize()
    assert all((dev[p].cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all() for p in PLANES) and all((hst[p] == 0x5A5A5A5A).all() for p in PLANES)
    # and the call still works afterwards
    V(n, R, K)
    torch.cuda.synchronize()
    want = layers(accel, rays[:n], K)
    for p in PLANES:
        assert dev[p].cpu().numpy().view(np.uint32).tobytes() == want[p].tobytes(), p
