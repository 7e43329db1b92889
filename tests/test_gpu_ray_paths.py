"""Ray paths (include/lasgun_hip.h: lg_trace_paths, lg_trace_paths_device): each ray followed through up to K vertices in one launch, the
next segment formed in the kernel by the rule of the hit's material, the answer as vertex-major and per-ray planes.

The reference is the contract restated in numpy over lg_intersect (tests/bounce_ref.py, `chain`; its `bounce` is held word for word to
lasgun_amd/csrc/bounce.h on the CPU by tests/test_bounce_host.py): a loop of K calls, the rays compacted between the calls, every operation
one rounded f64 operation.  NOTHING is tolerated: every plane is compared as uint32 words, NaNs included.  The inputs are the hit layers'
(tests/test_gpu_hit_layers.py, setup): 8385 rays, 131 full tiles and one ray, on cornell_glass, instanced and mesh_glass.

Rule tables (gains 0.5 + m / 16 per material m, so `gain` is not a plane of ones): glass_else_reflect = glass refracts with its eta,
everything else reflects; optics = la.path_rules, default absorb; reflect_all; pass_all.

  1  every traversal form x K in {1, 2, 3, 8} x both normals, all nine planes, glass_else_reflect (reflect_all on instanced); runs of 1, 63,
     64, 65 and 129 rays at the first tile with a wave-divergent ending; for K = 1, hits[0] is lg_intersect's array;
  2  optics on the two glass scenes; pass_all: point and hits equal lg_hit_layers', bit for bit;
  3  resuming: (a, b) = (3, 5) and (1, 7), the second call on last and medium of the first one's cut rays;
  4  against the same loop over the CPU oracle's intersect, K = 8, the rule from the oracle's material POD per hit;
  5  lg_accel_set_query_order(1) on the shuffled subset: the bytes of order 0;
  6  (LDS form) more tiles than twice the grid's waves;
  7  every plane alone and three subsets over garbage, the same call twice; the device form on a second stream over a prefill with guard
     words behind every buffer, planes not asked for untouched;
  8  edge inputs: NaN, +-inf, -0.0 and zero directions, origins at 1e300, tests/edge_rays.py's families; DEGENERATE must occur;
  9  the limit scenes chain8_shallow, accels65 and deep_a in the default and one forced form, K = 4, reflect_all;
  10 every error refused with every output at its prefill; n == 0 a no-op with NULL everything.
No vacuous comparison (not_vacuous, asserted on the reference's answer before anything is compared; conditions, not measurements).  At
K = 8 on every scene with its table: >= 15 % of the rays with count 0 (measured on the CPU oracle's chain: 61 %), >= 15 % with count >= 1,
>= 3 % with count >= 3 (measured: 29-34 %; 4-7 % with optics), >= 3 % reach K at K = 2 and K = 3, at least half of the 131 full tiles hold
a count-0 lane and a count->=3 lane (measured: 95-97 %; 52-56 % with optics).  With glass_else_reflect on the two glass scenes: >= 5 % of
the rays refract inward (measured: 21-23 %), >= 5 % outward (20-22 %), >= 1 % meet total internal reflection (4.2-4.3 %).  With optics:
>= 15 % ABSORBED (38 %) and >= 15 % ESCAPED (61 %).  On cornell_glass the two normals give the same count plane (spheres and boxes: ns is ng
up to sign); on instanced and mesh_glass they must differ."""
import ctypes

import numpy as np
import pytest

import bounce_ref as B
import edge_rays as E
import lasgun_amd as la
from lasgun_amd import _capi
from oracle_lib import oracle
import test_gpu_hit_layers as HL
from test_gpu_visibility import SCENES, FORMS, set_form, reset

pytestmark = pytest.mark.gpu

G = la.api
PLANES = la.PATH_PLANES
PER_VERTEX = ("hits", "point", "id", "along")
KS = (1, 2, 3, 8)
setup = HL.setup
words = HL.words


def test_the_restatement_speaks_of_the_librarys_records():
    assert B.HIT_DTYPE == la.HIT_DTYPE and B.RULE_DTYPE == la.PATH_RULE_DTYPE
    assert (B.ABSORB, B.REFLECT, B.PASS, B.REFRACT) == (la.PATH_ABSORB, la.PATH_REFLECT, la.PATH_PASS, la.PATH_REFRACT)
    assert (B.END_CUT, B.END_ESCAPED, B.END_ABSORBED, B.END_DEGENERATE) == (la.PATH_END_CUT, la.PATH_END_ESCAPED, la.PATH_END_ABSORBED, la.PATH_END_DEGENERATE)


def table(accel, which):
    r = la.path_rules(accel)  # glass refracts with its eta, mirror and metal reflect, the rest absorbs
    assert len(r) == G.material_count(accel)
    r["gain"] = 0.5 + np.arange(len(r)) / 16.0
    if which == "glass_else_reflect":
        r["action"][r["action"] != la.PATH_REFRACT] = la.PATH_REFLECT
    elif which == "reflect_all":
        r["action"] = la.PATH_REFLECT
    elif which == "pass_all":
        r["action"] = la.PATH_PASS
    else:
        assert which == "optics"
    return r


def main_table(name):
    return "reflect_all" if name == "instanced" else "glass_else_reflect"


def compare(ctx, got, want, planes=PLANES):
    assert set(got) == set(planes), (ctx, sorted(got))
    for p in planes:
        g, w = got[p], want[p]
        assert g.shape == w.shape and g.dtype == w.dtype, (ctx, p, g.shape, w.shape, g.dtype, w.dtype)
        diff = words(g).reshape(-1) != words(w).reshape(-1)
        assert not diff.any(), (ctx, p, int(diff.sum()), "words differ; first at word", int(np.argmax(diff)), "of", diff.size)


def take(want, idx):
    """The planes of the rays `idx` of a reference (per ray: a path depends on its ray alone)."""
    return {p: np.ascontiguousarray(want[p][:, idx] if p in PER_VERTEX else want[p][idx]) for p in PLANES}


_ref = {}


def reference(name, form, accel, K, which, normal):
    """The subset's planes by the loop over lg_intersect in the accel's current form; computed once per case, never changed."""
    key = (name, form, K, which, normal)
    if key not in _ref:
        _ref[key] = B.chain(lambda r: G.intersect(accel, r), setup(name)[1], K, B.table_rule(table(accel, which)), normal)
    return _ref[key]


def mixed_tiles(count):
    c = count[:len(count) // 64 * 64].reshape(-1, 64)
    return (c == 0).any(axis=1) & (c >= 3).any(axis=1)


def not_vacuous(name, form, accel, which, normal):
    w8 = reference(name, form, accel, 8, which, normal)
    c = w8["count"]
    assert (c == 0).mean() >= 0.15 and (c >= 1).mean() >= 0.15 and (c >= 3).mean() >= 0.03, (name, form, which, (c == 0).mean(), (c >= 1).mean(), (c >= 3).mean())
    m = mixed_tiles(c)
    assert 2 * int(m.sum()) >= len(m) == 131, (name, form, "tiles mixing a lane with count 0 and a lane with count >= 3", int(m.sum()), len(m))
    for K in (2, 3):
        assert (reference(name, form, accel, K, which, normal)["count"] == K).mean() >= 0.03, (name, form, K, "rays that reach K")
    if which == "glass_else_reflect":
        d = w8["did"]
        assert d["inward"].mean() >= 0.05 and d["outward"].mean() >= 0.05 and d["tir"].mean() >= 0.01, (name, form, d["inward"].mean(), d["outward"].mean(), d["tir"].mean())
    if which == "optics":
        assert (w8["end"] == la.PATH_END_ABSORBED).mean() >= 0.15 and (w8["end"] == la.PATH_END_ESCAPED).mean() >= 0.15, (name, form, np.bincount(w8["end"]))
    assert not (w8["gain"] == 1.0).all() and (w8["gain"][c == 0] == 1.0).all()


def paths(accel, rays, K, rules, normal=0, start_medium=None, planes=PLANES):
    return G.trace_paths(accel, rays, K, rules, normal, start_medium, planes)


# ---- 1: bit for bit against the restatement, every form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_planes_equal_the_restatement(name, form):
    accel, sub, _ = setup(name)
    which = main_table(name)
    rules = table(accel, which)
    set_form(accel, form)
    try:
        first = G.intersect(accel, sub)
        for normal in (0, 1):
            not_vacuous(name, form, accel, which, normal)
            c8 = reference(name, form, accel, 8, which, normal)["count"]
            start = 64 * int(np.argmax(mixed_tiles(c8)))  # the first tile with the wave-divergent ending
            ones = [int(np.argmax(c8 == 0)), int(np.argmax(c8 >= 3))]
            assert c8[ones[0]] == 0 and c8[ones[1]] >= 3
            for K in KS:
                want = reference(name, form, accel, K, which, normal)
                got = paths(accel, sub, K, rules, normal)
                compare((name, form, K, normal, "subset"), got, want)
                assert (want["count"][want["end"] == la.PATH_END_CUT] == K).all() and (want["count"][want["end"] == la.PATH_END_ESCAPED] < K).all()
                if K == 1:
                    assert got["hits"][0].tobytes() == first.tobytes(), "for K = 1, hits[0] is lg_intersect's array itself"
                    assert got["along"][0].tobytes() == first["t"].tobytes(), "... and along[0] its t"
                for n in (63, 64, 65, 129):
                    idx = np.arange(start, start + n)
                    part = take(want, idx)
                    if n >= 64:  # (the whole mixed tile is in)
                        assert (part["count"] == 0).any() and (part["count"] >= min(K, 3)).any(), (name, form, K, n)
                    compare((name, form, K, normal, n), paths(accel, np.ascontiguousarray(sub[idx]), K, rules, normal), part)
                for i in ones:  # n = 1: once a ray with count 0, once a ray with count >= 3
                    part = take(want, np.array([i]))
                    assert int(part["count"][0]) == min(int(c8[i]), K)
                    compare((name, form, K, normal, "one ray", i), accel.trace_paths(sub[i:i + 1].copy(), K, rules, normal, None, PLANES), part)
        counts = [reference(name, form, accel, 8, which, normal)["count"] for normal in (0, 1)]
        if name == "cornell_glass":  # spheres and boxes alone: ns is ng up to sign, and the rule flips either against d
            assert np.array_equal(*counts)
        else:
            assert not np.array_equal(*counts), (name, "the two normals give different paths")
    finally:
        reset(accel)


# ---- 2: the wrapper's table; PASS is the layers' step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("mesh_glass", "fast")])
def test_optics_and_pass(name, form):
    accel, sub, _ = setup(name)
    set_form(accel, form)
    try:
        not_vacuous(name, form, accel, "optics", 1)
        for K in (1, 3, 8):
            compare((name, form, K, "optics"), paths(accel, sub, K, table(accel, "optics"), 1), reference(name, form, accel, K, "optics", 1))
            compare((name, form, K, "the default table"), accel.trace_paths(sub, K, normal=1, planes=("id", "count", "end", "last", "medium")),
                    B.chain(lambda r: G.intersect(accel, r), sub, K, B.table_rule(la.path_rules(accel)), 1), ("id", "count", "end", "last", "medium"))
        K = 8
        got = paths(accel, sub, K, table(accel, "pass_all"))
        compare((name, form, "pass_all"), got, reference(name, form, accel, K, "pass_all", 0))
        layers = G.hit_layers(accel, sub, K, ("hits", "along", "id", "count"))
        assert (layers["count"] >= 3).mean() >= 0.03
        for p in ("hits", "along", "id", "count"):
            assert got[p].tobytes() == layers[p].tobytes(), (name, form, p, "a table of PASS everywhere walks the hit layers")
        assert got["point"].tobytes() == np.ascontiguousarray(layers["hits"]["p"]).tobytes()
        assert np.array_equal(got["medium"], layers["count"] & 1), "the parity of the crossings"
    finally:
        reset(accel)


# ---- 3: resuming ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("mesh_glass", "reference"), ("instanced", "prune")])
def test_a_cut_path_resumes_bit_for_bit(name, form):
    accel, sub, _ = setup(name)
    which = main_table(name)
    rules = table(accel, which)
    set_form(accel, form)
    try:
        whole = paths(accel, sub, 8, rules, 1)
        compare((name, form, "a + b"), whole, reference(name, form, accel, 8, which, 1))
        for a, b in ((3, 5), (1, 7)):
            one = paths(accel, sub, a, rules, 1)
            cut = np.flatnonzero(one["end"] == la.PATH_END_CUT)
            assert len(cut) >= 0.03 * len(sub) and (one["count"][cut] == a).all()
            if which == "glass_else_reflect":
                assert one["medium"][cut].any() and not one["medium"][cut].all(), "cut inside and outside the glass"
            two = paths(accel, np.ascontiguousarray(one["last"][cut]), b, rules, 1, np.ascontiguousarray(one["medium"][cut]))
            for p in ("hits", "point", "id"):
                assert two[p].tobytes() == np.ascontiguousarray(whole[p][a:, cut]).tobytes(), (name, form, a, b, p)
                assert one[p].tobytes() == np.ascontiguousarray(whole[p][:a]).tobytes(), (name, form, a, b, p, "the first rows")
            assert np.array_equal(one["count"][cut] + two["count"], whole["count"][cut])
            for p in ("end", "last", "medium"):
                assert two[p].tobytes() == np.ascontiguousarray(whole[p][cut]).tobytes(), (name, form, a, b, p)
            done = np.flatnonzero(one["end"] != la.PATH_END_CUT)
            for p in ("count", "end", "last", "medium", "gain"):
                assert np.ascontiguousarray(one[p][done]).tobytes() == np.ascontiguousarray(whole[p][done]).tobytes(), (name, form, a, b, p, "paths that ended below a")
    finally:
        reset(accel)


# ---- 4: against the CPU oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_glass", "instanced", "mesh_glass"])
def test_count_end_medium_along_and_ids_equal_the_cpu_oracles_chain(name):
    accel, sub, _ = setup(name)
    which = main_table(name)
    rules = table(accel, which)
    o = oracle()
    oaccel = o.Accel(SCENES[name](o))
    pods = {}

    def intersect(r):
        h, pods["m"] = o.intersect(oaccel, r, 16)
        return h

    def rule_of(h):  # from the oracle's material POD per hit: glass refracts with its eta, the rest reflects
        m = pods["m"]
        glass = (m["kind"] == 3) & (which == "glass_else_reflect")
        return np.where(h["kind"] == 0, B.ABSORB, np.where(glass, B.REFRACT, B.REFLECT)), np.where(glass, m["p"][:, 6], 1.0), np.ones(len(h))

    o.set_trig_mode(True)
    try:
        want = B.chain(intersect, sub, 8, rule_of, 1)
    finally:
        o.set_trig_mode(False)
    c = want["count"]
    assert (c == 0).mean() >= 0.15 and (c >= 1).mean() >= 0.15 and (c >= 3).mean() >= 0.03, (name, "oracle")
    if which == "glass_else_reflect":
        d = want["did"]
        assert d["inward"].mean() >= 0.05 and d["outward"].mean() >= 0.05 and d["tir"].mean() >= 0.01, (name, "oracle")
    got = paths(accel, sub, 8, rules, 1, None, ("along", "id", "count", "end", "medium"))
    compare((name, "oracle"), {p: got[p] for p in ("count", "end", "medium", "along")}, want, ("count", "end", "medium", "along"))
    assert np.array_equal(got["id"][..., :3], want["id"][..., :3]), (name, "kind, prim, instance")


# ---- 5: query order 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "prune")])
def test_the_sorted_order_gives_the_bytes_of_the_given_order(name, form):
    accel, sub, _ = setup(name)
    which = main_table(name)
    rules = table(accel, which)
    shuffle = np.random.default_rng(21).permutation(len(sub))
    rays = np.ascontiguousarray(sub[shuffle])
    set_form(accel, form)
    try:
        for K in (1, 3, 8):
            want = take(reference(name, form, accel, K, which, 0), shuffle)
            as_given = paths(accel, rays, K, rules)
            compare((name, form, K, "order 0"), as_given, want)
            G.set_query_order(accel, 1)
            try:
                assert G.get_query_order(accel) == 1
                compare((name, form, K, "order 1"), paths(accel, rays, K, rules), as_given)
            finally:
                G.set_query_order(accel, 0)
    finally:
        G.set_query_order(accel, 0)
        reset(accel)


# ---- 6: the tile claim's other path ----------------------------------------------------------------------------------------------------------
def test_more_tiles_than_twice_the_grids_waves():
    """LDS form: one 1024-lane workgroup per CU, 16 waves each; the full set repeated until its 64-ray tiles pass 2 x 16 x CUs."""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    accel, _, full = setup("cornell_glass")
    rules = table(accel, "glass_else_reflect")
    reps = 1
    while (reps * len(full) + 63) // 64 <= 2 * 16 * cus:
        reps += 1
    set_form(accel, "lds")
    try:
        once = B.chain(lambda r: G.intersect(accel, r), full, 2, B.table_rule(rules), 0)
        assert (once["count"] == 0).mean() >= 0.15 and (once["count"] == 2).mean() >= 0.03
        rays = np.ascontiguousarray(np.tile(full, (reps, 1)))
        assert (len(rays) + 63) // 64 > 2 * 16 * cus
        want = take(once, np.tile(np.arange(len(full)), reps))
        compare(("lds", "more tiles than twice the grid's waves", reps), paths(accel, rays, 2, rules), want)
    finally:
        reset(accel)


# ---- 7: outputs ------------------------------------------------------------------------------------------------------------------------------
SUBSETS = [(p,) for p in PLANES] + [("point", "id", "count", "end"), ("hits", "gain", "last"), ("count", "medium")]


def test_outputs_alone_in_subsets_over_garbage_and_twice():
    name, form, K = "mesh_glass", "reference", 3
    accel, sub, _ = setup(name)
    rules = table(accel, "glass_else_reflect")
    rays = np.ascontiguousarray(sub[:64 * 20 + 9])
    want = take(reference(name, form, accel, K, "glass_else_reflect", 0), np.arange(len(rays)))
    assert (want["count"] == 0).any() and (want["count"] == K).any()
    rng = np.random.default_rng(5)
    for planes in SUBSETS:
        bufs = {p: rng.integers(1, 2 ** 32, want[p].size * want[p].dtype.itemsize // 4, dtype=np.uint64).astype(np.uint32).view(want[p].dtype).reshape(want[p].shape)
                for p in PLANES}
        for p in PLANES:
            if p not in planes:
                words(bufs[p])[...] = 0xA5A5A5A5
        for _ in range(2):  # the same call twice: the same bytes
            got = G.trace_paths(accel, rays, K, rules, 0, None, planes, into={p: bufs[p] for p in planes})
            assert all(got[p] is bufs[p] for p in planes)
            compare(("outputs", planes), got, want, planes)
        assert all((words(bufs[p]) == 0xA5A5A5A5).all() for p in PLANES if p not in planes), ("unrequested buffers are untouched", planes)
    got = accel.trace_paths(rays, K, rules)
    assert list(got) == ["point", "id", "count", "end"]
    compare("the default planes", got, want, ("point", "id", "count", "end"))


PLANE_WORDS = {"hits": 24, "point": 6, "id": 4, "along": 2, "count": 1, "end": 1, "gain": 2, "last": 12, "medium": 1}  # uint32 words an element
GUARD = 64                                                                                                          # guard words behind every device buffer
FILL = 0x25A5A5A5


@pytest.mark.parametrize("name,form", [("cornell_glass", "lds"), ("instanced", "reference"), ("mesh_glass", "fast")])
def test_device_form_on_a_torch_stream(name, form):
    torch = pytest.importorskip("torch")
    accel, sub, _ = setup(name)
    which = main_table(name)
    K, n = 3, len(sub)
    set_form(accel, form)
    try:
        medium0 = (np.arange(n) % 3 == 0).astype(np.uint32) * 0xFFFFFFFF  # (only bit 0 is read)
        want = B.chain(lambda r: G.intersect(accel, r), sub, K, B.table_rule(table(accel, which)), 1, medium0)
        host = paths(accel, sub, K, table(accel, which), 1, medium0)
        compare(("host form", name, form), host, want)
        elems = {p: (K * n if p in PER_VERTEX else n) * PLANE_WORDS[p] for p in PLANES}
        drays, dmedium = torch.from_numpy(sub).cuda(), torch.from_numpy(medium0.view(np.int32)).cuda()
        stream = torch.cuda.Stream()
        for planes in (PLANES, ("point", "count", "end"), ("last",)):
            dev = {p: torch.full((elems[p] + GUARD,), FILL, dtype=torch.int32, device="cuda") for p in PLANES}
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                s = torch.cuda.current_stream().cuda_stream
                assert s != 0
                for _ in range(2):  # the second call runs over the first one's results
                    rules = table(accel, which)  # (a table of the call's own, gone when the call returns)
                    G.trace_paths_device(accel, n, drays.data_ptr(), K, rules, 1, dmedium.data_ptr(), stream=s, **{p + "_ptr": dev[p].data_ptr() for p in planes})
                    rules["action"], rules["ior"] = 7, np.nan
                    del rules
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


# ---- 8: edge inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", [("subset", "lds"), ("subset", "reference"), ("f3", "reference"), ("f7", "reference"), ("mesh", "prune"), ("mesh", "fast")])
def test_edge_inputs_equal_the_restatement(case, form):
    if case == "subset":
        accel, sub, _ = setup("cornell_glass")
        rays = HL.odd_rays(sub[:64 * 40 + 17])
    elif case == "mesh":
        accel, sub, _ = setup("mesh_glass")
        rays = HL.odd_rays(sub[64 * 50:64 * 90 + 5])
    elif case == "f3":
        accel = G.Accel.from_scene(E.f3_scene(G))
        rays = E.edge_rays(*E.F3_BOUNDS, boxes=E.F3_BOXES, seed=3)[0]
    else:
        accel = G.Accel.from_scene(E.f7_scene(G))
        rays = E.edge_rays(*E.F7_BOUNDS, boxes=E.F7_BOXES, huge=True, seed=7)[0]
    rays = np.ascontiguousarray(rays)
    set_form(accel, form)
    try:
        for which in ("glass_else_reflect", "reflect_all"):
            rules = table(accel, which)
            rules["ior"][rules["action"] != la.PATH_REFRACT] = 1.5
            if case in ("f3", "f7") and which == "glass_else_reflect":
                rules["action"] = la.PATH_REFRACT  # (no glass among the edge scenes' materials: every surface refracts)
            for K, normal in ((1, 0), (2, 1), (8, 1)):
                want = B.chain(lambda r: G.intersect(accel, r), rays, K, B.table_rule(rules), normal)
                if K == 8:
                    assert (want["count"] == 0).any() and (want["count"] >= 2).any(), (case, form, "hits and misses among the edge rays")
                    if case != "mesh" or which == "reflect_all":
                        assert (want["end"] == la.PATH_END_DEGENERATE).any(), (case, form, which, "a path that ends on a ray that is not finite")
                compare((case, form, which, K), paths(accel, rays, K, rules, normal), want)
    finally:
        reset(accel)


# ---- 9: the scene graph's limits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain8_shallow", "accels65", "deep_a"])
def test_the_limit_scenes(name):
    import test_gpu_scene_limits as SL
    c, accel = SL.case(name), SL.accel_of(name)
    rules = table(accel, "reflect_all")
    try:
        for form in ("default", SL.FORCED[name]):
            if form != "default":
                set_form(accel, form)
            want = B.chain(lambda r: G.intersect(accel, r), c.plain130, 4, B.table_rule(rules), 1)
            assert (want["count"] == 0).any() and (want["count"] >= 2).any(), (name, np.bincount(want["count"]))
            compare((name, form), paths(accel, c.plain130, 4, rules, 1), want)
    finally:
        SL.restore(accel)


# ---- 10: errors and the empty set ---------------------------------------------------------------------------------------------------------------
def test_errors_are_refused_before_any_launch_and_an_empty_set_is_a_no_op():
    torch = pytest.importorskip("torch")
    accel, sub, _ = setup("cornell_glass")
    n, K = 70, 3
    rules = table(accel, "glass_else_reflect")
    nr = len(rules)
    rays = np.ascontiguousarray(sub[:n + 1])
    drays = torch.from_numpy(rays).cuda()
    dmed = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    sizes = {p: (K * n if p in PER_VERTEX else n) * PLANE_WORDS[p] for p in PLANES}
    dev = {p: torch.full((sizes[p],), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for p in PLANES}
    hst = {p: np.full(sizes[p], 0x5A5A5A5A, dtype=np.uint32) for p in PLANES}
    torch.cuda.synchronize()
    R, M = drays.data_ptr(), dmed.data_ptr()
    D = {p: dev[p].data_ptr() for p in PLANES}
    H = {p: hst[p].ctypes.data for p in PLANES}
    A = ctypes.addressof

    def V(n_, rays_, k_, rules_=rules, nr_=None, normal=0, start=None, **out):
        ptrs = dict(D)
        ptrs.update(out)
        f = _capi.CPathsOut(*[ptrs[p] for p in PLANES])
        tab = None if rules_ is None else rules_.ctypes.data
        if G.call("trace_paths_device", accel.h, rays_, n_, k_, tab, len(rules) if nr_ is None else nr_, normal, start, A(f), None):
            raise la.LasgunError(G.last_error())

    def bad_rule(**kw):
        r = rules.copy()
        for k, v in kw.items():
            r[k][nr - 1] = v
        return r

    bad = [lambda: V(n, rays.ctypes.data, K)]                             # host pointers
    bad += [lambda p=p: V(n, R, K, **{p: H[p]}) for p in PLANES]
    bad += [lambda: V(n, R, K, start=hst["count"].ctypes.data)]
    bad += [lambda: V(n, R + 4, K)]                                       # misaligned
    bad += [lambda p=p: V(n, R, K, **{p: D[p] + 2}) for p in PLANES]
    bad += [lambda: V(n, R, K, start=M + 2)]
    bad += [lambda: V(n, R, K, hits=D["hits"] + 8),                       # hits and id are 16-byte aligned
            lambda: V(n, R, K, id=D["id"] + 8),
            lambda: V(n, R, K, point=D["point"] + 4),                     # point, along, gain and last 8
            lambda: V(n, R, K, along=D["along"] + 4),
            lambda: V(n, R, K, gain=D["gain"] + 4),
            lambda: V(n, R, K, last=D["last"] + 4),
            lambda: V(n, R, K, **{p: None for p in PLANES}),              # all nine planes NULL
            lambda: V(n, None, K),                                        # NULL rays
            lambda: V(n, R, K, rules_=None),                              # NULL rules
            lambda: V(n, R, 0),                                           # max_bounces == 0
            lambda: V(n, R, K, nr_=nr - 1),                               # n_rules is not the accel's material count
            lambda: V(n, R, K, nr_=nr + 1),
            lambda: V(n, R, K, nr_=0),
            lambda: V(n, R, K, rules_=bad_rule(action=4)),                # an unknown action
            lambda: V(n, R, K, rules_=bad_rule(action=0xFFFFFFFF)),
            lambda: V(n, R, K, rules_=bad_rule(reserved=1)),              # reserved != 0
            lambda: V(n, R, K, normal=2),                                 # normal outside {0, 1}
            lambda: V(n, R, K, normal=-1),
            lambda: V(1 << 38, R, 1),                                     # n > (2^32 - 1) * 64
            lambda: V(1 << 37, R, 1 << 31),                               # n * max_bounces beyond size_t
            lambda: V(1 << 30, R, 1 << 28),                               # ... fits, its bytes do not
            lambda: V(1 << 24, R, 1, **{p: None for p in PLANES if p != "count"})]  # 768 MiB of rays: the buffer ends long before
    for k, call in enumerate(bad):
        try:
            call()
        except la.LasgunError as e:
            assert str(e), k
        else:
            raise AssertionError(("not refused", k))
    G.set_query_order(accel, 1)
    try:
        with pytest.raises(la.LasgunError):  # the sorted order's own limit
            V(1 << 32, R, 1)
    finally:
        G.set_query_order(accel, 0)
    hr, tab = rays.ctypes.data, rules.ctypes.data
    full = _capi.CPathsOut(*[H[p] for p in PLANES])
    none = _capi.CPathsOut()
    host = [(accel.h, hr, n, K, tab, nr, 0, None, A(none)),
            (accel.h, hr, n, K, tab, nr, 0, None, None),
            (accel.h, None, n, K, tab, nr, 0, None, A(full)),
            (None, hr, n, K, tab, nr, 0, None, A(full)),
            (accel.h, hr, n, K, None, nr, 0, None, A(full)),
            (accel.h, hr, n, K, tab, nr - 1, 0, None, A(full)),
            (accel.h, hr, n, K, bad_rule(action=9).ctypes.data, nr, 0, None, A(full)),
            (accel.h, hr, n, K, bad_rule(reserved=2).ctypes.data, nr, 0, None, A(full)),
            (accel.h, hr, n, K, tab, nr, 2, None, A(full)),
            (accel.h, hr, n, 0, tab, nr, 0, None, A(full)),
            (accel.h, hr, 1 << 38, 1, tab, nr, 0, None, A(full)),
            (accel.h, hr, 1 << 37, 1 << 31, tab, nr, 0, None, A(full)),
            (accel.h, hr, 1 << 30, 1 << 28, tab, nr, 0, None, A(full))]
    for k, args in enumerate(host):
        assert G.call("trace_paths", *args) != 0 and G.last_error(), k
    # the empty set: success, nothing written (whatever the pointers, whatever max_bounces)
    V(0, R, K)
    V(0, R, 0, rules_=None, nr_=99, normal=5)
    assert G.call("trace_paths", accel.h, hr, 0, K, tab, nr, 0, None, A(full)) == 0 and G.call("trace_paths", accel.h, hr, 0, 0, None, 0, 3, None, A(none)) == 0
    assert G.call("trace_paths", None, None, 0, 0, None, 0, 0, None, None) == 0 and G.call("trace_paths_device", None, None, 0, 0, None, 0, 0, None, None, None) == 0
    empty = paths(accel, np.zeros((0, 6)), K, rules)
    assert empty["hits"].shape == (K, 0) and empty["point"].shape == (K, 0, 3) and empty["last"].shape == (0, 6) and empty["count"].shape == (0,)
    torch.cuda.synchronize()
    assert all((dev[p].cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all() for p in PLANES) and all((hst[p] == 0x5A5A5A5A).all() for p in PLANES)
    # and the call still works afterwards
    V(n, R, K, start=M)
    torch.cuda.synchronize()
    want = paths(accel, rays[:n], K, rules)
    for p in PLANES:
        assert dev[p].cpu().numpy().view(np.uint32).tobytes() == want[p].tobytes(), p
