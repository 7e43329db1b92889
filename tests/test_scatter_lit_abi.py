"""Lit scatter (include/lasgun_hip.h: lg_scatter_lit, lg_scatter_lit_device) through every layer that has to carry it, checked without a
GPU: the built library exports the symbols, the header declares them with the arity, the parameter names and the types the wrappers use
and states the contract, lg_light is 72 bytes, lg_light_set 40 and lg_lit_out 72 with the stated offsets in every mirror, the device code
is level 0 as a chain of one level with a shadow pass of its own behind the pipeline's hook, and the Python, C++ and Rust bindings mirror
the entry points.  On top: the numpy restatements on stubs, the errors answered before any HIP call, the no-op of an empty set."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ARITY = {"lg_scatter_lit": 5, "lg_scatter_lit_device": 6}
NAMES = tuple(ARITY)


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_built_library_exports_the_symbols():
    import lasgun_amd as la
    lib = ctypes.CDLL(la.LIB_PATH)
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_the_header_declares_them_and_states_the_contract():
    import gen_rust_sys
    header = read("include", "lasgun_hip.h")
    decl = {name: (ret, params) for ret, name, params in gen_rust_sys.declarations(header)}
    for name in NAMES:
        assert name in decl, name
        ret, params = decl[name]
        assert ret == "int" and len(params) == ARITY[name], (name, ret, params)
        assert "lg_accel" in params[0] and "const" in params[0]
    names = lambda key: [p.split()[-1].lstrip("*") for p in decl[key][1]]  # noqa: E731
    assert names("lg_scatter_lit")[1:] == ["rays", "n", "lights", "out"]
    assert names("lg_scatter_lit_device")[1:] == ["dev_rays", "n", "lights", "dev_out", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "size_t", "const lg_light_set *", "const lg_lit_out *"]
    assert types("lg_scatter_lit")[1:] == host and types("lg_scatter_lit_device")[1:] == host + ["void *"]
    assert re.search(r"^#define LG_MAX_CALL_LIGHTS\s+1024u\b", header, flags=re.M)
    order = ["int lg_scatter_device(", "/* Lit scatter:", "typedef struct lg_light {", "typedef struct lg_light_set {", "typedef struct lg_lit_out {", "int lg_scatter_lit(",
             "int lg_scatter_lit_device(", "int lg_accel_light_count("]
    at = [header.index(o) for o in order]
    assert at == sorted(at)
    assert "typedef struct lg_light { double position[3], intensity[3], falloff[3]; } lg_light;" in header
    ls = header[header.index("typedef struct lg_light_set {"):header.index("} lg_light_set;")]
    assert re.findall(r"^\s+(?:const )?(\w+)\s*\*?\s*(\w+)(?:\[3\])?;", ls, flags=re.M) == [("lg_light", "lights"), ("uint32_t", "count"), ("uint32_t", "per_ray"), ("double", "ambient")]
    lo = header[header.index("typedef struct lg_lit_out {"):header.index("} lg_lit_out;")]
    assert re.findall(r"^\s+(\w+)\s*\*?\s*(\w+);", lo, flags=re.M) == [("lg_scatter_out", "scatter"), ("double", "terms"), ("uint32_t", "visible")]
    text = header[header.index("/* Lit scatter:"):header.index("#define LG_MAX_CALL_LIGHTS")]
    for phrase in ("An EXTRA; no counterpart in the reference",
                   "lg_scene_add_point_light's arguments",
                   "per_ray == 0: lights[count], shared by every ray; per_ray == 1: lights[n][count], ray i's lights at",
                   "are lg_scatter's, bit for bit",
                   "The scene's own lights and ambient colour play no part in any",
                   "a scene with more than 32 lights is accepted",
                   "sh.p (= p + ng * 2^-36)",
                   "!(t < 1.0): lg_occluded of that ray, negated",
                   "term_k = mul_ew(PI * intensity, bsdf_f(..)) * wi_dot_n / f_att",
                   "added iff the light is visible and f_att != 0.0",
                   "the sequential sum over k = 0 .. K-1 from +0.0 of the added terms, then mul_ew(ambient, bsdf_f(.., ns, ..)) added last",
                   "terms[i][k] = +0.0 + term_k where the term is added, +0.0 otherwise",
                   "single-light group of lg_radiance_groups",
                   "visible[i][k >> 5] bit k & 31 is set iff light k is visible by the test above, whatever its f_att",
                   "bits at or above K are 0",
                   "For a miss: direct[i] is the background, as lg_scatter's; its terms are +0.0 and its visible words 0",
                   "K == 0: no shadow pass runs, direct is the ambient term alone; terms and visible have no elements",
                   "direct and\n * terms are the same bytes with and without `visible`",
                   "written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill",
                   "a per-ray light row follows its ray's index, not its slot",
                   "LASGUN_WF_BUDGET_MB chunks are the pipeline's own",
                   "n == 0 is a successful no-op that writes nothing, answered BEFORE every other check",
                   "a NULL `lights`",
                   "count > LG_MAX_CALL_LIGHTS; per_ray not 0 or 1; count > 0 with a NULL table",
                   "n * K * 72, n * K * 24 or n * W * 4 that does not fit size_t",
                   "terms and a per-ray table 8 bytes, visible 4",
                   "ends beyond its allocation",
                   "when per_ray == 0 it is a HOST table, staged into a table of the call's own on the stream: it may be freed on return",
                   "lights->lights is DEVICE memory when per_ray == 1"):
        assert phrase in text, phrase
    for scope in ("lights for the other radiance entry points", "emitters that are not points", "sampling the lights on the device", "multi-device split"):
        assert scope in text[text.index("Out of scope:"):], scope


def test_the_structs_have_their_sizes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    L, S, O = _capi.CLight, _capi.CLightSet, _capi.CLitOut
    assert ctypes.sizeof(L) == 72 and [(f[0], getattr(L, f[0]).offset) for f in L._fields_] == [("position", 0), ("intensity", 24), ("falloff", 48)]
    assert ctypes.sizeof(S) == 40 and [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [("lights", 0), ("count", 8), ("per_ray", 12), ("ambient", 16)]
    assert ctypes.sizeof(O) == 72 and [(f[0], getattr(O, f[0]).offset) for f in O._fields_] == [("scatter", 0), ("terms", 56), ("visible", 64)]
    assert la.LIT_PLANES == la.SCATTER_PLANES + ("terms", "visible") and la.MAX_CALL_LIGHTS == 1024
    assert la.LIGHT_DTYPE.itemsize == 72 and [la.LIGHT_DTYPE.fields[f][1] for f in ("position", "intensity", "falloff")] == [0, 24, 48]
    host = read("lasgun_amd", "csrc", "lit_host.h")  # static_asserts of the library's own build
    for claim in ("sizeof(lg_light) == 72", "offsetof(lg_light, intensity) == 24", "offsetof(lg_light, falloff) == 48", "sizeof(lg_light_set) == 40",
                  "offsetof(lg_light_set, count) == 8", "offsetof(lg_light_set, per_ray) == 12", "offsetof(lg_light_set, ambient) == 16", "sizeof(lg_lit_out) == 72",
                  "offsetof(lg_lit_out, terms) == 56", "offsetof(lg_lit_out, visible) == 64", "LG_MAX_CALL_LIGHTS == 1024u"):
        assert claim in host, claim
    assert "MAX_CALL_LIGHTS == LG_MAX_CALL_LIGHTS && sizeof(DLight) == sizeof(lg_light)" in read("lasgun_amd", "csrc", "query.cpp")
    assert "sizeof(lg_light) == 72 && sizeof(lg_light_set) == 40 && sizeof(lg_lit_out) == 72" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    for struct, fields in (("lg_light", [("position", "[f64; 3]"), ("intensity", "[f64; 3]"), ("falloff", "[f64; 3]")]),
                           ("lg_light_set", [("lights", "*const lg_light"), ("count", "u32"), ("per_ray", "u32"), ("ambient", "[f64; 3]")]),
                           ("lg_lit_out", [("scatter", "lg_scatter_out"), ("terms", "*mut f64"), ("visible", "*mut u32")])):
        m = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct %s \{(.*?)\n\}" % struct, sys_src, flags=re.S)
        assert m and re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == fields, struct
    assert "pub const LG_MAX_CALL_LIGHTS: u32 = 1024;" in sys_src
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    assert "size_of::<sys::lg_light>() == 72 && std::mem::size_of::<sys::lg_light_set>() == 40 && std::mem::size_of::<sys::lg_lit_out>() == 72" in safe


def test_the_sys_crate_is_the_generators_output():
    import contextlib
    import io
    import gen_rust_sys
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        gen_rust_sys.main()
    assert buf.getvalue() == read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")


def test_capi_and_the_python_wrappers_mirror_them():
    import gen_rust_sys
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.LIT_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    decl = {name: params for _, name, params in gen_rust_sys.declarations(read("include", "lasgun_hip.h"))}
    ctype = {"usize": ctypes.c_size_t, "u32": ctypes.c_uint32, "c_int": ctypes.c_int}
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
        want = [ctype.get(gen_rust_sys.rust_type(p), ctypes.c_void_p) for p in decl["lg_" + key]]  # (every pointer travels as c_void_p)
        assert list(argtypes) == want, (key, argtypes, want)
    for wrapper in ("scatter_lit", "scatter_lit_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.scatter_lit), "accel.scatter_lit(rays, lights, ambient, planes=...)"
    for bad in (("hits", "colour"), ("Terms",)):
        try:
            la.api.scatter_lit(None, np.zeros((1, 6)), [], planes=bad)
        except ValueError:
            continue
        raise AssertionError("a plane that lg_lit_out does not have is refused by name")
    # lights_array: Light()s, records, and nine doubles a light; shared (K,) and per ray (n, K)
    one = la.Light([1, 2, 3], [0.5, 0.25, 0.125])
    a = la.lights_array([one, la.Light([0, 0, 0], [1, 1, 1], [0, 0, 1])])
    assert a.dtype == la.LIGHT_DTYPE and a.shape == (2,) and a["falloff"].tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]] and a["position"][0].tolist() == [1.0, 2.0, 3.0]
    flat = np.arange(4 * 3 * 9, dtype=np.float64).reshape(4, 3, 9)
    b = la.lights_array(flat)
    assert b.shape == (4, 3) and b["intensity"][2, 1].tolist() == flat[2, 1, 3:6].tolist() and la.lights_array(b) is b
    ls, count, per_ray, _ = la.api._light_set(b, 4, (0.1, 0.2, 0.3))
    assert (ls.count, ls.per_ray, count, bool(per_ray), list(ls.ambient)) == (3, 1, 3, True, [0.1, 0.2, 0.3]) and ls.lights == b.ctypes.data
    ls, count, per_ray, _ = la.api._light_set(a, 4, (0, 0, 0))
    assert (ls.count, ls.per_ray) == (2, 0)
    for wrong in (lambda: la.api._light_set(b, 5, (0, 0, 0)), lambda: la.lights_array(np.zeros((3, 8)))):
        try:
            wrong()
        except ValueError:
            continue
        raise AssertionError("a table of the wrong shape is refused")


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_scatter_lit\(", src) and re.search(r"\blg_scatter_lit_device\(", src)
    assert re.search(r"void scatter_lit\(", src) and re.search(r"void scatter_lit_device\(", src) and "struct ScatterLit {" in src


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn scatter_lit\(", safe) and re.search(r"pub unsafe fn scatter_lit_device\(", safe) and "pub struct ScatterLit<'a>" in safe
    assert "lights: *const lg_light_set, out: *const lg_lit_out" in sys_src and "dev_out: *const lg_lit_out" in sys_src
    assert "was NOT compiled" in read("bindings", "rust", "README.md") and "`Accel::scatter_lit`" in read("bindings", "rust", "README.md")


def test_the_device_code_is_level_0_with_a_shadow_pass_of_its_own():
    """The closest pass is the shared body over a source derived from ScatterSource in the five forms x PERM; the shadow pass is new, in
    the five forms x PER_RAY, over (hit tile, word) work tiles, one word a lane; the emit kernel restates shade_lights under the call's
    lights; the host reaches the shadow pass through a hook of Level0 and sizes a chunk's visibility by vis_words."""
    src = read("lasgun_amd", "csrc", "k_lit.hip")
    assert "template <bool PERM> struct LitSource : ScatterSource<PERM> {" in src and "l0_closest_body<FAST, LDSS, PRUNE>(P, LitSource<PERM>{{Q}, Q})" in src
    assert re.search(r"template <bool FAST, bool LDSS, bool PRUNE, bool PER_RAY>\n__global__ void __launch_bounds__\(LDSS \? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD\) lit_shadow_kernel\(", src)
    assert re.search(r"template <bool PERM>\n__global__ void __launch_bounds__\(LG_BLOCK, 3\) lit_emit_kernel\(", src)
    code = src.split("namespace lg {")[1]
    bare = re.sub(r"//[^\n]*", "", code)
    assert "atomic" not in bare and "wave_append" not in bare and "wf_q_next" not in bare and "wf_spec" not in bare and "P.lights" not in bare and "P.nlights" not in bare and "P.ambient" not in bare
    shadow = code[code.index("lit_shadow_kernel("):code.index("// In scatter_emit_kernel's place")]
    for call in ("hit_slots(P, 0u, 64u)", "const uint32_t ntiles = hs.tiles * W;", "const uint32_t tile = id / W, w = id - tile * W;", "hit_of(P, hs, tile, lane, h)",
                 "const V3 hit_p = praw + ng * err;", "PER_RAY ? Q.lights + (unsigned long long)K * r : Q.lights", "walk<LDSS, FAST, PRUNE>(P, sray, true, stack, stride, b, scn, cnt, arec);",
                 "if (!(b.t < 1.0)) vis |= 1u << k;", "P.vis[(unsigned long long)w * n + h] = vis;", "if (Q.skip) {", "light_irrelevant(t)", "t.f_att == 0.0",
                 "copy_to_lds(", "claim_tile(P.tile_counter, ntiles, band, bands_left, final)", "claim_tile_single(P.tile_counter, ntiles, final)"):
        assert call in shadow, call
    assert shadow.count("P.vis[") == 1, "one store of one word a lane"
    emit = code[code.index("lit_emit_kernel("):code.index("// ---- host-callable launchers")]
    for call in ("hit_of(P, hs, (uint32_t)t, lane, h)", "wo_terms(m, sh, sh.wo)", "P.vis[(unsigned long long)(k >> 5) * n + h]", "light_term(L, sh)", "if (lt.f_att != 0.0) {",
                 "mul_ew(PI * li_col, fr) * lt.wi_dot_n / lt.f_att", "output = output + added;", "term = vzero() + added;", "Q.ambient[0], Q.ambient[1], Q.ambient[2]",
                 "bsdf_f(m, sh, wt, nrm, bsdf_reflect(sh, sh.wo, nrm))", "sample_specular_transmission(m, sh, st)", "sample_specular_reflection(m, sh, sr)",
                 "-1.0 * sh.wo + 2.0 * dot(sh.wo, sh.ns) * sh.ns", "sh.p = p + p_err; sh.pm = p - p_err"):
        assert call in emit, call
    for family in ("LitClosestKernels", "LitShadowKernels"):
        assert "trav_launch<%s>" % family in src and "trav_set_lds_limit<%s>" % family in src, family
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_lit.o" in make and "lit_host.h" in make and "scatter_source.h" in make
    assert "lit_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    assert '#include "scatter_source.h"' in read("lasgun_amd", "csrc", "k_scatter.hip") and "template <bool PERM> struct ScatterSource {" in read("lasgun_amd", "csrc", "scatter_source.h")
    launch = read("lasgun_amd", "csrc", "launch.cpp")
    fn = launch[launch.index("void enqueue_scatter_lit("):launch.index("// A radiance gather (query.cpp")]
    assert "call.one_level = true;" in fn and "call.vis_words = std::max(1u, Q.vis_words);" in fn and "enqueue_level0_query(a, call," in fn and "launch_wf_trace" not in fn
    assert "l0.own_shadow = true;" in fn and "if (Q.n_lights) l0.shadow_ = l0_closest<LitArgs, launch_lit_shadow>;" in fn and "stage_rule_table(shared" in fn
    assert "static size_t extra_per_item(uint32_t levels, uint32_t groups = 1, uint32_t vis_words = 1)" in launch and "vis = (uint32_t *)take(hit_len() * 4 * vis_words);" in launch
    assert "if (own0 && l0.own_shadow) {" in launch and "do not fit 32 bits" in launch
    diff = read("profiles", "r23_kernel_resources_diff.txt")
    assert "no line removed, no line changed" in diff and "lit_shadow_kernel" in diff and "lit_emit_kernel" in diff


def test_the_restatements_on_stubs():
    import lit_ref as L
    pool = L.pool()
    assert pool.shape == (70,) and pool.tobytes() == L.pool().tobytes(), "a fixed seed"
    for a, (lo, hi) in enumerate(L.POOL_BOX):
        assert (pool["position"][:, a] >= lo).all() and (pool["position"][:, a] <= hi).all()
    zero = (pool["falloff"] == 0.0).all(axis=1)
    assert zero.sum() == 1 and zero[L.ZERO_FALLOFF] and len({tuple(f) for f in pool["falloff"].tolist()}) >= 4
    # bits: word k >> 5, bit k & 31; nothing at or above K
    v = np.zeros((2, 70), dtype=bool)
    v[0, [0, 31, 32, 69]] = True
    w = L.pack_bits(v)
    assert w.shape == (2, 3) and w[0].tolist() == [0x80000001, 1, 1 << 5] and not w[1].any()
    assert np.array_equal(L.unpack_bits(w, 70), v) and L.unpack_bits(w, 0).shape == (2, 0) and L.pack_bits(v[:, :0]).shape == (2, 0)
    # the sum: in order from +0.0, the ambient term last
    t = np.array([[[1e16, 0, -0.0], [1.0, 0, 0.0], [-1e16, 0, 0.0]]])
    s = L.sequential_sum(t, np.array([[0.5, -0.0, -0.0]]))
    assert s[0].tolist() == [0.5, 0.0, 0.0] and not np.signbit(s[0, 1]) and not np.signbit(s[0, 2])  # ((1e16 + 1) - 1e16) + 0.5, and +0 + -0 = +0
    # the segments: from p + ng * 2^-36 towards the light, shared and per ray
    import lasgun_amd as la
    hits = np.zeros(2, dtype=la.HIT_DTYPE)
    hits["p"] = [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]
    hits["ng"] = [[0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]
    seg = L.shadow_segments(hits, np.array([[1.0, 5.0, 3.0]]))
    assert seg.shape == (2, 1, 6) and seg[0, 0].tolist() == [1.0, 2.0 + 2.0 ** -36, 3.0, 0.0, 5.0 - (2.0 + 2.0 ** -36), 0.0] and seg[1, 0, 2] == -(2.0 ** -36)
    per = L.shadow_segments(hits, np.array([[[1.0, 5.0, 3.0]], [[0.0, 0.0, 1.0]]]))
    assert per[0].tolist() == seg[0].tolist() and per[1, 0, 5] == 1.0 + 2.0 ** -36


def test_the_no_device_errors_are_refused_and_touch_nothing():
    """A NULL accel with n > 0 is answered before anything else is looked at, whatever the other arguments."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    n, k = 5, 3
    arrs = [np.full(n * words, 0xA5A5A5A5, dtype=np.uint32) for words in (24, 6, 1, 12, 6, 12, 10, 6 * k, 1)]
    out = _capi.CLitOut(_capi.CScatterOut(*[a.ctypes.data for a in arrs[:7]]), arrs[7].ctypes.data, arrs[8].ctypes.data)
    table = la.lights_array([la.Light([0, 1, 0], [1, 1, 1])] * k)
    ls = _capi.CLightSet(table.ctypes.data, k, 0, (ctypes.c_double * 3)(0, 0, 0))
    G = la.api
    rays = np.zeros((n, 6))
    rays[:, 5] = 1.0
    A = ctypes.addressof
    for fn, tail in (("scatter_lit", ()), ("scatter_lit_device", (None,))):
        assert G.call(fn, None, rays.ctypes.data, n, A(ls), A(out), *tail) != 0 and "accel is NULL" in G.last_error(), fn
        assert G.call(fn, None, None, n, None, None, *tail) != 0 and G.last_error(), fn
        assert all((a == 0xA5A5A5A5).all() for a in arrs), fn
    check = read("tools", "lit_host_check.cpp")  # (the stand-alone check exercises every other refusal through check_lit)
    assert "refused(&accel, D, 3, nullptr, &all)" in check and "refused(&accel, D, 3, &one, &none)" in check and "set_of(&ONE_LIGHT, 1, 2)" in check


def test_an_empty_set_is_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    assert G.call("scatter_lit", None, None, 0, None, None) == 0
    assert G.call("scatter_lit_device", None, None, 0, None, None, None) == 0
