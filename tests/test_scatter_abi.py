"""Surface scatter (include/lasgun_hip.h: lg_scatter, lg_scatter_device) through every layer that has to carry it, checked without a GPU:
the built library exports the symbols, the header declares them with the arity, the parameter names and the types the wrappers use and
states the contract -- the record, the light sum and the shadow test, the children as the render's shade pass makes them, misses and
absent children, the composition rule and what it equals, the NaN rule, the limits, what is out of scope --, lg_scatter_out is 56 bytes
with the stated offsets in every mirror, the device code is level 0 of the level-by-level pipeline over the shared closest body with an
emit kernel of its own and no copy of the chain, and the Python, C++ and Rust bindings mirror the entry points.  On top: the composition
loop on a stub, the errors answered before any HIP call, the no-op of an empty set."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_scatter": 4, "lg_scatter_device": 5}
NAMES = tuple(ARITY)
MEMBERS = [("lg_hit", "hits"), ("double", "direct"), ("uint32_t", "flags"), ("double", "reflect"), ("double", "reflect_weight"), ("double", "refract"),
           ("double", "refract_weight")]
PLANES = tuple(m[1] for m in MEMBERS)
CONSTANTS = {"LG_SCATTER_HIT": 1, "LG_SCATTER_REFLECT": 2, "LG_SCATTER_REFRACT": 4}


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
    assert names("lg_scatter")[1:] == ["rays", "n", "out"]
    assert names("lg_scatter_device")[1:] == ["dev_rays", "n", "dev_out", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "size_t", "const lg_scatter_out *"]
    assert types("lg_scatter")[1:] == host and types("lg_scatter_device")[1:] == host + ["void *"]
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s\s+%du\b" % (name, value), header, flags=re.M), name
    order = ["int lg_radiance_groups_device(", "/* Surface scatter:", "typedef struct lg_scatter_out {", "int lg_scatter(", "int lg_scatter_device("]
    at = [header.index(o) for o in order]
    assert at == sorted(at)
    struct = header[header.index("typedef struct lg_scatter_out {"):header.index("} lg_scatter_out;")]
    assert re.findall(r"^\s+(\w+)\s*\*(\w+);", struct, flags=re.M) == MEMBERS
    text = header[header.index("/* Surface scatter:"):header.index("typedef struct lg_scatter_out {")]
    for phrase in ("An EXTRA; no counterpart in the reference",
                   "hits[i] is lg_intersect's record of ray i, bit for bit",
                   "in lg_scene_add_point_light order from zero",
                   "ambient term added last (integrate.rs:47-67)",
                   "!(t < 1.0)",
                   "whatever depth the accel",
                   "!(pdf <= 0 || spectrum == 0 || |wi . ns| == 0)",
                   "!(pdf <= 0 || spectrum == 0 || wi . ns <= 0)",
                   "origin p + ng*(2^-52 * 2^16), direction -wo + 2 (wo . ns) ns",
                   "p - ng*2^-36",
                   "direct[i] = background(normalize(d))",
                   "An absent child's ray and weight elements are +0.0",
                   "the same scene built at two depths gives the same bytes",
                   "= (direct + 0) + 0",
                   "= (direct + R) + T",
                   "R = reflect_weight * L(reflect, d+1), or +0 if the child is absent",
                   "T = ((spectrum * L(refract, d+1)) * cos) / pdf, or +0 if absent",
                   "(0 + L(ray, 0)) * 1.0 is lg_radiance's value",
                   "SOME NaN",
                   "written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill",
                   "lg_accel_set_query_order(1) is honoured exactly as lg_radiance honours it",
                   "n == 0 is a successful no-op that writes nothing, answered BEFORE every other check",
                   "n > (2^32 - 1) * 64",
                   "all seven planes NULL",
                   "more than 32",
                   "the accel's recursion depth is never a reason to refuse",
                   "rays 8 bytes; hits 16; direct, reflect, reflect_weight, refract and",
                   "a buffer that ends beyond its allocation",
                   "dev_out is a HOST struct of device pointers",
                   "come back into staging and are copied out at the end"):
        assert phrase in text, phrase
    for scope in ("the visibility word as a plane", "BSDF evaluation for a caller-supplied wi", "non-specular sampling", "multi-device split", "re-packing of lanes"):
        assert scope in text[text.index("Out of scope:"):], scope


def test_the_struct_is_56_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    C = _capi.CScatterOut
    assert ctypes.sizeof(C) == 56 and [f[0] for f in C._fields_] == list(la.SCATTER_PLANES)
    assert la.SCATTER_PLANES == PLANES
    assert [getattr(C, p).offset for p in la.SCATTER_PLANES] == [8 * k for k in range(7)]
    assert (la.SCATTER_HIT, la.SCATTER_REFLECT, la.SCATTER_REFRACT) == (1, 2, 4)
    host = read("lasgun_amd", "csrc", "scatter_host.h")  # static_asserts of the library's own build
    assert "sizeof(lg_scatter_out) == 56" in host and all("offsetof(lg_scatter_out, %s) == %d" % (p, 8 * k) in host for k, p in enumerate(la.SCATTER_PLANES))
    assert "SCATTER_HIT == LG_SCATTER_HIT && SCATTER_REFLECT == LG_SCATTER_REFLECT && SCATTER_REFRACT == LG_SCATTER_REFRACT" in read("lasgun_amd", "csrc", "query.cpp")
    assert "static_assert(sizeof(lg_scatter_out) == 56" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_scatter_out \{(.*?)\n\}", sys_src, flags=re.S)
    rust = {"lg_hit": "lg_hit", "double": "f64", "uint32_t": "u32"}
    assert struct and re.findall(r"pub (\w+): \*mut (\w+),", struct.group(1)) == [(n, rust[t]) for t, n in MEMBERS]
    for name, value in CONSTANTS.items():
        assert "pub const %s: u32 = %d;" % (name, value) in sys_src, name
    assert "std::mem::size_of::<sys::lg_scatter_out>() == 56" in read("bindings", "rust", "lasgun", "src", "lib.rs")


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
    sigs = _capi.SCATTER_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    decl = {name: params for _, name, params in gen_rust_sys.declarations(read("include", "lasgun_hip.h"))}
    ctype = {"usize": ctypes.c_size_t, "u32": ctypes.c_uint32, "c_int": ctypes.c_int}
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
        want = [ctype.get(gen_rust_sys.rust_type(p), ctypes.c_void_p) for p in decl["lg_" + key]]  # (every pointer travels as c_void_p)
        assert list(argtypes) == want, (key, argtypes, want)
    for wrapper in ("scatter", "scatter_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.scatter), "accel.scatter(rays, planes=...)"
    for bad in (("hits", "colour"), ("Direct",)):
        try:
            la.api.scatter(None, np.zeros((1, 6)), bad)
        except ValueError:
            continue
        raise AssertionError("a plane that lg_scatter_out does not have is refused by name")


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_scatter\(", src) and re.search(r"\blg_scatter_device\(", src)
    assert re.search(r"void scatter\(", src) and re.search(r"void scatter_device\(", src) and "struct Scatter {" in src


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn scatter\(", safe) and re.search(r"pub unsafe fn scatter_device\(", safe)
    assert "out: *const lg_scatter_out" in sys_src and "dev_out: *const lg_scatter_out" in sys_src
    assert "was NOT compiled" in read("bindings", "rust", "README.md") and "`Accel::scatter`" in read("bindings", "rust", "README.md")


def test_the_device_code_is_level_0_as_a_chain_of_one_level():
    """The closest pass is the shared body over a source of its own in the five forms x PERM, the shadow pass is the render's, one emit
    kernel stands where the shade pass stands; the host takes the source through the Level0 generalisation, not a copy of the chain."""
    src = read("lasgun_amd", "csrc", "k_scatter.hip")
    assert re.search(r"__global__ void [^\n]*\bscatter_closest_kernel\(", src) and "l0_closest_body<FAST, LDSS, PRUNE>(P, ScatterSource<PERM>{Q})" in src
    assert re.search(r"template <bool PERM>\n__global__ void __launch_bounds__\(LG_BLOCK, 3\) scatter_emit_kernel\(", src)
    code = src.split("namespace lg {")[1]
    bare = re.sub(r"//[^\n]*", "", code)  # (the comments speak of what the render does with these)
    assert "walk<" not in bare and "wave_append" not in bare and "atomic" not in bare and "wf_q_next" not in bare and "wf_spec" not in bare and "wf_child" not in bare
    emit = code[code.index("scatter_emit_kernel("):code.index("// ---- host-callable launchers")]
    for call in ("hit_slots(P, 0u, 64u)", "hit_of(P, hs, (uint32_t)t, lane, h)", "shade_lights(P, m, sh, vis)", "sample_specular_transmission(m, sh, st)",
                 "sample_specular_reflection(m, sh, sr)", "!(st.pdf <= 0.0 || veq(st.spectrum, vzero()) || fabs(dot(st.wi, sh.ns)) == 0.0)",
                 "!(sr.pdf <= 0.0 || veq(sr.spectrum, vzero()) || dot(sr.wi, sh.ns) <= 0.0)", "-1.0 * sh.wo + 2.0 * dot(sh.wo, sh.ns) * sh.ns",
                 "sh.p = p + p_err; sh.pm = p - p_err", "sh.ts = cross(sh.ns, sh.ss)"):
        assert call in emit, call
    assert "trav_launch<ScatterClosestKernels>" in src and "trav_set_lds_limit<ScatterClosestKernels>" in src
    body = read("lasgun_amd", "csrc", "level0.h")
    assert "template <class SRC> __device__ __forceinline__ void l0_closest_hit(const SRC &, const DParams &, const typename SRC::Item &, const Best &, const Shade &) {}" in body
    assert body.count("l0_closest_hit(src, P, it, b, sh);") == 1
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_scatter.o" in make and "-ffp-contract=off" in make and "scatter_host.h" in make
    assert "scatter_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    launch = read("lasgun_amd", "csrc", "launch.cpp")
    fn = launch[launch.index("void enqueue_scatter("):launch.index("// A radiance gather (query.cpp")]
    assert "call.one_level = true;" in fn and "enqueue_level0_query(a, call," in fn and "launch_wf_trace" not in fn and "for (" not in fn
    assert "l0_closest<ScatterArgs, launch_scatter_closest>" in fn and "l0_flat<ScatterArgs, launch_scatter_emit>" in fn
    assert "if (call.one_level) P0.recursion = 0;" in launch
    host = read("lasgun_amd", "csrc", "query.cpp")
    whole = host[host.index("// ---- surface scatter"):host.index("// ---- lens rays")]
    assert whole.count("enqueue_scatter(a, rays, n, Q, perm, c, stream)") == 1 and "radiance_possible" not in whole and "guarded(" in whole
    diff = read("profiles", "r22_kernel_resources_diff.txt")
    assert "no line removed, no line changed" in diff and "scatter_emit_kernel" in diff


def test_the_composition_loop_on_a_stub():
    """scatter_ref.compose over a stub of three levels: the operation order of the header, absent children as +0, the finish."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scatter_ref as R

    def stub(rays):
        n = len(rays)
        k = rays[:, 0]  # the ray's "kind" travels in its first component: 0 miss, 1 plain hit, 2 both children, 3 reflect only, 4 refract only
        flags = np.where(k == 0, 0, 1).astype(np.uint32) | np.where((k == 2) | (k == 3), 2, 0).astype(np.uint32) | np.where((k == 2) | (k == 4), 4, 0).astype(np.uint32)
        out = {"flags": flags, "direct": np.tile([0.1, 0.2, -0.0], (n, 1)), "reflect": np.zeros((n, 6)), "refract": np.zeros((n, 6)),
               "reflect_weight": np.tile([0.5, 0.25, 1.0], (n, 1)), "refract_weight": np.tile([0.9, 0.8, 0.7, 0.3, 0.6], (n, 1))}
        out["reflect"][:, 0] = 1.0   # a reflected child is a plain hit
        out["refract"][:, 0] = 0.0   # a transmitted child misses
        return out

    rays = np.zeros((5, 6))
    rays[:, 0] = [0, 1, 2, 3, 4]
    d = np.array([0.1, 0.2, -0.0])
    hit0 = (d + 0.0) + 0.0
    refl, refr = np.array([0.5, 0.25, 1.0]) * hit0, ((np.array([0.9, 0.8, 0.7]) * d) * 0.3) / 0.6
    want = np.array([d, hit0, (d + refl) + refr, (d + refl) + 0.0, (d + 0.0) + refr])
    got = R.compose(stub, rays, 1)
    assert got.tobytes() == ((0.0 + want) * 1.0).tobytes()
    assert not np.signbit(got[0, 2]), "the finish turns a miss's -0.0 into +0.0"
    flat = R.compose(stub, rays, 0)
    assert flat.tobytes() == ((0.0 + np.array([d, hit0, hit0, hit0, hit0])) * 1.0).tobytes()
    assert R.classes(stub(rays)["flags"]) == {"miss": 1, "no_child": 1, "reflect_only": 1, "refract_only": 1, "both": 1}


def outputs(n):
    """The seven planes of lg_scatter_out over a 0xA5 prefill (as uint32 words, whatever the plane's type) and the struct that names them."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    arrs = [np.full(n * words, 0xA5A5A5A5, dtype=np.uint32) for words in (24, 6, 1, 12, 6, 12, 10)]
    return arrs, _capi.CScatterOut(*[a.ctypes.data for a in arrs]), la


def test_the_no_device_errors_are_refused_and_touch_nothing():
    """A NULL accel with n > 0 is answered before anything else is looked at, whatever the other arguments."""
    n = 5
    arrs, out, la = outputs(n)
    G = la.api
    rays = np.zeros((n, 6))
    rays[:, 5] = 1.0
    A = ctypes.addressof
    for fn, tail in (("scatter", ()), ("scatter_device", (None,))):
        assert G.call(fn, None, rays.ctypes.data, n, A(out), *tail) != 0 and "accel is NULL" in G.last_error(), fn
        assert G.call(fn, None, None, n, None, *tail) != 0 and G.last_error(), fn
        assert all((a == 0xA5A5A5A5).all() for a in arrs), fn
    check = read("tools", "scatter_host_check.cpp")  # (the stand-alone check exercises every other refusal through check_scatter)
    assert "refused(&accel, D, 3, &none)" in check and "refused(nullptr, D, 3, &all)" in check and "refused(&accel, nullptr, 3, &all)" in check


def test_an_empty_set_is_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    assert G.call("scatter", None, None, 0, None) == 0
    assert G.call("scatter_device", None, None, 0, None, None) == 0
