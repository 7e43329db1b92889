"""Hit attributes (include/lasgun_hip.h: lg_hit_attributes, lg_hit_attributes_device, lg_hit_attributes_of, lg_hit_attributes_of_device)
through every layer that has to carry them, checked without a GPU: the built library exports the symbols, the header declares them with
the arity, the parameter names and the types the wrappers use and states the contract -- the two forms, the local ray, every plane's
formula per primitive kind, the _of form's four verdicts, the NaN rule, the limits, what is out of scope --, lg_attr_out is 56 bytes with
the stated offsets in every mirror, the device code is query_kernel's closest form over the unchanged walk with the planes from a second
evaluation behind the barrier and a grid-stride kernel that checks a record before it reads through it, and the Python, C++ and Rust
bindings mirror the entry points.  On top: the errors answered before any HIP call, the no-op of an empty set."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_hit_attributes": 4, "lg_hit_attributes_device": 5, "lg_hit_attributes_of": 5, "lg_hit_attributes_of_device": 6}
NAMES = tuple(ARITY)
MEMBERS = [("lg_hit", "hits"), ("uint32_t", "flags"), ("double", "bary"), ("double", "uv"), ("double", "local"), ("double", "frame"), ("double", "dp")]
PLANES = tuple(m[1] for m in MEMBERS)
CONSTANTS = {"LG_ATTR_HIT": 1, "LG_ATTR_NO_HIT": 2, "LG_ATTR_BAD_RECORD": 4}


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
    assert names("lg_hit_attributes")[1:] == ["rays", "n", "out"]
    assert names("lg_hit_attributes_device")[1:] == ["dev_rays", "n", "dev_out", "hip_stream"]
    assert names("lg_hit_attributes_of")[1:] == ["rays", "hits", "n", "out"]
    assert names("lg_hit_attributes_of_device")[1:] == ["dev_rays", "dev_hits", "n", "dev_out", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    assert types("lg_hit_attributes")[1:] == ["const double *", "size_t", "const lg_attr_out *"]
    assert types("lg_hit_attributes_device")[1:] == ["const double *", "size_t", "const lg_attr_out *", "void *"]
    assert types("lg_hit_attributes_of")[1:] == ["const double *", "const lg_hit *", "size_t", "const lg_attr_out *"]
    assert types("lg_hit_attributes_of_device")[1:] == ["const double *", "const lg_hit *", "size_t", "const lg_attr_out *", "void *"]
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s\s+%du\b" % (name, value), header, flags=re.M), name
    order = ["int lg_scatter_lit_device(", "/* Hit attributes:", "typedef struct lg_attr_out {", "int lg_hit_attributes(", "int lg_hit_attributes_device(",
             "int lg_hit_attributes_of(", "int lg_hit_attributes_of_device("]
    at = [header.index(o) for o in order]
    assert at == sorted(at)
    struct = header[header.index("typedef struct lg_attr_out {"):header.index("} lg_attr_out;")]
    assert re.findall(r"^\s+(\w+)\s*\*(\w+);", struct, flags=re.M) == MEMBERS
    text = header[header.index("/* Hit attributes:"):header.index("typedef struct lg_attr_out {")]
    for phrase in ("An EXTRA; no counterpart in the reference",
                   "Everything is f64, nothing is fused",
                   "hits[i] is lg_intersect's record of",
                   "lg_accel_set_query_order(1) is honoured as lg_intersect honours it",
                   "flags[i] = 0 for a miss, LG_ATTR_HIT for a hit",
                   "A miss writes\n * +0.0 into every other plane",
                   "Only kind, prim and instance of each record are read; out->hits must be NULL",
                   "a pure function of (ray, kind, prim, instance)",
                   "local = lr.o + lr.d * t; for a sphere taken before the centre is subtracted and before the pole nudge",
                   "e0*invdet, e1*invdet, e2*invdet of Triangle::intersect (triangle.rs:161-251)",
                   "u = (b0*u0 + b1*u1) + b2*u2",
                   "(0,0), (1,0), (1,1)",
                   "u = phi / (2.0*PI), v = theta / PI",
                   "the p.x = 1e-5*r nudge",
                   "the +2*PI wrap",
                   "u = (local[j] - min[j]) / (max[j] - min[j])",
                   "a flat box gives whatever IEEE gives",
                   "bary, uv and local are primitive-local: no transform and no swap_backface changes them",
                   "transform_ray_intersection of every accel on the way up (transform.rs:243-264)",
                   "face_forward(normalize(cross(gu, gv)), -normalize(d))",
                   "ts = cross(ns, ss) with ns lg_hit's",
                   "kind == 0 gives flags 0 and +0.0 in every plane",
                   "LG_ATTR_BAD_RECORD and +0.0, and nothing is dereferenced through it",
                   "kind > 3; instance >= the accel's instance count",
                   "a sphere or box that does not sit in\n * `instance`",
                   "a sphere with t < 0 (as bvh.rs accepts)",
                   "the planes are the walking form's, the same bytes",
                   "SOME NaN",
                   "written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill",
                   "a scene of 40 lights is accepted",
                   "n == 0 is a successful no-op that writes nothing, answered BEFORE every other check",
                   "n > (2^32 - 1) * 64",
                   "all planes NULL",
                   "a\n * NULL `hits` argument or a non-NULL out->hits",
                   "rays 8 bytes; hits 16; flags 4; bary, uv, local, frame and dp 8",
                   "a buffer that ends beyond its allocation",
                   "dev_out is a HOST struct of device pointers",
                   "come back into staging and are copied out at the end"):
        assert phrase in text, phrase
    for scope in ("texture lookup itself", "ray differentials", "a maximum range in the walk", "a multi-device split"):
        assert scope in text[text.index("Out of scope:"):], scope


def test_the_struct_is_56_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    C = _capi.CAttrOut
    assert ctypes.sizeof(C) == 56 and [f[0] for f in C._fields_] == list(la.ATTR_PLANES)
    assert la.ATTR_PLANES == PLANES
    assert [getattr(C, p).offset for p in la.ATTR_PLANES] == [8 * k for k in range(7)]
    assert (la.ATTR_HIT, la.ATTR_NO_HIT, la.ATTR_BAD_RECORD) == (1, 2, 4)
    host = read("lasgun_amd", "csrc", "attributes_host.h")  # static_asserts of the library's own build
    assert "sizeof(lg_attr_out) == 56" in host and all("offsetof(lg_attr_out, %s) == %d" % (p, 8 * k) in host for k, p in enumerate(la.ATTR_PLANES))
    assert "ATTR_HIT == LG_ATTR_HIT && ATTR_NO_HIT == LG_ATTR_NO_HIT && ATTR_BAD_RECORD == LG_ATTR_BAD_RECORD" in host
    assert "static_assert(sizeof(lg_attr_out) == 56" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_attr_out \{(.*?)\n\}", sys_src, flags=re.S)
    rust = {"lg_hit": "lg_hit", "double": "f64", "uint32_t": "u32"}
    assert struct and re.findall(r"pub (\w+): \*mut (\w+),", struct.group(1)) == [(n, rust[t]) for t, n in MEMBERS]
    for name, value in CONSTANTS.items():
        assert "pub const %s: u32 = %d;" % (name, value) in sys_src, name
    assert "std::mem::size_of::<sys::lg_attr_out>() == 56" in read("bindings", "rust", "lasgun", "src", "lib.rs")


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
    sigs = _capi.ATTRIBUTES_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    decl = {name: params for _, name, params in gen_rust_sys.declarations(read("include", "lasgun_hip.h"))}
    ctype = {"usize": ctypes.c_size_t, "u32": ctypes.c_uint32, "c_int": ctypes.c_int}
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
        want = [ctype.get(gen_rust_sys.rust_type(p), ctypes.c_void_p) for p in decl["lg_" + key]]  # (every pointer travels as c_void_p)
        assert list(argtypes) == want, (key, argtypes, want)
    for wrapper in ("hit_attributes", "hit_attributes_device", "hit_attributes_of", "hit_attributes_of_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.hit_attributes), "accel.hit_attributes(rays, planes=...)"
    for bad in (("hits", "colour"), ("UV",)):
        try:
            la.api.hit_attributes(None, np.zeros((1, 6)), bad)
        except ValueError:
            continue
        raise AssertionError("a plane that lg_attr_out does not have is refused by name")
    try:  # the _of form has no hits plane
        la.api.hit_attributes_of(None, np.zeros((1, 6)), np.zeros(1, dtype=la.HIT_DTYPE), ("hits",))
    except ValueError:
        pass
    else:
        raise AssertionError("hit_attributes_of refuses the hits plane by name")


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, src), name
    assert re.search(r"void hit_attributes\(", src) and re.search(r"void hit_attributes_device\(", src) and "struct Attributes {" in src


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn hit_attributes\(", safe) and re.search(r"pub fn hit_attributes_of\(", safe)
    assert re.search(r"pub unsafe fn hit_attributes_device\(", safe) and re.search(r"pub unsafe fn hit_attributes_of_device\(", safe)
    assert "out: *const lg_attr_out" in sys_src and "dev_out: *const lg_attr_out" in sys_src and "dev_hits: *const lg_hit" in sys_src
    assert "was NOT compiled" in read("bindings", "rust", "README.md") and "`Accel::hit_attributes`" in read("bindings", "rust", "README.md")


def test_the_device_code_is_the_unchanged_walk_with_a_second_evaluation():
    """attr_kernel: query_kernel's prologue, claim and record stores in the five forms x PERM; the record's evaluation has shade_frame's
    uses alone, the planes come from attr_resolve behind the barrier; attr_of_kernel has no walk and no LDS stack; walk.h and shade.h carry
    nothing of it."""
    src = read("lasgun_amd", "csrc", "k_attributes.hip")
    code = src.split("namespace lg {")[1]
    bare = re.sub(r"//[^\n]*", "", code)
    walk = bare[bare.index("attr_kernel(const DParams P"):bare.index("attr_of_kernel(const DParams P")]
    for call in ("walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec)", "claim_tile(P.tile_counter, ntiles, band, bands_left, final)",
                 "claim_tile_single(P.tile_counter, ntiles, final)", "if (PERM && active) i = Q.perm[i];", "shade_frame(P, ray, b, sh);",
                 "out[5] = make_uint4(pk + 1u, prim, b.accel, (uint32_t)sh.mat);", "attr_store(Q, i, ATTR_HIT, attr_planes_of(P, ray, b));",
                 "attr_store(Q, i, 0u, attr_zero());"):
        assert call in walk, call
    assert walk.count("shade_frame(") == 1 and "attr_resolve(" not in walk, "the record's evaluation has query_kernel's uses alone"
    barrier = bare[bare.index("attr_planes_of(const DParams &P"):bare.index("template <bool FAST, bool LDSS, bool PRUNE, bool PERM>")]
    assert barrier.count("attr_opaque(") == 6 and "attr_resolve(P, ray," in barrier and 'asm volatile("" : "+v"(x));' in bare
    of = bare[bare.index("attr_of_kernel(const DParams P"):bare.index("template <bool F, bool L, bool Z> struct AttrKernels")]
    assert "walk<" not in of and "lds_stack" not in of and "shade_frame" not in of and "atomic" not in bare
    assert "trav_launch<AttrKernels>" in src and "trav_set_lds_limit<AttrKernels>" in src and "trav_occupancy<AttrKernels>" in src
    resolve = read("lasgun_amd", "csrc", "attr_resolve.h")
    for call in ("local_ray(P, wray, accel)", "triangle_t(p0, p1, p2, lr, h)", "cuboid_hit<true>(c.mn, c.mx, lr, t, d0, d1)", "sphere_t(lr, V3{s.cx, s.cy, s.cz}, s.r, inside)",
                 "at.u = phi / (2.0 * PI);", "at.v = theta / PI;", "at.u = (h.b0 * uv[0][0] + h.b1 * uv[1][0]) + h.b2 * uv[2][0];", "at.ss = normalize(is.su);",
                 "at.ts = cross(ns, at.ss);"):
        assert call in resolve, call
    for untouched in ("walk.h", "shade.h", "dscene.h", "k_query.hip"):
        assert "attr" not in read("lasgun_amd", "csrc", untouched).lower().replace("__attribute__", "").replace("hipfuncattribute", ""), untouched
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_attributes.o" in make and "-ffp-contract=off" in make and "attributes_host.h" in make and "attr_resolve.h" in make
    assert "attributes_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    host = read("lasgun_amd", "csrc", "query.cpp")
    whole = host[host.index("// ---- hit attributes"):host.index("// ---- ray paths")]
    assert whole.count("traversal_grid(a, P, attributes_occupancy, c, stream)") == 1 and whole.count("launch_attributes(") == 1 and whole.count("launch_attr_of(") == 1
    assert "for (" not in whole and "guarded(" in whole, "one launch, no chunks"
    diff = read("profiles", "r26_kernel_resources_diff.txt")
    assert "no line removed, no line changed" in diff and "attr_of_kernel" in diff and diff.count("> k_attributes") == 11 and "lg::query_kernel<" in diff


def outputs(n):
    """The seven planes of lg_attr_out over a 0xA5 prefill (as uint32 words, whatever the plane's type) and the struct that names them."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    arrs = [np.full(n * words, 0xA5A5A5A5, dtype=np.uint32) for words in (24, 1, 6, 4, 6, 12, 12)]
    return arrs, _capi.CAttrOut(*[a.ctypes.data for a in arrs]), la


def test_the_no_device_errors_are_refused_and_touch_nothing():
    """A NULL accel with n > 0 is answered before anything else is looked at, whatever the other arguments."""
    n = 5
    arrs, out, la = outputs(n)
    G = la.api
    rays = np.zeros((n, 6))
    rays[:, 5] = 1.0
    recs = np.zeros(n, dtype=la.HIT_DTYPE)
    A = ctypes.addressof
    for fn, mid, tail in (("hit_attributes", (), ()), ("hit_attributes_device", (), (None,)), ("hit_attributes_of", (recs.ctypes.data,), ()),
                          ("hit_attributes_of_device", (recs.ctypes.data,), (None,))):
        assert G.call(fn, None, rays.ctypes.data, *mid, n, A(out), *tail) != 0 and "accel is NULL" in G.last_error(), fn
        assert G.call(fn, None, None, *((None,) * len(mid)), n, None, *tail) != 0 and G.last_error(), fn
        assert all((a == 0xA5A5A5A5).all() for a in arrs), fn
    check = read("tools", "attributes_host_check.cpp")  # (the stand-alone check exercises every other refusal through check_attributes)
    assert "refused(&accel, D, nullptr, false, 3, &none)" in check and "refused(nullptr, D, nullptr, false, 3, &all)" in check


def test_an_empty_set_is_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    assert G.call("hit_attributes", None, None, 0, None) == 0
    assert G.call("hit_attributes_device", None, None, 0, None, None) == 0
    assert G.call("hit_attributes_of", None, None, None, 0, None) == 0
    assert G.call("hit_attributes_of_device", None, None, None, 0, None, None) == 0
