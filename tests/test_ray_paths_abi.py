"""Ray paths (include/lasgun_hip.h: lg_trace_paths, lg_trace_paths_device) through every layer that has to carry them, checked without a
GPU: the built library exports the symbols, the header declares them with the arity, the parameter names and the types the wrappers use
and states the contract -- the loop over lg_intersect, the three bounce rules word for word, the crossing parity, the vertex-major planes
and what stands behind a path's last vertex, the four endings and what `last` holds for each, resuming, the limits, what is out of scope --,
lg_path_rule is 24 and lg_paths_out 72 bytes with the stated offsets in every mirror, the kernel is a HIP kernel of its own in the build
over the unchanged walk with the bounce arithmetic in its own header, and the Python, C++ and Rust bindings mirror the entry points.  On
top: the wrapper's rule convention on a table of all five materials, the errors answered before any HIP call, the no-op of an empty set."""
import ctypes
import os
import re
import sys

import numpy as np
import tilewalk_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_trace_paths": 9, "lg_trace_paths_device": 10}
NAMES = tuple(ARITY)
MEMBERS = [("lg_hit", "hits"), ("double", "point"), ("uint32_t", "id"), ("double", "along"), ("uint32_t", "count"), ("uint32_t", "end"), ("double", "gain"),
           ("double", "last"), ("uint32_t", "medium")]
PLANES = tuple(m[1] for m in MEMBERS)
CONSTANTS = {"LG_PATH_ABSORB": 0, "LG_PATH_REFLECT": 1, "LG_PATH_PASS": 2, "LG_PATH_REFRACT": 3, "LG_PATH_END_CUT": 0, "LG_PATH_END_ESCAPED": 1,
             "LG_PATH_END_ABSORBED": 2, "LG_PATH_END_DEGENERATE": 3}


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
    assert names("lg_trace_paths")[1:] == ["rays", "n", "max_bounces", "rules", "n_rules", "normal", "start_medium", "out"]
    assert names("lg_trace_paths_device")[1:] == ["dev_rays", "n", "max_bounces", "rules", "n_rules", "normal", "dev_start_medium", "dev_out", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "size_t", "uint32_t", "const lg_path_rule *", "size_t", "int", "const uint32_t *", "const lg_paths_out *"]
    assert types("lg_trace_paths")[1:] == host
    assert types("lg_trace_paths_device")[1:] == host + ["void *"]
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s\s+%du\b" % (name, value), header, flags=re.M), name
    # among the extras, behind the hit layers, the structs declared with the entry points
    order = ["EXTRAS", "int lg_hit_layers_device(", "/* Ray paths:", "typedef struct lg_path_rule {", "typedef struct lg_paths_out {", "int lg_trace_paths(",
             "int lg_trace_paths_device("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), order
    rule = re.search(r"typedef struct lg_path_rule \{(.*?)\} lg_path_rule;\s*/\* 24 bytes \*/", header, flags=re.S)
    assert rule and re.findall(r"^\s*(uint32_t|double)\s+(\w+);", rule.group(1), flags=re.M) == [("uint32_t", "action"), ("uint32_t", "reserved"), ("double", "ior"), ("double", "gain")]
    struct = re.search(r"typedef struct lg_paths_out \{(.*?)\} lg_paths_out;", header, flags=re.S)
    assert struct and re.findall(r"^\s*(lg_hit|double|uint32_t)\s*\*(\w+);", struct.group(1), flags=re.M) == MEMBERS
    assert "72 bytes; each pointer may be NULL, all NULL is an error" in header
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header[header.index("/* Ray paths:"):header.index("#define LG_PATH_ABSORB")]))
    assert "The contract is a loop over lg_intersect" in text and "NOT the path the render follows" in text
    assert "Segment 0 of ray i is that ray, bit for bit" in text
    assert "what lg_intersect returns for segment j, bit for bit, exact ties included" in text and "no switch of its own" in text
    assert "A miss ends the path with LG_PATH_END_ESCAPED" in text
    assert "rules has exactly lg_accel_material_count entries" in text and "HOST array in both forms" in text and "may be freed on return" in text
    assert "A material outside 0 .. n_rules-1 is treated as LG_PATH_ABSORB" in text
    assert "gain = gain * r.gain (from 1.0, sequential in f64; a NaN stays" in text
    assert "nothing fused" in text and "dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z" in text
    assert "N = normal ? ns : ng" in text and "s = dot(d, N). If s > 0.0: N = -N and s = -s, per component" in text
    assert "LG_PATH_REFLECT: k = 2.0*s; d'[c] = d[c] - k*N[c]; o'[c] = p[c] + ng[c]*0x1p-36" in text
    assert "LG_PATH_PASS: d' is d's bits; o'[c] = p[c] - ng[c]*0x1p-36; medium ^= 1" in text
    assert "L = sqrt(dot(d,d)), q = 1.0/L, u[c] = d[c]*q, ci = -dot(u,N). eta = medium ? r.ior : 1.0/r.ior" in text
    assert "sin2 = (eta*eta) * fmax(1.0 - ci*ci, 0.0), fmax the NaN-ignoring one" in text
    assert "If sin2 >= 1.0 (total internal reflection): REFLECT's two lines on d, no toggle" in text
    assert "ct = sqrt(1.0 - sin2), a = eta*ci - ct, w[c] = eta*u[c] + a*N[c], d'[c] = w[c]*L, o'[c] = p[c] - ng[c]*0x1p-36, medium ^= 1" in text
    assert "crossing parity in medium, not a normal's sign" in text and "never leaves a glass sphere" in text and "only bit 0 is read" in text
    assert "The offset is always along ng, the geometric normal, which faces -d" in text
    assert "is not finite, the path ends with LG_PATH_END_DEGENERATE" in text and "if j + 1 == max_bounces, it ends with LG_PATH_END_CUT" in text
    assert "VERTEX-MAJOR" in text and "element (j, i) is at j*n + i" in text
    assert "t = +INF, zeros, kind 0, prim and instance ~0, material -1" in text and "id holds 0, ~0, ~0, -1" in text and "point holds +0s" in text and "along holds +INF" in text
    assert "for CUT the next ray (o', d'); for ESCAPED the segment that missed; for ABSORBED and DEGENERATE the segment that found the last vertex" in text
    assert "gives rows a .. a+b-1 of one call of a+b, bit for bit, in hits, point and id" in text and "along and gain RESTART" in text, "resuming"
    assert "written" in text and "by exactly one lane: no atomics, no pre-fill" in text
    assert "lg_accel_set_query_order(1) is honoured exactly as lg_hit_layers honours it" in text and "the same bytes as order 0" in text
    assert "n == 0 is a successful no-op that writes nothing, answered BEFORE every other check" in text
    assert "max_bounces == 0" in text and "n > (2^32 - 1) * 64" in text and "n * max_bounces or a plane's byte size that does not fit size_t" in text
    assert "all nine planes NULL" in text and "n_rules != lg_accel_material_count" in text and "an action above LG_PATH_REFRACT" in text
    assert "reserved != 0" in text and "normal outside {0, 1}" in text
    assert "rays 8 bytes; hits and id 16; point, along, gain and last 8; count, end, medium and start_medium 4" in text
    assert "it only enqueues on hip_stream" in text and "leaves the caller's arrays as they were" in text
    for scope in ("branching", "re-packing of lanes or re-sorting of rays between bounces", "a maximum range", "nested or overlapping media beyond the one parity bit",
                  "multi-device"):
        assert scope in text[text.index("Out of scope:"):], scope


def test_the_structs_are_24_and_72_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    R, C = _capi.CPathRule, _capi.CPathsOut
    assert ctypes.sizeof(R) == 24 and [(f[0], getattr(R, f[0]).offset) for f in R._fields_] == [("action", 0), ("reserved", 4), ("ior", 8), ("gain", 16)]
    assert la.PATH_RULE_DTYPE.itemsize == 24 and [(n, la.PATH_RULE_DTYPE.fields[n][1]) for n in la.PATH_RULE_DTYPE.names] == [("action", 0), ("reserved", 4), ("ior", 8), ("gain", 16)]
    assert ctypes.sizeof(C) == 72 and [f[0] for f in C._fields_] == list(la.PATH_PLANES)
    assert la.PATH_PLANES == PLANES
    assert [getattr(C, p).offset for p in la.PATH_PLANES] == [8 * k for k in range(9)]
    assert (la.PATH_ABSORB, la.PATH_REFLECT, la.PATH_PASS, la.PATH_REFRACT) == (0, 1, 2, 3)
    assert (la.PATH_END_CUT, la.PATH_END_ESCAPED, la.PATH_END_ABSORBED, la.PATH_END_DEGENERATE) == (0, 1, 2, 3)
    host = read("lasgun_amd", "csrc", "paths_host.h")  # static_asserts of the library's own build
    assert "sizeof(lg_paths_out) == 72" in host and all("offsetof(lg_paths_out, %s) == %d" % (p, 8 * k) in host for k, p in enumerate(la.PATH_PLANES))
    assert "sizeof(lg_path_rule) == 24" in host and "offsetof(lg_path_rule, ior) == 8" in host and "offsetof(lg_path_rule, gain) == 16" in host
    assert "static_assert(sizeof(PathRule) == 24" in read("lasgun_amd", "csrc", "k_paths.hip")
    assert "static_assert(sizeof(lg_paths_out) == 72 && sizeof(lg_path_rule) == 24" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_paths_out \{(.*?)\n\}", sys_src, flags=re.S)
    rust = {"lg_hit": "lg_hit", "double": "f64", "uint32_t": "u32"}
    assert struct and re.findall(r"pub (\w+): \*mut (\w+),", struct.group(1)) == [(n, rust[t]) for t, n in MEMBERS]
    rule = re.search(r"pub struct lg_path_rule \{(.*?)\n\}", sys_src, flags=re.S)
    assert rule and re.findall(r"pub (\w+): (\w+),", rule.group(1)) == [("action", "u32"), ("reserved", "u32"), ("ior", "f64"), ("gain", "f64")]
    for name, value in CONSTANTS.items():
        assert "pub const %s: u32 = %d;" % (name, value) in sys_src, name
    assert "std::mem::size_of::<sys::lg_paths_out>() == 72 && std::mem::size_of::<sys::lg_path_rule>() == 24" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_python_wrappers_mirror_them():
    import gen_rust_sys
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.PATHS_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    decl = {name: params for _, name, params in gen_rust_sys.declarations(read("include", "lasgun_hip.h"))}
    ctype = {"usize": ctypes.c_size_t, "u32": ctypes.c_uint32, "c_int": ctypes.c_int}
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
        want = [ctype.get(gen_rust_sys.rust_type(p), ctypes.c_void_p) for p in decl["lg_" + key]]  # (every pointer travels as c_void_p)
        assert list(argtypes) == want, (key, argtypes, want)
    for wrapper in ("trace_paths", "trace_paths_device", "path_rules"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.trace_paths) and callable(la.path_rules), "accel.trace_paths(rays, max_bounces, rules=...), la.path_rules(accel)"


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_trace_paths\(", src) and re.search(r"\blg_trace_paths_device\(", src)
    assert re.search(r"void trace_paths\(", src) and re.search(r"void trace_paths_device\(", src) and "struct Paths {" in src


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn trace_paths\(", safe) and re.search(r"pub unsafe fn trace_paths_device\(", safe)
    assert "out: *const lg_paths_out" in sys_src and "max_bounces: u32" in sys_src and "rules: *const lg_path_rule" in sys_src


def test_the_kernel_is_a_device_kernel_of_its_own_over_the_unchanged_walk():
    """The segments are formed and walked in a HIP kernel the library launches: one launch, the render's walk in its closest-hit form, the
    bounce from bounce.h on a second shade_frame behind the barrier; nothing loops over lg_intersect on the host."""
    src = read("lasgun_amd", "csrc", "k_paths.hip")
    assert re.search(r"__global__ void [^\n]*\bpaths_kernel\(", src) and "template <bool FAST, bool LDSS, bool PRUNE, bool PERM>" in src
    assert len(re.findall(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", src)) == 1, "closest hit"
    tilewalk_text.over_tilewalk(src)  # the prologue, the cursor, the record, the id word and the barrier helper: the shared header's
    assert "const uint4 id = hit_id(b, sh, Q.tri_base);" in src and "wave_any(alive)" in src
    assert "if (Q.hits) store_hit(Q.hits + 6ull * e, b, sh, id);" in src and "if (Q.hits) store_hit_none(Q.hits + 6ull * e);" in src
    assert '#include "bounce.h"' in src and src.count("shade_frame(P, ray, b, sh)") == 2 and "const Ray ray = ray_opaque(r);" in src
    assert "bounce_next(action, ior, v.d, v.p, v.ng, Q.use_ns ? v.ns : v.ng, medium)" in src, "the next ray from the second evaluation"
    assert "gain = gain != gain ? gain : gain * rgain" in src and "T != T ? T : T + b.t" in src, "a NaN stays: selected, not left to the operation"
    assert "atomic" not in src.split("#include")[1], "no atomics: every element is written by exactly one lane"
    assert "trav_launch<PathsKernels>" in src and "trav_occupancy<PathsKernels>" in src and "trav_set_lds_limit<PathsKernels>" in src
    bounce = read("lasgun_amd", "csrc", "bounce.h")
    assert '#include "vecmath.h"' in bounce and "LG_HD Bounce bounce_next(" in bounce and "hip" not in bounce.split("#pragma once")[1].lower()
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_paths.o" in make and "-ffp-contract=off" in make and "paths_host.h" in make and "k_paths.o: bounce.h" in make
    assert "trace_paths_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    host = read("lasgun_amd", "csrc", "query.cpp")
    body = host[host.index("static void enqueue_trace_paths("):host.index('extern "C" int lg_trace_paths(')]
    assert body.index("stage_rule_table(") < body.index("query_order_of(") < body.index("traversal_grid(") < body.index("launch_trace_paths(") and "trace_paths_occupancy" in body
    assert body.count("launch_trace_paths(") == 1 and "for (" not in body and "while (" not in body, "one launch, no chunks"
    assert "subsets_enqueued(a, stream)" in body and "subsets_abandoned(a, stream)" in body, "the staged table is released behind the launch"
    whole = host[host.index("// ---- ray paths"):host.index("// ---- lens rays")]
    assert "launch_query(" not in whole and "enqueue_query(" not in whole and "guarded(" in whole, "no loop of lg_intersect on the host"


class FiveMaterials:
    """What path_rules asks an api for, over a table of all five material kinds (and a second glass): no accel, no device."""

    def __init__(self, api):
        M = api.Material
        self.table = [M.matte([0.5, 0.5, 0.5], 0.0), M.plastic([0.1, 0.2, 0.3], [0.4, 0.4, 0.4], 0.2), M.metal([0.2, 0.9, 1.1], [3.9, 2.4, 2.2], 0.1, 0.1),
                      M.glass([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], 1.5), M.mirror([0.9, 0.9, 0.9]), M.glass([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 1.33)]

    def material_count(self, accel):
        return len(self.table)

    def accel_material(self, accel, i):
        c = self.table[i].c
        return {"kind": int(c.kind), "p": tuple(c.p)}


def test_path_rules_on_all_five_materials():
    import lasgun_amd as la
    stub = FiveMaterials(la.api)
    assert [stub.accel_material(None, i)["kind"] for i in range(6)] == [0, 1, 2, 3, 4, 3]
    r = la.HipApi.path_rules(stub, None)
    assert r.dtype == la.PATH_RULE_DTYPE and r.shape == (6,)
    assert r["action"].tolist() == [la.PATH_ABSORB, la.PATH_ABSORB, la.PATH_REFLECT, la.PATH_REFRACT, la.PATH_REFLECT, la.PATH_REFRACT]
    assert r["ior"].tolist() == [1.0, 1.0, 1.0, 1.5, 1.0, 1.33] and r["gain"].tolist() == [1.0] * 6 and not r["reserved"].any()
    r = la.HipApi.path_rules(stub, None, default=la.PATH_REFLECT, gain=0.5)
    assert r["action"].tolist() == [la.PATH_REFLECT, la.PATH_REFLECT, la.PATH_REFLECT, la.PATH_REFRACT, la.PATH_REFLECT, la.PATH_REFRACT]
    assert r["gain"].tolist() == [0.5] * 6
    assert la.HipApi._path_rules(r) is r
    for bad in (np.zeros(3), np.zeros((2, 2), dtype=la.PATH_RULE_DTYPE)):
        try:
            la.HipApi._path_rules(bad)
        except ValueError:
            continue
        raise AssertionError("a table that is not 1-D PATH_RULE_DTYPE is refused")


def outputs(n, k):
    """The nine planes of lg_paths_out over a 0xA5 prefill (as uint32 words, whatever the plane's type) and the struct that names them."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    arrs = [np.full(size, 0xA5A5A5A5, dtype=np.uint32) for size in (n * k * 24, n * k * 6, n * k * 4, n * k * 2, n, n, n * 2, n * 12, n)]
    return arrs, _capi.CPathsOut(*[a.ctypes.data for a in arrs]), la


def test_the_no_device_errors_are_refused_and_touch_nothing():
    """A NULL accel with n > 0 is answered before anything else is looked at, whatever the other arguments."""
    n, k = 5, 3
    arrs, out, la = outputs(n, k)
    G = la.api
    rays = np.zeros((n, 6))
    rays[:, 5] = 1.0
    rules = np.zeros(2, dtype=la.PATH_RULE_DTYPE)
    A = ctypes.addressof
    for fn, tail in (("trace_paths", ()), ("trace_paths_device", (None,))):
        assert G.call(fn, None, rays.ctypes.data, n, k, rules.ctypes.data, 2, 0, None, A(out), *tail) != 0 and "accel is NULL" in G.last_error(), fn
        assert G.call(fn, None, rays.ctypes.data, n, 0, None, 0, 7, None, None, *tail) != 0 and G.last_error(), fn
        assert all((a == 0xA5A5A5A5).all() for a in arrs), fn
    check = read("tools", "paths_host_check.cpp")  # (the stand-alone check exercises every other refusal through check_paths)
    assert "refused(&accel, D, 1, 0, &all)" in check and "refused(&accel, D, 3, 5, &none)" in check and "refused(nullptr, D, 3, 5, &all)" in check
    assert "refused(&accel, D, 3, 5, &all, RULES, 2, 3)" in check and "refused(&accel, D, 3, 5, &all, RULES, 3, 3, normal)" in check


def test_an_empty_set_is_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    for k in (0, 1, 8, 2 ** 32 - 1):  # (the empty set is answered before every other check, max_bounces included)
        assert G.call("trace_paths", None, None, 0, k, None, 0, 0, None, None) == 0, k
        assert G.call("trace_paths_device", None, None, 0, k, None, 5, 9, None, None, None) == 0, k
