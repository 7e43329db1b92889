"""Hit layers (include/lasgun_hip.h: lg_hit_layers, lg_hit_layers_device) through every layer that has to carry them, checked without a GPU:
the built library exports the symbols, the header declares them with the arity, the parameter names and the types the wrappers use and
states the contract -- the segment rule with its constant and operation count, layer-major planes, what stands behind a ray's last layer,
along without the steps, inside over the odd layers, the query order, the limits --, lg_layers_out is 40 bytes with the stated offsets in
every mirror, the kernel is a HIP kernel of its own in the build over the unchanged walk, and the Python, C++ and Rust bindings mirror the
entry points.  On top: the errors that are answered before any HIP call, and the no-op of an empty set."""
import ctypes
import os
import re
import sys

import numpy as np
import tilewalk_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_hit_layers": 5, "lg_hit_layers_device": 6}
NAMES = tuple(ARITY)
MEMBERS = [("lg_hit", "hits"), ("double", "along"), ("uint32_t", "id"), ("uint32_t", "count"), ("double", "inside")]


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
    assert names("lg_hit_layers")[1:] == ["rays", "n", "max_layers", "out"]
    assert names("lg_hit_layers_device")[1:] == ["dev_rays", "n", "max_layers", "dev_out", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "size_t", "uint32_t", "const lg_layers_out *"]
    assert types("lg_hit_layers")[1:] == host
    assert types("lg_hit_layers_device")[1:] == host + ["void *"]
    # among the extras, the struct declared with the entry points
    order = ["EXTRAS", "typedef struct lg_hit {", "/* Hit layers:", "typedef struct lg_layers_out {", "int lg_hit_layers(", "int lg_hit_layers_device("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), order
    struct = re.search(r"typedef struct lg_layers_out \{(.*?)\} lg_layers_out;", header, flags=re.S)
    assert struct and re.findall(r"^\s*(lg_hit|double|uint32_t)\s*\*(\w+);", struct.group(1), flags=re.M) == MEMBERS
    assert "40 bytes; each pointer may be NULL, all NULL is an error" in header
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header[header.index("/* Hit layers:"):header.index("typedef struct lg_layers_out")]))
    assert "Segment 0 of ray i is that ray, bit for bit" in text
    assert "what lg_intersect returns for segment j, bit for bit, exact ties included" in text and "no switch of its own" in text
    assert "o'[c] = p[c] - ng[c]*0x1p-36" in text and "one f64 product and one f64 subtraction per component, nothing fused" in text, "the segment rule"
    assert "keeps the direction of ray i bit for bit" in text and "If layer j is a miss, the ray is finished" in text
    assert "LAYER-MAJOR" in text and "element (j, i) is at j*n + i" in text
    assert "written" in text and "by exactly one lane: no atomics, no pre-fill" in text
    assert "T_0 = t_0 and T_j = T_(j-1) + t_j" in text and "the 2^-36 steps are NOT added" in text, "along"
    assert "A NaN stays: where T_(j-1) is NaN, T_j is T_(j-1) bit for bit, and so for inside" in text
    assert "t = +INF, zeros, kind 0, prim and instance ~0, material -1" in text and "id holds 0, ~0, ~0, -1" in text and "along holds +INF" in text
    assert "count[i] == max_layers means the ray may have been cut short" in text
    assert "from +0.0, of t_j over the odd j < count[i]" in text, "inside"
    assert "lg_accel_set_query_order(1) is honoured exactly as lg_intersect honours it" in text and "the same bytes as order 0" in text
    assert "n == 0 is a successful no-op that writes nothing, answered BEFORE every other check" in text
    assert "max_layers == 0" in text and "n > (2^32 - 1) * 64" in text and "n * max_layers or a plane's byte size that does not fit size_t" in text
    assert "all five planes NULL" in text and "rays 8 bytes; hits and id 16; along and inside 8; count 4" in text
    assert "it only enqueues on hip_stream" in text and "leaves the caller's arrays as they were" in text
    assert "no maximum range and no material filter" in text and "not re-packed" in text and "no multi-device split" in text, "what is out of scope"
    assert "may find the same surface again" in text and "max_layers bounds it" in text


def test_lg_layers_out_is_40_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    C = _capi.CLayersOut
    assert ctypes.sizeof(C) == 40 and [f[0] for f in C._fields_] == list(la.LAYER_PLANES)
    assert la.LAYER_PLANES == ("hits", "along", "id", "count", "inside")
    assert [getattr(C, p).offset for p in la.LAYER_PLANES] == [0, 8, 16, 24, 32]
    host = read("lasgun_amd", "csrc", "layers_host.h")  # a static_assert of the library's own build
    assert "sizeof(lg_layers_out) == 40" in host and all("offsetof(lg_layers_out, %s) == %d" % (p, 8 * k) in host for k, p in enumerate(la.LAYER_PLANES))
    assert "static_assert(sizeof(lg_layers_out) == 40" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_layers_out \{(.*?)\n\}", sys_src, flags=re.S)
    assert struct and re.findall(r"pub (\w+): \*mut (\w+),", struct.group(1)) == [("hits", "lg_hit"), ("along", "f64"), ("id", "u32"), ("count", "u32"), ("inside", "f64")]
    assert "std::mem::size_of::<sys::lg_layers_out>() == 40" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.HIT_LAYERS_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
        assert argtypes[2] is ctypes.c_size_t and argtypes[3] is ctypes.c_uint32, key
        assert all(a is ctypes.c_void_p for i, a in enumerate(argtypes) if i not in (2, 3)), key
    for wrapper in ("hit_layers", "hit_layers_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.hit_layers), "accel.hit_layers(rays, max_layers, planes=...)"


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_hit_layers\(", src) and re.search(r"\blg_hit_layers_device\(", src)
    assert re.search(r"void hit_layers\(", src) and re.search(r"void hit_layers_device\(", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn hit_layers\(", safe) and re.search(r"pub unsafe fn hit_layers_device\(", safe)
    assert "out: *const lg_layers_out" in sys_src and "max_layers: u32" in sys_src


def test_the_kernel_is_a_device_kernel_of_its_own_over_the_unchanged_walk():
    """The segments are made and walked in a HIP kernel the library launches: one launch, the render's walk in its closest-hit form, the
    next origin shade_frame's own pm; nothing loops over lg_intersect on the host."""
    src = read("lasgun_amd", "csrc", "k_layers.hip")
    assert re.search(r"__global__ void [^\n]*\blayers_kernel\(", src)
    assert len(re.findall(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", src)) == 1, "closest hit"
    tilewalk_text.over_tilewalk(src)  # the prologue, the cursor, the record, the id word and the barrier helper: the shared header's
    assert "shade_frame(" in src and "const uint4 id = hit_id(b, sh, Q.tri_base);" in src and "wave_any(alive)" in src
    assert "if (Q.hits) store_hit(Q.hits + 6ull * e, b, sh, id);" in src and "if (Q.hits) store_hit_none(Q.hits + 6ull * e);" in src
    assert "const Ray ray = ray_opaque(r);" in src, "pm comes from an evaluation of its own behind the barrier"
    assert "return sh.pm;" in src and "ray_new(layer_next_origin(P, ray, b), ray.d)" in src, "the next segment starts at shade_frame's pm, the direction kept"
    assert "atomic" not in src.split("#include")[1], "no atomics: every element is written by exactly one lane"
    assert "trav_launch<LayersKernels>" in src and "trav_occupancy<LayersKernels>" in src and "trav_set_lds_limit<LayersKernels>" in src
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_layers.o" in make and "-ffp-contract=off" in make and "layers_host.h" in make
    assert "hit_layers_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    host = read("lasgun_amd", "csrc", "query.cpp")
    body = host[host.index("static void enqueue_hit_layers("):host.index('extern "C" int lg_hit_layers(')]
    assert body.index("query_order_of(") < body.index("traversal_grid(") < body.index("launch_hit_layers(") and "hit_layers_occupancy" in body
    assert body.count("launch_hit_layers(") == 1 and "for (" not in body and "while (" not in body, "one launch, no chunks"
    whole = host[host.index("// ---- hit layers"):host.index("// ---- lens rays")]
    assert "launch_query(" not in whole and "enqueue_query(" not in whole, "no loop of lg_intersect on the host"


def outputs(n, k):
    """The five planes of lg_layers_out over a 0xA5 prefill (as uint32 words, whatever the plane's type) and the struct that names them."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    arrs = [np.full(size, 0xA5A5A5A5, dtype=np.uint32) for size in (n * k * 24, n * k * 2, n * k * 4, n, n * 2)]
    return arrs, _capi.CLayersOut(*[a.ctypes.data for a in arrs]), la


def test_the_no_device_errors_are_refused_and_touch_nothing():
    """A NULL accel with n > 0, max_layers == 0, all planes NULL and the limits are answered before anything looks behind the accel handle
    (the handle given here for all but the first is not an accel: a pointer to zeros that no check may follow)."""
    from lasgun_amd import _capi
    n, k = 5, 3
    arrs, out, la = outputs(n, k)
    G = la.api
    rays = np.zeros((n, 6))
    rays[:, 5] = 1.0
    A = ctypes.addressof
    none = _capi.CLayersOut()
    fake = ctypes.create_string_buffer(4096)  # (zeros; refused before anything reads it)
    for fn, tail in (("hit_layers", ()), ("hit_layers_device", (None,))):
        assert G.call(fn, None, rays.ctypes.data, n, k, A(out), *tail) != 0 and "accel is NULL" in G.last_error(), fn
        assert G.call(fn, None, rays.ctypes.data, n, 0, A(out), *tail) != 0 and G.last_error(), fn
        assert G.call(fn, A(fake), rays.ctypes.data, n, 0, A(out), *tail) != 0 and "max_layers is 0" in G.last_error(), fn
        assert G.call(fn, A(fake), rays.ctypes.data, n, k, A(none), *tail) != 0 and "every plane of out is NULL" in G.last_error(), fn
        assert G.call(fn, A(fake), rays.ctypes.data, n, k, None, *tail) != 0 and "out is NULL" in G.last_error(), fn
        assert G.call(fn, A(fake), None, n, k, A(out), *tail) != 0 and "rays is NULL" in G.last_error(), fn
        assert G.call(fn, A(fake), rays.ctypes.data, 2 ** 38, k, A(out), *tail) != 0 and "too many rays" in G.last_error(), fn
        assert G.call(fn, A(fake), rays.ctypes.data, 2 ** 37, 2 ** 31, A(out), *tail) != 0 and "does not fit the address space" in G.last_error(), fn
        assert all((a == 0xA5A5A5A5).all() for a in arrs), fn
    import gen_rust_sys  # noqa: F401  (tools/ is importable: the stand-alone check exercises the same refusals through check_layers)
    check = read("tools", "layers_host_check.cpp")
    assert "refused(&accel, D, 1, 0, &all)" in check and "refused(&accel, D, 3, 5, &none)" in check and "refused(nullptr, D, 3, 5, &all)" in check


def test_an_empty_set_is_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    for k in (0, 1, 8, 2 ** 32 - 1):  # (the empty set is answered before every other check, max_layers included)
        assert G.call("hit_layers", None, None, 0, k, None) == 0, k
        assert G.call("hit_layers_device", None, None, 0, k, None, None) == 0, k
