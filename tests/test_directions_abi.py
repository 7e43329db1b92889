"""Direction sets (include/lasgun_hip.h: lg_open_directions, lg_open_directions_device) through every layer that has to carry them, checked
without a GPU: the built library exports the symbols, the header declares them with the arity and the parameter names the wrappers use and
states the bit order, the "written, not accumulated" rule, the horizon test with its operation order, "not walked", the NULL normals and
the tile limit, the kernel is a HIP kernel of its own in the build, and the Python, C++ and Rust bindings mirror the entry points.  On
top: the errors that are answered before any HIP call (a NULL accel), the no-op of empty sets, and the wrapper's Fibonacci directions."""
import ctypes
import os
import re
import sys

import numpy as np
import tilewalk_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_open_directions": 10, "lg_open_directions_device": 11}
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
    assert names("lg_open_directions")[1:] == ["points", "normals", "n_points", "dirs", "n_dirs", "bits", "row_bytes", "open", "above"]
    assert names("lg_open_directions_device")[1:] == ["dev_points", "dev_normals", "n_points", "dev_dirs", "n_dirs", "dev_bits", "row_bytes", "dev_open",
                                                      "dev_above", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "const double *", "size_t", "const double *", "size_t", "uint8_t *", "size_t", "uint32_t *", "uint32_t *"]
    assert types("lg_open_directions")[1:] == host
    assert types("lg_open_directions_device")[1:] == host + ["void *"]
    # directly after lg_visibility_device, among the extras
    assert header.index("EXTRAS") < header.index("lg_visibility_device(") < header.index("lg_open_directions(") < header.index("lg_radiance(")
    between = gen_rust_sys.strip_comments(header[header.index("lg_visibility_device("):header.index("int lg_open_directions(")])
    assert between.count(";") == 1, "nothing is declared between the two"
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("Direction sets"):header.index("int lg_open_directions(")])
    assert "(bits[i*row_bytes + (k >> 3)] >> (k & 7)) & 1" in text, "the bit order"
    assert 'packbits(..., bitorder="little")' in text
    assert re.search(r"written,? not accumulated", text, flags=re.I), "the counts are written, not accumulated"
    assert "s = (n.x*d.x + n.y*d.y) + n.z*d.z" in text and "s > 0.0" in text and "no contraction" in text, "the horizon test and its order"
    assert re.search(r"not walked", text, flags=re.I)
    assert re.search(r"normals[^.]*may be NULL", text, flags=re.I)
    assert "ceil(n_points / 64) * ceil(n_dirs / 8) > 2^32 - 1" in text and "n_dirs > 2^32 - 1" in text, "the tile limit"
    assert "padding bits" in text and "never touched" in text
    assert "lg_accel_set_query_order plays no part" in text
    assert "all three NULL is an error" in text


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.DIRECTIONS_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
        assert [i for i, a in enumerate(argtypes) if a is ctypes.c_size_t] == [3, 5, 7], key
    for wrapper in ("open_directions", "open_directions_device", "ambient_occlusion"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.open_directions), "accel.open_directions(points, dirs, normals=None, counts=False)"
    assert callable(la.sphere_directions)


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_open_directions\(", src)
    assert re.search(r"std::vector<uint8_t> open_directions\(", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn open_directions\(", safe)
    assert re.search(r"pub unsafe fn open_directions_device\(", safe)


def test_the_kernel_is_a_device_kernel_of_its_own():
    """The rays are made and walked in a HIP kernel the library launches, through the render's walk in its any-hit form, and the count
    buffers are zeroed on the caller's stream ahead of it; nothing expands the pairs into rays on the host."""
    src = read("lasgun_amd", "csrc", "k_directions.hip")
    assert re.search(r"__global__ void [^\n]*\bdirections_kernel\(", src)
    assert re.search(r"walk<LDSS, FAST, PRUNE>\(P, ray, true,", src)
    tilewalk_text.over_tilewalk(src)
    assert "atomicAdd(" in src
    assert "k_directions.o" in read("lasgun_amd", "csrc", "Makefile")
    host = read("lasgun_amd", "csrc", "query.cpp")
    body = host[host.index("static void enqueue_open_directions("):host.index('extern "C" int lg_open_directions(')]
    assert body.index("hipMemsetAsync(open, 0,") < body.index("launch_open_directions(")
    assert body.index("hipMemsetAsync(above, 0,") < body.index("launch_open_directions(")
    assert "open_directions_occupancy" in body
    whole = host[host.index("static void check_open_directions("):host.index("// ---- radiance queries")]
    assert "lg_occluded" not in whole and "launch_query(" not in whole and "enqueue_query(" not in whole, "no rays are built on the host"
    assert "n_points * 6" not in whole and "n_dirs * 6" not in whole


def test_a_null_accel_is_refused_and_touches_nothing():
    import lasgun_amd as la
    G = la.api
    n, k = 5, 11
    pts, dirs = np.zeros((n, 3)), np.ones((k, 3))
    for fn, tail in (("open_directions", ()), ("open_directions_device", (None,))):
        bits = np.full((n, 2), 0xA5, dtype=np.uint8)
        nopen, above = np.full(n, 0x5A5A5A5A, dtype=np.uint32), np.full(n, 0x5A5A5A5A, dtype=np.uint32)
        rc = G.call(fn, None, pts.ctypes.data, pts.ctypes.data, n, dirs.ctypes.data, k, bits.ctypes.data, 2, nopen.ctypes.data, above.ctypes.data, *tail)
        assert rc != 0 and G.last_error(), fn
        assert (bits == 0xA5).all() and (nopen == 0x5A5A5A5A).all() and (above == 0x5A5A5A5A).all(), fn


def test_zero_counts_are_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    for n, k in ((0, 0), (0, 7), (7, 0)):
        assert G.call("open_directions", None, None, None, n, None, k, None, 0, None, None) == 0, (n, k)
        assert G.call("open_directions_device", None, None, None, n, None, k, None, 0, None, None, None) == 0, (n, k)


def test_sphere_directions_have_the_length_asked_for():
    import lasgun_amd as la
    for k, length in ((1, 1.0), (7, 1.0), (64, 0.37), (257, 1234.5), (1031, 3e-9)):
        d = la.sphere_directions(k, length)
        assert d.shape == (k, 3) and d.dtype == np.float64 and d.flags["C_CONTIGUOUS"]
        assert np.all(np.abs(np.linalg.norm(d, axis=1) - length) <= 1e-15 * length), (k, length)
        if k > 1:
            assert np.abs(d.mean(axis=0)).max() < 0.05 * length and len(np.unique(d, axis=0)) == k, "spread over the whole sphere"
    assert la.sphere_directions(64).shape == (64, 3) and abs(np.linalg.norm(la.sphere_directions(64)[5]) - 1.0) <= 1e-15
