"""Range scans (include/lasgun_hip.h: lg_range_scan, lg_range_scan_device, lg_range_scan_lanes) through every layer that has to carry them,
checked without a GPU: the built library exports the symbols, the header declares them with the arity, the parameter names and the types
the wrappers use, directly after lg_open_directions_device, and states the contract -- the frame expression with its operation order,
"written, not accumulated", the nearest rule with its pre-fill, both tile limits, the auto rule --, lg_scan_out is 48 bytes in every
mirror, the kernel is a HIP kernel of its own in the build, and the Python, C++ and Rust bindings mirror the entry points.  On top: the
lane rule over a table of shapes, the errors that are answered before any HIP call (a NULL accel), the no-op of empty sets, and the
wrapper's spinning-lidar beams."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_range_scan": 8, "lg_range_scan_device": 9, "lg_range_scan_lanes": 3}
NAMES = tuple(ARITY)
TOP = 2 ** 64 - 1


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
    for name in NAMES[:2]:
        assert "lg_accel" in decl[name][1][0] and "const" in decl[name][1][0]
    names = lambda key: [p.split()[-1].lstrip("*") for p in decl[key][1]]  # noqa: E731
    assert names("lg_range_scan")[1:] == ["origins", "frames", "n_poses", "beams", "n_beams", "lanes", "out"]
    assert names("lg_range_scan_device")[1:] == ["dev_origins", "dev_frames", "n_poses", "dev_beams", "n_beams", "lanes", "dev_out", "hip_stream"]
    assert names("lg_range_scan_lanes") == ["n_poses", "n_beams", "lanes"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "const double *", "size_t", "const double *", "size_t", "int", "const lg_scan_out *"]
    assert types("lg_range_scan")[1:] == host
    assert types("lg_range_scan_device")[1:] == host + ["void *"]
    assert types("lg_range_scan_lanes") == ["size_t", "size_t", "int"]
    # directly after lg_open_directions_device, among the extras: nothing but the struct is declared between the two
    assert header.index("EXTRAS") < header.index("lg_open_directions_device(") < header.index("int lg_range_scan(") < header.index("int lg_range_scan_device(")
    assert header.index("int lg_range_scan_device(") < header.index("int lg_range_scan_lanes(") < header.index("int lg_radiance(")
    between = gen_rust_sys.strip_comments(header[header.index("lg_open_directions_device("):header.index("int lg_range_scan(")])
    struct = re.search(r"typedef struct lg_scan_out \{(.*?)\} lg_scan_out;", between, flags=re.S)
    assert struct, "lg_scan_out is declared with the entry points"
    members = re.findall(r"(float|uint32_t)\s*\*(\w+);", struct.group(1))
    assert members == [("float", "range"), ("float", "point"), ("float", "normal"), ("uint32_t", "id"), ("uint32_t", "hits"), ("float", "nearest")], members
    assert between.replace(struct.group(0), "").count(";") == 1, "nothing else is declared between the two"
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("Range scans"):header.index("typedef struct lg_scan_out")])
    assert "d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z" in text and "in this order" in text and "no contraction" in text, "the frame expression and its order"
    assert re.search(r"frames[^.]*MAY BE NULL", text) and "no arithmetic makes the ray" in text
    assert re.search(r"identity frame is therefore NOT the same as NULL", text) and "-0.0" in text
    assert "not normalised" in text
    assert "what lg_intersect returns for that ray, bit for bit" in text and "no switch of its own" in text
    assert "lg_accel_set_query_order plays no part" in text
    assert "element (i, k) is at i*n_beams + k" in text and "range = (float)t, +INF on a miss" in text
    assert "geometric normal faced toward the sensor" in text and "not ns" in text
    assert "0, ~0, ~0, -1 on a miss" in text and "rounds to nearest even" in text
    assert re.search(r"written,? not accumulated", text, flags=re.I), "the reductions are written, not accumulated"
    assert "bit pattern, read as uint32, is smallest among the pose's hits" in text and "0x7F800000" in text and "atomicMin" in text, "the nearest rule"
    assert "NaN, negative or has overflowed to +INF never wins" in text
    assert "n_poses * ceil(n_beams / 64) > 2^32 - 1" in text and "ceil(n_poses / 64) * ceil(n_beams / 8) > 2^32 - 1" in text, "both tile limits"
    assert "n_beams > 2^32 - 1" in text
    assert "pose lanes iff n_poses >= n_beams" in text and "not a measured optimum" in text, "the auto rule"
    assert "Every output is the same bytes in either form" in text
    assert "successful no-op that writes nothing" in text and "all six outputs NULL" in text
    assert "answered BEFORE every other check" in text, "an empty set comes first: a bad lanes or a NULL out is not looked at"
    assert "no maximum range" in text and "no noise or intensity model" in text and "no multi-device split" in text, "what is out of scope"
    assert "48 bytes; each pointer may be NULL, all NULL is an error" in header


def test_lg_scan_out_is_48_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    assert ctypes.sizeof(_capi.CScanOut) == 48 and [f[0] for f in _capi.CScanOut._fields_] == list(la.SCAN_PLANES)
    assert la.SCAN_PLANES == ("range", "point", "normal", "id", "hits", "nearest")
    assert "sizeof(lg_scan_out) == 48" in read("lasgun_amd", "csrc", "scan_host.h")  # a static_assert of the library's own build
    assert "static_assert(sizeof(lg_scan_out) == 48" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_scan_out \{(.*?)\n\}", sys_src, flags=re.S)
    assert struct and re.findall(r"pub (\w+): \*mut (\w+),", struct.group(1)) == [("range", "f32"), ("point", "f32"), ("normal", "f32"), ("id", "u32"), ("hits", "u32"),
                                                                                ("nearest", "f32")]
    assert "std::mem::size_of::<sys::lg_scan_out>() == 48" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.RANGE_SCAN_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    assert [i for i, a in enumerate(sigs["range_scan"][1]) if a is ctypes.c_size_t] == [3, 5] and sigs["range_scan"][1][6] is ctypes.c_int
    assert [i for i, a in enumerate(sigs["range_scan_device"][1]) if a is ctypes.c_size_t] == [3, 5] and sigs["range_scan_device"][1][6] is ctypes.c_int
    assert sigs["range_scan_lanes"][1] == [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    for wrapper in ("range_scan", "range_scan_device", "range_scan_lanes"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.range_scan), "accel.range_scan(origins, beams, frames=None, planes=(\"range\",), lanes=0)"
    assert callable(la.spinning_lidar_beams)


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_range_scan\(", src) and re.search(r"\blg_range_scan_device\(", src)
    assert re.search(r"void range_scan\(", src) and re.search(r"void range_scan_device\(", src)


def test_the_rust_crates_carry_them():
    import gen_rust_sys  # noqa: F401
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn range_scan\(", safe) and re.search(r"pub unsafe fn range_scan_device\(", safe) and re.search(r"pub fn range_scan_lanes\(", safe)
    assert "out: *const lg_scan_out" in sys_src and "lanes: c_int" in sys_src


def test_the_kernel_is_a_device_kernel_of_its_own():
    """The rays are made and walked in a HIP kernel the library launches, through the render's walk in its closest-hit form, and the two
    reduction buffers are pre-filled on the caller's stream ahead of it; nothing expands the pairs into rays on the host."""
    src = read("lasgun_amd", "csrc", "k_scan.hip")
    assert re.search(r"__global__ void [^\n]*\bscan_kernel\(", src)
    assert len(re.findall(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", src)) == 2, "both lane forms, closest hit"
    assert "claim_tile(" in src and "claim_tile_single(" in src and "atomicAdd(" in src and "atomicMin(" in src and "shade_frame(" in src and "tri_base" in src
    assert "(M[0] * b.x + M[1] * b.y) + M[2] * b.z" in src and "(M[6] * b.x + M[7] * b.y) + M[8] * b.z" in src
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_scan.o" in make and "-ffp-contract=off" in make and "scan_host.h" in make
    assert "range_scan_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    host = read("lasgun_amd", "csrc", "query.cpp")
    body = host[host.index("static void enqueue_range_scan("):host.index('extern "C" int lg_range_scan(')]
    assert body.index("hipMemsetAsync(out.hits, 0,") < body.index("launch_range_scan(")
    assert body.index("hipMemsetD32Async((hipDeviceptr_t)out.nearest, 0x7F800000,") < body.index("launch_range_scan(")
    assert "range_scan_occupancy" in body and "traversal_grid(" in body
    whole = host[host.index("// ---- range scans"):host.index("// ---- radiance queries")]
    assert "lg_intersect" not in whole and "launch_query(" not in whole and "enqueue_query(" not in whole, "no rays are built on the host"
    assert "n_poses * 6" not in whole and "n_beams * 6" not in whole and "pairs * 6" not in whole


def test_the_lane_rule_over_a_table_of_shapes():
    import lasgun_amd as la
    G = la.api
    M = 2 ** 32 - 1
    for n, k, auto in ((0, 0, 2), (0, 1, 1), (1, 0, 2), (1, 1, 2), (1, 64, 1), (64, 1, 2), (63, 64, 1), (64, 64, 2), (65, 64, 2), (1024, 65536, 1), (1 << 20, 64, 2),
                       (M, M, 2), (M, M + 1, 1), (M + 1, M, 2), (TOP, TOP, 2), (TOP - 1, TOP, 1), (TOP, TOP - 1, 2), (0, TOP, 1), (TOP, 0, 2)):
        assert G.call("range_scan_lanes", n, k, 0) == auto, (n, k)
        assert G.range_scan_lanes(n, k) == auto and G.range_scan_lanes(n, k, "auto") == auto
        assert G.call("range_scan_lanes", n, k, 1) == 1 and G.call("range_scan_lanes", n, k, 2) == 2, (n, k)
        assert G.range_scan_lanes(n, k, "beam") == 1 and G.range_scan_lanes(n, k, "pose") == 2
        for bad in (-1, 3, 64, -2 ** 31, 2 ** 31 - 1):
            assert G.call("range_scan_lanes", n, k, bad) == -1, (n, k, bad)


def outputs(n, k):
    """The six outputs of lg_scan_out over a 0xA5 prefill (as uint32 words, whatever the plane's type) and the struct that names them."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    arrs = [np.full(size, 0xA5A5A5A5, dtype=np.uint32) for size in (n * k, n * k * 3, n * k * 3, n * k * 4, n, n)]
    return arrs, _capi.CScanOut(*[a.ctypes.data for a in arrs]), la


def test_a_null_accel_is_refused_and_touches_nothing():
    n, k = 5, 11
    arrs, out, la = outputs(n, k)
    G = la.api
    pts, frames, beams = np.zeros((n, 3)), np.zeros((n, 9)), np.ones((k, 3))
    for fn, tail in (("range_scan", ()), ("range_scan_device", (None,))):
        for lanes in (0, 1, 2):
            rc = G.call(fn, None, pts.ctypes.data, frames.ctypes.data, n, beams.ctypes.data, k, lanes, ctypes.addressof(out), *tail)
            assert rc != 0 and G.last_error(), fn
            assert all((a == 0xA5A5A5A5).all() for a in arrs), fn


def test_zero_counts_are_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    for n, k in ((0, 0), (0, 7), (7, 0)):
        for lanes in (0, 1, 2, 7, -1):  # (the empty set is answered before every other check, the lanes included)
            assert G.call("range_scan", None, None, None, n, None, k, lanes, None) == 0, (n, k, lanes)
            assert G.call("range_scan_device", None, None, None, n, None, k, lanes, None, None) == 0, (n, k, lanes)


def test_spinning_lidar_beams_are_ring_major_unit_vectors():
    import lasgun_amd as la
    for rings, az, lo, hi in ((1, 1, 0.0, 0.0), (1, 360, -3.0, 5.0), (4, 64, -15.0, 15.0), (64, 1024, -25.0, 15.0), (16, 100, 0.0, 89.0), (3, 7, -90.0, 90.0)):
        b = la.spinning_lidar_beams(rings, az, lo, hi)
        assert b.shape == (rings * az, 3) and b.dtype == np.float64 and b.flags["C_CONTIGUOUS"]
        assert np.all(np.abs(np.linalg.norm(b, axis=1) - 1.0) <= 1e-15), (rings, az)
        g = b.reshape(rings, az, 3)
        elev = np.rad2deg(np.arcsin(np.clip(g[..., 2], -1.0, 1.0)))
        want = np.linspace(lo, hi, rings) if rings > 1 else np.array([0.5 * (lo + hi)])
        assert np.abs(elev - want[:, None]).max() < 1e-9, "ring-major: beam r * azimuths + a has ring r's elevation"
        if abs(lo) < 90.0 and abs(hi) < 90.0:
            phi = np.arctan2(g[..., 1], g[..., 0]) % (2.0 * np.pi)
            step = np.arange(az) * (2.0 * np.pi / az)
            d = np.abs(phi - step[None, :])
            assert np.minimum(d, 2.0 * np.pi - d).max() < 1e-9, "within a ring the azimuth steps through a full turn"
    b = la.spinning_lidar_beams(64, 1024, -25.0, 15.0).reshape(64, 1024, 3)
    # 64 consecutive beams are neighbours: a stretch of one ring, each a step of 2 pi / 1024 from the last
    assert np.arccos(np.clip((b[:, :-1] * b[:, 1:]).sum(axis=-1), -1.0, 1.0)).max() <= 2.0 * np.pi / 1024 + 1e-12
