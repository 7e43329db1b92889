"""Radiance gathers (include/lasgun_hip.h: lg_radiance_gather, lg_radiance_gather_device, lg_radiance_gather_lanes) through every layer that
has to carry them, checked without a GPU: the built library exports the symbols, the header declares them with the arity, the parameter
names and the types the wrappers use, directly after lg_radiance_device, and states the contract -- the frame expression with its
operation order, the sequential sum, "written, not accumulated", both tile limits, the auto rule, where li lives --, lg_gather_out is 16
bytes in every mirror, the kernels are HIP kernels of their own in the build, and the Python, C++ and Rust bindings mirror the entry points.
On top: the lane rule over a table of shapes, the errors that are answered before any HIP call (a NULL accel), the no-op of empty sets, and
the wrapper's three conventions against their formulas."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_radiance_gather": 10, "lg_radiance_gather_device": 11, "lg_radiance_gather_lanes": 3}
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
    assert names("lg_radiance_gather")[1:] == ["origins", "frames", "n_poses", "dirs", "n_dirs", "weights", "n_weights", "lanes", "out"]
    assert names("lg_radiance_gather_device")[1:] == ["dev_origins", "dev_frames", "n_poses", "dev_dirs", "n_dirs", "dev_weights", "n_weights", "lanes", "dev_out",
                                                      "hip_stream"]
    assert names("lg_radiance_gather_lanes") == ["n_poses", "n_dirs", "lanes"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "const double *", "size_t", "const double *", "size_t", "const double *", "size_t", "int", "const lg_gather_out *"]
    assert types("lg_radiance_gather")[1:] == host
    assert types("lg_radiance_gather_device")[1:] == host + ["void *"]
    assert types("lg_radiance_gather_lanes") == ["size_t", "size_t", "int"]
    # directly after lg_radiance_device, among the extras: nothing but the struct is declared between the two
    assert header.index("EXTRAS") < header.index("int lg_range_scan_lanes(") < header.index("int lg_radiance(") < header.index("int lg_radiance_device(")
    assert header.index("int lg_radiance_device(") < header.index("int lg_radiance_gather(") < header.index("int lg_radiance_gather_device(")
    assert header.index("int lg_radiance_gather_device(") < header.index("int lg_radiance_gather_lanes(") < header.index("int lg_camera_rays(")
    between = gen_rust_sys.strip_comments(header[header.index("int lg_radiance_device("):header.index("int lg_radiance_gather(")])
    struct = re.search(r"typedef struct lg_gather_out \{(.*?)\} lg_gather_out;", between, flags=re.S)
    assert struct, "lg_gather_out is declared with the entry points"
    assert re.findall(r"(double)\s*\*(\w+);", struct.group(1)) == [("double", "radiance"), ("double", "sums")]
    assert between.replace(struct.group(0), "").count(";") == 1, "nothing else is declared between the two"
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("Radiance gathers"):header.index("typedef struct lg_gather_out")])
    assert "An EXTRA; no counterpart in the reference" in text
    assert "d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z" in text and "in this order" in text and "no contraction" in text, "the frame expression and its order"
    assert re.search(r"frames[^.]*MAY BE NULL", text) and "exactly the range scans' rule" in text and "dirs[k] bit for bit" in text
    assert "not normalised" in text and "W[k*n_weights + c]" in text and "k-major" in text
    assert "what lg_radiance returns for that ray, bit for bit" in text and "(0 + li) * 1.0" in text and "no switch of its own" in text
    assert "lg_accel_set_query_order plays no part" in text
    assert "more than 32 lights" in text and "recursion depth of 20 or more" in text, "lg_radiance's refusals"
    assert "radiance[i*n_dirs + k] = L(i,k)" in text and "sums[(i*n_weights + c)*3 + ch]" in text
    assert "acc = +0.0" in text and "acc = acc + L(i,k)[ch] * W[k*n_weights + c]" in text and "in that order" in text, "the sequential sum"
    assert "one f64 product then one f64 sum, nothing fused" in text and "0 * inf is NaN" in text and "a zero weight is not skipped" in text
    assert re.search(r"written,? not accumulated", text, flags=re.I) and "exactly one lane" in text and "no atomics" in text
    assert "tile = pose * ceil(n_dirs/64) + block" in text and "tile = pose_block * n_dirs + k" in text, "both work items"
    assert "pose lanes iff n_poses >= n_dirs" in text and "not a measured optimum" in text, "the auto rule"
    assert "Every output is the same bytes in either form" in text
    assert "n_dirs > 2^32 - 1" in text and "n_poses * ceil(n_dirs/64)" in text and "ceil(n_poses/64) * n_dirs" in text, "both tile limits"
    assert all(s in text for s in ("n_poses*n_dirs*24", "n_poses*72", "n_dirs*n_weights*8", "n_poses*n_weights*24")), "the four sizes"
    assert "successful no-op that writes nothing" in text and "answered BEFORE every other check" in text
    assert "both outputs NULL" in text and "weights == NULL or n_weights == 0" in text and "looked at only where sums is asked for" in text
    assert "LASGUN_GATHER_PARK_MB" in text and "default 1024" in text and "never fewer than one pose a batch" in text and "Batching cannot change a bit" in text
    assert "kind 1" in text and "HOST struct of device pointers" in text and "synchronises the device first" in text
    assert "leaves the caller's arrays as they were" in text
    assert "16 bytes; both NULL is an error" in header


def test_lg_gather_out_is_16_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    assert ctypes.sizeof(_capi.CGatherOut) == 16 and [f[0] for f in _capi.CGatherOut._fields_] == list(la.GATHER_PLANES)
    assert la.GATHER_PLANES == ("radiance", "sums")
    assert "sizeof(lg_gather_out) == 16" in read("lasgun_amd", "csrc", "gather_host.h")  # a static_assert of the library's own build
    assert "static_assert(sizeof(lg_gather_out) == 16" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_gather_out \{(.*?)\n\}", sys_src, flags=re.S)
    assert struct and re.findall(r"pub (\w+): \*mut (\w+),", struct.group(1)) == [("radiance", "f64"), ("sums", "f64")]
    assert "std::mem::size_of::<sys::lg_gather_out>() == 16" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.GATHER_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    for key in ("radiance_gather", "radiance_gather_device"):
        assert [i for i, a in enumerate(sigs[key][1]) if a is ctypes.c_size_t] == [3, 5, 7] and sigs[key][1][8] is ctypes.c_int, key
    assert sigs["radiance_gather_lanes"][1] == [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    for wrapper in ("radiance_gather", "radiance_gather_device", "radiance_gather_lanes"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.radiance_gather), "accel.radiance_gather(origins, dirs, frames=None, weights=None, planes=(\"sums\",), lanes=0)"
    assert callable(la.sh_weights) and callable(la.cosine_directions) and callable(la.frames_from_normals)


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_radiance_gather\(", src) and re.search(r"\blg_radiance_gather_device\(", src)
    assert re.search(r"void radiance_gather\(", src) and re.search(r"void radiance_gather_device\(", src)


def test_the_rust_crates_carry_them():
    import gen_rust_sys  # noqa: F401
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn radiance_gather\(", safe) and re.search(r"pub unsafe fn radiance_gather_device\(", safe) and re.search(r"pub fn radiance_gather_lanes\(", safe)
    assert "out: *const lg_gather_out" in sys_src and "n_weights: usize" in sys_src


def test_the_kernels_are_device_kernels_of_their_own():
    """The rays are made, walked and shaded in HIP kernels the library launches -- level 0's three passes in gather forms over the render's
    unchanged walk, and one reduction --; nothing expands the pairs into rays on the host, and no existing kernel file is touched for it."""
    from level0_text import calls_the_bodies, level0_bodies
    src = read("lasgun_amd", "csrc", "k_gather.hip")
    for kernel in ("gather_closest_kernel", "gather_shade_kernel", "gather_combine_kernel", "gather_resolve_kernel"):
        assert re.search(r"__global__ void [^\n]*\b%s\(" % kernel, src), kernel
    level0_bodies()  # one walk, closest hit, a finished ray is (0 + li) * 1.0 ...
    calls_the_bodies(src, 1, 1, 1)  # ... and the lane form is a template bool of the source
    assert "wave_append(" not in src and "trav_launch<GatherKernels>" in src and "trav_set_lds_limit<GatherKernels>" in src
    assert "(M[0] * b.x + M[1] * b.y) + M[2] * b.z" in src and "(M[6] * b.x + M[7] * b.y) + M[8] * b.z" in src
    assert "l0_finish_at(Q.li + 3ull * (it.pose * Q.n_dirs + it.k), value)" in src and "GatherSource<POSE>{Q}" in src, "a finished ray goes to its index of li"
    resolve = src[src.index("void __launch_bounds__(LG_BLOCK) gather_resolve_kernel("):src.index("// ---- host-callable launchers")]
    assert "atomic" not in resolve and "acc = acc + V3{l[0], l[1], l[2]} * w[0]" in resolve and "k < n_dirs; ++k" in resolve, "the sequential loop, one lane per (pose, c)"
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_gather.o" in make and "-ffp-contract=off" in make and "gather_host.h" in make
    assert "gather_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    launch = read("lasgun_amd", "csrc", "launch.cpp")
    assert "bind_level0<GatherArgs, launch_gather_closest, launch_gather_shade, launch_gather_combine>(G)" in launch
    assert re.search(r"timed\(a, 1, stream, \[&\] \{ return launch_gather_resolve\(", launch), "the reduction is credited to kind 1"
    assert launch.count("static void enqueue_level0_query(") == 1, "one level-0 query over the ray source, not a copy"
    host = read("lasgun_amd", "csrc", "query.cpp")
    whole = host[host.index("// ---- radiance gathers"):host.index("// ---- ray films")]
    assert "radiance_possible(*a)" in whole and "enqueue_radiance_gather(" in whole
    assert "lg_radiance(" not in whole and "enqueue_radiance_query(" not in whole and "pairs * 6" not in whole, "no rays are built on the host"
    assert "rq_closest_body.h" in read("profiles", "r16_kernel_resources_diff.txt") and "gather_closest_kernel" in read("profiles", "level0_shared_kernel_resources_diff.txt")


def test_the_lane_rule_over_a_table_of_shapes():
    import lasgun_amd as la
    G = la.api
    M = 2 ** 32 - 1
    for n, k, auto in ((0, 0, 2), (0, 1, 1), (1, 0, 2), (1, 1, 2), (1, 64, 1), (64, 1, 2), (63, 64, 1), (64, 64, 2), (65, 64, 2), (4096, 6144, 1), (1 << 20, 64, 2),
                       (M, M, 2), (M, M + 1, 1), (M + 1, M, 2), (TOP, TOP, 2), (TOP - 1, TOP, 1), (TOP, TOP - 1, 2), (0, TOP, 1), (TOP, 0, 2)):
        assert G.call("radiance_gather_lanes", n, k, 0) == auto, (n, k)
        assert G.radiance_gather_lanes(n, k) == auto and G.radiance_gather_lanes(n, k, "auto") == auto
        assert G.call("radiance_gather_lanes", n, k, 1) == 1 and G.call("radiance_gather_lanes", n, k, 2) == 2, (n, k)
        assert G.radiance_gather_lanes(n, k, "direction") == 1 and G.radiance_gather_lanes(n, k, "pose") == 2
        for bad in (-1, 3, 64, -2 ** 31, 2 ** 31 - 1):
            assert G.call("radiance_gather_lanes", n, k, bad) == -1, (n, k, bad)


def test_a_null_accel_is_refused_and_touches_nothing():
    import lasgun_amd as la
    from lasgun_amd import _capi
    G = la.api
    n, k, c = 5, 11, 3
    arrs = [np.full(n * k * 3, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(n * c * 3, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)]
    out = _capi.CGatherOut(*[a.ctypes.data for a in arrs])
    pts, frames, dirs, w = np.zeros((n, 3)), np.zeros((n, 9)), np.ones((k, 3)), np.ones((k, c))
    for fn, tail in (("radiance_gather", ()), ("radiance_gather_device", (None,))):
        for lanes in (0, 1, 2):
            rc = G.call(fn, None, pts.ctypes.data, frames.ctypes.data, n, dirs.ctypes.data, k, w.ctypes.data, c, lanes, ctypes.addressof(out), *tail)
            assert rc != 0 and G.last_error(), fn
            assert all((a == 0xA5A5A5A5A5A5A5A5).all() for a in arrs), fn


def test_zero_counts_are_a_no_op_with_every_pointer_null():
    import lasgun_amd as la
    G = la.api
    for n, k in ((0, 0), (0, 7), (7, 0)):
        for lanes in (0, 1, 2, 7, -1):  # (the empty set is answered before every other check, the lanes included)
            assert G.call("radiance_gather", None, None, None, n, None, k, None, 0, lanes, None) == 0, (n, k, lanes)
            assert G.call("radiance_gather_device", None, None, None, n, None, k, None, 0, lanes, None, None) == 0, (n, k, lanes)


# ---- the wrapper's three conventions, each against the formula its docstring states ----------------------------------------------------
def test_cosine_directions_follow_their_formula():
    import lasgun_amd as la
    assert "A convention of this WRAPPER" in la.cosine_directions.__doc__ and "u = (j + 0.5) / k" in la.cosine_directions.__doc__
    for k in (1, 2, 63, 64, 65, 1024):
        d = la.cosine_directions(k)
        assert d.shape == (k, 3) and d.dtype == np.float64 and d.flags["C_CONTIGUOUS"]
        j = np.arange(k, dtype=np.float64)
        u = (j + 0.5) / k
        r, phi = np.sqrt(u), j * (np.pi * (3.0 - np.sqrt(5.0)))
        assert np.array_equal(d, np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], axis=1)), k
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 4e-16 and (d[:, 2] > 0.0).all(), "unit vectors above the horizon"
    # cosine-distributed: the mean of cos(theta) over a cosine density is 2/3, of a constant 1 (so a plain mean of li estimates E / pi)
    assert abs(la.cosine_directions(4096)[:, 2].mean() - 2.0 / 3.0) < 1e-3


def test_sh_weights_follow_their_formula():
    import lasgun_amd as la
    assert "A convention of this WRAPPER" in la.sh_weights.__doc__ and "4 pi / K" in la.sh_weights.__doc__
    rng = np.random.default_rng(9)
    d = rng.normal(size=(257, 3)) * rng.uniform(0.1, 10.0, size=(257, 1))  # not unit vectors: the basis is of d / |d|
    n = d / np.linalg.norm(d, axis=1)[:, None]
    x, y, z = n.T
    Y = np.stack([np.full(257, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                  1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0), 1.0925484305920792 * (x * z),
                  0.5462742152960396 * (x * x - y * y)], axis=1)
    for bands in (1, 2, 3):
        w = la.sh_weights(d, bands)
        assert w.shape == (257, bands * bands) and w.dtype == np.float64 and w.flags["C_CONTIGUOUS"]
        assert np.array_equal(w, Y[:, :bands * bands] * (4.0 * np.pi / 257)), bands
    assert np.array_equal(la.sh_weights(d), la.sh_weights(d, 3))
    # the constants are the orthonormal real basis': sqrt(1/4pi), sqrt(3/4pi), sqrt(15/4pi), sqrt(5/16pi), sqrt(15/16pi)
    assert np.allclose([0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396],
                       np.sqrt(np.array([1.0, 3.0, 15.0, 5.0 / 4.0, 15.0 / 4.0]) / (4.0 * np.pi)), rtol=1e-15, atol=0.0)
    # ... so that the weights of an even lattice project a basis function onto itself: W^T Y = I up to the lattice's quadrature error
    lattice = la.sphere_directions(4096)
    W = la.sh_weights(lattice)
    assert np.abs(W.T @ (W * (4096 / (4.0 * np.pi))) - np.eye(9)).max() < 1e-3
    for bad in (0, 4):
        try:
            la.sh_weights(d, bad)
        except ValueError:
            continue
        raise AssertionError("bands outside 1 .. 3 is refused")


def test_frames_from_normals_follow_their_formula():
    import lasgun_amd as la
    assert "A convention of this WRAPPER" in la.frames_from_normals.__doc__ and "copysign(1, n.z)" in la.frames_from_normals.__doc__
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.normal(size=(500, 3)) * rng.uniform(0.1, 10.0, size=(500, 1)),
                        [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -2.0, 0.0], [1e-9, 0.0, -1.0], [0.0, 1.0, -0.0]]])
    f = la.frames_from_normals(v)
    assert f.shape == (len(v), 3, 3) and f.dtype == np.float64 and f.flags["C_CONTIGUOUS"]
    n = v / np.linalg.norm(v, axis=1)[:, None]
    x, y, z = n.T
    sg = np.copysign(1.0, z)
    a = -1.0 / (sg + z)
    b = x * y * a
    t = np.stack([1.0 + sg * x * x * a, sg * b, -sg * x], axis=1)
    s = np.stack([b, sg + y * y * a, -y], axis=1)
    assert np.array_equal(f[:, :, 0], t) and np.array_equal(f[:, :, 1], s) and np.array_equal(f[:, :, 2], n), "columns t, s, n"
    assert np.abs(np.einsum("nij,nkj->nik", f, f) - np.eye(3)).max() < 1e-14, "orthonormal"
    assert np.abs(np.linalg.det(f) - 1.0).max() < 1e-14, "right-handed"
    # the library's rule d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z takes (0, 0, 1) to the normal, bit for bit
    M = f.reshape(-1, 9)
    d = np.stack([(M[:, 3 * c] * 0.0 + M[:, 3 * c + 1] * 0.0) + M[:, 3 * c + 2] * 1.0 for c in range(3)], axis=1)
    assert np.array_equal(d, n)
