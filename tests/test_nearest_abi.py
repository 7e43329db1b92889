"""Proximity queries (include/lasgun_hip.h: lg_nearest, lg_nearest_device, lg_scene_nearest_lds) through every layer that has to carry
them, checked without a GPU: the built library exports the symbols, the header declares them with the arity, the parameter names and the
types the wrappers use and states the contract -- the candidates, the radius of a point, admissibility and the order, the slots and the
miss row, the writes, k, the errors in their order, the LDS formula and its limit, the stream, what is out of scope --, lg_nearest_out is
40 bytes with the stated offsets in every mirror, the kernel is a translation unit of its own over the walk and the list that the CPU
checks run, and the Python, C++ and Rust bindings mirror the entry points.  On top: the errors answered before any HIP call and the no-op
of an empty set."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_nearest": 7, "lg_nearest_device": 8, "lg_scene_nearest_lds": 2}
NAMES = tuple(ARITY)
MEMBERS = [("uint8_t", "touch"), ("uint32_t", "count"), ("double", "distance"), ("double", "point"), ("uint32_t", "id")]
PLANES = tuple(m[1] for m in MEMBERS)


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
        assert ret == ("size_t" if name == "lg_scene_nearest_lds" else "int") and len(params) == ARITY[name], (name, ret, params)
    names = lambda key: [p.split()[-1].lstrip("*") for p in decl[key][1]]  # noqa: E731
    assert names("lg_nearest")[1:] == ["points", "radii", "n", "radius", "k", "out"]
    assert names("lg_nearest_device")[1:] == ["dev_points", "dev_radii", "n", "radius", "k", "dev_out", "hip_stream"]
    assert names("lg_scene_nearest_lds")[1:] == ["k"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "const double *", "size_t", "double", "uint32_t", "const lg_nearest_out *"]
    assert types("lg_nearest")[1:] == host and types("lg_nearest_device")[1:] == host + ["void *"]
    assert "lg_accel" in decl["lg_nearest"][1][0] and "lg_scene" in decl["lg_scene_nearest_lds"][1][0]
    order = ["int lg_closest_points_device(", "int lg_scene_closest_depth(", "/* Proximity queries:", "#define LG_NEAREST_MAX_K 8", "typedef struct lg_nearest_out {",
             "int lg_nearest(", "int lg_nearest_device(", "size_t lg_scene_nearest_lds("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), "beside lg_closest_points"
    struct = header[header.index("typedef struct lg_nearest_out {"):header.index("} lg_nearest_out;")]
    assert re.findall(r"^\s+(\w+)\s*\*(\w+);", struct, flags=re.M) == MEMBERS
    text = " ".join(re.sub(r"\n \*", "\n", header[header.index("/* Proximity queries:"):header.index("#define LG_NEAREST_MAX_K 8")]).split())
    for needle in ("An EXTRA", "bit for bit", "one candidate per primitive of the scene", "exactly as lg_closest_points defines them", "ONE candidate per box",
                   "instance << 34 | kind << 32 | prim", "radii[i] where `radii` is not NULL, otherwise `radius`", "radius is not read and not checked",
                   "NaN or < 0 makes that point a miss", "-0.0 is zero", "A shared radius that is NaN or negative is an error",
                   "d2 <= r_i*r_i && d2 < +INF, r_i*r_i one f64 product", "non-finite coordinate has no admissible candidate", "ascending by (d2, key)",
                   "j < min(count, k)", "distance = +INF, point = +0.0, id = 0, ~0, ~0, -1", "slot 0 is lg_closest_points' planes byte for byte",
                   "element (j, i) at j*n + i", "ALL of them, not capped at k", "touch is 1 iff count > 0", "exactly one lane: no atomics, no pre-fill",
                   "the same bytes in every mode", "more than 32 lights is accepted", "k == 0 is legal iff no slot plane", "k then plays no part",
                   "ends at its first admissible candidate", "visits every primitive for every point", "n == 0 is a successful no-op", "in this order",
                   "k > LG_NEAREST_MAX_K, or k == 0 with a slot plane", "(2^32 - 1) * 64", "n * k or a plane's byte size", "refused, never truncated",
                   "touch 1 byte, count 4, points, radii, distance and point 8; id 16", "ends beyond its allocation",
                   "lg_scene_nearest_lds(scene, k) = 256 * (8 * depth + 20 * k) bytes", "The limit is 160 KiB on gfx950", "refuses exactly where",
                   "answered up to k = 6", "only enqueues on hip_stream", "first call of either builds and uploads",
                   "Out of scope: de-duplicating coplanar neighbours", "a normal at the point", "world-space vertex tables or run skipping inside fat leaves",
                   "a multi-device split"):
        assert needle in text, needle
    closest = " ".join(re.sub(r"\n \*", "\n", header[header.index("/* Closest points:"):header.index("typedef struct lg_closest_out {")]).split())
    assert "per-point radii and the k nearest are lg_nearest's, below" in closest, "lg_closest_points' comment points here"


def test_the_struct_is_40_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd._capi import CNearestOut
    assert ctypes.sizeof(CNearestOut) == 40 and [f[0] for f in CNearestOut._fields_] == list(PLANES) == list(la.NEAREST_PLANES)
    assert [getattr(CNearestOut, p).offset for p in PLANES] == [0, 8, 16, 24, 32]
    assert la.NEAREST_MAX_K == 8 and la.NEAREST_SLOT_PLANES == ("distance", "point", "id")
    host = read("lasgun_amd", "csrc", "nearest_host.h")
    assert "sizeof(lg_nearest_out) == 40" in host and "offsetof(lg_nearest_out, count) == 8" in host and "offsetof(lg_nearest_out, id) == 32" in host
    for line in ('f(out.touch, n, 1, "touch");', 'f(out.count, n, 4, "count");', 'f(out.distance, nk, 8, "distance");', 'f(out.point, nk * 3, 8, "point");',
                 'f(out.id, nk * 4, 16, "id");'):
        assert line in host, line
    assert "NEAREST_MAX_K = LG_NEAREST_MAX_K" in host and "NEAREST_LDS_LIMIT = (size_t)160 << 10" in host
    assert "sizeof(lg_nearest_out) == 40" in read("include", "lasgun.hpp")
    rust = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    block = rust[rust.index("pub struct lg_nearest_out {"):]
    block = block[:block.index("}")]
    assert re.findall(r"pub (\w+): \*mut (\w+),", block) == [("touch", "u8"), ("count", "u32"), ("distance", "f64"), ("point", "f64"), ("id", "u32")]
    assert "pub const LG_NEAREST_MAX_K: u32 = 8;" in rust
    assert "size_of::<sys::lg_nearest_out>() == 40" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_the_kernel_is_its_own_unit_over_the_checked_text():
    kernel = read("lasgun_amd", "csrc", "k_nearest.hip")
    assert '#define LG_CLOSEST_WALK_ONLY\n#include "k_closest.hip"' in kernel, "the walk's pieces are closest points' own text, not a copy"
    assert '#include "nearest_list.h"' in kernel and '#include "nearest_host.h"' in kernel
    assert '#include "walk.h"' not in kernel and '#include "shade.h"' not in kernel, "the ray walk and the shading stay untouched and unused"
    for name in ("closest_world", "closest_enter", "closest_box_d2", "closest_skip", "closest_candidate", "closest_leaf", "closest_material", "closest_begin", "closest_next_tile"):
        assert not re.search(r"__device__ __forceinline__ [\w ]+ " + name + r"\(", kernel), (name, "defined once, in k_closest.hip")
        assert re.search(r"__device__ __forceinline__ [\w ]+ " + name + r"\(", read("lasgun_amd", "csrc", "k_closest.hip")), name
    for needle in ("if (!closest_begin(ntiles)) return;", "closest_next_tile(Q, ntiles, final)", "template <int FORM> __global__ void __launch_bounds__(LG_BLOCK) nearest_kernel(const DParams P, const NearestArgs N)",
                   "extern __shared__ uint32_t nearest_lds[];", "const double lim = FORM == NEAREST_LIST ? fmin(worst, r2) : r2;", "closest_skip(L, d0, lim, eta, prune)",
                   "if (FORM == NEAREST_TOUCH && total != 0ull) break;", "nearest_insert(list, m, kcap, ", "closest_candidate(P, Q, instance, e.slot, "):
        assert needle in kernel, needle
    assert "atomic" not in kernel.replace("no atomics", ""), "every element is written by exactly one lane"
    closest = read("lasgun_amd", "csrc", "k_closest.hip")
    guarded = closest[closest.index("#ifndef LG_CLOSEST_WALK_ONLY\n__global__"):closest.index("#endif // LG_CLOSEST_WALK_ONLY")]
    assert "closest_kernel(" in guarded and "launch_closest(" in guarded and "closest_set_lds_limit(" in guarded, "what k_nearest.hip leaves out of k_closest.hip"
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_nearest.o" in make[make.index("KOBJS"):make.index("KHDRS")] and "k_nearest.o: k_closest.hip closest_prim.h closest_host.h nearest_host.h nearest_list.h planes_host.h" in make
    assert "nearest_host.h" in make[make.index("query.o:"):] and "nearest_host.h" in make[make.index("capi.o:"):make.index("launch.o:")]


def test_the_bindings_mirror_the_entry_points():
    import lasgun_amd as la
    from lasgun_amd._capi import NEAREST_SIGNATURES
    assert set(NEAREST_SIGNATURES) == {n[3:] for n in NAMES}
    assert [len(NEAREST_SIGNATURES[n[3:]][1]) for n in NAMES] == [ARITY[n] for n in NAMES]
    assert NEAREST_SIGNATURES["scene_nearest_lds"][0] is ctypes.c_size_t
    for attr in ("nearest", "nearest_device", "scene_nearest_lds", "touching"):
        assert callable(getattr(la.api, attr)), attr
    assert callable(la.api.Accel.nearest) and callable(la.api.Accel.touching)
    assert "SURFACE" in la.api.touching.__doc__ and "first contact" in la.api.touching.__doc__, "the convenience's meaning is documented"
    hpp = read("include", "lasgun.hpp")
    for needle in ("struct Nearest {", "void nearest(const std::vector<std::array<double, 3>> &points, const std::vector<double> *radii, uint32_t k, const Nearest &out, double radius = INFINITY) const",
                   "lg_nearest(h_, ", "lg_nearest_device(h_, dev_points, dev_radii, n, radius, k, &dev_out, hip_stream)"):
        assert needle in hpp, needle
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for needle in ("pub struct Nearest<'a>", "pub fn nearest(&self, points: &[[f64; 3]], radii: Option<&[f64]>, radius: f64, k: u32, out: Nearest)", "sys::lg_nearest(self.ptr, ",
                   "pub unsafe fn nearest_device(", "uncompiled"):
        assert needle in safe, needle
    assert "`Accel::nearest`" in read("bindings", "rust", "README.md") and "NOT" in read("bindings", "rust", "README.md")


def test_the_errors_before_any_device_call_and_the_empty_set():
    import lasgun_amd as la
    from lasgun_amd._capi import CNearestOut
    lib = ctypes.CDLL(la.LIB_PATH)
    fn = lib.lg_nearest
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p]
    dev = lib.lg_nearest_device
    dev.restype, dev.argtypes = ctypes.c_int, fn.argtypes + [ctypes.c_void_p]
    lds = lib.lg_scene_nearest_lds
    lds.restype, lds.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_uint32]
    lib.lg_last_error.restype = ctypes.c_char_p
    pts = np.zeros((4, 3))
    d = np.full(2 * 4 * 4, 7.0)
    out = CNearestOut(None, None, d.ctypes.data, None, None)
    flags = CNearestOut(d.ctypes.data, d.ctypes.data, None, None, None)
    none = CNearestOut(None, None, None, None, None)
    fake = ctypes.c_void_p(0x1000)  # an accel that is never looked at: each of these is refused before it would be
    P, O, F = pts.ctypes.data, ctypes.addressof(out), ctypes.addressof(flags)
    assert fn(None, None, None, 0, -1.0, 99, None) == 0 and dev(None, None, None, 0, float("nan"), 99, None, None) == 0, "n == 0 is answered before every other check"
    for args, what in (((None, P, None, 4, 1.0, 2, O), "accel is NULL"), ((fake, None, None, 4, 1.0, 2, O), "points is NULL"), ((fake, P, None, 4, 1.0, 2, None), "out is NULL"),
                       ((fake, P, None, 4, 1.0, 2, ctypes.addressof(none)), "every plane of out is NULL"), ((fake, P, None, 4, -1.0, 2, O), "radius is NaN or negative"),
                       ((fake, P, None, 4, float("nan"), 2, O), "radius is NaN or negative"), ((fake, P, None, 4, 1.0, 9, O), "k is beyond LG_NEAREST_MAX_K"),
                       ((fake, P, None, 4, 1.0, 9, F), "k is beyond LG_NEAREST_MAX_K"), ((fake, P, None, 4, 1.0, 0, O), "k is 0 and a slot plane"),
                       ((fake, P, P, 4, -1.0, 0, O), "k is 0 and a slot plane"),  # (with radii a bad shared radius is not an error: the next one is named)
                       ((fake, P, None, (2 ** 32 - 1) * 64 + 1, 1.0, 2, O), "too many points")):
        assert fn(*args) != 0 and what in lib.lg_last_error().decode(), (what, lib.lg_last_error())
        assert dev(*args, None) != 0 and what in lib.lg_last_error().decode(), (what, lib.lg_last_error())
    assert dev(fake, ctypes.c_void_p(P + 4), None, 4, 1.0, 2, O, None) != 0 and "points is not 8-byte aligned" in lib.lg_last_error().decode()
    assert dev(fake, P, ctypes.c_void_p(P + 4), 4, 1.0, 2, O, None) != 0 and "radii is not 8-byte aligned" in lib.lg_last_error().decode()
    bad_id = CNearestOut(None, None, None, None, d.ctypes.data + 8)
    assert dev(fake, P, None, 4, 1.0, 2, ctypes.addressof(bad_id), None) != 0 and "id is not 16-byte aligned" in lib.lg_last_error().decode()
    bad_count = CNearestOut(None, d.ctypes.data + 2, None, None, None)
    assert dev(fake, P, None, 4, 1.0, 2, ctypes.addressof(bad_count), None) != 0 and "count is not 4-byte aligned" in lib.lg_last_error().decode()
    assert (d == 7.0).all()
    assert lds(None, 1) == 0 and "scene is NULL" in lib.lg_last_error().decode()
    with pytest.raises(ValueError):
        la.api.nearest(None, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        la.api.nearest(None, np.zeros((4, 3)), planes=("distance", "normal"))
    with pytest.raises(ValueError):
        la.api.nearest(None, np.zeros((4, 3)), k=9)
    with pytest.raises(ValueError):
        la.api.nearest(None, np.zeros((4, 3)), radii=np.zeros(3))
    with pytest.raises(ValueError, match="no array for the plane 'count'"):
        la.api.nearest(None, np.zeros((4, 3)), planes=("touch", "count"), into={"touch": np.zeros(4, dtype=np.uint8)})
    assert re.search(r"^#define LG_NEAREST_MAX_K\s+8\b", read("include", "lasgun_hip.h"), flags=re.M)
