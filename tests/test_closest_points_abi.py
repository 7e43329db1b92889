"""Closest points (include/lasgun_hip.h: lg_closest_points, lg_closest_points_device, lg_scene_closest_gate) through every layer that has to
carry it, checked without a GPU: the built library exports the symbols, the header declares them with the arity, the parameter names and
the types the wrappers use and states the contract -- the world position, the triangle's seven steps, the box's twelve triangles, the
sphere, the winner and its tie rule, the miss record, the gate, the limits, what is out of scope --, lg_closest_out is 24 bytes with the
stated offsets in every mirror, the kernel is a translation unit of its own over the arithmetic that the CPU check runs, and the Python,
C++ and Rust bindings mirror the entry points.  On top: the errors answered before any HIP call, the no-op of an empty set, the gate's
verdicts (which need no device)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_closest_points": 5, "lg_closest_points_device": 6, "lg_scene_closest_gate": 3, "lg_scene_closest_depth": 1}
NAMES = tuple(ARITY)
MEMBERS = [("double", "distance"), ("double", "point"), ("uint32_t", "id")]
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
        assert ret == "int" and len(params) == ARITY[name], (name, ret, params)
    names = lambda key: [p.split()[-1].lstrip("*") for p in decl[key][1]]  # noqa: E731
    assert names("lg_closest_points")[1:] == ["points", "n", "radius", "out"]
    assert names("lg_closest_points_device")[1:] == ["dev_points", "n", "radius", "dev_out", "hip_stream"]
    assert names("lg_scene_closest_gate")[1:] == ["shrink", "cap"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "size_t", "double", "const lg_closest_out *"]
    assert types("lg_closest_points")[1:] == host and types("lg_closest_points_device")[1:] == host + ["void *"]
    assert "lg_accel" in decl["lg_closest_points"][1][0] and "lg_scene" in decl["lg_scene_closest_gate"][1][0]
    order = ["int lg_hit_attributes_of_device(", "/* Closest points:", "typedef struct lg_closest_out {", "int lg_closest_points(", "int lg_closest_points_device(",
             "int lg_scene_closest_gate("]
    at = [header.index(o) for o in order]
    assert at == sorted(at)
    struct = header[header.index("typedef struct lg_closest_out {"):header.index("} lg_closest_out;")]
    assert re.findall(r"^\s+(\w+)\s*\*(\w+);", struct, flags=re.M) == MEMBERS
    text = " ".join(re.sub(r"\n \*", "\n", header[header.index("/* Closest points:"):header.index("typedef struct lg_closest_out {")]).split())
    for needle in ("An EXTRA", "bit for bit", "the same bytes in every mode", "dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z", "((c0*x + c1*y) + c2*z) + c3*1.0",
                   "up to and including the root's", "d1<=0 && d2<=0: x = a", "d3>=0 && d4<=d3: x = b", "vc=d1*d4-d3*d2", "x = a+ab*(d1/(d1-d3))",
                   "d6>=0 && d5<=d6: x = c", "vb=d5*d2-d1*d6", "x = a+ac*(d2/(d2-d6))", "va=d3*d6-d5*d4", "x = b+(c-b)*((d4-d3)/((d4-d3)+(d5-d6)))",
                   "den=1/((va+vb)+vc), x = (a+ab*(vb*den))+ac*(vc*den)", "-x (0,2,6) (0,6,4); +x (1,3,7) (1,7,5)", "-y (0,1,5) (0,5,4); +y (2,3,7) (2,7,6)",
                   "-z (0,1,3) (0,3,2); +z (4,5,7) (4,7,6)", "the first triangle a tie", "pw = W_A(c + (r,0,0))", "d = fabs(l-rw)", "x = pw where l == 0",
                   "<= radius*radius and < +INF (a NaN never wins)", "smallest (instance, kind, prim)", "id = 0, ~0, ~0, -1", "non-finite coordinate",
                   "more than 32 lights is accepted", "within 2^-40", "n == 0 is a successful no-op", "NaN or negative", "(2^32 - 1) * 64", "refused, never truncated",
                   "points, distance and point 8 bytes; id 16", "ends beyond its allocation", "exactly one lane: no atomics",
                   "Out of scope: per-point radii, the k nearest, a normal at the closest point, the sorted order, a multi-device split"):
        assert needle in text, needle


def test_the_struct_is_24_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd._capi import CClosestOut
    assert ctypes.sizeof(CClosestOut) == 24 and [f[0] for f in CClosestOut._fields_] == list(PLANES) == list(la.CLOSEST_PLANES)
    assert [getattr(CClosestOut, p).offset for p in PLANES] == [0, 8, 16]
    host = read("lasgun_amd", "csrc", "closest_host.h")
    assert "sizeof(lg_closest_out) == 24" in host and "offsetof(lg_closest_out, point) == 8" in host and "offsetof(lg_closest_out, id) == 16" in host
    for line in ('f(out.distance, n, 8, "distance");', 'f(out.point, n * 3, 8, "point");', 'f(out.id, n * 4, 16, "id");'):
        assert line in host, line
    assert "sizeof(lg_closest_out) == 24" in read("include", "lasgun.hpp")
    rust = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    block = rust[rust.index("pub struct lg_closest_out {"):]
    block = block[:block.index("}")]
    assert re.findall(r"pub (\w+): \*mut (\w+),", block) == [("distance", "f64"), ("point", "f64"), ("id", "u32")]
    assert "size_of::<sys::lg_closest_out>() == 24" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_the_kernel_is_its_own_unit_over_the_checked_arithmetic():
    kernel = read("lasgun_amd", "csrc", "k_closest.hip")
    assert '#include "closest_prim.h"' in kernel and '#include "closest_host.h"' in kernel
    assert '#include "walk.h"' not in kernel and '#include "shade.h"' not in kernel, "the ray walk and the shading stay untouched and unused"
    for needle in ("claim_tile_single(Q.tile_counter, ntiles, final)", "__launch_bounds__(LG_BLOCK) closest_kernel(const DParams P, const ClosestArgs Q)",
                   "extern __shared__ uint32_t closest_stack[];", "closest_triangle(qw, a, b, cc)", "closest_box(qw, w)", "closest_sphere(qw, ",
                   "closest_offer(best, c, Q.r2, closest_key(L.accel, kind + 1u, prim))", "return lb > 0.0 && lb * lb > lim * (1.0 + 0x1p-40);"):
        assert needle in kernel, needle
    assert "atomic" not in kernel.replace("no atomics", ""), "every element is written by exactly one lane"
    assert "#if LG_CLOSEST_FAULT != 0\n#error" in kernel, "a seeded fault can never be built into the kernel, whatever flags leak in"
    prim = read("lasgun_amd", "csrc", "closest_prim.h")
    assert prim.count("#if LG_CLOSEST_FAULT") == 3 and "#define LG_CLOSEST_FAULT 0" in prim
    assert "-DLG_CLOSEST_FAULT" not in read("lasgun_amd", "csrc", "Makefile"), "the product is built without a seeded fault"
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_closest.o" in make and "k_closest.o: closest_prim.h closest_host.h planes_host.h" in make and "closest_host.h" in make[make.index("query.o:"):]
    query = read("lasgun_amd", "csrc", "query.cpp")
    for needle in ("check_closest(a, points, n, radius, out);", "check_closest(a, dev_points, n, radius, dev_out);", "check_closest_alignment(dev_points, *dev_out);",
                   "closest_planes(dev, n, staged_planes(trip));", "closest_planes(*dev_out, n, device_planes(*a));"):
        assert needle in query, needle
    body = query[query.index("static void enqueue_closest("):query.index('extern "C" int lg_closest_points(')]
    assert body.count("launch_closest(") == 1, "one launch, no chunks"


def test_the_bindings_mirror_the_entry_points():
    import lasgun_amd as la
    from lasgun_amd._capi import CLOSEST_SIGNATURES
    assert set(CLOSEST_SIGNATURES) == {n[3:] for n in NAMES}
    assert [len(CLOSEST_SIGNATURES[n[3:]][1]) for n in NAMES] == [ARITY[n] for n in NAMES]
    for attr in ("closest_points", "closest_points_device", "scene_closest_gate", "scene_closest_depth", "signed_distance"):
        assert callable(getattr(la.api, attr)), attr
    assert callable(la.api.Accel.closest_points) and callable(la.api.Accel.signed_distance)
    assert "CLOSED solids only" in la.api.signed_distance.__doc__, "the convention's limits are documented"
    hpp = read("include", "lasgun.hpp")
    for needle in ("struct Closest {", "void closest_points(const std::vector<std::array<double, 3>> &points, const Closest &out, double radius = INFINITY) const",
                   "lg_closest_points(h_, ", "lg_closest_points_device(h_, dev_points, n, radius, &dev_out, hip_stream)"):
        assert needle in hpp, needle
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for needle in ("pub struct Closest<'a>", "pub fn closest_points(&self, points: &[[f64; 3]], radius: f64, out: Closest)", "sys::lg_closest_points(self.ptr, ",
                   "pub unsafe fn closest_points_device(", "uncompiled"):
        assert needle in safe, needle
    assert "`Accel::closest_points`" in read("bindings", "rust", "README.md")


def test_the_errors_before_any_device_call_and_the_empty_set():
    import lasgun_amd as la
    from lasgun_amd._capi import CClosestOut
    lib = ctypes.CDLL(la.LIB_PATH)
    fn = lib.lg_closest_points
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p]
    dev = lib.lg_closest_points_device
    dev.restype, dev.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    lib.lg_last_error.restype = ctypes.c_char_p
    pts = np.zeros((4, 3))
    d = np.full(4, 7.0)
    out = CClosestOut(d.ctypes.data, None, None)
    none = CClosestOut(None, None, None)
    fake = ctypes.c_void_p(0x1000)  # an accel that is never looked at: each of these is refused before it would be
    assert fn(None, None, 0, -1.0, None) == 0 and dev(None, None, 0, float("nan"), None, None) == 0, "n == 0 is answered before every other check"
    for args, what in (((None, pts.ctypes.data, 4, 1.0, ctypes.addressof(out)), "accel is NULL"), ((fake, None, 4, 1.0, ctypes.addressof(out)), "points is NULL"),
                       ((fake, pts.ctypes.data, 4, 1.0, None), "out is NULL"), ((fake, pts.ctypes.data, 4, 1.0, ctypes.addressof(none)), "every plane of out is NULL"),
                       ((fake, pts.ctypes.data, 4, -1.0, ctypes.addressof(out)), "radius is NaN or negative"),
                       ((fake, pts.ctypes.data, 4, float("nan"), ctypes.addressof(out)), "radius is NaN or negative"),
                       ((fake, pts.ctypes.data, (2 ** 32 - 1) * 64 + 1, 1.0, ctypes.addressof(out)), "too many points")):
        assert fn(*args) != 0 and what in lib.lg_last_error().decode(), (what, lib.lg_last_error())
        assert dev(*args, None) != 0 and what in lib.lg_last_error().decode(), (what, lib.lg_last_error())
    assert dev(fake, ctypes.c_void_p(pts.ctypes.data + 4), 4, 1.0, ctypes.addressof(out), None) != 0 and "points is not 8-byte aligned" in lib.lg_last_error().decode()
    bad_id = CClosestOut(None, None, d.ctypes.data + 8)
    assert dev(fake, pts.ctypes.data, 4, 1.0, ctypes.addressof(bad_id), None) != 0 and "id is not 16-byte aligned" in lib.lg_last_error().decode()
    assert (d == 7.0).all()
    with pytest.raises(ValueError):
        la.api.closest_points(None, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        la.api.closest_points(None, np.zeros((4, 3)), planes=("distance", "normal"))
    with pytest.raises(ValueError, match="no array for the plane 'point'"):
        la.api.closest_points(None, np.zeros((4, 3)), planes=("distance", "point"), into={"distance": np.zeros(4)})
    assert re.search(r"^#define LG_CLOSEST_MAX_DEPTH\s+64\b", read("include", "lasgun_hip.h"), flags=re.M) and la.api.CLOSEST_MAX_DEPTH == 64
    assert "CLOSEST_MAX_DEPTH = LG_CLOSEST_MAX_DEPTH" in read("lasgun_amd", "csrc", "closest_host.h")
