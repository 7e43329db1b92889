"""Segment proximity (include/lasgun_hip.h: lg_closest_segments, lg_closest_segments_device) through every layer that has to carry it,
checked without a GPU: the built library exports the symbols, the header declares them with the arity, the parameter names and the types the
wrappers use and states the contract, lg_segments_out is 40 bytes with the stated offsets in every mirror, the Python plane table is the
struct's, the kernel is a translation unit of its own over closest points' walk and the arithmetic that the CPU checks run, and the Python,
C++ and Rust bindings mirror the entry points.  On top: the errors answered before any HIP call and the no-op of an empty set, answered
before every other check."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_closest_segments": 6, "lg_closest_segments_device": 7}
NAMES = tuple(ARITY)
MEMBERS = [("uint8_t", "touch"), ("double", "distance"), ("double", "param"), ("double", "point"), ("uint32_t", "id")]
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
    assert names("lg_closest_segments")[1:] == ["segments", "radii", "n", "radius", "out"]
    assert names("lg_closest_segments_device")[1:] == ["dev_segments", "dev_radii", "n", "radius", "dev_out", "hip_stream"]
    order = ["size_t lg_scene_nearest_lds(", "/* Segment proximity:", "typedef struct lg_segments_out {", "int lg_closest_segments(", "int lg_closest_segments_device("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), "beside lg_nearest"
    struct = header[header.index("typedef struct lg_segments_out {"):header.index("} lg_segments_out;")]
    assert re.findall(r"^\s+(\w+)\s*\*(\w+);", struct, flags=re.M) == MEMBERS
    text = " ".join(re.sub(r"\n \*", "\n", header[header.index("/* Segment proximity:"):header.index("typedef struct lg_segments_out {")]).split())
    for needle in ("An EXTRA", "bit for bit", "n x 6 f64, world space: p0, then p1", "one candidate (d2, s, x) per primitive", "ON THE PRIMITIVE", "never -0.0",
                   "p0 == p1 in all three components", "lg_nearest's k = 1 bytes", "six sub-candidates in this order", "the first a tie", "Ericson 5.3.6, two-sided",
                   "CONFIRMED", "Ericson 5.1.9 with EPSILON = 0", "never an algebraic shortcut", "twelve triangles in lg_closest_points' order",
                   "wholly inside a box gets the distance to its surface", "lmin>rw", "lmax<rw", "crosses the surface", "s=s*, x=m",
                   "radii may be NULL", "NaN or < 0 makes that segment a miss, not an error", "-0.0 is zero", "d2 <= r_i*r_i && d2 < +INF",
                   "non-finite coordinate is a miss", "smallest (d2, key)", "touch 0, distance +INF, param +0.0, point +0.0, id 0, ~0, ~0, -1",
                   "written by exactly one lane", "more than 32 lights is accepted", "ends at its first admissible candidate", "n == 0 is a successful no-op",
                   "answered BEFORE every other check", "in this order", "(2^32 - 1) * 64", "lg_scene_closest_gate", "lg_scene_closest_depth",
                   "touch 1 byte; segments, radii, distance, param and point 8; id 16", "ends beyond its allocation", "LDS is the stack alone, 256 * 8 * depth bytes",
                   "only enqueues on hip_stream", "Out of scope: k > 1 and counts", "a time of impact along the segment", "world-space vertex tables for fat leaves",
                   "a multi-device split"):
        assert needle in text, needle


def test_the_struct_is_40_bytes_in_every_mirror_and_the_plane_table_is_the_structs():
    import lasgun_amd as la
    from lasgun_amd._capi import CSegmentsOut
    assert ctypes.sizeof(CSegmentsOut) == 40 and [f[0] for f in CSegmentsOut._fields_] == list(PLANES) == list(la.SEGMENT_PLANES)
    assert [getattr(CSegmentsOut, p).offset for p in PLANES] == [0, 8, 16, 24, 32]
    host = read("lasgun_amd", "csrc", "segments_host.h")
    assert "sizeof(lg_segments_out) == 40" in host and "offsetof(lg_segments_out, param) == 16" in host and "offsetof(lg_segments_out, id) == 32" in host
    for line in ('f(out.touch, n, 1, "touch");', 'f(out.distance, n, 8, "distance");', 'f(out.param, n, 8, "param");', 'f(out.point, n * 3, 8, "point");',
                 'f(out.id, n * 4, 16, "id");'):
        assert line in host, line
    assert "sizeof(lg_segments_out) == 40" in read("include", "lasgun.hpp")
    rust = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    block = rust[rust.index("pub struct lg_segments_out {"):]
    block = block[:block.index("}")]
    assert re.findall(r"pub (\w+): \*mut (\w+),", block) == [("touch", "u8"), ("distance", "f64"), ("param", "f64"), ("point", "f64"), ("id", "u32")]
    assert "size_of::<sys::lg_segments_out>() == 40" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_the_kernel_is_its_own_unit_over_the_checked_text():
    kernel = read("lasgun_amd", "csrc", "k_segments.hip")
    assert '#define LG_CLOSEST_WALK_ONLY\n#include "k_closest.hip"' in kernel, "the walk's pieces are closest points' own text, not a copy"
    assert '#include "segment_prim.h"' in kernel and '#include "segments_host.h"' in kernel
    assert '#include "walk.h"' not in kernel and '#include "shade.h"' not in kernel
    for name in ("closest_world", "closest_enter", "closest_box_d2", "closest_skip", "closest_candidate", "closest_leaf", "closest_material", "closest_begin", "closest_next_tile"):
        assert not re.search(r"__device__ __forceinline__ [\w ]+ " + name + r"\(", kernel), (name, "defined once, in k_closest.hip")
    for needle in ("if (!closest_begin(ntiles)) return;", "closest_next_tile(Q, ntiles, final)",
                   "template <int FORM> __global__ void __launch_bounds__(LG_BLOCK) segments_kernel(const DParams P, const SegmentsArgs N)",
                   "extern __shared__ uint32_t segments_stack[];", "const double lim = FORM == SEGMENTS_BEST ? fmin(best.d2, r2) : r2;", "closest_skip(S.L, d0, lim, eta, prune)",
                   "if (FORM == SEGMENTS_TOUCH && touched) break;", "closest_leaf(P, Q, S.L, p0, n, stack, sp, ", "seg_offer(best, c, r2, closest_key(S.L.accel, kind + 1u, prim));",
                   "segments_slab_miss(S, n0, rho)", "tmin > tmax + 0x1p-40", "#ifdef LG_SEGMENTS_NO_STAGE2"):
        assert needle in kernel, needle
    assert "atomic" not in kernel.replace("no atomics", ""), "every element is written by exactly one lane"
    prim = read("lasgun_amd", "csrc", "segment_prim.h")
    assert "for (int t = 0; t < 12; ++t)" in prim and prim.count("    LG_SEG_LOOP\n") == 3, "twelve triangles times six sub-candidates stay loops"
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_segments.o" in make[make.index("KOBJS"):make.index("KHDRS")] and "k_segments.o: k_closest.hip closest_prim.h segment_prim.h closest_host.h segments_host.h planes_host.h" in make
    assert "segments_host.h" in make[make.index("query.o:"):]


def test_the_bindings_mirror_the_entry_points():
    import lasgun_amd as la
    from lasgun_amd._capi import SEGMENTS_SIGNATURES
    assert set(SEGMENTS_SIGNATURES) == {n[3:] for n in NAMES}
    assert [len(SEGMENTS_SIGNATURES[n[3:]][1]) for n in NAMES] == [ARITY[n] for n in NAMES]
    for attr in ("closest_segments", "closest_segments_device", "capsules_touching", "sweep_touching"):
        assert callable(getattr(la.api, attr)), attr
    assert callable(la.api.Accel.closest_segments) and callable(la.api.Accel.capsules_touching) and callable(la.api.Accel.sweep_touching)
    assert "SURFACE" in la.api.capsules_touching.__doc__ and "first contact" in la.api.capsules_touching.__doc__
    assert "No time of impact" in la.api.sweep_touching.__doc__
    hpp = read("include", "lasgun.hpp")
    for needle in ("struct Segments {", "void closest_segments(const std::vector<std::array<double, 6>> &segments, const std::vector<double> *radii, const Segments &out, double radius = INFINITY) const",
                   "lg_closest_segments(h_, ", "lg_closest_segments_device(h_, dev_segments, dev_radii, n, radius, &dev_out, hip_stream)"):
        assert needle in hpp, needle
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for needle in ("pub struct Segments<'a>", "pub fn closest_segments(&self, segments: &[[f64; 6]], radii: Option<&[f64]>, radius: f64, out: Segments)", "sys::lg_closest_segments(self.ptr, ",
                   "pub unsafe fn closest_segments_device(", "uncompiled"):
        assert needle in safe, needle
    assert "`Accel::closest_segments`" in read("bindings", "rust", "README.md")


def test_the_errors_before_any_device_call_and_the_empty_set():
    import lasgun_amd as la
    from lasgun_amd._capi import CSegmentsOut
    lib = ctypes.CDLL(la.LIB_PATH)
    fn = lib.lg_closest_segments
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p]
    dev = lib.lg_closest_segments_device
    dev.restype, dev.argtypes = ctypes.c_int, fn.argtypes + [ctypes.c_void_p]
    lib.lg_last_error.restype = ctypes.c_char_p
    segs = np.zeros((4, 6))
    d = np.full(4 * 4, 7.0)
    out = CSegmentsOut(None, d.ctypes.data, None, None, None)
    none = CSegmentsOut(None, None, None, None, None)
    fake = ctypes.c_void_p(0x1000)  # an accel that is never looked at: each of these is refused before it would be
    P, O = segs.ctypes.data, ctypes.addressof(out)
    assert fn(None, None, None, 0, -1.0, None) == 0 and dev(None, None, None, 0, float("nan"), None, None) == 0, "n == 0 is answered before every other check"
    for args, what in (((None, P, None, 4, 1.0, O), "accel is NULL"), ((fake, None, None, 4, 1.0, O), "segments is NULL"), ((fake, P, None, 4, 1.0, None), "out is NULL"),
                       ((fake, P, None, 4, 1.0, ctypes.addressof(none)), "every plane of out is NULL"), ((fake, P, None, 4, -1.0, O), "radius is NaN or negative"),
                       ((fake, P, None, 4, float("nan"), O), "radius is NaN or negative"),
                       ((fake, P, P, (2 ** 32 - 1) * 64 + 1, -1.0, O), "too many segments"),  # (with radii a bad shared radius is not an error: the next one is named)
                       ((fake, P, None, (2 ** 32 - 1) * 64 + 1, 1.0, O), "too many segments")):
        assert fn(*args) != 0 and what in lib.lg_last_error().decode(), (what, lib.lg_last_error())
        assert dev(*args, None) != 0 and what in lib.lg_last_error().decode(), (what, lib.lg_last_error())
    assert dev(fake, ctypes.c_void_p(P + 4), None, 4, 1.0, O, None) != 0 and "segments is not 8-byte aligned" in lib.lg_last_error().decode()
    assert dev(fake, P, ctypes.c_void_p(P + 4), 4, 1.0, O, None) != 0 and "radii is not 8-byte aligned" in lib.lg_last_error().decode()
    bad_id = CSegmentsOut(None, None, None, None, d.ctypes.data + 8)
    assert dev(fake, P, None, 4, 1.0, ctypes.addressof(bad_id), None) != 0 and "id is not 16-byte aligned" in lib.lg_last_error().decode()
    bad_param = CSegmentsOut(None, None, d.ctypes.data + 4, None, None)
    assert dev(fake, P, None, 4, 1.0, ctypes.addressof(bad_param), None) != 0 and "param is not 8-byte aligned" in lib.lg_last_error().decode()
    assert (d == 7.0).all()
    with pytest.raises(ValueError):
        la.api.closest_segments(None, np.zeros((4, 3)))
    with pytest.raises(ValueError):
        la.api.closest_segments(None, np.zeros((4, 6)), planes=("distance", "count"))
    with pytest.raises(ValueError):
        la.api.closest_segments(None, np.zeros((4, 6)), radii=np.zeros(3))
    with pytest.raises(ValueError, match="no array for the plane 'param'"):
        la.api.closest_segments(None, np.zeros((4, 6)), planes=("touch", "param"), into={"touch": np.zeros(4, dtype=np.uint8)})
    with pytest.raises(ValueError):
        la.api.capsules_touching(None, np.zeros((4, 3)), np.zeros((3, 3)), 1.0)
