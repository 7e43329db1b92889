"""Radiance queries (include/lasgun_hip.h: lg_radiance, lg_radiance_device) through every layer that has to carry them, checked without a
GPU: the built library exports the two symbols, the header declares them, and the Python, C++ and Rust bindings mirror them."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("lg_radiance", "lg_radiance_device")
ARITY = {"lg_radiance": 4, "lg_radiance_device": 5}


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_built_library_exports_both_symbols():
    import lasgun_amd as la
    lib = ctypes.CDLL(la.LIB_PATH)
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_the_header_declares_them():
    import gen_rust_sys
    header = read("include", "lasgun_hip.h")
    decl = {name: (ret, params) for ret, name, params in gen_rust_sys.declarations(header)}
    for name in NAMES:
        assert name in decl, name
        ret, params = decl[name]
        assert ret == "int" and len(params) == ARITY[name], (name, ret, params)
        assert "lg_accel" in params[0] and "const" in params[0], (name, params[0])
    assert [p.split()[-1].lstrip("*") for p in decl["lg_radiance"][1][1:]] == ["rays", "n", "radiance"]
    assert [p.split()[-1].lstrip("*") for p in decl["lg_radiance_device"][1][1:]] == ["dev_rays", "n", "dev_radiance", "hip_stream"]
    assert "const double" in decl["lg_radiance"][1][1] and "const" not in decl["lg_radiance"][1][3]
    assert re.search(r"32\s+LIGHTS", header, flags=re.I), "the header says what the 32-bit visibility word means for a query"


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.RADIANCE_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    for wrapper in ("radiance", "radiance_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    src = read("lasgun_amd", "_capi.py")
    for key in sigs:
        assert '"%s"' % key in src, key


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_radiance\(", src)
    assert re.search(r"std::vector<std::array<double, 3>> radiance\(const std::vector<std::array<double, 6>> &rays\) const", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    for fn in ("radiance", "radiance_device"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, safe), fn


def test_no_host_path_answers_without_the_device_kernels():
    """The query's level 0 is device code of its own: the library carries its kernels' launchers and nothing that shades on the host."""
    src = read("lasgun_amd", "csrc", "k_radiance.hip")
    for kernel in ("rq_closest_kernel", "rq_shade_kernel", "rq_combine_kernel"):
        assert re.search(r"__global__ void [^\n]*\b%s\(" % kernel, src), kernel
    assert "k_radiance.o" in read("lasgun_amd", "csrc", "Makefile")
