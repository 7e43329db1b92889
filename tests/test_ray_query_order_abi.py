"""The opt-in ray order of ray queries (include/lasgun_hip.h: lg_accel_set_query_order, lg_accel_get_query_order, lg_query_order,
lg_query_order_device) through every layer that has to carry it, checked without a GPU: the built library exports the four symbols,
the header declares them, and the Python, C++ and Rust bindings mirror them."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("lg_accel_set_query_order", "lg_accel_get_query_order", "lg_query_order", "lg_query_order_device")
ARITY = {"lg_accel_set_query_order": 2, "lg_accel_get_query_order": 1, "lg_query_order": 5, "lg_query_order_device": 6}


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_built_library_exports_the_four_symbols():
    import lasgun_amd as la
    lib = ctypes.CDLL(la.LIB_PATH)
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_the_header_declares_them():
    import gen_rust_sys
    decl = {name: (ret, params) for ret, name, params in gen_rust_sys.declarations(read("include", "lasgun_hip.h"))}
    for name in NAMES:
        assert name in decl, name
        ret, params = decl[name]
        assert ret == "int" and len(params) == ARITY[name], (name, ret, params)
        assert "lg_accel" in params[0] and "const" in params[0], (name, params[0])
    assert [p.split()[-1].lstrip("*") for p in decl["lg_query_order_device"][1][1:]] == ["dev_rays", "n", "dev_perm", "dev_keys", "hip_stream"]
    assert all("uint32_t" in p for p in decl["lg_query_order"][1][3:5])


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.QUERY_ORDER_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    for wrapper in ("set_query_order", "get_query_order", "query_order", "query_order_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    src = read("lasgun_amd", "_capi.py")
    for key in sigs:
        assert '"%s"' % key in src, key


def test_the_cpp_wrapper_calls_them():
    src = read("include", "lasgun.hpp")
    for name in ("lg_accel_set_query_order", "lg_accel_get_query_order", "lg_query_order"):
        assert re.search(r"\b%s\(" % name, src), name
    assert "void set_query_order(int order) const" in src


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    for fn in ("set_query_order", "get_query_order", "query_order", "query_order_device"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, safe), fn
