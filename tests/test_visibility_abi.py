"""Visibility matrices (include/lasgun_hip.h: lg_visibility, lg_visibility_device) through every layer that has to carry them, checked
without a GPU: the built library exports the symbols, the header declares them with the arity and the parameter names the wrappers use and
states the bit order and the "written, not accumulated" rule, the kernel is a HIP kernel of its own in the build, and the Python, C++ and
Rust bindings mirror the entry points."""
import ctypes
import os
import re
import sys
import tilewalk_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_visibility": 8, "lg_visibility_device": 9}
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
    assert names("lg_visibility")[1:] == ["from", "n_from", "to", "n_to", "bits", "row_bytes", "blocked"]
    assert names("lg_visibility_device")[1:] == ["dev_from", "n_from", "dev_to", "n_to", "dev_bits", "row_bytes", "dev_blocked", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    assert types("lg_visibility")[1:] == ["const double *", "size_t", "const double *", "size_t", "uint8_t *", "size_t", "uint32_t *"]
    assert types("lg_visibility_device")[1:] == ["const double *", "size_t", "const double *", "size_t", "uint8_t *", "size_t", "uint32_t *", "void *"]
    # beside lg_occluded*, among the extras
    assert header.index("EXTRAS") < header.index("lg_occluded_device(") < header.index("lg_visibility(") < header.index("lg_radiance(")
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("Visibility matrices"):header.index("int lg_visibility(")])
    assert "(bits[i*row_bytes + (j >> 3)] >> (j & 7)) & 1" in text, "the bit order"
    assert 'packbits(..., bitorder="little")' in text
    assert re.search(r"written,? not accumulated", text, flags=re.I), "blocked is written, not accumulated"
    assert "padding bits" in text and "never touched" in text
    assert "lg_accel_set_query_order plays no part" in text
    assert re.search(r"neighbours in the array are neighbours in space", text)
    assert "2^32 - 1" in text and "both NULL is an error" in text


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.VISIBILITY_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    assert [a for a in sigs["visibility"][1] if a is ctypes.c_size_t] == [ctypes.c_size_t] * 3
    for wrapper in ("visibility", "visibility_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.visibility), "accel.visibility(from_pts, to_pts, counts=False)"


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_visibility\(", src)
    assert re.search(r"std::vector<uint8_t> visibility\(", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    for fn in ("visibility", "visibility_device"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, safe), fn


def test_the_kernel_is_a_device_kernel_of_its_own():
    """The segments are made and walked in a HIP kernel the library launches, through the render's walk in its any-hit form, and the count
    buffer is zeroed on the caller's stream ahead of it; nothing expands the matrix into rays on the host."""
    src = read("lasgun_amd", "csrc", "k_visibility.hip")
    assert re.search(r"__global__ void [^\n]*\bvisibility_kernel\(", src)
    assert re.search(r"walk<LDSS, FAST, PRUNE>\(P, ray, true,", src)
    tilewalk_text.over_tilewalk(src)
    assert "__builtin_amdgcn_ballot_w64(" in src
    assert "k_visibility.o" in read("lasgun_amd", "csrc", "Makefile")
    host = read("lasgun_amd", "csrc", "query.cpp")
    body = host[host.index("static void enqueue_visibility("):host.index('extern "C" int lg_visibility(')]
    assert body.index("hipMemsetAsync(blocked, 0,") < body.index("launch_visibility(")
    assert "lg_occluded" not in body and "launch_query(" not in body
