"""Ray films and lens rays (include/lasgun_hip.h: lg_capture_rays, lg_capture_rays_device, lg_lens_rays, lg_lens_rays_device) through every
layer that has to carry them, checked without a GPU: the built library exports the symbols, the header declares them with the arity the
wrappers use, lg_lens is 112 bytes without padding, and the Python, C++ and Rust bindings mirror them."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_capture_rays": 9, "lg_capture_rays_device": 10, "lg_lens_rays": 7, "lg_lens_rays_device": 9}
NAMES = tuple(ARITY)


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_built_library_exports_the_symbols():
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
    names = lambda key: [p.split()[-1].lstrip("*") for p in decl[key][1]]  # noqa: E731
    assert names("lg_capture_rays")[1:] == ["rays", "pixels", "samples", "pixel_offsets", "film", "rgb", "width", "height"]
    assert names("lg_capture_rays_device")[1:] == ["dev_rays", "pixels", "samples", "dev_pixel_offsets", "width", "height", "dev_rgba", "dev_rgb", "hip_stream"]
    assert names("lg_lens_rays")[1:] == ["width", "height", "samples_root", "pixel_offsets", "pixels", "rays"]
    assert names("lg_lens_rays_device")[0] == "device" and names("lg_lens_rays_device")[-2:] == ["dev_rays", "hip_stream"]
    for key in ("lg_capture_rays", "lg_capture_rays_device"):
        assert "lg_accel" in decl[key][1][0] and "const" in decl[key][1][0]
    assert re.search(r"32\s+LIGHTS", header[header.index("Ray films"):], flags=re.I)
    assert "EXTRA" in header[header.index("Lens rays"):], "the lens cameras have no counterpart in the reference, and the header says so"


def test_lg_lens_is_112_bytes_without_padding():
    import lasgun_amd as la
    from lasgun_amd import _capi
    L = _capi.CLens
    assert ctypes.sizeof(L) == 112
    assert sum(ctypes.sizeof(t) for _, t in L._fields_) == 112  # no padding
    assert [(n, getattr(L, n).offset) for n, _ in L._fields_] == [("kind", 0), ("reserved", 4), ("origin", 8), ("right", 32), ("up", 56), ("forward", 80),
                                                                  ("fov_deg", 104)]
    m = re.search(r"typedef struct lg_lens \{(.*?)\} lg_lens;", read("include", "lasgun_hip.h"), flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t kind; int32_t reserved; double origin[3], right[3], up[3], forward[3]; double fov_deg;"
    assert re.search(r"sizeof\(lg_lens\) == 112", read("lasgun_amd", "csrc", "query.cpp")), "the library asserts the layout it reads"
    lens = la.Lens(la.LENS_FISHEYE, (1, 2, 3), (1, 0, 0), (0, 1, 0), (0, 0, -1), 150.0)
    assert (lens.kind, lens.reserved, tuple(lens.origin), tuple(lens.forward), lens.fov_deg) == (1, 0, (1.0, 2.0, 3.0), (0.0, 0.0, -1.0), 150.0)


def test_capi_and_the_python_wrappers_mirror_them():
    import numpy as np
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.RAY_FILM_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    for wrapper in ("capture_rays", "capture_rays_device", "lens_rays", "lens_rays_device", "capture_lens"):
        assert callable(getattr(la.api, wrapper)), wrapper
    offs = la.tile_order_offsets(20, 12)
    assert offs.dtype == np.uint64 and sorted(offs.tolist()) == list(range(240))
    assert offs[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 20] and offs[64] == 8 and offs[128] == 16 and offs[128 + 4] == 36  # (the last tile column is 4 wide)


def test_the_cpp_wrapper_calls_them():
    src = read("include", "lasgun.hpp")
    for name in ("lg_capture_rays", "lg_lens_rays"):
        assert re.search(r"\b%s\(" % name, src), name
    assert re.search(r"\bcapture_rays\(", src) and re.search(r"struct Lens\b", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    assert re.search(r"pub struct lg_lens \{", sys_src)
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    for fn in ("capture_rays", "capture_rays_device", "lens_rays", "lens_rays_device"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, safe), fn


def test_the_film_forms_are_device_kernels_of_their_own():
    """The film forms of level 0, the resolve pass and the lens rays are HIP kernels the library launches; nothing sums or quantises on the host."""
    src = read("lasgun_amd", "csrc", "k_radiance.hip")
    for kernel in ("rf_closest_kernel", "rf_shade_kernel", "rf_combine_kernel", "rf_resolve_kernel"):
        assert re.search(r"__global__ void [^\n]*\b%s\(" % kernel, src), kernel
    assert re.search(r"__global__ void [^\n]*\blens_rays_kernel\(", read("lasgun_amd", "csrc", "k_lens.hip"))
    assert "k_lens.o" in read("lasgun_amd", "csrc", "Makefile")
