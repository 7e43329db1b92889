"""Feature buffers (include/lasgun_hip.h: lg_capture_features, lg_capture_features_device, lg_accel_material_count) through every layer
that has to carry them, checked without a GPU: the built library exports the symbols, the header declares them with the arity, the
parameter names and the types the wrappers use, lg_features is 40 bytes, the header states the contract (the accumulation order,
"premultiplied", the depth rule, "never touched"), the kernel is a HIP kernel of its own in the build, and the Python, C++ and Rust
bindings mirror the entry points."""
import ctypes
import os
import re
import sys
import tilewalk_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_capture_features": 9, "lg_capture_features_device": 10, "lg_accel_material_count": 1}
NAMES = tuple(ARITY)


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_built_library_exports_the_symbols():
    import lasgun_amd as la
    lib = ctypes.CDLL(la.LIB_PATH)
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    lib.lg_accel_material_count.restype, lib.lg_accel_material_count.argtypes = ctypes.c_size_t, [ctypes.c_void_p]
    assert lib.lg_accel_material_count(None) == 0  # (needs no device)


def test_the_header_declares_them_and_states_the_contract():
    import gen_rust_sys
    header = read("include", "lasgun_hip.h")
    decl = {name: (ret, params) for ret, name, params in gen_rust_sys.declarations(header)}
    for name in NAMES:
        assert name in decl, name
        ret, params = decl[name]
        assert ret == ("size_t" if name == "lg_accel_material_count" else "int") and len(params) == ARITY[name], (name, ret, params)
        assert "lg_accel" in params[0] and "const" in params[0]
    names = lambda key: [p.split()[-1].lstrip("*") for p in decl[key][1]]  # noqa: E731
    rect = ["width", "height", "x0", "y0", "x1", "y1"]
    assert names("lg_capture_features")[1:] == rect + ["out", "material_rgb"]
    assert names("lg_capture_features_device")[1:] == rect + ["dev_out", "dev_material_rgb", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    assert types("lg_capture_features")[1:] == ["uint32_t"] * 6 + ["const lg_features *", "const double *"]
    assert types("lg_capture_features_device")[1:] == ["uint32_t"] * 6 + ["const lg_features *", "const double *", "void *"]
    # among the extras, after the ray films and before the lens rays
    assert header.index("EXTRAS") < header.index("lg_capture_rays_device(") < header.index("typedef struct lg_features") \
        < header.index("lg_capture_features(") < header.index("lg_capture_features_device(") < header.index("typedef struct lg_lens")
    struct = re.search(r"typedef struct lg_features \{(.*?)\} lg_features;", header, flags=re.S).group(1)
    members = re.findall(r"^\s*(float|uint32_t)\s*\*(\w+);", struct, flags=re.M)
    assert members == [("float", "depth"), ("float", "normal"), ("float", "albedo"), ("float", "coverage"), ("uint32_t", "id")]
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("Feature buffers:"):header.index("size_t lg_accel_material_count(")])
    assert "tsum, nsum[3] and asum[3] start at +0.0" in text and "For s ascending, a hit adds t to tsum" in text, "the accumulation order"
    assert "material_rgb[3*material + c] to asum[c]" in text and "A miss adds nothing" in text
    assert "premultiplied by coverage" in text
    assert "depth = nhit ? (float)(tsum * (1.0 / (double)nhit)) : +INFINITY" in text, "the depth rule"
    assert "normal[c] = (float)(nsum[c] * inv)" in text and "coverage = (float)((double)nhit * inv)" in text and "inv = 1.0 / (double)S" in text
    assert "never touched" in text and "pixel y*width + x" in text
    assert "lg_accel_set_query_order plays no part" in text and "bit for bit" in text
    assert "kind != 0" in text and "(0, ~0, ~0, -1 on a miss)" in text and "one 16-byte store" in text
    assert "2^32 - 1" in text and "lg_capture_rect's rule" in text and "An empty rectangle is a successful no-op" in text
    assert "id 16-byte aligned, material_rgb 8, the float planes 4" in text
    assert "required iff albedo is requested" in text and "outside 0 .. count-1 adds nothing" in text


def test_lg_features_is_forty_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    assert ctypes.sizeof(_capi.CFeatures) == 40 and [f[0] for f in _capi.CFeatures._fields_] == list(la.FEATURE_PLANES)
    assert "sizeof(lg_features) == 40" in read("lasgun_amd", "csrc", "features_host.h")  # a static_assert of the library's own build
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    body = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_features \{(.*?)\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): \*mut (\w+),", body) == [("depth", "f32"), ("normal", "f32"), ("albedo", "f32"), ("coverage", "f32"), ("id", "u32")]


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.FEATURES_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is (ctypes.c_size_t if key == "accel_material_count" else ctypes.c_int) and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    assert sigs["capture_features"][1][1:7] == [ctypes.c_uint32] * 6
    for wrapper in ("capture_features", "capture_features_device", "material_count", "default_albedo_table"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.features), "accel.features(w, h, rect=None, planes=..., material_rgb=None)"
    assert "convention of this WRAPPER, not of the C contract" in la.api.default_albedo_table.__doc__


def test_the_cpp_wrapper_calls_them():
    src = read("include", "lasgun.hpp")
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, src), name
    assert re.search(r"void capture_features\(", src) and re.search(r"void capture_features_device\(", src) and re.search(r"size_t material_count\(\)", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    for fn in ("capture_features", "capture_features_device", "material_count"):
        assert re.search(r"pub (unsafe )?fn %s\(" % fn, safe), fn


def test_the_kernel_is_a_device_kernel_of_its_own():
    """The rays are made and walked in a HIP kernel the library launches, through the render's walk in its closest-hit form, a pixel per lane
    and its samples in a loop; nothing writes rays or lg_hit records on the way, and walk.h is not what changed."""
    src = read("lasgun_amd", "csrc", "k_features.hip")
    assert re.search(r"__global__ void [^\n]*\bfeatures_kernel\(", src)
    assert re.search(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", src)
    tilewalk_text.over_tilewalk(src)  # the claim, the LDS copy, the accel records and the id word: the shared header's
    assert "pixel_of(P, tile, lane)" in src and "camera_ray(P, px.x, px.y, s)" in src
    assert "shade_frame(" in src and "id0 = hit_id(b, sh, Q.tri_base);" in src and "uint4 id0 = hit_id_none();" in src
    assert "atomic" not in src, "the sums need no cross-lane or cross-wave step"
    assert "k_features.o" in read("lasgun_amd", "csrc", "Makefile")
    host = read("lasgun_amd", "csrc", "query.cpp")
    body = host[host.index("static void enqueue_features("):host.index('extern "C" int lg_capture_features(')]
    assert "set_rect(P, x0, y0, x1, y1)" in body and "P.out_row0 = y0; P.out_x0 = x0; P.out_pitch = x1 - x0;" in body
    grid = host[host.index("static TraversalGrid traversal_grid("):host.index("static void enqueue_query(")]  # the one place that sizes a query-style launch
    assert "hipMemsetAsync(c.tile_counter.p, 0," in grid and body.index("traversal_grid(") < body.index("launch_features(")
    assert "launch_query(" not in body and "launch_camera_rays(" not in body
