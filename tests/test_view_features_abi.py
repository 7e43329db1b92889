"""View features (include/lasgun_hip.h: lg_view_features, lg_capture_view_features, lg_capture_view_features_device) through every layer
that has to carry them, checked without a GPU: the built library exports the two symbols, the header declares them with the arities,
names and types the wrappers use, beside the views section, and states the contract -- the addressing, "written exactly once", the point
rule, the 32-bit tile limit, the 2^32 - 8 rule, "nothing is shaded" --, lg_view_features is 48 bytes in every mirror, the kernel is a HIP
kernel of its own in the build, and the errors that need no HIP call are refused on this machine."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_capture_view_features": 7, "lg_capture_view_features_device": 8}
NAMES = tuple(ARITY)
MEMBERS = [("float", "depth"), ("float", "normal"), ("float", "albedo"), ("float", "coverage"), ("uint32_t", "id"), ("float", "point")]


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
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    assert names("lg_capture_view_features")[1:] == ["views", "n_views", "width", "height", "out", "material_rgb"]
    assert names("lg_capture_view_features_device")[1:] == ["views", "n_views", "width", "height", "dev_out", "dev_material_rgb", "hip_stream"]
    host = ["const lg_view *", "size_t", "uint32_t", "uint32_t", "const lg_view_features *", "const double *"]
    assert types("lg_capture_view_features")[1:] == host and types("lg_capture_view_features_device")[1:] == host + ["void *"]
    assert "lg_accel" in decl[NAMES[0]][1][0] and "const" in decl[NAMES[0]][1][0]
    # an EXTRA beside the views section: after lg_capture_views_device, before lg_accel_set_query_order
    order = ["int lg_capture_views_device(", "typedef struct lg_view_features {", "int lg_capture_view_features(", "int lg_capture_view_features_device(",
             "int lg_accel_set_query_order("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), order
    struct = re.search(r"typedef struct lg_view_features \{(.*?)\} lg_view_features;", header, flags=re.S).group(1)
    assert re.findall(r"^\s*(float|uint32_t)\s*\*(\w+);", struct, flags=re.M) == MEMBERS
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header[header.index("/* View features:"):header.index("int lg_capture_view_features(")]))
    assert "An EXTRA: no counterpart in the reference" in text and "48 bytes; each pointer may be NULL, all NULL is an error" in text
    assert "always a host struct" in text
    assert "v*width*height + y*width + x" in text and "there is no rectangle" in text
    assert "Every pixel of every requested plane is written exactly once" in text and "nothing outside n_views*width*height elements is touched" in text
    assert "a plane that is not requested is not touched" in text
    assert "lg_view_rays' rays for view v and that pixel, s = 0 .. S-1 in camera order" in text and "spelled out under lg_capture_views" in text
    assert "what lg_intersect returns for that ray, bit for bit" in text and "lg_accel_set_query_order plays no part" in text
    assert "lg_capture_features' accumulators, order and roundings word for word" in text and "inv = 1.0 / (double)S" in text
    assert "+INFINITY where there are none" in text and "id sample 0's" in text
    assert "these five planes are lg_capture_features' bytes for the full film" in text
    assert "psum[3] starts at +0.0" in text and "a hit adds lg_hit::p per component" in text
    assert "point[c] = nhit ? (float)(psum[c] * (1.0 / (double)nhit)) : 0.0f" in text and "lg_hit's zeros on a miss" in text, "the point rule"
    assert "views is a HOST array in both forms" in text and "pinned staging" in text
    assert "an error on the way leaves them as they were" in text and "it only enqueues on hip_stream" in text and "one stream at a time per accel" in text
    assert "n_views == 0 is a successful no-op, answered before every other check" in text
    assert "a NULL accel, views or out" in text and "all six planes NULL" in text and "albedo without material_rgb" in text
    assert "above 2^32 - 8" in text and "a samples_root of 0 or above 256" in text and "reserved != 0" in text and "uniform-samples rule" in text
    assert "n_views * ceil(width/8) * ceil(height/8) > 2^32 - 1" in text and "counted in 32 bits" in text, "the 32-bit tile limit"
    assert "SIZE_MAX" in text and "id 16-byte aligned, material_rgb 8, the float planes 4" in text and "ends beyond its allocation" in text
    assert "More than 32 lights or a deep recursion is NOT an error here: nothing is shaded" in text


def test_lg_view_features_is_48_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    assert la.CViewFeatures is _capi.CViewFeatures and ctypes.sizeof(_capi.CViewFeatures) == 48
    assert [f[0] for f in _capi.CViewFeatures._fields_] == list(la.VIEW_FEATURE_PLANES) == [m[1] for m in MEMBERS]
    assert la.VIEW_FEATURE_PLANES[:5] == la.FEATURE_PLANES
    host = read("lasgun_amd", "csrc", "view_features_host.h")
    assert "static_assert(sizeof(lg_view_features) == 48" in host and "offsetof(lg_view_features, point) == 40" in host  # the library's own build
    assert "static_assert(sizeof(lg_view_features) == 48" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    body = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_view_features \{(.*?)\}", sys_src, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): \*mut (\w+),", body) == [(n, "u32" if t == "uint32_t" else "f32") for t, n in MEMBERS]
    assert "std::mem::size_of::<sys::lg_view_features>() == 48" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_wrappers_mirror_them():
    import gen_rust_sys
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.VIEW_FEATURES_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert argtypes[2] is ctypes.c_size_t and argtypes[3] is ctypes.c_uint32 and argtypes[4] is ctypes.c_uint32, key
        assert key in la.api._fn, key  # bound to the built library at import
    for wrapper in ("capture_view_features", "capture_view_features_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.view_features), "accel.view_features(views, w, h, planes=..., material_rgb=None)"
    hpp = read("include", "lasgun.hpp")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hpp), name
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"void capture_view_features\(", hpp) and re.search(r"void capture_view_features_device\(", hpp)
    assert re.search(r"pub fn capture_view_features\(", safe) and re.search(r"pub unsafe fn capture_view_features_device\(", safe)
    assert "lg_view_features" in gen_rust_sys.STRUCTS
    assert "NOT compiled" in read("bindings", "rust", "README.md")


def test_the_kernel_is_a_device_kernel_of_its_own():
    """The rays are made and walked in a HIP kernel the library launches: features_kernel's body over view_ray's rays, the view's record
    read once per tile through a wave-uniform index; the ray expression is ONE text that k_views.hip shares; no atomics."""
    src = read("lasgun_amd", "csrc", "k_view_features.hip")
    assert re.search(r"__global__ void [^\n]*\bview_features_kernel\(", src)
    assert len(re.findall(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", src)) == 1, "one walk, closest hit"
    assert "claim_tile(" in src and "claim_tile_single(" in src and "shade_frame(" in src and "copy_to_lds(" in src and "load_accel_image(" in src and "Q.tri_base[" in src
    assert "view_pixel(V, G, lane)" in src and "view_ray(P, view, px.x, px.y, s)" in src and "__builtin_amdgcn_readfirstlane" in src
    tile_loop = src[src.index("if (tile == NO_TILE) break;"):src.index("for (uint32_t s = 0u; s < S; ++s)")]
    assert tile_loop.count("view_load(") == 1 and src.count("view_load(") == 1, "the record is loaded once per tile, outside the sample loop"
    assert "psum = psum + sh.praw" in src and "trav_launch<ViewFeatureKernels>" in src
    assert "atomic" not in src.replace("claim_tile", ""), "the sums need no cross-lane or cross-wave step"
    assert '#include "view_ray.h"' in src and '#include "view_ray.h"' in read("lasgun_amd", "csrc", "k_views.hip")
    shared = read("lasgun_amd", "csrc", "view_ray.h")
    for fn in ("ViewPixel view_pixel(", "DView view_load(", "Ray view_ray("):
        assert fn in shared and fn not in src and fn not in read("lasgun_amd", "csrc", "k_views.hip"), fn
    make = read("lasgun_amd", "csrc", "Makefile")
    kobjs = re.search(r"^KOBJS = (.*)$", make, flags=re.M).group(1).split()
    assert "k_view_features.o" in kobjs and "view_ray.h" in make and "view_features_host.h" in make
    assert "view_features_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    host = read("lasgun_amd", "csrc", "query.cpp")
    assert host.index("// ---- feature buffers") < host.index("// ---- view features") < host.index("// ---- lens rays")
    body = host[host.index("static void enqueue_view_features("):host.index('extern "C" int lg_capture_view_features(')]
    assert "base_params(a, w, h)" in body and "P.ss_root = shape.samples_root" in body and "P.ntiles = shape.pixel_tiles" in body
    assert body.index("stage_view_table(") < body.index("traversal_grid(a, P, view_features_occupancy") < body.index("launch_view_features(") < body.index("subsets_enqueued(")
    assert body.count("launch_view_features(") == 1 and "subsets_abandoned(" in body, "one launch, no chunks"
    assert "launch_query(" not in body and "launch_camera_rays(" not in body and "radiance_possible(" not in host[host.index("// ---- view features"):host.index("// ---- lens rays")]
    assert "live_table(c)" in read("lasgun_amd", "csrc", "launch.cpp").split("const DView *stage_view_table(")[1].split("\n}\n")[0]


def test_errors_before_any_hip_call_and_the_empty_batch():
    import lasgun_amd as la
    G = la.api
    good = la.view_look_at((-6.0, 3.0, 5.0), (0.5, -0.3, 0.0), (0.0, 1.0, 0.1), fov=65.0)
    t = (la.View * 2)(good, good)
    bufs = {p: np.full(2 * 4 * 4 * 4, 0xA5A5A5A5, dtype=np.uint32) for p in la.VIEW_FEATURE_PLANES}
    table = np.full(3, -7.0)
    f = la.CViewFeatures(*[bufs[p].ctypes.data for p in la.VIEW_FEATURE_PLANES])
    none = la.CViewFeatures()
    adr = ctypes.addressof
    fake = ctypes.c_void_p(1)  # (never looked behind: every case below is refused before the accel is touched)
    for fn, tail in (("capture_view_features", ()), ("capture_view_features_device", (None,))):
        call = lambda acc, views, k, w, h, out=adr(f), tab=table.ctypes.data: G.call(fn, acc, views, k, w, h, out, tab, *tail)  # noqa: E731
        assert call(None, adr(t), 2, 4, 4) != 0 and "accel is NULL" in G.last_error(), fn
        assert call(fake, None, 2, 4, 4) != 0 and "views is NULL" in G.last_error(), fn
        assert call(fake, adr(t), 2, 4, 4, None) != 0 and "out is NULL" in G.last_error(), fn
        assert call(fake, adr(t), 2, 4, 4, adr(none)) != 0 and "every plane of out is NULL" in G.last_error(), fn
        assert call(fake, adr(t), 2, 4, 4, adr(f), None) != 0 and "material_rgb is NULL" in G.last_error(), fn
        assert call(fake, adr(t), 2, 0, 4) != 0 and G.last_error() and call(fake, adr(t), 2, 4, 0) != 0 and G.last_error(), fn
        assert call(fake, adr(t), 1, 0xFFFFFFF9, 1) != 0 and "2^32 - 8" in G.last_error() and call(fake, adr(t), 1, 1, 0xFFFFFFFF) != 0 and "2^32 - 8" in G.last_error(), fn
        for field, value, word in (("samples_root", 0, "samples_root"), ("samples_root", 257, "samples_root"), ("reserved", 7, "reserved"), ("samples_root", 3, "differs")):
            bad = (la.View * 2)(good, good)
            setattr(bad[1], field, value)
            assert call(fake, adr(bad), 2, 4, 4) != 0 and word in G.last_error(), (fn, field, value)
        four = (la.View * 4)(good, good, good, good)
        assert call(fake, adr(four), 4, 1 << 18, 1 << 18) != 0 and "32 bits" in G.last_error(), fn  # 2^32 pixel tiles: one above the limit
        assert call(fake, adr(t), 1 << 62, 8, 8) != 0 and G.last_error(), fn                          # no table is that long, no plane that large
        # n_views == 0: a successful no-op, answered before every other check
        assert call(None, None, 0, 0, 0, None, None) == 0 and call(fake, adr(t), 0, 4, 4) == 0 and call(None, adr(t), 0, 4, 4, adr(none)) == 0, fn
    # the device form's alignment rule needs no HIP call either
    for p, shift in (("id", 4), ("id", 8), ("depth", 2), ("normal", 1), ("albedo", 2), ("coverage", 3), ("point", 2)):
        g = la.CViewFeatures(*[bufs[q].ctypes.data + (shift if q == p else 0) for q in la.VIEW_FEATURE_PLANES])
        assert G.call("capture_view_features_device", fake, adr(t), 2, 4, 4, adr(g), table.ctypes.data, None) != 0 and ("%s is not" % p) in G.last_error(), p
    assert G.call("capture_view_features_device", fake, adr(t), 2, 4, 4, adr(f), table.ctypes.data + 4, None) != 0 and "material_rgb is not 8-byte aligned" in G.last_error()
    assert all((b == 0xA5A5A5A5).all() for b in bufs.values()) and (table == -7.0).all(), "an error or an empty batch touched an output"
    for views in ([good, 3], "nonsense"):
        try:
            G.capture_view_features(None, views, 4, 4)
        except (TypeError, AttributeError):
            continue
        raise AssertionError("capture_view_features takes View records")
    try:
        G.capture_view_features(None, [good], 4, 4, planes=("depth", "colour"))
    except ValueError:
        pass
    else:
        raise AssertionError("planes: any of VIEW_FEATURE_PLANES")
