"""Views (include/lasgun_hip.h: lg_view, lg_view_look_at, lg_scene_view, lg_accel_view, lg_view_rays*, lg_capture_views*) through every
layer that has to carry them, checked without a GPU: the built library exports the seven symbols, the header declares them with the arities
and types the wrappers use, between lg_lens_rays_device and lg_accel_set_query_order, and states the contract -- the ray expression,
"written exactly once", the 32-bit tile limit, the uniform-samples rule --, lg_view is 120 bytes in every mirror, the kernels are HIP
kernels of their own in the build.  On top: lg_view_look_at against lg_scene_view of a scene given the same three calls, byte for byte, and
against a numpy restatement of look_at; the errors that are answered before any HIP call and the no-op of n_views == 0; the wrapper's two
conventions against their formulas."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_view_look_at": 7, "lg_scene_view": 2, "lg_accel_view": 2, "lg_view_rays": 9, "lg_view_rays_device": 10, "lg_capture_views": 7,
         "lg_capture_views_device": 8}
NAMES = tuple(ARITY)
# every camera of SECOND (four scenes, three each) in tests/test_gpu_radiance_query.py (that file imports the GPU suite's helpers; the values are restated here and
# compared with it where it can be imported)
CAMERAS = [("perspective", 65.0, (-6.0, 3.0, 5.0), (0.5, -0.3, 0.0), (0.0, 1.0, 0.1)), ("orthographic", 5.5, (3.0, 3.0, 8.0), (0.0, -0.5, 0.5), (0.0, 1.0, 0.0)),
           ("perspective", 80.0, (0.9, -0.2, 0.9), (-2.2, -0.4, 0.5), (0.0, 1.0, 0.0)), ("perspective", 60.0, (2.0, 0.8, 6.0), (0.0, -0.5, 0.0), (0.0, 1.0, 0.0)),
           ("orthographic", 3.0, (0.5, 0.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ("perspective", 95.0, (-0.3, 0.2, -1.5), (0.8, -1.0, 3.0), (0.0, 1.0, 0.0)),
           ("perspective", 50.0, (-500.0, 200.0, 600.0), (0.0, 0.0, -200.0), (0.0, 1.0, 0.0)), ("orthographic", 900.0, (300.0, 300.0, 800.0), (0.0, 0.0, -200.0), (0.0, 1.0, 0.0)),
           ("perspective", 90.0, (20.0, 30.0, -180.0), (200.0, 50.0, -100.0), (0.0, 1.0, 0.0)), ("perspective", 60.0, (6.0, 2.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
           ("orthographic", 9.0, (-3.0, 5.0, 8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ("perspective", 85.0, (0.3, 0.2, 0.5), (2.0, 0.0, -2.0), (0.0, 1.0, 0.0))]


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def look_at_view(la, cam, supersampling=0):
    kind, par, eye, look, up = cam
    return la.view_look_at(eye, look, up, supersampling=supersampling, **({"scale": par} if kind == "orthographic" else {"fov": par}))


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
    types = lambda key: [re.sub(r"\s*\w+(\[3\])?$", r"\1", p).strip() for p in decl[key][1]]  # noqa: E731
    assert types("lg_view_look_at") == ["lg_view *", "int", "double", "const double[3]", "const double[3]", "const double[3]", "uint8_t"]
    assert types("lg_scene_view") == ["const lg_scene *", "lg_view *"] and types("lg_accel_view") == ["const lg_accel *", "lg_view *"]
    rect = ["const lg_accel *", "const lg_view *"] + ["uint32_t"] * 6 + ["double *"]
    assert types("lg_view_rays") == rect and types("lg_view_rays_device") == rect + ["void *"]
    assert types("lg_capture_views") == ["const lg_accel *", "const lg_view *", "size_t", "uint32_t", "uint32_t", "uint8_t *", "double *"]
    assert types("lg_capture_views_device") == ["const lg_accel *", "const lg_view *", "size_t", "uint32_t", "uint32_t", "void *", "double *", "void *"]
    # after lg_lens_rays_device and before lg_accel_set_query_order, in the issue's order
    order = ["int lg_lens_rays_device("] + ["int %s(" % n for n in NAMES] + ["int lg_accel_set_query_order("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), order
    struct = re.search(r"typedef struct lg_view \{(.*?)\} lg_view;", gen_rust_sys.strip_comments(header), flags=re.S)
    assert struct and header.index("int lg_lens_rays_device(") < header.index("typedef struct lg_view {") < header.index("int lg_view_look_at(")
    fields = re.sub(r"\s+", " ", struct.group(1)).strip()
    assert fields == "double origin[3], view[3], up[3], aux[3]; double image_plane_height, pixel_separation; uint32_t samples_root; uint32_t reserved;"
    assert "120 bytes, no padding" in header
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header[header.index("/* Views:"):header.index("int lg_view_look_at(")]))
    assert "An EXTRA: no counterpart in the reference" in text and "used AS GIVEN" in text
    assert "Camera::init(perspective, param), Camera::look_at(origin, look, up), Camera::set_supersampling(supersampling)" in text and "byte for byte" in text
    assert "a view has none" in text, "the aperture radius"
    # the ray expression and its order
    assert "ss_distance = 1.0 / (double)samples_root" in text and "all f64, nothing contracted, in this order" in text
    assert "sox = ((double)x * winv - 0.5) * plane_w" in text and "soy = (0.5 - (double)(y + 1) * hinv) * image_plane_height" in text
    assert "o = (origin + ((soy * pixel_separation) * up)) + ((sox * pixel_separation) * aux)" in text and "d = (view + (soy * up)) + (sox * aux)" in text
    assert "direction = ((d + ((double)j * updiff)) + ((double)i * auxdiff)) + half" in text and "i = s / samples_root; j = s % samples_root" in text
    assert "summed from zero in camera order" in text and "1.0 / (double)S" in text and "to_byte per channel with A = 255" in text
    assert "lg_capture's and the doubles are lg_capture_radiance(0, 1, ..)'s, bit for bit" in text
    assert "Non-finite fields are accepted as they are" in text
    assert "Every pixel of every film is written exactly once" in text and "nothing outside n_views*width*height elements is touched" in text
    assert "views is a HOST array in both forms" in text and "pinned staging" in text
    assert "LASGUN_WF_BUDGET_MB" in text and "always the level-by-level pipeline" in text and "lg_accel_set_query_order plays no part" in text
    assert "n_views == 0 is a successful no-op" in text
    assert "n_views * ceil(width/8) * ceil(height/8) * S > 2^32 - 1" in text and "counted in 32 bits" in text, "the 32-bit tile limit"
    assert "views of one call that differ in samples_root" in text and "uniform-samples rule" in text
    assert "samples_root of 0 or above 256" in text and "reserved != 0" in text and "SIZE_MAX" in text and "both outputs NULL" in text
    assert "MORE THAN 32 LIGHTS" in text and "recursion depth of 20 or more" in text
    assert "dev_rgba not 4-byte aligned" in text and "dev_rgb not 8-byte aligned" in text and "ends beyond its allocation" in text


def test_lg_view_is_120_bytes_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    assert la.View is _capi.CView and ctypes.sizeof(la.View) == 120
    assert [f[0] for f in la.View._fields_] == ["origin", "view", "up", "aux", "image_plane_height", "pixel_separation", "samples_root", "reserved"]
    assert la.View.image_plane_height.offset == 96 and la.View.samples_root.offset == 112 and la.View.reserved.offset == 116
    assert "sizeof(lg_view) == 120" in read("lasgun_amd", "csrc", "views_host.h")  # a static_assert of the library's own build
    assert "static_assert(sizeof(lg_view) == 120" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_view \{(.*?)\n\}", sys_src, flags=re.S)
    assert struct and re.findall(r"pub (\w+): ([^,]+),", struct.group(1)) == [("origin", "[f64; 3]"), ("view", "[f64; 3]"), ("up", "[f64; 3]"), ("aux", "[f64; 3]"),
                                                                              ("image_plane_height", "f64"), ("pixel_separation", "f64"), ("samples_root", "u32"),
                                                                              ("reserved", "u32")]
    assert "std::mem::size_of::<sys::lg_view>() == 120" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.VIEWS_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    assert sigs["capture_views"][1][2] is ctypes.c_size_t and sigs["capture_views_device"][1][2] is ctypes.c_size_t
    for wrapper in ("view_look_at", "scene_view", "accel_view", "view_rays", "view_rays_device", "capture_views", "capture_views_device"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.views) and callable(la.view_look_at) and callable(la.cube_map_views) and callable(la.orbit_views)
    hpp = read("include", "lasgun.hpp")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hpp), name
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"void capture_views\(", hpp) and re.search(r"void capture_views_device\(", hpp)
    assert re.search(r"pub fn capture_views\(", safe) and re.search(r"pub unsafe fn capture_views_device\(", safe) and re.search(r"pub fn view_look_at\(", safe)


def test_the_kernels_are_device_kernels_of_their_own():
    from level0_text import calls_the_bodies, level0_bodies
    src = read("lasgun_amd", "csrc", "k_views.hip")
    for kernel in ("view_closest_kernel", "view_shade_kernel", "view_combine_kernel", "view_resolve_kernel"):
        assert re.search(r"__global__ void [^\n]*\b%s\(" % kernel, src), kernel
    level0_bodies()  # one walk, closest hit
    calls_the_bodies(src, 1, 1, 1)
    assert "wave_append(" not in src and "trav_launch<ViewKernels>" in src and "trav_set_lds_limit<ViewKernels>" in src
    assert "film_store(Q, it.px.pix, l0_finished(value))" in src and "l0_tile(" in src and "__builtin_amdgcn_readfirstlane" in src
    assert "view_ray(P, view_load(Q, it.px.v), it.px.x, it.px.y, it.sample)" in src and "ViewSource{Q}" in src
    make = read("lasgun_amd", "csrc", "Makefile")
    kobjs = re.search(r"^KOBJS = (.*)$", make, flags=re.M).group(1).split()
    assert "k_views.o" in kobjs and "-ffp-contract=off" in make and "views_host.h" in make
    assert "view_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    launch = read("lasgun_amd", "csrc", "launch.cpp")
    assert "bind_level0<ViewArgs, launch_view_closest, launch_view_shade, launch_view_combine>(V)" in launch
    assert "l0.resolve_ = l0_flat<ViewArgs, launch_view_resolve>" in launch
    assert re.search(r"timed\(a, 1, stream, \[&\] \{ return l0\.resolve\(", launch), "the resolve is credited to kind 1"
    assert launch.count("static void enqueue_level0_query(") == 1 and launch.count("struct WfChunk {") == 1, "one level-0 query over the ray source, not a copy"
    host = read("lasgun_amd", "csrc", "query.cpp")
    whole = host[host.index("// ---- views"):host.index("// ---- feature buffers")]
    assert "radiance_possible(*a)" in whole and "enqueue_view_batch(" in whole and "c.init(perspective != 0, param)" in whole and "c.look_at(" in whole
    assert "c.set_supersampling(supersampling)" in whole and "std::tan" not in whole and "cross(" not in whole, "the scene camera's own host code, not restated"


def test_look_at_views_are_the_scene_cameras_bytes():
    import lasgun_amd as la
    G = la.api
    try:
        from test_gpu_radiance_query import SECOND
    except Exception:  # (the GPU suite's helpers need what a CPU-only checkout may not have)
        SECOND = None
    if SECOND is not None:
        assert [tuple(c) for s in SECOND for c in s[3]] == CAMERAS
    assert len(CAMERAS) == 12
    for cam in CAMERAS:
        kind, par, eye, look, up = cam
        for ss in (0, 1, 2):
            scene = G.Scene.new()
            c = scene.set_orthographic_camera(par) if kind == "orthographic" else scene.set_perspective_camera(par)
            c.look_at(list(eye), list(look), list(up))
            c.set_supersampling(ss)
            c.set_aperture_radius(0.25)  # (stored by the scene, used by nothing: a view has none)
            want, got = G.scene_view(scene), look_at_view(la, cam, ss)
            assert bytes(got) == bytes(want) and len(bytes(got)) == 120, (cam, ss)
            assert got.samples_root == ss + 1 and got.reserved == 0 and got.pixel_separation == (1.0 if kind == "orthographic" else 0.0)
    # a scene whose look_at was never called: Camera::init's defaults
    for persp, par in ((True, 37.5), (False, 4.25)):
        scene = G.Scene.new()
        scene.set_perspective_camera(par) if persp else scene.set_orthographic_camera(par)
        v = G.scene_view(scene)
        assert (list(v.origin), list(v.view), list(v.up), list(v.aux)) == ([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
        assert v.samples_root == 1 and v.reserved == 0 and v.pixel_separation == (0.0 if persp else 1.0)
        want = np.tan(par * np.pi / 360.0) * 2.0 if persp else par  # (focal length 1; tan is libm's: 1 ulp)
        assert abs(v.image_plane_height - want) <= (np.spacing(want) if persp else 0.0), (persp, par, v.image_plane_height)


def test_look_at_against_a_numpy_restatement():
    """cross, normalise as a sqrt and a division -- v * (1.0 / sqrt((x*x + y*y) + z*z)), the vector layer's own order (vecmath.h, as cgmath's) --,
    |v| * tan(param * pi / 360) * 2: the vectors exact (IEEE operations in the stated order), the plane height within 1 ulp (tan is libm's,
    and nothing says it is correctly rounded)."""
    import lasgun_amd as la

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    def normalize(a):
        return a * (1.0 / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))

    for cam in CAMERAS:
        kind, par, eye, look, up = cam
        got = look_at_view(la, cam)
        o, l, u = (np.array(x, dtype=np.float64) for x in (eye, look, up))
        v = l - o
        a = cross(v, u)
        assert np.array_equal(np.array(got.origin[:]), o) and np.array_equal(np.array(got.view[:]), v), cam
        assert np.array_equal(np.array(got.up[:]), normalize(cross(a, v))) and np.array_equal(np.array(got.aux[:]), normalize(a)), cam
        if kind == "orthographic":
            assert got.image_plane_height == par
        else:
            want = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) * np.tan(par * np.pi / 360.0) * 2.0
            assert abs(got.image_plane_height - want) <= np.spacing(want), (cam, got.image_plane_height, want)


def test_errors_before_any_hip_call_and_the_empty_batch():
    import lasgun_amd as la
    G = la.api
    good = look_at_view(la, CAMERAS[0])
    t = (la.View * 2)(good, good)
    rgba, rgb = np.full(2 * 4 * 4 * 4, 0xA5, dtype=np.uint8), np.full(2 * 4 * 4 * 3, -7.0)
    adr = ctypes.addressof
    fake = ctypes.c_void_p(1)  # (never looked behind: every case below is refused before the accel is touched)
    for fn, tail in (("capture_views", ()), ("capture_views_device", (None,))):
        call = lambda acc, views, k, w, h, a=rgba.ctypes.data, d=rgb.ctypes.data: G.call(fn, acc, views, k, w, h, a, d, *tail)  # noqa: E731
        assert call(None, adr(t), 2, 4, 4) != 0 and "accel is NULL" in G.last_error(), fn
        assert call(fake, None, 2, 4, 4) != 0 and "views is NULL" in G.last_error(), fn
        assert call(fake, adr(t), 2, 4, 4, None, None) != 0 and "both NULL" in G.last_error(), fn
        assert call(fake, adr(t), 2, 0, 4) != 0 and G.last_error() and call(fake, adr(t), 2, 4, 0) != 0 and G.last_error(), fn
        for field, value, word in (("samples_root", 0, "samples_root"), ("samples_root", 257, "samples_root"), ("reserved", 7, "reserved"), ("samples_root", 3, "differs")):
            bad = (la.View * 2)(good, good)
            setattr(bad[1], field, value)
            assert call(fake, adr(bad), 2, 4, 4) != 0 and word in G.last_error(), (fn, field, value)
        four = (la.View * 4)(good, good, good, good)
        assert call(fake, adr(four), 4, 1 << 18, 1 << 18) != 0 and "32 bits" in G.last_error(), fn  # 2^32 work tiles: one above the limit
        # n_views == 0: a successful no-op, whatever the pointers
        assert call(None, None, 0, 0, 0, None, None) == 0 and call(fake, adr(t), 0, 4, 4) == 0, fn
    assert (rgba == 0xA5).all() and (rgb == -7.0).all(), "an error or an empty batch touched an output"
    # lg_view_look_at / lg_scene_view / lg_accel_view / lg_view_rays: NULL pointers
    from lasgun_amd._capi import _v3
    z = _v3((0, 0, 0))
    assert G.call("view_look_at", None, 1, 45.0, z, z, z, 0) != 0 and G.last_error()
    assert G.call("scene_view", None, adr(good)) != 0 and G.call("accel_view", None, adr(good)) != 0
    assert G.call("view_rays", None, adr(good), 4, 4, 0, 0, 4, 4, None) != 0 and G.call("view_rays", fake, None, 4, 4, 0, 0, 4, 4, None) != 0
    for views in ([good, 3], "nonsense"):
        try:
            G.capture_views(None, views, 4, 4)
        except (TypeError, AttributeError):
            continue
        raise AssertionError("capture_views takes View records")


def test_cube_map_views_follow_their_formula():
    import lasgun_amd as la
    doc = la.cube_map_views.__doc__
    assert "A convention of this WRAPPER" in doc and "+X -X +Y -Y +Z -Z" in doc and "fov 90" in doc and "look=origin + axis_f" in doc
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    ups = [(0, -1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0), (0, -1, 0)]
    for origin in ((0.0, 0.0, 0.0), (0.3, -1.25, 7.5)):
        for ss in (0, 2):
            views = la.cube_map_views(origin, supersampling=ss)
            assert len(views) == 6
            for v, axis, up in zip(views, axes, ups):
                look = [origin[c] + float(axis[c]) for c in range(3)]
                assert bytes(v) == bytes(la.view_look_at(origin, look, up, fov=90.0, supersampling=ss))
                assert v.samples_root == ss + 1 and v.pixel_separation == 0.0
                # a face looks along its axis with a plane two units high at distance one: the six frusta tile the sphere
                assert np.allclose(np.array(v.view[:]), axis, atol=1e-15) and abs(v.image_plane_height - 2.0) <= 1e-15
                assert np.allclose(np.array(v.up[:]), up, atol=1e-15)
    assert bytes(la.cube_map_views((0, 0, 0))[0]) == bytes(la.cube_map_views((0, 0, 0), 0)[0])


def test_orbit_views_follow_their_formula():
    import lasgun_amd as la
    doc = la.orbit_views.__doc__
    assert "A convention of this WRAPPER" in doc and "eye_k = center + radius * (cos(e) * (cos(a_k) * t + sin(a_k) * s) + sin(e) * u)" in doc and "a_k = 2 pi k / n" in doc
    for center, radius, elev, n, fov, up in (((0.0, 0.0, 0.0), 5.0, 20.0, 7, 40.0, (0, 1, 0)), ((1.0, -2.0, 0.5), 3.25, -35.0, 130, 65.0, (0.2, 0.1, 1.0))):
        views = la.orbit_views(center, radius, elev, n, fov, up=up)
        assert len(views) == n
        c, u = np.array(center, dtype=np.float64), np.array(up, dtype=np.float64)
        u = u / np.linalg.norm(u)
        f = la.frames_from_normals(u)[0]
        t, s = f[:, 0], f[:, 1]
        e = np.radians(float(elev))
        for k, v in enumerate(views):
            a = 2.0 * np.pi * k / n
            eye = c + float(radius) * (np.cos(e) * (np.cos(a) * t + np.sin(a) * s) + np.sin(e) * u)
            assert bytes(v) == bytes(la.view_look_at(eye, c, up, fov=float(fov))), k
            assert abs(np.linalg.norm(np.array(v.origin[:]) - c) - radius) <= 1e-14 * radius, "on the sphere of that radius"
            assert abs(np.dot(np.array(v.origin[:]) - c, u) - radius * np.sin(e)) <= 1e-14 * radius, "at that elevation"
        assert len({bytes(v) for v in views}) == n
    assert la.orbit_views((0, 0, 0), 1.0, 0.0, 0, 45.0) == []
