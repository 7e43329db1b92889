"""Light groups (include/lasgun_hip.h: lg_radiance_groups, lg_radiance_groups_device, lg_accel_light_count) through every layer that has
to carry them, checked without a GPU: the built library exports the symbols, the header declares them with the arity, names and types the
wrappers use and states the contract, lg_light_group is 8 bytes and the constants agree in every mirror, the kernels are HIP kernels of
their own in the build beside the unchanged walk, and the Python, C++ and Rust bindings mirror the entry points.  On top: the errors that
are answered before any HIP call, the no-op of an empty query, and the wrapper's two conventions, per_light_groups and relight."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARITY = {"lg_radiance_groups": 6, "lg_radiance_groups_device": 7, "lg_accel_light_count": 1}
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
    assert names("lg_radiance_groups")[1:] == ["rays", "n", "groups", "n_groups", "radiance"]
    assert names("lg_radiance_groups_device")[1:] == ["dev_rays", "n", "groups", "n_groups", "dev_radiance", "hip_stream"]
    types = lambda key: [re.sub(r"\s*\w+$", "", p).strip() for p in decl[key][1]]  # noqa: E731
    host = ["const double *", "size_t", "const lg_light_group *", "size_t", "double *"]
    assert types("lg_radiance_groups")[1:] == host
    assert types("lg_radiance_groups_device")[1:] == host + ["void *"]
    order = ["EXTRAS", "/* Light groups:", "typedef struct lg_light_group {", "#define LG_GROUP_AMBIENT 1u", "#define LG_MAX_LIGHT_GROUPS 64", "int lg_radiance_groups(",
             "int lg_radiance_groups_device(", "int lg_accel_light_count("]
    at = [header.index(o) for o in order]
    assert at == sorted(at), order
    struct = re.search(r"typedef struct lg_light_group \{(.*?)\} lg_light_group;", header, flags=re.S)
    assert struct and re.findall(r"^\s*(uint32_t)\s+(\w+);", struct.group(1), flags=re.M) == [("uint32_t", "lights"), ("uint32_t", "flags")]
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", header[header.index("/* Light groups:"):header.index("typedef struct lg_light_group")]))
    assert "GROUP-MAJOR, element (g, r, c) at (g*n + r)*3 + c" in text and "n_groups * n * 3 doubles" in text
    assert "by exactly one lane: no atomics, no pre-fill" in text
    assert "bit l of `lights` names light l, in lg_scene_add_point_light order" in text
    assert "only the lights of groups[g].lights added, in their original order" in text and "the ambient colour (+0, +0, +0) unless LG_GROUP_AMBIENT is set" in text
    assert "bit for bit and in the accel's traversal mode" in text and "The background belongs to every group" in text
    assert "a light outside the mask skipped exactly as an invisible light is" in text
    assert "the product with the BSDF is still formed: a NaN there stays a NaN" in text
    assert "(output + reflected) + refracted per group with the same weights" in text and "a finished ray is (0 + li) * 1.0" in text
    assert "a group with ALL lights and LG_GROUP_AMBIENT holds lg_radiance's very bytes" in text, "said in the header"
    assert 'holds the "base"' in text and "shadow-skip stays valid" in text
    assert "lg_accel_set_query_order(1) and the LASGUN_WF_BUDGET_MB chunks" in text and "24 * (n_groups - 1) bytes per ray of every level" in text
    assert "n == 0 is a successful no-op whatever the pointers are" in text
    assert "n_groups == 0 or > LG_MAX_LIGHT_GROUPS" in text and "at or above the scene's light count" in text and "an unknown `flags` bit" in text
    assert "more than 32 lights or a recursion depth of 20 or more" in text and "n > (2^32 - 1) * 64" in text and "n * n_groups * 24 that does not fit size_t" in text
    assert "`groups` is a HOST array in both forms" in text and "it only enqueues on hip_stream" in text and "leaves the caller's array as it was" in text
    assert "films per group" in text and "a background flag" in text, "what is out of scope"


def test_lg_light_group_is_8_bytes_and_the_constants_agree_in_every_mirror():
    import lasgun_amd as la
    from lasgun_amd import _capi
    C = _capi.CLightGroup
    assert ctypes.sizeof(C) == 8 and [f[0] for f in C._fields_] == ["lights", "flags"] and [C.lights.offset, C.flags.offset] == [0, 4]
    assert _capi.GROUP_AMBIENT == 1 and _capi.MAX_LIGHT_GROUPS == 64 and la.GROUP_AMBIENT == 1 and la.MAX_LIGHT_GROUPS == 64
    host = read("lasgun_amd", "csrc", "light_groups_host.h")  # static_asserts of the library's own build
    assert "sizeof(lg_light_group) == 8" in host and "offsetof(lg_light_group, flags) == 4" in host and "LG_MAX_LIGHT_GROUPS == 64 && LG_GROUP_AMBIENT == 1u" in host
    dscene = read("lasgun_amd", "csrc", "dscene.h")
    assert "MAX_LIGHT_GROUPS = 64u" in dscene and "GROUP_AMBIENT = 1u" in dscene
    assert "sizeof(DLightGroup) == sizeof(lg_light_group) && MAX_LIGHT_GROUPS == LG_MAX_LIGHT_GROUPS && GROUP_AMBIENT == LG_GROUP_AMBIENT" in read("lasgun_amd", "csrc", "query.cpp")
    assert "static_assert(sizeof(lg_light_group) == 8" in read("include", "lasgun.hpp")
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    struct = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct lg_light_group \{(.*?)\n\}", sys_src, flags=re.S)
    assert struct and re.findall(r"pub (\w+): (\w+),", struct.group(1)) == [("lights", "u32"), ("flags", "u32")]
    assert "pub const LG_GROUP_AMBIENT: u32 = 1;" in sys_src and "pub const LG_MAX_LIGHT_GROUPS: usize = 64;" in sys_src
    assert "std::mem::size_of::<sys::lg_light_group>() == 8" in read("bindings", "rust", "lasgun", "src", "lib.rs")


def test_capi_and_the_python_wrappers_mirror_them():
    import lasgun_amd as la
    from lasgun_amd import _capi
    sigs = _capi.LIGHT_GROUPS_SIGNATURES
    assert set("lg_" + k for k in sigs) == set(NAMES)
    for key, (restype, argtypes) in sigs.items():
        assert restype is ctypes.c_int and len(argtypes) == ARITY["lg_" + key], key
        assert key in la.api._fn, key  # bound to the built library at import
    for key in ("radiance_groups", "radiance_groups_device"):
        argtypes = sigs[key][1]
        assert argtypes[2] is ctypes.c_size_t and argtypes[4] is ctypes.c_size_t, key
        assert all(a is ctypes.c_void_p for i, a in enumerate(argtypes) if i not in (2, 4)), key
    for wrapper in ("radiance_groups", "radiance_groups_device", "light_count"):
        assert callable(getattr(la.api, wrapper)), wrapper
    assert callable(la.Accel.radiance_groups), "accel.radiance_groups(rays, groups)"
    g = la.LightGroup([0, 5, 31], ambient=True)
    assert (g.lights, g.flags) == (1 | 1 << 5 | 1 << 31, 1) and (la.LightGroup(6).lights, la.LightGroup(6).flags) == (6, 0)
    assert la.LightGroup(1, flags=4).flags == 4
    with pytest.raises(ValueError):
        la.LightGroup([32])


def test_the_cpp_wrapper_calls_it():
    src = read("include", "lasgun.hpp")
    assert re.search(r"\blg_radiance_groups\(", src) and re.search(r"\blg_radiance_groups_device\(", src) and re.search(r"\blg_accel_light_count\(", src)
    assert re.search(r"radiance_groups\(const std::vector", src) and re.search(r"void radiance_groups_device\(", src)


def test_the_rust_crates_carry_them():
    sys_src = read("bindings", "rust", "lasgun-hip-sys", "src", "lib.rs")
    safe = read("bindings", "rust", "lasgun", "src", "lib.rs")
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, sys_src), name
        assert "sys::%s(" % name in safe, name
    assert re.search(r"pub fn radiance_groups\(", safe) and re.search(r"pub unsafe fn radiance_groups_device\(", safe) and re.search(r"pub fn light_count\(", safe)
    assert "groups: *const lg_light_group, n_groups: usize" in sys_src


def test_the_kernels_are_device_kernels_of_their_own_beside_the_unchanged_walk():
    """G planes come from HIP kernels the library launches in one chain: the shared closest body, a shade and a combine kernel with the
    group loop, the spread pass; the table travels by value and DParams has no field for it; nothing loops over lg_radiance on the host."""
    src = read("lasgun_amd", "csrc", "k_light_groups.hip")
    for kernel in ("lg_closest_kernel", "lg_shade_kernel", "lg_combine_kernel", "lg_spread_kernel"):
        assert re.search(r"__global__ void [^\n]*\b%s\(const DParams P, const GroupArgs Q\)" % kernel, src), kernel
    assert src.count("l0_closest_body<FAST, LDSS, PRUNE>(P, GroupRaySource<PERM>{Q})") == 1 and "__launch_bounds__(LG_BLOCK, 3) lg_shade_kernel" in src
    shared = read("lasgun_amd", "csrc", "level0.h")
    assert len(re.findall(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", shared)) == 1 and "walk<" not in src and "claim_tile" not in src
    for fn in ("unsigned long long rq_ray_index(", "Ray rq_load_ray("):
        assert shared.count(fn) == 1 and fn not in src, fn
    finish = src[src.index("template <bool PERM> struct GroupRaySource {"):src.index("// plane g of a level's li")]
    assert "for (uint32_t g = 0; g < Q.n_groups; ++g) lg_finish(Q, r, g, value);" in finish, "a finished miss goes to all G planes, in the source's own finish"
    code = "\n".join(line.split("//")[0] for line in src.split("#include", 1)[1].splitlines())
    assert "atomic" not in code.replace("wave_append", ""), "no atomics of its own: every element is written by exactly one lane"
    assert "trav_launch<GroupClosestKernels>" in src and "trav_set_lds_limit<GroupClosestKernels>" in src
    assert "vis & grp.lights" in src and "(grp.flags & GROUP_AMBIENT) ? P.ambient : vzero()" in src and "mul_ew(ambient, amb_f)" in src
    dscene = read("lasgun_amd", "csrc", "dscene.h")
    params = dscene[dscene.index("struct DParams"):dscene.index("static_assert(sizeof(DParams)")]
    assert "LightGroup" not in params and "n_groups" not in params and "xout" not in params, "DParams gets no new field"
    assert "DLightGroup groups[MAX_LIGHT_GROUPS];" in dscene[dscene.index("struct GroupArgs"):]
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "k_light_groups.o" in make and "-ffp-contract=off" in make and "light_groups_host.h" in make
    assert "light_groups_set_lds_limit" in read("lasgun_amd", "csrc", "accel.cpp")
    launch = read("lasgun_amd", "csrc", "launch.cpp")
    assert launch.count("void run(") == 1, "one chain, not a copy of it"
    assert "l0.spread(P, flat_cap, ls)" in launch and '"radiance groups"' in launch
    host = read("lasgun_amd", "csrc", "query.cpp")
    whole = host[host.index("// ---- light groups"):host.index("// ---- radiance gathers")]
    assert whole.count("enqueue_radiance_groups(") == 1 and "enqueue_radiance(" not in whole and "for (" not in whole, "one chain for all groups"


def test_the_no_device_errors_are_refused_and_touch_nothing():
    """A NULL accel with n > 0 is answered before anything else; an empty query is a no-op whatever the pointers and counts are."""
    import lasgun_amd as la
    from lasgun_amd import _capi
    G = la.api
    n = 5
    rays = np.zeros((n, 6))
    rays[:, 5] = 1.0
    out = np.full((2, n, 3), np.nan)
    table = (_capi.CLightGroup * 2)(_capi.CLightGroup(0, 0), _capi.CLightGroup(0, 1))
    for fn, tail in (("radiance_groups", ()), ("radiance_groups_device", (None,))):
        assert G.call(fn, None, rays.ctypes.data, n, ctypes.addressof(table), 2, out.ctypes.data, *tail) != 0 and "accel is NULL" in G.last_error(), fn
        for k in (0, 1, 64, 65, 2 ** 40):
            assert G.call(fn, None, None, 0, None, k, None, *tail) == 0, (fn, k)
    assert np.isnan(out).all()
    assert G.call("accel_light_count", None) == -1
    check = read("tools", "light_groups_host_check.cpp")  # every other refusal, through the same text, in the stand-alone check
    assert "refused(nullptr, D, 3, one, 1, OUT, 1)" in check and "refused(&accel, D, 3, many, 0, OUT, 1)" in check and "(bit != 0)" in check


def test_per_light_groups_is_base_ambient_then_one_group_per_light():
    import lasgun_amd as la
    for n in (0, 1, 3, 32):
        groups = la.per_light_groups(n)
        assert [(g.lights, g.flags) for g in groups] == [(0, 0), (0, 1)] + [(1 << l, 0) for l in range(n)], n
    assert len(la.per_light_groups(32)) == 34 <= la.MAX_LIGHT_GROUPS
    for bad in (-1, 33):
        with pytest.raises(ValueError):
            la.per_light_groups(bad)


def test_relight_is_the_formula_exact_on_small_integer_planes():
    """base + a * (amb - base) + sum s_i * (L_i - base): on small integers every product and sum is exact, so the formula is pinned whole."""
    import lasgun_amd as la
    rng = np.random.default_rng(7)
    n_lights, shape = 3, (4, 5, 3)
    base = rng.integers(0, 8, shape).astype(np.float64)
    amb = base + rng.integers(0, 8, shape)
    lights = [base + rng.integers(0, 8, shape) for _ in range(n_lights)]
    planes = np.stack([base, amb] + lights)
    # all scales 1: base + every contribution, i.e. the full frame
    full = base + (amb - base) + sum(l - base for l in lights)
    assert np.array_equal(la.relight(planes), full)
    # all scales 0: the base
    assert np.array_equal(la.relight(planes, 0.0, [0.0] * n_lights), base)
    # integer scales, per light and per channel
    a, s = 3.0, np.array([[2.0, 0.0, 1.0], [1.0, 4.0, 0.0], [0.0, 0.0, 5.0]])
    want = base + a * (amb - base)
    for i in range(n_lights):
        want = want + s[i] * (lights[i] - base)
    assert np.array_equal(la.relight(planes, a, s), want)
    assert np.array_equal(la.relight(planes, a, [2.0, 1.0, 0.0]), base + a * (amb - base) + 2.0 * (lights[0] - base) + 1.0 * (lights[1] - base))
    # one light switched off: the frame without it
    assert np.array_equal(la.relight(planes, 1.0, [1.0, 0.0, 1.0]), base + (amb - base) + (lights[0] - base) + (lights[2] - base))
    assert np.array_equal(la.relight(planes[:2], 2.0), base + 2.0 * (amb - base)), "a scene without lights"
    with pytest.raises(ValueError):
        la.relight(planes, 1.0, [1.0, 2.0])
    with pytest.raises(ValueError):
        la.relight(planes[:1])
    assert "NOT bit-exact against a rebuilt render" in la.relight.__doc__
