"""The device-free host code of lg_nearest* (lasgun_amd/csrc/nearest_host.h: the five-plane table, every check and every refusal in its
order, k against the planes asked for, n * k and the sizes through checked_bytes, the alignment rule, the LDS rule at its edge, the host
form's staging for every subset of the planes through tools/host_check.h's staged_round) under AddressSanitizer and UBSan on the CPU: a
stand-alone program with its own main (tools/nearest_host_check.cpp) that includes exactly the text query.cpp, capi.cpp and k_nearest.hip
include.  On top, without a device: the library's lg_scene_nearest_lds is the stated formula over lg_scene_closest_depth for the scenes of
the GPU test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path_factory.mktemp("nearest_host") / "nearest_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "nearest_host_check.cpp"), "-o", exe])
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_host_code_is_clean_under_asan_and_ubsan(program):
    run = subprocess.run([program], capture_output=True, text=True, env=ENV)
    assert run.returncode == 0 and "nearest_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = read("lasgun_amd", "csrc", "query.cpp")
    for needle in ('#include "nearest_host.h"', "check_nearest(a, points, radii, n, radius, k, out);", "check_nearest(a, dev_points, dev_radii, n, radius, k, dev_out);",
                   "check_nearest_alignment(dev_points, dev_radii, *dev_out);", "nearest_planes(dev, n, nk, staged_planes(trip));",
                   "nearest_planes(*dev_out, n, nk, device_planes(*a));", "check_nearest_lds(t.depth, entries);", "check_closest_scene(a)"):
        assert needle in query, ("query.cpp runs the text that was checked", needle)
    body = query[query.index("static void enqueue_nearest("):query.index('extern "C" int lg_nearest(')]
    assert body.count("launch_nearest(") == 1, "one launch, no chunks"
    assert "HIP_TRY(nearest_set_lds_limit(NEAREST_LDS_LIMIT));" in body and query.count("nearest_set_lds_limit(") == 1, \
        "the kernels' dynamic-LDS limit is only ever raised to the most any call may ask for"
    assert "nearest_lds_bytes(closest_tables(ClosestScene{" in read("lasgun_amd", "csrc", "capi.cpp")
    assert '#include "nearest_host.h"' in read("lasgun_amd", "csrc", "k_nearest.hip")
    check = read("tools", "nearest_host_check.cpp")
    for edge in ("QUERY_MAX_RAYS + 1", "planes < 32", "staged_round(", '== "accel is NULL"', '== "points is NULL"', '== "out is NULL"', "radius is NaN or negative",
                 "k is beyond LG_NEAREST_MAX_K", "k is 0 and a slot plane", "id is not 16-byte aligned", "radii is not 8-byte aligned", "count is not 4-byte aligned",
                 "check_nearest_lds(60, 8)", "check_nearest_lds(61, 8)", "SIZE_MAX / 24 + 1"):
        assert edge in check, ("the checks at their edges", edge)


def test_scene_nearest_lds_is_the_stated_formula():
    import closest_cases as C
    import lasgun_amd as la
    seen = set()
    for name in list(C.SCENES) + list(C.LIMIT_SCENES):
        depth = la.api.scene_closest_depth(C.builder(name)(la.api))
        for k in (0, 1, 8):
            assert la.api.scene_nearest_lds(C.builder(name)(la.api), k) == 256 * (8 * depth + 20 * k), (name, k, depth)
        seen.add(depth)
    assert len(seen) > 1
    with pytest.raises(la.LasgunError, match="LG_NEAREST_MAX_K"):
        la.api.scene_nearest_lds(C.builder("own")(la.api), 9)
