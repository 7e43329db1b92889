"""The device-free host code of lg_closest_segments* (lasgun_amd/csrc/segments_host.h: the five-plane table, every check and every refusal
in its order, the sizes through checked_bytes, the alignment rule, which plane set is the touch-only form, the host form's staging for
every subset of the planes through tools/host_check.h's staged_round) under AddressSanitizer and UBSan on the CPU: a stand-alone program
with its own main (tools/segments_host_check.cpp) that includes exactly the text query.cpp and k_segments.hip include."""
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
    exe = str(tmp_path_factory.mktemp("segments_host") / "segments_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "segments_host_check.cpp"), "-o", exe])
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_host_code_is_clean_under_asan_and_ubsan(program):
    run = subprocess.run([program], capture_output=True, text=True, env=ENV)
    assert run.returncode == 0 and "segments_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = read("lasgun_amd", "csrc", "query.cpp")
    for needle in ('#include "segments_host.h"', "check_segments(a, segments, radii, n, radius, out);", "check_segments(a, dev_segments, dev_radii, n, radius, dev_out);",
                   "check_segments_alignment(dev_segments, dev_radii, *dev_out);", "segments_planes(dev, n, staged_planes(trip));",
                   "segments_planes(*dev_out, n, device_planes(*a));", "segments_touch_only(out)"):
        assert needle in query, ("query.cpp runs the text that was checked", needle)
    body = query[query.index("static void enqueue_segments("):query.index('extern "C" int lg_closest_segments(')]
    assert body.count("launch_segments(") == 1, "one launch, no chunks"
    assert "check_closest_scene(*a)" in query[query.index('extern "C" int lg_closest_segments('):], "the gate and the depth rule are closest points' own"
    assert '#include "segments_host.h"' in read("lasgun_amd", "csrc", "k_segments.hip")
    check = read("tools", "segments_host_check.cpp")
    for edge in ("QUERY_MAX_RAYS + 1", "planes < 32", "staged_round(", '== "accel is NULL"', '== "segments is NULL"', '== "out is NULL"', "radius is NaN or negative",
                 "id is not 16-byte aligned", "radii is not 8-byte aligned", "param is not 8-byte aligned", "SIZE_MAX / 48 + 1"):
        assert edge in check, ("the checks at their edges", edge)
