"""The device-free host code of lg_radiance_groups* (lasgun_amd/csrc/light_groups_host.h: n_groups of 0, 1, 64, 65 and 2^64 - 1, a mask bit
against every light count 0 .. 32, every unknown flag bit, the ray limit with 1 and 64 groups, the NULL and alignment rules, the table as
it travels and the host form's staging) under AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main
(tools/light_groups_host_check.cpp) that includes exactly the text query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "light_groups_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "light_groups_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "light_groups_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "light_groups_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_light_groups(a, rays, n, groups, n_groups, radiance, a->flat.lights.size(), table)" in query
    assert "check_light_groups(a, dev_rays, n, groups, n_groups, dev_radiance, a->flat.lights.size(), table)" in query
    assert "check_light_groups_alignment(dev_rays, dev_radiance)" in query and "trip.staged(radiance, shape.out_doubles)" in query
    check = open(os.path.join(ROOT, "tools", "light_groups_host_check.cpp")).read()
    for edge in ("LG_MAX_LIGHT_GROUPS + 1, OUT, 0)", "n_lights <= 32", "(bit >= n_lights)", "QUERY_MAX_RAYS + 1, many, 1", "many, TOP, OUT, 0)"):
        assert edge in check, ("the checks at their edges", edge)
