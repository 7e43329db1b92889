"""The device-free host code of lg_trace_paths* (lasgun_amd/csrc/paths_host.h: the limits, n * max_bounces just under and over
SIZE_MAX / 96, max_bounces of 0, 1 and 2^32 - 1, every NULL combination of the nine planes and the alignment rule of lg_paths_out, the rule
table's validation, the host form's staging for every subset of the planes) under AddressSanitizer and UBSan on the CPU: a stand-alone
program with its own main (tools/paths_host_check.cpp) that includes exactly the text query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "paths_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "paths_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "paths_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "paths_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_paths(a, rays, n, max_bounces, rules, n_rules, lg_accel_material_count(a), normal, out)" in query
    assert "check_paths(a, dev_rays, n, max_bounces, rules, n_rules, lg_accel_material_count(a), normal, dev_out)" in query
    assert "check_paths_alignment(dev_rays, dev_start_medium, *dev_out)" in query and "path_planes(dev, n, total, staged_planes(trip))" in query
    check = open(os.path.join(ROOT, "tools", "paths_host_check.cpp")).read()
    for edge in ("EDGE = TOP / 96", "refused(&accel, D, under + 1, k, &all)", "refused(&accel, D, 1, 0, &all)", "checked(&accel, 1, KMAX, &all) == KMAX",
                 "planes < 512", "action > LG_PATH_REFRACT", "r[m].reserved = 1u"):
        assert edge in check, ("the checks at their edges", edge)
