"""The device-free host code of lg_hit_layers* (lasgun_amd/csrc/layers_host.h: the limits, n * max_layers just under and over
SIZE_MAX / 96, max_layers of 0, 1 and 2^32 - 1, every NULL combination and the alignment rule of lg_layers_out, the host form's staging
for every subset of the planes) under AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main
(tools/layers_host_check.cpp) that includes exactly the text query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "layers_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "layers_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "layers_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "layers_host.h"' in query and "check_layers(a, rays, n, max_layers, out)" in query and "check_layers(a, dev_rays, n, max_layers, dev_out)" in query, \
        "query.cpp runs the text that was checked"
    assert "check_layers_alignment(dev_rays, *dev_out)" in query and "layer_planes(dev, n, total, staged_planes(trip))" in query
    check = open(os.path.join(ROOT, "tools", "layers_host_check.cpp")).read()
    for edge in ("EDGE = TOP / 96", "refused(&accel, D, under + 1, k, &all)", "refused(&accel, D, 1, 0, &all)", "check_layers(&accel, D, 1, KMAX, &all) == KMAX",
                 "planes < 32"):
        assert edge in check, ("the checks at their edges", edge)
