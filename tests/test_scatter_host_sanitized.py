"""The device-free host code of lg_scatter* (lasgun_amd/csrc/scatter_host.h: the ray limit and one above, the planes' sizes at the edge of
the address space, 32 and 33 lights, every NULL combination of the seven planes and the alignment rule of lg_scatter_out, the host form's
staging for every subset of the planes) under AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main
(tools/scatter_host_check.cpp) that includes exactly the text query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "scatter_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "scatter_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "scatter_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "scatter_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_scatter(a, rays, n, out, a ? a->flat.lights.size() : 0)" in query
    assert "check_scatter(a, dev_rays, n, dev_out, a ? a->flat.lights.size() : 0)" in query
    assert "check_scatter_alignment(dev_rays, *dev_out)" in query and "scatter_planes(dev, n, staged_planes(trip))" in query
    check = open(os.path.join(ROOT, "tools", "scatter_host_check.cpp")).read()
    for edge in ("EDGE = TOP / 96", "refused(&accel, D, QUERY_MAX_RAYS + 1, &all)", "refused(&accel, D, 3, &none)", "planes < 128", "(size_t)33", "(size_t)32",
                 "want_align[7] = {16, 8, 4, 8, 8, 8, 8}"):
        assert edge in check, ("the checks at their edges", edge)
