"""The device-free host code of lg_scatter_lit* (lasgun_amd/csrc/lit_host.h: the light set's rules, W at the word edges, n * K * 72,
n * K * 24 and n * W * 4 at the edge of the address space, every NULL combination of the nine planes and the alignment rule of lg_lit_out,
the host form's staging for every subset of the planes, shared and per ray) under AddressSanitizer and UBSan on the CPU: a stand-alone
program with its own main (tools/lit_host_check.cpp) that includes exactly the text query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "lit_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "lit_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "lit_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "lit_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_lit(a, rays, n, lights, out)" in query and "check_lit(a, dev_rays, n, lights, dev_out)" in query
    assert "check_lit_alignment(dev_rays, *lights, *dev_out, z)" in query and "lit_planes(dev, z, staged_planes(trip))" in query
    check = open(os.path.join(ROOT, "tools", "lit_host_check.cpp")).read()
    for edge in ("TOP / 72 / 1024 + 1", "TOP / 24 / 1024 + 1", "TOP / 4 / 32 + 1", "QUERY_MAX_RAYS + 1", "LG_MAX_CALL_LIGHTS + 1", "planes < 512",
                 "want_align[9] = {16, 8, 4, 8, 8, 8, 8, 8, 4}", "{0, 1, 31, 32, 33, 64, 65, 70}"):
        assert edge in check, ("the checks at their edges", edge)
