"""The device-free host code of lg_range_scan* (lasgun_amd/csrc/scan_host.h: the lane rule, the two tile counts at their 32-bit limit and
one above in both forms, the planes' byte sizes, the NULL and alignment rules of lg_scan_out, the host form's staging) under
AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main (tools/scan_host_check.cpp) that includes exactly the text
query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "scan_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "scan_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "scan_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "scan_host.h"' in query and "check_scan(a, origins," in query and "check_scan(a, dev_origins," in query, "query.cpp runs the text that was checked"
    assert "check_scan_alignment(dev_origins," in query and "scan_planes(dev, n_poses, pairs, staged_planes(trip))" in query and "return scan_lanes(n_poses, n_beams, lanes)" in query
    check = open(os.path.join(ROOT, "tools", "scan_host_check.cpp")).read()
    for limit in ("tiles(M, 64, 1) == (long long)M", "tiles(M + 1, 64, 1) == -1", "tiles(64 * M, 8, 2) == (long long)M", "tiles(64 * M + 1, 8, 2) == -1"):
        assert limit in check, ("the tile counts at their limit and one above, both forms", limit)
