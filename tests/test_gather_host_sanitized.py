"""The device-free host code of lg_radiance_gather* (lasgun_amd/csrc/gather_host.h: the lane rule, the two tile counts at their 32-bit limit
and one above in both forms, the four byte sizes at SIZE_MAX, the NULL and alignment rules of lg_gather_out, the batch rule down to a cap
below one pose, the host form's staging) under AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main
(tools/gather_host_check.cpp) that includes exactly the text query.cpp includes, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "gather_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gather_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "gather_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "gather_host.h"' in query and "check_gather(a, origins," in query and "check_gather(a, dev_origins," in query, "query.cpp runs the text that was checked"
    assert "check_gather_alignment(dev_origins," in query and "trip.staged(out->radiance, shape.pairs * 3), trip.staged(out->sums, n_poses * n_weights * 3)" in query and "return gather_lanes(n_poses, n_dirs, lanes)" in query
    assert "gather_batch_poses(n_poses, n_dirs, shape.form, park_bytes)" in query and 'gather_park_bytes(std::getenv("LASGUN_GATHER_PARK_MB"))' in query
    check = open(os.path.join(ROOT, "tools", "gather_host_check.cpp")).read()
    for limit in ("tiles(M, 64, 1) == (long long)M", "tiles(M + 1, 64, 1) == -1", "tiles(64 * M, 1, 2) == (long long)M", "tiles(64 * M + 1, 1, 2) == -1",
                  "bytes(TOP / 24 + 1, 1, 24) == -1", "bytes(TOP / 8 + 1, 1, 8) == -1", "bytes(TOP / 72 + 1, 9, 8) == -1", "gather_batch_poses(257, 1031, 1, 1031 * 24 - 1) == 1"):
        assert limit in check, ("the tile counts and sizes at their limit and one above, the batch rule below one pose", limit)
