"""The device-free host code of lg_capture_views* (lasgun_amd/csrc/views_host.h: the work-tile count at its 32-bit limit and one above,
both byte sizes at SIZE_MAX and one above, the view validation and the uniform-samples rule, the NULL and alignment rules, lg_view ->
DView) under AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main (tools/views_host_check.cpp) that includes
exactly the text query.cpp includes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "views_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "views_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "views_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "views_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_views(a, views, n_views, w, h, rgba, rgb)" in query and "check_views(a, views, n_views, w, h, dev_rgba, dev_rgb)" in query
    assert "check_views_alignment(dev_rgba, dev_rgb)" in query and "to_dviews(views, n_views)" in query and query.count("check_view(*view, 0)") == 2
    check = open(os.path.join(ROOT, "tools", "views_host_check.cpp")).read()
    for limit in ("tiles(M, 8, 8, 1) == (long long)M", "tiles(M + 1, 8, 8, 1) == -1", "tiles(3, 5 * 8, 17 * 8, 16843010) == -1", "tiles(1, 65536 * 8, 65536 * 8, 1) == -1",
                  "bytes(TOP / 4 + 1, 1, 1, 4) == -1", "bytes(TOP / 24 + 1, 1, 1, 24) == -1", "bytes(TOP / 4, 1, 1, 4) ==", "bytes(TOP / 24, 1, 1, 24) =="):
        assert limit in check, ("the tile count at 2^32 - 1 and one above, each byte size at SIZE_MAX and one above", limit)
