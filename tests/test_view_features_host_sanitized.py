"""The device-free host code of lg_capture_view_features* (lasgun_amd/csrc/view_features_host.h: the plane table, every NULL rule, the
2^32 - 8 rule, the pixel-tile count at its 32-bit limit and one above, each plane's byte size at SIZE_MAX and one above, the views' own
rules and the uniform-samples rule, the alignment rule) under AddressSanitizer and UBSan on the CPU: a stand-alone program with its own
main (tools/view_features_host_check.cpp) that includes exactly the text query.cpp includes.  Nothing is preloaded anywhere."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "view_features_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "view_features_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "view_features_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "view_features_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_view_features(a, views, n_views, w, h, out, material_rgb)" in query and "check_view_features(a, views, n_views, w, h, dev_out, dev_material_rgb)" in query
    assert "check_view_features_alignment(*dev_out, dev_material_rgb)" in query and query.count("view_feature_planes(") == 2
    check = open(os.path.join(ROOT, "tools", "view_features_host_check.cpp")).read()
    assert '#include "../lasgun_amd/csrc/view_features_host.h"' in check
    for limit in ("refusal(&accel, two.get(), 1, 65535 * 8, 65537 * 8, &depth).empty()", 'refusal(&accel, two.get(), 1, 65536 * 8, 65536 * 8, &depth), "32 bits"',
                  "view_tiles(M, 8, 8, 1, &per, &tiles) && tiles == M && !view_tiles(M + 1, 8, 8, 1, &per, &tiles)",
                  "bytes(TOP / b, 1, 1, b) ==", "bytes(TOP / b + 1, 1, 1, b) == -1", "refusal(&accel, two.get(), 1, EDGE, 1, &depth).empty()",
                  'refusal(&accel, two.get(), 1, EDGE + 1u, 1, &depth), "2^32 - 8"'):
        assert limit in check, ("the tile count at 2^32 - 1 and one above, each plane's size at SIZE_MAX and one above, the 2^32 - 8 rule", limit)
    host = open(os.path.join(ROOT, "lasgun_amd", "csrc", "view_features_host.h")).read()
    for reused in ("check_view(", "view_tiles(", "view_bytes("):  # views_host.h's, not restated
        assert reused in host and ("inline bool " + reused not in host) and ("inline void " + reused not in host) and ("inline size_t " + reused not in host), reused
