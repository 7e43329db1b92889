"""The bit-row host code of lg_visibility* and lg_open_directions* (lasgun_amd/csrc/bitrows_host.h: the used bytes of a row, row_bytes
against them, the tile count at its 32-bit limit and one above for both tile heights, the rows that do not fit the address space, the
extent of the bits buffer, the compact-to-stride placement into a block of exactly that extent) under AddressSanitizer and UBSan on the
CPU: a stand-alone program with its own main (tools/bitrows_host_check.cpp) that includes exactly the text query.cpp includes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "bitrows_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "bitrows_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "bitrows_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "bitrows_host.h"' in query, "query.cpp runs the text that was checked"
    assert "check_bit_rows(n_from, n_to, 8, bits, row_bytes," in query and "check_bit_rows(n_points, n_dirs, 64, bits, row_bytes," in query
    assert query.count("bit_rows_extent(") == 2 and query.count("place_bit_rows(") == 2, "both families, the device extent and the host placement"
    assert "bit_row_used_bytes(" in query and "% 8 ?" not in query and "/ 8 +" not in query, "the used bytes of a row are the header's alone"
    assert "#include <hip" not in open(os.path.join(ROOT, "lasgun_amd", "csrc", "bitrows_host.h")).read()
    check = open(os.path.join(ROOT, "tools", "bitrows_host_check.cpp")).read()
    for limit in ("!refused(8 * M, 8, 8, b, 1)", "refused(8 * M + 1, 8, 8, b, 1)", "!refused(64 * M, 8, 64, b, 1)", "refused(64 * M + 1, 8, 64, b, 1)",
                  "refused(rows, cols, 8, p, limit + 1) && !refused(rows, cols, 8, p, limit)", "!refused(1, 9, 8, p, TOP)"):
        assert limit in check, ("the limits exactly and one above, both tile heights", limit)
