"""What every query's host code shares (lasgun_amd/csrc/planes_host.h: checked_bytes at 0, SIZE_MAX / 96 and one above, check_alignment for
offsets 1 .. 16 against 4, 8 and 16 bytes, the NULL and alignment rules over a plane table, and HostStaging -- hold and stage of 0, 1 and
several elements of 1, 4, 8 and 96 bytes, a NULL host, nothing staged, destruction without place(), two planes placed in order) under
AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main (tools/planes_host_check.cpp) that includes exactly the
text query.cpp includes and RoundTrip stages through."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "planes_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "planes_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "planes_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = open(os.path.join(ROOT, "lasgun_amd", "csrc", "query.cpp")).read()
    assert '#include "planes_host.h"' in query, "query.cpp runs the text that was checked"
    trip = query[query.index("class RoundTrip {"):query.index("// Both host forms:")]
    assert "HostStaging staging;" in trip and "staging.hold<T>(n)" in trip and "staging.stage(host, n)" in trip, "RoundTrip stages through HostStaging"
    run_body = trip[trip.index("void run(Enqueue &&enqueue)"):]
    assert run_body.index("sync_checked(a);") < run_body.index("staging.place();"), "run() places after the synchronise"
    assert "memcpy(" not in trip.replace("hipMemcpyAsync(", ""), "no placement of RoundTrip's own"
    host = open(os.path.join(ROOT, "lasgun_amd", "csrc", "planes_host.h")).read()
    assert not re.search(r"#include\s*<hip|hipStream|hipMemcpy", host), "no HIP type in the shared host text"
    check = open(os.path.join(ROOT, "tools", "planes_host_check.cpp")).read()
    for edge in ("EDGE = SIZE_MAX / 96", "checked_bytes(EDGE + 1, 96,", "checked_bytes(5, 0, \"x\") == 0", "{(size_t)1, (size_t)2, (size_t)4, (size_t)8, (size_t)16}",
                 "{(size_t)4, (size_t)8, (size_t)16}", "check_alignment(nullptr, align,", "elements<Wide>(n)", "st.stage((double *)nullptr, 7) == nullptr",
                 "{ HostStaging st; st.place(); }", "destroyed without place()", "second = st.stage(target.get(), 2)"):
        assert edge in check, ("the checks at their edges", edge)
