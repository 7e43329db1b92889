"""The device-free host code of lg_hit_attributes* / lg_hit_attributes_of* (lasgun_amd/csrc/attributes_host.h: the limits, every NULL
combination and the alignment rule of lg_attr_out and of the _of form's records, the host forms' staging for every subset of the planes,
the counts table and attr_record_ok over an exhaustive small grid of records) under AddressSanitizer and UBSan on the CPU: a stand-alone
program with its own main (tools/attributes_host_check.cpp) that includes exactly the text query.cpp, accel.cpp and k_attributes.hip
include, with the launch stubbed out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "attributes_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "attributes_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "attributes_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = read("lasgun_amd", "csrc", "query.cpp")
    assert '#include "attributes_host.h"' in query and "check_attributes(a, rays, records, of_form, n, out)" in query and \
        "check_attributes(a, dev_rays, dev_records, of_form, n, dev_out)" in query, "query.cpp runs the text that was checked"
    assert "check_attributes_alignment(dev_rays, dev_records, *dev_out)" in query and "attr_planes(dev, n, staged_planes(trip))" in query
    kernel = read("lasgun_amd", "csrc", "k_attributes.hip")
    assert '#include "attributes_host.h"' in kernel and "if (!attr_record_ok(Q.counts, id.x, id.y, id.z)) flags = ATTR_BAD_RECORD;" in kernel, \
        "the kernel checks a record with the function that was checked, before it reads through it"
    assert kernel.index("attr_record_ok(Q.counts") < kernel.index("attr_triangle_index(Q.counts") < kernel.index("attr_resolve(P, ray, pk, idx, id.z, got)")
    assert "attr_counts_build(faces, tri_base, sphere_accel, cuboid_accel)" in read("lasgun_amd", "csrc", "accel.cpp")
    check = read("tools", "attributes_host_check.cpp")
    for edge in ("EDGE = TOP / 96", "QUERY_MAX_RAYS + 1", "planes < 128", "refused(&accel, D, h, true, 2, &all)", "refused(&accel, D, nullptr, true, 2, &no_hits)",
                 "new uint32_t[table.size()]", "0xFFFFFFFFu}"):
        assert edge in check, ("the checks at their edges", edge)
