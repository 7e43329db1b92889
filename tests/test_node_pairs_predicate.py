"""The pair form of the LDS image without a device (lasgun_amd/csrc/pairs_host.h): a stand-alone program with its
own main (tools/node_pairs_host_check.cpp) over exactly the text accel.cpp includes, under AddressSanitizer and UBSan on the CPU.  It
compares the builder's image with a restatement from the node records, record by record in all bytes -- one pair record per interior node,
every leaf reachable with its slot range, the root record present, nothing written outside the stated ranges, the image within the stated
bound -- walks random rays (zero and negative-zero direction components and origins on the root box's faces among them) through the
pair form and the node form: the same leaves in the same order, the same multiset of box tests with each box tested at most once, a stack
that never holds more than the node form's; with the any-hit walk's early exit, the same leaves and a superset of the box tests.  And the
packing's range checks refuse synthetic trees that do not fit.  A restatement of the packing in Python pins the words' layout."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_LEAF, SLOT_BITS, COUNT_BITS = 0x80000000, 16, 15


def leaf_word(first, count):  # pairs_host.h, pair_leaf_word
    if count == 0 or count >= 1 << COUNT_BITS or first >= 1 << SLOT_BITS or first + count > 1 << SLOT_BITS:
        return None
    return PAIR_LEAF | first | count << SLOT_BITS


def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "node_pairs_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "node_pairs_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "node_pairs_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])


def test_the_packing_restated():
    assert leaf_word(0, 1) == 0x80010000 and leaf_word(65535, 1) == 0x8001FFFF and leaf_word(1000, 32767) == 0xFFFF03E8
    assert leaf_word(65536, 1) is None and leaf_word(65535, 2) is None and leaf_word(0, 32768) is None and leaf_word(0, 0) is None
    # the headline: 2,037 node records of 80 bytes against 1,018 pair records of 112 and one root record
    assert 1018 * 112 + 64 <= 2037 * 80
