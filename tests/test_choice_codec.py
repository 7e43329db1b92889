"""The encoding of a launch's organisation (lasgun_amd/csrc/choice.h: what lg_accel_last_organisation returns, lg_tune_entry.choice, the
lines of a LASGUN_TUNE_FILE) and the candidates of the measured choice, held to the literals of the ABI under AddressSanitizer and UBSan on
the CPU: a stand-alone program with its own main (tools/choice_check.cpp) that includes the header alone.  And the header is what runs:
launch.cpp, capi.cpp and tune.cpp include it and spell no bit of their own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_codec_and_the_race_slots_are_the_literals_of_the_abi(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "choice_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "choice_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "choice_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    check = open(os.path.join(ROOT, "tools", "choice_check.cpp")).read()
    includes = [line for line in check.splitlines() if line.startswith("#include \"")]
    assert includes == ['#include "../lasgun_amd/csrc/choice.h"'], "the check program includes the header alone"
    header = open(os.path.join(ROOT, "lasgun_amd", "csrc", "choice.h")).read()
    assert "#include" not in header, "choice.h is device-free: no HIP include, nothing from internal.h"


@pytest.mark.parametrize("unit", ["launch.cpp", "capi.cpp", "tune.cpp"])
def test_the_host_units_go_through_the_header(unit):
    text = open(os.path.join(ROOT, "lasgun_amd", "csrc", unit)).read()
    assert '#include "choice.h"' in text
    for literal in ("& 15", "TUNE_REV", "TUNE_MID", "TUNE_SERIAL", "TUNE_SPLIT"):
        assert literal not in text, (unit, literal, "the bits of a choice are spelled in choice.h alone")
