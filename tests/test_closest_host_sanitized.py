"""The device-free host code of lg_closest_points* (lasgun_amd/csrc/closest_host.h: the plane table, every check and every refusal in its
order, the alignment rule, the host form's staging for every subset of the planes through tools/host_check.h's staged_round, the sphere
gate, the constants of the pruning test and the stack depth of the kernel's push rule over scenes built in the program) under
AddressSanitizer and UBSan on the CPU: a stand-alone program with its own main (tools/closest_host_check.cpp) that includes exactly the
text query.cpp, capi.cpp and k_closest.hip include.  The shrink bound is held to numpy's SVD: the same program answers 1000 seeded random
chains of depth 1 to 8, and the library's device-free gate the accels of the GPU test's scenes; shrink[a] must not exceed the smallest
singular value of accel a's composed local -> world linear part."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path_factory.mktemp("closest_host") / "closest_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "closest_host_check.cpp"), "-o", exe])
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_host_code_is_clean_under_asan_and_ubsan(program):
    run = subprocess.run([program], capture_output=True, text=True, env=ENV)
    assert run.returncode == 0 and "closest_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    query = read("lasgun_amd", "csrc", "query.cpp")
    assert '#include "closest_host.h"' in query and "check_closest(a, points, n, radius, out);" in query and "closest_tables(ClosestScene{" in query, \
        "query.cpp runs the text that was checked"
    assert "if (t.depth > CLOSEST_MAX_DEPTH)" in query and "if (t.refused >= 0)" in query and query.index("if (t.refused >= 0)") < query.index("if (t.depth > CLOSEST_MAX_DEPTH)")
    assert "closest_gate(ClosestScene{" in read("lasgun_amd", "csrc", "capi.cpp")
    assert "HIP_TRY(closest_set_lds_limit(closest_stack_bytes(CLOSEST_MAX_DEPTH)));" in query and query.count("closest_set_lds_limit(") == 1, \
        "the kernel's dynamic-LDS limit is only ever raised to the most any scene may ask for"
    assert '#include "closest_host.h"' in read("lasgun_amd", "csrc", "k_closest.hip")
    check = read("tools", "closest_host_check.cpp")
    for edge in ("QUERY_MAX_RAYS + 1", "planes < 8", "staged_round(", '== "accel is NULL"', '== "points is NULL"', '== "out is NULL"', "radius is NaN or negative",
                 "id is not 16-byte aligned", "{1u, 2u, 7u, 40u, 70u}", "affine_scale(1.2, 0.8, 1.0)", "a tree that does not end", "a sphere below the magnitude range"):
        assert edge in check, ("the checks at their edges", edge)


def random_chain(rng, depth):
    """depth x (m, minv) as Affine holds them (column-major 3 x 4), and the composed linear part."""
    rec, total = [], np.eye(3)
    for _ in range(depth):
        kind = rng.integers(0, 4)
        q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (3, 3)))
        if kind == 0:
            lin = q * rng.uniform(0.2, 5.0)                                  # a similarity
        elif kind == 1:
            lin = q @ np.diag(rng.uniform(0.05, 20.0, 3))                    # rotation and non-uniform scale
        elif kind == 2:
            lin = rng.normal(0.0, 1.0, (3, 3))                               # general
        else:
            lin = q @ np.diag([1.0, 1.0, 10.0 ** rng.uniform(-9.0, 0.0)])    # nearly flat: often beyond the condition limit (shrink 0)
        t = rng.uniform(-10.0, 10.0, 3)
        inv = np.linalg.inv(lin)
        m = np.concatenate([lin.T.reshape(-1), t])            # columns c0, c1, c2, then the translation
        mi = np.concatenate([inv.T.reshape(-1), -inv @ t])
        total = total @ lin
        rec.append((np.concatenate([m, mi]), total.copy()))
    return rec


def test_shrink_holds_against_numpys_svd_on_1000_random_chains(program, tmp_path):
    rng = np.random.default_rng(28)
    chains, words = [], []
    for _ in range(1000):
        depth = int(rng.integers(1, 9))
        chain = random_chain(rng, depth)
        chains.append(chain)
        words.append(np.array([float(depth)]))
        words += [c[0] for c in chain]
    src, dst = str(tmp_path / "chains.bin"), str(tmp_path / "shrink.bin")
    np.concatenate(words).tofile(src)
    run = subprocess.run([program, src, dst], capture_output=True, text=True, env=ENV)
    assert run.returncode == 0 and "closest_host_check: ok, 1000 chains" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    shrink = np.fromfile(dst, dtype=np.float64)
    assert len(shrink) == sum(len(c) for c in chains)
    k, proven, tight = 0, 0, 0
    for chain in chains:
        for _, total in chain:
            smin = np.linalg.svd(total, compute_uv=False).min()
            assert 0.0 <= shrink[k] <= smin, (k, shrink[k], smin)
            proven += shrink[k] > 0.0
            tight += shrink[k] > 0.5 * smin
            k += 1
    assert proven >= 0.5 * len(shrink) and tight >= 0.3 * len(shrink), (proven, tight, len(shrink))  # (a bound of 0 everywhere would hold too)


def test_shrink_holds_on_the_accels_of_the_gpu_tests_scenes():
    import closest_cases as C
    import lasgun_amd as la
    for name in list(C.SCENES) + list(C.LIMIT_SCENES):
        _, b, _, _ = C.case(name)
        verdict, shrink = la.api.scene_closest_gate(C.builder(name)(la.api))
        assert verdict == C.gate(b.cat), name
        assert len(shrink) == len(b.cat.accels), name
        depth = la.api.scene_closest_depth(C.builder(name)(la.api))
        assert 1 <= depth <= la.api.CLOSEST_MAX_DEPTH, (name, depth)
        if name in ("deep_a", "deep_c"):
            assert depth > 32, (name, depth, "these scenes take the launch beyond the default 64 KiB of dynamic LDS")
        for a, acc in enumerate(b.cat.accels):
            smin = np.linalg.svd(C.linear_part(acc["chain"]), compute_uv=False).min()
            assert 0.0 < shrink[a] <= smin, (name, a, shrink[a], smin)
