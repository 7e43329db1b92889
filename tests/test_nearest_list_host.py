"""The per-point list of lg_nearest* on the CPU: lasgun_amd/csrc/nearest_list.h (admissibility, the order, the rule between a candidate and a
full list, the insertion) compiled into a stand-alone program (tools/nearest_list_check.cpp, its own main, nothing loaded into python) under
AddressSanitizer and UBSan, against numpy's lexsort of (d2, key) word for word on seeded streams: every k from 1 to 8, streams shorter and
longer than k, runs of equal d2 (the key alone decides, also at the cut), NaN and +INF candidates, radii 0, finite and +INF, ascending,
descending and shuffled arrival.  Three seeded faults, built into the check program alone with -DLG_NEAREST_FAULT, must each fail the same
comparison: a swapped tie, a full list that refuses a candidate tying its last entry whatever the key, an admissibility test that lets +INF
through."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined,float-cast-overflow",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def streams():
    """[(k, d2 (m,), key (m,) uint64, slot (m,) uint64, r2)]: one point's candidates in their order of arrival."""
    rng = np.random.default_rng(29)
    out = []
    for trial in range(1200):
        k = 1 + trial % 8
        m = int(rng.integers(0, 40))
        family = trial % 6
        if family == 0:    # distinct distances
            d2 = rng.uniform(0.0, 4.0, m)
        elif family == 1:  # runs of equal d2: a few values, many candidates
            d2 = rng.choice(np.array([0.0, 0.25, 0.25 + 2.0 ** -54, 1.0, 2.5]), m)
        elif family == 2:  # every candidate ties
            d2 = np.full(m, 0.5)
        elif family == 3:  # NaN and +INF among them
            d2 = rng.choice(np.array([0.1, 0.7, 0.7, NAN, INF, 3.0]), m)
        elif family == 4:  # ascending arrival: a full list takes nothing more
            d2 = np.sort(rng.choice(np.array([0.0, 0.5, 0.5, 1.0, 1.5, 2.0]), m))
        else:              # descending arrival: every candidate enters at the front
            d2 = np.sort(rng.choice(np.array([0.0, 0.5, 0.5, 1.0, 1.5, 2.0]), m))[::-1].copy()
        instance, kind, prim = rng.integers(0, 5, m).astype(np.uint64), rng.integers(1, 4, m).astype(np.uint64), rng.permutation(1000)[:m].astype(np.uint64)
        key = (instance << np.uint64(34)) | (kind << np.uint64(32)) | prim  # distinct: prim is
        r2 = [INF, 1.0, 0.5, 0.0, 2.0 ** 60][int(rng.integers(0, 5))]
        out.append((k, d2.astype(np.float64), key, rng.integers(0, 2 ** 32, m).astype(np.uint64), r2))
    return out


def expected(k, d2, key, slot, r2):
    with np.errstate(invalid="ignore"):
        ok = (d2 <= r2) & (d2 < INF)
    d2, key, slot = d2[ok], key[ok], slot[ok]
    order = np.lexsort((key, d2))[:k]
    words = np.full(1 + 3 * 8, ONES, dtype=np.uint64)
    words[0] = len(order)
    for j, w in enumerate(order):
        words[1 + 3 * j:4 + 3 * j] = [d2[w:w + 1].view(np.uint64)[0], key[w], slot[w]]
    return words


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    s = streams()
    rec = []
    for g, (k, d2, key, slot, r2) in enumerate(s):
        m = len(d2)
        block = np.zeros((m, 6), dtype=np.uint64)
        block[:, 0], block[:, 1], block[:, 2], block[:, 3], block[:, 4] = g, k, d2.view(np.uint64), key, slot
        block[:, 5] = np.array([r2], dtype=np.float64).view(np.uint64)[0]
        rec.append(block)
    src = str(tmp_path_factory.mktemp("nearest_list") / "streams.bin")
    np.concatenate(rec).tofile(src)
    want = np.concatenate([expected(*c) for c in s if len(c[1])])  # (a stream of no candidate is no group of the file)
    return src, want, s


def build(tmp_path_factory, fault):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path_factory.mktemp("nearest_list_%d" % fault) / "nearest_list_check")
    subprocess.check_call([cxx] + FLAGS + (["-DLG_NEAREST_FAULT=%d" % fault] if fault else []) + [os.path.join(ROOT, "tools", "nearest_list_check.cpp"), "-o", exe])
    return exe


def run(exe, src, tmp_path):
    dst = str(tmp_path / "lists.bin")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    return done, (np.fromfile(dst, dtype=np.uint64) if done.returncode == 0 else None)


def test_the_list_is_numpys_lexsort_word_for_word(cases, tmp_path_factory, tmp_path):
    src, want, s = cases
    done, got = run(build(tmp_path_factory, 0), src, tmp_path)
    assert done.returncode == 0 and "nearest_list_check: ok" in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    assert got.shape == want.shape and (got == want).all(), np.nonzero(got != want)[0][:8]
    ks = {c[0] for c in s}
    assert ks == set(range(1, 9))
    full = sum(1 for k, d2, _, _, r2 in s if ((d2 <= r2) & (d2 < INF)).sum() > k)
    cut_ties = 0
    for k, d2, key, _, r2 in s:
        with np.errstate(invalid="ignore"):
            a = np.sort(d2[(d2 <= r2) & (d2 < INF)])
        cut_ties += len(a) > k and a[k - 1] == a[k]
    print("nearest list: %d streams, %d of them longer than their list, %d with an exact tie across the cut" % (len(s), full, cut_ties))
    assert full >= 200 and cut_ties >= 100
    assert any(np.isnan(c[1]).any() for c in s) and any(np.isinf(c[1]).any() and c[4] == INF for c in s)


@pytest.mark.parametrize("fault", [1, 2, 3])
def test_each_seeded_fault_is_caught(cases, tmp_path_factory, tmp_path, fault):
    src, want, _ = cases
    done, got = run(build(tmp_path_factory, fault), src, tmp_path)
    assert done.returncode == 0, (done.stdout[-2000:], done.stderr[-4000:])  # (a fault of arithmetic: the program runs, its answer differs)
    assert got.shape != want.shape or (got != want).any(), "seeded fault %d went unnoticed" % fault


def test_the_kernel_runs_this_text_and_never_a_fault():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()  # noqa: E731
    kernel, header = read("lasgun_amd", "csrc", "k_nearest.hip"), read("lasgun_amd", "csrc", "nearest_list.h")
    assert '#include "nearest_list.h"' in kernel and "nearest_insert(list, m, kcap, " in kernel and "nearest_admissible(c.d2, r2)" in kernel
    assert "#if LG_NEAREST_FAULT != 0\n#error" in kernel, "a seeded fault can never be built into the kernel, whatever flags leak in"
    assert header.count("#if LG_NEAREST_FAULT") == 3 and "#define LG_NEAREST_FAULT 0" in header
    assert "-DLG_NEAREST_FAULT" not in read("lasgun_amd", "csrc", "Makefile"), "the product is built without a seeded fault"
