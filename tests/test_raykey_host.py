"""The coherence key of a query ray on the CPU: lasgun_amd/csrc/raykey.h compiled into a stand-alone program (tools/raykey_check.cpp, its
own main, nothing loaded into python) under AddressSanitizer and UBSan with float-cast-overflow, against the numpy restatement
(tests/raykey_ref.py) word for word, on the ray sets the device is asked about (tests/raykey_cases.py; tests/test_gpu_query_key.py).
With this green, a mismatch on the GPU is the device build's, not the restatement's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import edge_rays as E
import pyref
import raykey_cases as C
import raykey_ref as R
from query_witness import Witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
# -fsanitize=undefined leaves float-cast-overflow out with g++: it is named
FLAGS = ["-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined,float-cast-overflow",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """run(records) -> [keys]: records = [(lo, hi, rays)], through the sanitized program; a sanitizer report fails the test."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    tmp = tmp_path_factory.mktemp("raykey")
    exe = str(tmp / "raykey_check")
    subprocess.check_call([cxx] + FLAGS + [os.path.join(ROOT, "tools", "raykey_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")

    def run(records):
        with open(src, "wb") as f:
            for lo, hi, rays in records:
                rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
                f.write(np.uint64(len(rays)).tobytes() + np.asarray(lo, dtype=np.float64).tobytes() + np.asarray(hi, dtype=np.float64).tobytes())
                f.write(rays.tobytes())
        done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
        total = sum(len(r[2]) for r in records)
        assert done.returncode == 0 and "raykey_check: ok, %d records, %d keys" % (len(records), total) in done.stdout, \
            (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
        keys = np.fromfile(dst, dtype=np.uint32)
        assert len(keys) == total
        return np.split(keys, np.cumsum([len(r[2]) for r in records])[:-1])
    return run


def rotated_bounds():
    wit = Witness(C.rotated_root_scene(pyref.Api))
    box = wit.root.nodes[0][0]
    return wit, R.world_bounds(box[0], box[1], wit.root.m)


def first_difference(got, want, rays):
    bad = np.nonzero(got != want)[0]
    return None if len(bad) == 0 else (len(bad), int(bad[0]), rays[bad[0]].tolist(), hex(int(got[bad[0]])), hex(int(want[bad[0]])))


def test_the_restatement_is_not_the_header_in_disguise():
    """The Morton spreads by bit loop against a third form (string formatting), and a few keys worked out by hand from the layout."""
    for v in list(range(16)) + [0x155, 0x2AA, 0x3FF]:
        b = format(v, "010b")
        assert int(R.spread(np.array([v]), 10, 2)[0]) == int("".join("0" + c for c in b), 2)
        assert int(R.spread(np.array([v]), 10, 3)[0]) == int("".join("00" + c for c in b), 2)
    b = R.key_bounds((0.0, 0.0, 0.0), (16.0, 16.0, 16.0))
    key = lambda *r: int(R.ray_key(np.array([r]), b)[0])  # noqa: E731
    # origin cell (1, 0, 0) is bit 20, (0, 1, 0) bit 21, (0, 0, 1) bit 22, (2, 0, 0) bit 23; +z is the map's centre: u = v = 512
    centre = (1 << 18) | (1 << 19)
    assert key(0.5, 0.5, 0.5, 0.0, 0.0, 1.0) == centre
    assert key(1.5, 0.5, 0.5, 0.0, 0.0, 1.0) == centre | 1 << 20
    assert key(0.5, 1.5, 0.5, 0.0, 0.0, 1.0) == centre | 1 << 21
    assert key(0.5, 0.5, 1.5, 0.0, 0.0, 1.0) == centre | 1 << 22
    assert key(2.5, 0.5, 0.5, 0.0, 0.0, 1.0) == centre | 1 << 23
    assert key(15.5, 15.5, 15.5, 0.0, 0.0, 1.0) == centre | 0xFFF << 20
    # +x: u = 1023 (clamped from 1024), v = 512; -x: u = 0; +y: v = 1023; u is the even bits, v the odd ones
    assert key(0.5, 0.5, 0.5, 1.0, 0.0, 0.0) == 0x55555 | 1 << 19
    assert key(0.5, 0.5, 0.5, -1.0, 0.0, 0.0) == 1 << 19
    assert key(0.5, 0.5, 0.5, 0.0, 1.0, 0.0) == 0xAAAAA | 1 << 18
    # -z unfolds onto the corners: (+0, +0) -> (1, 1); the sign of a zero picks the corner
    assert key(0.5, 0.5, 0.5, 0.0, 0.0, -1.0) == 0xFFFFF
    assert key(0.5, 0.5, 0.5, -0.0, 0.0, -1.0) == 0xAAAAA
    assert key(0.5, 0.5, 0.5, 0.0, -0.0, -1.0) == 0x55555
    # (1, 1, -2) / 4 = (0.25, 0.25): unfolded (0.75, 0.75), cell 896 = 0b1110000000 on both axes
    assert key(0.5, 0.5, 0.5, 1.0, 1.0, -2.0) == 0xFC000 and 896 == 0b1110000000
    # NaN and the zero direction fall to cell 0; an origin far outside clamps to the border cells
    assert key(NAN, NAN, NAN, NAN, NAN, NAN) == 0 and key(0.5, 0.5, 0.5, 0.0, 0.0, 0.0) == 0
    assert key(-1e300, 1e300, INF, 0.0, 0.0, 1.0) == centre | (0x492 | 0x924) << 20


def test_world_bounds_take_all_eight_corners():
    wit, (lo, hi) = rotated_bounds()
    box, m = wit.root.nodes[0][0], wit.root.m
    two = np.array([pyref.transform_point(m, box[0]), pyref.transform_point(m, box[1])])
    assert not np.array_equal(lo, two.min(axis=0)) and not np.array_equal(hi, two.max(axis=0))
    # every transformed corner is inside, and each face of the bounds is touched by one
    corners = np.array([pyref.transform_point(m, (box[c & 1][0], box[c >> 1 & 1][1], box[c >> 2 & 1][2])) for c in range(8)])
    assert np.array_equal(corners.min(axis=0), lo) and np.array_equal(corners.max(axis=0), hi)
    assert (hi - lo > 1.0).all()
    # an identity root: the witness's own bound() (the reference's transform_bounds) is the same box
    grid = Witness(E.grid_scene(pyref.Api))
    glo, ghi = R.world_bounds(grid.root.nodes[0][0][0], grid.root.nodes[0][0][1], grid.root.m)
    assert np.array_equal(glo, grid.root.bound()[0]) and np.array_equal(ghi, grid.root.bound()[1])
    # (edge_rays.GRID_BOUNDS is the box the edge rays are aimed through, a little deeper than the scene: the key's bounds are the witness's)
    assert np.array_equal(glo, (0.0, 0.0, 0.0)) and np.array_equal(ghi, E.GRID_BOUNDS[1])
    # a corner that is not finite is stepped over
    nlo, nhi = R.world_bounds((0.0, 0.0, 0.0), (1.0, INF, 1.0), pyref.mat_identity())
    assert np.array_equal(nlo, (0.0, 0.0, 0.0)) and np.array_equal(nhi, (1.0, 0.0, 1.0))


BOUNDS = [("grid", lambda: ((0.0, 0.0, 0.0), E.GRID_BOUNDS[1])), ("rotated", lambda: rotated_bounds()[1])]


@pytest.mark.parametrize("name,box", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_header_and_restatement_agree_word_for_word(program, name, box):
    lo, hi = box()
    rays = C.key_ray_set(lo, hi, seed=len(name))
    assert 150000 <= len(rays) <= 250000
    bounds = R.key_bounds(lo, hi)
    C.check_reach(rays, bounds)
    got, = program([(lo, hi, rays)])
    assert first_difference(got, R.ray_key(rays, bounds), rays) is None
    C.check_layout(lambda r: program([(lo, hi, r)])[0], lo, hi)
    C.check_layout(lambda r: R.ray_key(r, bounds), lo, hi)


def test_degenerate_bounds(program):
    """key_bounds: a scale of 0 for an extent that is not finite or not positive, and for a lo that is not finite (taken as 0)."""
    rng = np.random.default_rng(11)
    rays = np.concatenate([C._with(rng.uniform(-4.0, 4.0, (4000, 3)), rng.normal(0.0, 1.0, (4000, 3))), np.tile(np.array(C.ODD_ROWS), (4, 1))])
    boxes = [((0.0, 0.0, 0.0), (0.0, 2.0, 2.0)), ((1.0, 1.0, 1.0), (-1.0, 3.0, 0.5)), ((-INF, -1.0, -1.0), (1.0, INF, 1.0)), ((NAN, -2.0, -2.0), (2.0, NAN, 2.0)),
             ((-1e308, -1.0, -1.0), (1e308, 1.0, 5e-324 - 1.0)), ((0.0, 0.0, 0.0), (5e-324, 1e-310, 1e308))]
    for (lo, hi), got in zip(boxes, program([(lo, hi, rays) for lo, hi in boxes])):
        blo, scale = R.key_bounds(lo, hi)
        assert np.isfinite(blo).all() and not np.isnan(scale).any()
        assert first_difference(got, R.ray_key(rays, (blo, scale)), rays) is None, (lo, hi)
    assert np.array_equal(R.key_bounds(*boxes[0])[1], (0.0, 0.5, 0.5)) and np.array_equal(R.key_bounds(*boxes[1])[1], (0.0, 0.5, 0.0))
    assert np.array_equal(R.key_bounds(*boxes[2])[1], (0.0, 0.0, 0.5)) and np.array_equal(R.key_bounds(*boxes[2])[0], (0.0, -1.0, -1.0))
    assert np.array_equal(R.key_bounds(*boxes[3])[1], (0.0, 0.0, 0.25)) and np.array_equal(R.key_bounds(*boxes[3])[0], (0.0, -2.0, -2.0))
    assert R.key_bounds(*boxes[4])[1][0] == 0.0  # (the extent overflows)
