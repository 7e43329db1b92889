"""The level door's two rules on the witness (tests/pyref.py, tests/pyref_bvh.py), no GPU.
The probe: one row of a nested accel's inverse transform, the thinnest axis of its node-0 box, m = fmax(t1, t2) <= 0  =>  the reference's own
node-0 test (the whole local ray, Bounds::intersects) misses -- on the headline scene, the Cornell scenes and a scene with a rotated, unevenly
scaled group, over at least 1e5 (ray, door) entries each, on real walked entries of the witness, and on the edge-case rays; the numpy
restatement gives the same verdicts ray for ray.  The lone-mesh rule holds for the five walls and fails for a group with a mesh and a sphere.
The host's records (host.cpp, level_door_records) are checked by a stand-alone program under ASan + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pyref
import level_door_rays as R
import level_door_scenes as D
from lasgun_amd import scenes as S
from oracle_lib import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = 2.220446049250313e-16 * 65536.0
if not hasattr(pyref.Camera, "set_aperture_radius"):
    pyref.Camera.set_aperture_radius = lambda self, radius: self

SCENES = {"headline": (S.spheres_scene, 4096), "cornell_plastic": (lambda api: S.cornell_scene(api, "plastic"), 512),
          "cornell_glass": (lambda api: S.cornell_scene(api, "glass"), 512), "srt_lone": (D.srt_lone_scene, 512), "nested": (D.nested_scene, 512)}


def sample_rays(builder, film, n_pixels, seed):
    """Primary rays of random pixels of a film x film frame and, from their oracle hits, the shadow rays to the first light."""
    pscene = builder(pyref.Api)
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, film, size=(n_pixels, 2))
    prim = np.array([[*od[0], *od[1]] for x, y in xy.tolist() for od in pscene.camera.sample(x, y, film, film)], dtype=np.float64)
    o = oracle()
    hits, _ = o.intersect(o.Accel(builder(o)), prim, nthreads=16)
    hit = hits["kind"] != 0
    ng = hits["ng"][hit]
    ng = np.where((np.einsum("ij,ij->i", ng, -prim[hit, 3:]) < 0.0)[:, None], -ng, ng)
    p = hits["p"][hit] + ng * ERR
    shadow = np.concatenate([p, np.array(pscene.lights[0][0]) - p], axis=1)
    return pscene, prim, shadow


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_one_axis_miss_is_a_node0_miss(name):
    builder, film = SCENES[name]
    root, ds = R.doors(builder(pyref.Api))
    per_kind = -(-100000 // len(ds))  # the primary rays alone make 1e5 (ray, door) entries; the shadow rays of those that hit come on top
    pscene, prim, shadow = sample_rays(builder, film, per_kind, len(name))
    rays = np.concatenate([prim, shadow])
    entries = shut_total = 0
    for dr in ds:
        # the ray as the door's parent hands it over: through the chain's transforms, on Python floats (the witness's own functions)
        local = [R.parent_ray(dr, tuple(r[:3]), tuple(r[3:])) for r in rays.tolist()]
        lo = np.array([l[0] for l in local]); ld = np.array([l[1] for l in local])
        shut = R.probe_numpy(dr, lo, ld)
        for i, (o, d) in enumerate(local):
            s = R.probe(dr, o, d)
            assert s == bool(shut[i]), (name, dr.row, o, d)
            if s:
                assert not R.node0_hit(dr, o, d), (name, dr.row, dr.lo, dr.hi, o, d)
        entries += len(local)
        shut_total += int(shut.sum())
    assert entries >= 100000, entries
    assert 0.05 * entries < shut_total < 0.95 * entries, (shut_total, entries)  # the probe says both things, often
    # ... and on entries the witness's walk really makes (the reference's walk, no early exit): primary and shadow rays
    walked = []
    for r in np.concatenate([prim[:150], shadow[:150]]).tolist():
        R.walk_entries(root, ds, tuple(r[:3]), tuple(r[3:]), walked)
    n, miss0, shut = R.tally(walked)
    assert n >= 300 and 0 < shut <= miss0 < n, (n, miss0, shut)


def test_the_lone_rule_on_the_witness():
    for builder in (S.spheres_scene, lambda api: S.cornell_scene(api, "glass")):
        _, ds = R.doors(builder(pyref.Api))
        groups = [d for d in ds if not d.is_mesh]
        assert len(groups) == 5 and all(d.lone for d in groups), "the five walls"
        assert not any(d.lone for d in ds if d.is_mesh)
    _, ds = R.doors(D.mesh_and_sphere_scene(pyref.Api))
    assert [d.lone for d in ds] == [False, False], "a group with a mesh and a sphere"
    _, ds = R.doors(D.nested_scene(pyref.Api))
    assert [(d.is_mesh, d.lone) for d in ds] == [(False, False), (False, True), (True, False)], "group -> group -> mesh: the inner group alone"
    _, ds = R.doors(D.identity_lone_scene(pyref.Api))
    assert [(d.is_mesh, d.lone, len(d.chain)) for d in ds] == [(False, True, 1), (True, False, 2), (True, False, 1), (False, True, 1), (True, False, 2)]


@pytest.mark.parametrize("name", sorted(D.SMALL) + ["cornell"])
def test_edge_rays_numpy_and_witness_agree(name):
    builder = D.SMALL.get(name) or (lambda api: S.cornell_scene(api, "plastic"))
    pscene = builder(pyref.Api)
    rays, fam = R.edge_rays(pscene, seed=len(name))
    _, ds = R.doors(pscene)
    said = {f: [0, 0] for f in set(fam.tolist())}
    for dr in ds:
        local = [R.parent_ray(dr, tuple(r[:3]), tuple(r[3:])) for r in rays.tolist()]
        shut = R.probe_numpy(dr, np.array([l[0] for l in local]), np.array([l[1] for l in local]))
        for i, (o, d) in enumerate(local):
            s = R.probe(dr, o, d)
            assert s == bool(shut[i]), (name, fam[i], o, d)
            assert not (s and R.node0_hit(dr, o, d)), (name, fam[i], dr.row, dr.lo, dr.hi, o, d)
            said[fam[i]][int(s)] += 1
    for f in ("face", "dzero", "negzero", "random"):
        assert said[f][0] and said[f][1], (name, f, said[f])
    assert said["nonfinite"][0], name


def test_the_edge_cases_by_hand():
    """The verdicts the design argues for, on the floor wall of the Cornell shell (its door: row (0, 1, 0, 2) of minv, planes y' = 0 and 0)."""
    _, ds = R.doors(S.cornell_scene(pyref.Api, "plastic"))
    floor = ds[0]
    assert floor.row == (0.0, 1.0, 0.0, 2.0) and floor.lo == 0.0 and floor.hi == 0.0 and floor.k == 1
    inf, nan = float("inf"), float("nan")
    cases = [(((0.0, -2.0, 0.0), (0.3, -1.0, 0.2)), True),    # origin on the plane: t = 0, m = 0 <= 0 -- the box test's `tfar > 0` fails too
             (((0.0, -2.0, 0.0), (0.3, 1.0, 0.2)), True),
             (((0.0, -2.0, 0.0), (1.0, 0.0, 0.0)), False),    # on the plane, d'_k = +0: 0 * inf = NaN both, m NaN: the old path
             (((0.0, -2.0, 0.0), (1.0, -0.0, 0.0)), False),
             (((0.0, -1.0, 0.0), (1.0, 0.0, 0.0)), True),     # above the plane, d'_k = +0: (0 - 1) * inf = -inf both
             (((0.0, -1.0, 0.0), (1.0, -0.0, 0.0)), True),    # ... a -0 in d does not survive the row's sum here: (0*1 + 1*-0) + 0*0 = +0, + 2*0 = +0
             (((0.0, -3.0, 0.0), (1.0, 0.0, 0.0)), False),    # below it: +inf both
             (((0.0, -3.0, 0.0), (1.0, -0.0, 0.0)), False),
             (((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), True),     # leaving the floor
             (((0.0, -1.0, 0.0), (0.0, -1.0, 0.0)), False),   # towards it
             (((nan, -1.0, 0.0), (0.0, 1.0, 0.0)), False),    # a NaN or infinite origin component: every component of the local origin is NaN
             (((inf, -1.0, 0.0), (0.0, 1.0, 0.0)), False),
             (((0.0, -1.0, 0.0), (0.0, nan, 0.0)), False),
             (((0.0, -1.0, 0.0), (0.0, inf, 0.0)), True),     # inv = 0: t = -1 * 0 = -0 on both planes, m = -0 <= 0; tfar <= -0 as well
             (((0.0, -1.0, 0.0), (inf, 1.0, 0.0)), False)]    # 0 * inf in the row's sum: d'_k NaN
    # d'_k = -0 needs every term of the sum to be -0: the ceiling's row (0, 1, 0, -2) and a direction without a positive component
    ceiling = ds[2]
    assert ceiling.row == (0.0, 1.0, 0.0, -2.0) and ceiling.lo == 0.0 and ceiling.hi == 0.0
    for door, table in ((floor, cases), (ceiling, [(((0.0, 1.0, 0.0), (-1.0, -0.0, -1.0)), True),     # below the plane, d'_k = -0: (0 + 1) * -inf = -inf
                                                   (((0.0, 1.0, 0.0), (1.0, 0.0, 1.0)), False),       # d'_k = +0: +inf
                                                   (((0.0, 3.0, 0.0), (-1.0, -0.0, -1.0)), False),   # above it: +inf
                                                   (((0.0, 3.0, 0.0), (1.0, 0.0, 1.0)), True),
                                                   (((0.0, 2.0, 0.0), (-1.0, -0.0, -1.0)), False)])):  # on it: 0 * -inf = NaN
        for (o, d), want in table:
            assert R.probe(door, o, d) == want, (o, d)
            got = R.probe_numpy(door, np.array([o]), np.array([d]))
            assert bool(got[0]) == want, (o, d)
            assert not (want and R.node0_hit(door, o, d)), (o, d)


def test_the_host_records_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "level_door_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O0", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "level_door_host_check.cpp"),
                           os.path.join(ROOT, "lasgun_amd", "csrc", "host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "level_door_host_check: ok" in run.stdout and "walls: 5 of 5 groups lone" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    host = open(os.path.join(ROOT, "lasgun_amd", "csrc", "host.cpp")).read()
    assert "level_door_records(out);" in host, "flatten_scene runs the text that was checked"
