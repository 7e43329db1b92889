"""The frame table of flat triangles, the part without a device (lasgun_amd/csrc/tri_frames_host.h).

The predicate, the plan and the build kernel's list: tools/tri_frames_check.cpp, a stand-alone program with its own main over exactly the
text accel.cpp and launch.cpp include, under AddressSanitizer and UBSan on the CPU: every refusing condition alone flips the gate, the caps
hold at their last admitted value, and a list and a table block of exactly the stated size are never overrun.

And what the plan says for scenes (lg_scene_tri_frames_gate): the headline and the Cornell boxes get ten records, two for each wall; a
mesh with vertex normals, an instance of 1,025 triangles and an accel whose records would be 4,097 get none."""
import os
import shutil
import subprocess

import pytest

import lasgun_amd as la
import tri_frames_scenes as T
from lasgun_amd import scenes as S

G = la.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "tri_frames_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "tri_frames_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "tri_frames_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])


def plan(scene):
    records, base = G.scene_tri_frames_gate(scene)
    return records, [b for b in base if b is not None]


@pytest.mark.parametrize("name,build", [
    ("headline", lambda api: S.spheres_scene(api, nspheres=1024)),
    ("cornell_plastic", lambda api: S.cornell_scene(api, "plastic")),
    ("cornell_glass", lambda api: S.cornell_scene(api, "glass")),
])
def test_the_five_walls_get_two_records_each(name, build):
    records, bases = plan(build(G))
    assert records == 10 and bases == [0, 2, 4, 6, 8], (name, records, bases)


def test_uv_a_backface_swap_and_a_missing_material_are_in_the_record():
    for faces, build in ((2, lambda api: T.walls_scene(api)), (6, lambda api: T.walls_scene(api, T.strip_obj(6, uv="skew"), backface=True)),
                         (4, lambda api: T.walls_scene(api, T.strip_obj(4, uv="flat")))):
        records, bases = plan(build(G))
        assert records == 3 * faces and bases == [0, faces, 2 * faces], (faces, records, bases)


def test_a_mesh_with_vertex_normals_gets_none():
    assert plan(T.capped_scene(G, 6, normals=True)) == (0, [])
    assert plan(T.capped_scene(G, 6, normals=False)) == (6, [0])
    # ... and keeps no place among the others: the torus with normals between the walls of the instanced scene
    records, bases = plan(S.instanced_scene(G))
    assert records == 10 and bases == [0, 2, 4, 6, 8]


def test_the_instance_cap():
    assert plan(T.capped_scene(G, 1024)) == (1024, [0])
    assert plan(T.capped_scene(G, 1025)) == (0, [])


def test_the_accels_cap():
    assert plan(T.capped_scene(G, 1024, instances=4)) == (4096, [0, 1024, 2048, 3072])
    assert plan(T.capped_scene(G, 241, instances=17)) == (0, [])  # 17 x 241 = 4,097 records: no table at all
    assert plan(T.capped_scene(G, 256, instances=16)) == (4096, [256 * k for k in range(16)])
