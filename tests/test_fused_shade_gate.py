"""The gate of the fused form of the camera's level 0, without a device (lasgun_amd/csrc/fused_host.h).

The predicate: tools/fused_gate_check.cpp, a stand-alone program with its own main over exactly the text launch.cpp includes, under
AddressSanitizer and UBSan on the CPU: one asking passes, every refusing condition alone flips it, no other combination passes.

And what it says for scenes (lg_scene_fused_shade_gate: the launch's conditions restated from the scene alone): the headline and the
one-light test scenes pass; two lights, no light, glass or a mirror with recursion (two levels and more), a scene graph the packet walk's
gate refuses and a level 0 that is not the camera's each refuse, with their own reason."""
import os
import shutil
import subprocess

import pytest

import fused_shade_scenes as F
import lasgun_amd as la
import level_door_scenes as D
from lasgun_amd import scenes as S
from shadow_skip_scenes import LIGHTS

G = la.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OWN_LEVEL0, LEVELS, NLIGHTS, NOT_PACKET, NOT_PAIRS = 0, 2, 3, 4, 5, 6  # fused_host.h, FusedRefusal


def test_the_gate_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "fused_gate_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fused_gate_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "fused_gate_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])


GATE = {
    "headline": (lambda api: S.spheres_scene(api, nspheres=1024), OK),
    "cornell_plastic": (lambda api: S.cornell_scene(api, "plastic"), OK),
    "one_light": (lambda api: F.sphere_scene(api, "plastic", F.ONE), OK),
    "one_light_metal": (lambda api: F.sphere_scene(api, "metal", F.ONE), OK),
    "shadowed": (F.shadowed_scene, OK),
    "speck": (F.speck_scene, OK),
    "zero_falloff": (lambda api: F.sphere_scene(api, "plastic", F.ZERO_FALLOFF), OK),
    # specular materials without recursion levels are one level: the form takes them
    "glass_recursion_0": (lambda api: F.sphere_scene(api, "glass", F.ONE, recursion=0), OK),
    # each refusing condition alone
    "two_lights": (lambda api: F.sphere_scene(api, "plastic", LIGHTS["two"]), NLIGHTS),
    "no_lights": (lambda api: F.sphere_scene(api, "plastic", []), NLIGHTS),
    "glass": (lambda api: F.sphere_scene(api, "glass", F.ONE), LEVELS),
    "mirror": (lambda api: F.sphere_scene(api, "mirror", F.ONE), LEVELS),
    "nested_groups": (F.nested_group_scene, NOT_PACKET),
}


@pytest.mark.parametrize("name", sorted(GATE))
def test_what_the_gate_says_for_the_scenes(name):
    build, want = GATE[name]
    scene = build(G)
    assert G.scene_fused_shade_gate(scene) == want
    # an own level 0 (a radiance query, a gather, a view batch, light groups, lit scatter over the same scene) never takes the form
    assert G.scene_fused_shade_gate(scene, camera_level0=False) == OWN_LEVEL0


def test_the_packet_gates_refusals_are_the_fused_gates():
    """Every scene graph the packet walk's gate refuses (test_packet_walk_predicate.py's table) is refused here, and for that reason once the
    other conditions hold; the scenes of that table have glass in them, so the levels speak first unless the recursion is taken away."""
    for build in (D.nested_scene, D.mesh_and_sphere_scene, D.srt_lone_scene):
        scene = build(G)
        assert G.scene_packet_walk_gate(scene) != 0
        assert G.scene_fused_shade_gate(scene) != OK
        scene.set_max_recursion_depth(0)
        assert G.scene_fused_shade_gate(scene) in (NLIGHTS, NOT_PACKET, NOT_PAIRS)
