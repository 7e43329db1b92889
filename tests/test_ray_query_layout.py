"""Ray queries on the CPU: the lg_hit record as the C compiler lays it out against its Python mirror, every new entry point exported by the
library, and the identity-tracking witness of tests/test_gpu_ray_query.py against the plain one (tests/pyref.py through tests/pyref_bvh.py)."""
import ctypes
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import pyref
import pyref_bvh

import lasgun_amd as la
from lasgun_amd import scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("t", "p", "ng", "ns", "kind", "prim", "instance", "material")
ENTRY_POINTS = ("lg_intersect", "lg_intersect_device", "lg_occluded", "lg_occluded_device", "lg_camera_rays", "lg_camera_rays_device",
                "lg_camera_samples", "lg_accel_material", "lg_accel_instance")


def test_lg_hit_layout_matches_the_header():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no host C compiler")
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"lasgun_hip.h\"\nint main(void) {\n    printf(\"%zu\", sizeof(lg_hit));\n"
    src += "".join('    printf(" %%zu", offsetof(lg_hit, %s));\n' % f for f in FIELDS) + "    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "layout")
        subprocess.check_call([cc, "-x", "c" if not cc.endswith("++") else "c++", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got[0] == 96 == la.HIT_DTYPE.itemsize == ctypes.sizeof(la.Hit)
    assert got[1:] == [la.HIT_DTYPE.fields[f][1] for f in FIELDS] == [getattr(la.Hit, f).offset for f in FIELDS]


def test_every_query_entry_point_is_exported():
    lib = ctypes.CDLL(la.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("builder", [lambda api: S.kitchen_sink_scene(api), lambda api: S.random_scene(api, 2), lambda api: S.tie_mesh_scene(api)],
                         ids=["kitchen_sink", "random_2", "tie_mesh"])
def test_identity_witness_agrees_with_pyref(builder):
    from query_witness import Witness
    from test_gpu_ray_query import seeded_rays
    traced, plain = builder(pyref.Api), builder(pyref.Api)
    pyref_bvh.install(plain)
    wit = Witness(traced)
    rays = seeded_rays(traced, 77, n_random=60)
    hits = 0
    for ray in rays:
        got, want = wit.closest(ray[:3], ray[3:]), pyref.closest(plain, tuple(map(float, ray[:3])), tuple(map(float, ray[3:])))
        assert (got is None) == (want is None), ray
        if got is not None:
            hits += 1
            assert struct.pack("<d", got["t"]) == struct.pack("<d", want["t"]), ray
            kind, prim, inst = got["id"]
            assert kind in (1, 2, 3) and prim >= 0 and 0 <= inst < wit.count["accel"]
    assert hits > 0
    assert wit.count["sphere"] == sum(1 for _ in _spheres(traced.root))


def _spheres(agg):
    for node in agg.contents:
        if node[0] == "sphere":
            yield node
        elif node[0] == "group":
            yield from _spheres(node[1])
