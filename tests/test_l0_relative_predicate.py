"""The level-0 closest pass's origin-relative form, the parts that need no device.
The gate (host.cpp, l0_relative_camera / l0_relative_origins through lg_scene_l0_relative_origins): on for a perspective camera with a clean
origin, off for an orthographic one, an origin with a -0, infinite or NaN component, a non-finite up.  The host's table of per-accel local
origins against a plain-Python restatement of the parent chain (tests/pyref.py, transform_point), bit for bit.  The `_rel` slab forms and
the rel sphere slot (walk.h), restated in numpy beside the absolute forms, on >= 1e5 (box, origin, direction) triples and on the edge-case
rays: the same bits -- a guard against a slip in the transcription, not a proof.  The host functions once more in a stand-alone program
under ASan + UBSan (tools/l0_relative_host_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import edge_rays as E
import lasgun_amd as la
import level_door_scenes as D
import pyref
from lasgun_amd import scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = la.api
if not hasattr(pyref.Camera, "set_aperture_radius"):
    pyref.Camera.set_aperture_radius = lambda self, radius: self

SCENES = {"spheres64": lambda api: S.spheres_scene(api, nspheres=64), "cornell_plastic": lambda api: S.cornell_scene(api, "plastic"),
          "cornell_glass": lambda api: S.cornell_scene(api, "glass"), **D.SMALL}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def with_camera(builder, origin=None, look=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), ortho=False):
    scene = builder(G)
    if ortho:
        scene.set_orthographic_camera(4.5).look_at(list(origin or (0.3, 0.4, 5.0)), list(look), list(up))
    elif origin is not None:
        scene.camera.look_at(list(origin), list(look), list(up))
    return scene


def test_the_gate_table():
    b = SCENES["spheres64"]
    assert G.l0_relative_origins(with_camera(b)) is not None
    assert G.l0_relative_origins(with_camera(b, (0.3, 0.4, 5.0))) is not None
    assert G.l0_relative_origins(with_camera(b, (0.0, 0.4, 5.0))) is not None, "a +0 component is clean"
    assert G.l0_relative_origins(with_camera(b, ortho=True)) is None
    for bad in ((-0.0, 0.4, 5.0), (0.3, -0.0, 5.0), (0.3, 0.4, -0.0), (float("inf"), 0.4, 5.0), (0.3, float("-inf"), 5.0), (0.3, 0.4, float("nan"))):
        assert G.l0_relative_origins(with_camera(b, bad)) is None, bad
    assert G.l0_relative_origins(with_camera(b, (0.3, 0.4, 5.0), up=(float("nan"), 1.0, 0.0))) is None
    assert G.l0_relative_origins(with_camera(b, (0.3, 0.4, 5.0), up=(float("inf"), 1.0, 0.0))) is None
    assert G.l0_relative_origins(with_camera(b, (0.0, 0.0, 5.0), up=(0.0, 0.0, 1.0))) is None, "up along the view: cross() is zero, normalize() makes NaNs"


def python_origins(agg, origin, out):
    """The camera's origin in the local space of every accel, accels in pre-order (host.cpp, Flattener::aggregate): a group applies its minv to
    its parent's origin, a mesh is an accel of its own under the identity."""
    o = pyref.transform_point(agg.transform.minv, origin)
    out.append(o)
    for node in agg.contents:
        if node[0] == "group":
            python_origins(node[1], o, out)
        elif node[0] == "mesh":
            out.append(pyref.transform_point(pyref.mat_identity(), o))
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_host_table_is_the_parent_chain(name):
    for origin in (None, (0.0, 0.4, 5.0), (1e6, -3e5, 2.5e6)):
        got = G.l0_relative_origins(with_camera(SCENES[name], origin))
        pscene = SCENES[name](pyref.Api)
        if origin is not None:
            pscene.camera.look_at(origin, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        want = np.array(python_origins(pscene.root, pscene.camera.origin, []), dtype=np.float64)
        assert got is not None and got.shape == want.shape, (name, origin)
        assert np.array_equal(bits(got), bits(want)), (name, origin, got, want)
        assert np.array_equal(bits(got[0]), bits(np.array(pscene.camera.origin))), "the root of these scenes is the identity"
    if name in D.SMALL and name != "identity_lone":
        assert len({tuple(r) for r in bits(got).tolist()}) >= 2, "a transformed group sees the origin elsewhere"


# ---- the forms, restated from walk.h ---------------------------------------------------------------------------------------------------
def fmin(a, b):
    return np.fmin(a, b)  # NaN-ignoring, as f64::min


def fmax(a, b):
    return np.fmax(a, b)


def slab_nc(lo, hi, o, dinv, rel):
    """slab_intersects_nc / slab_intersects_nc_rel: `lo`, `hi` are bmin, bmax -- or, rel, the record's bmin - o, bmax - o."""
    tn = tf = None
    for a in range(3):
        t1 = (lo[:, a] * dinv[:, a]) if rel else ((lo[:, a] - o[:, a]) * dinv[:, a])
        t2 = (hi[:, a] * dinv[:, a]) if rel else ((hi[:, a] - o[:, a]) * dinv[:, a])
        tn = fmin(t1, t2) if tn is None else fmax(tn, fmin(t1, t2))
        tf = fmax(t1, t2) if tf is None else fmin(tf, fmax(t1, t2))
    return tn, tf, ~(tn > tf) & ~(tf <= 0.0)


def slab_sg(lo, hi, o, dinv, rel):
    """slab_intersects_sg<SG> / slab_intersects_sg_rel<SG>, SG per ray from the signs of dinv (the walk's neg_mask)."""
    near, far = [], []
    for a in range(3):
        neg = dinv[:, a] < 0.0
        n, f = np.where(neg, hi[:, a], lo[:, a]), np.where(neg, lo[:, a], hi[:, a])
        near.append(n * dinv[:, a] if rel else (n - o[:, a]) * dinv[:, a])
        far.append(f * dinv[:, a] if rel else (f - o[:, a]) * dinv[:, a])
    tn = fmax(fmax(near[0], near[1]), near[2])
    tf = fmin(fmin(far[0], far[1]), far[2])
    return tn, tf, ~(tn > tf) & ~(tf <= 0.0)


def sphere_slot(cen, r2, o, d, rel):
    """The sphere slot up to the discriminant (walk.h): rel, `cen` holds l = o - cen and `r2` holds c = dot(l, l) - r * r."""
    l = cen if rel else o - cen
    b = 2.0 * ((d[:, 0] * l[:, 0] + d[:, 1] * l[:, 1]) + d[:, 2] * l[:, 2])
    c = r2 if rel else ((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]) - r2
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return b, c, b * b - (4.0 * dd) * c


def same(a, b):
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def triples(n, seed):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-3.0, 3.0, (n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 1))
    hi = lo + rng.uniform(0.0, 2.0, (n, 3)) * (rng.random((n, 3)) > 0.1)  # some boxes without thickness on an axis
    o = rng.uniform(-6.0, 6.0, (n, 3))
    k = rng.integers(0, n, n // 8)
    o[k, rng.integers(0, 3, n // 8)] = lo[k, 0]  # origins that share a coordinate with a box plane
    d = rng.normal(size=(n, 3))
    aimed = rng.random(n) < 0.5  # half the rays are aimed at (about) their box, so that both verdicts are common
    d[aimed] = (lo + (hi - lo) * rng.uniform(-0.3, 1.3, (n, 3)) - o)[aimed]
    d *= rng.random((n, 3)) > 0.05  # some exact zeros
    d[rng.integers(0, n, n // 16), rng.integers(0, 3, n // 16)] = -0.0
    return lo, hi, o, d


def check_forms(lo, hi, o, d):
    with np.errstate(all="ignore"):
        dinv = 1.0 / d
        rlo, rhi = lo - o, hi - o  # what l0_rewrite leaves in a node record
        for form in (slab_nc, slab_sg):
            ta, fa, ha = form(lo, hi, o, dinv, False)
            tr, fr, hr = form(rlo, rhi, o, dinv, True)
            assert same(ta, tr) and same(fa, fr) and np.array_equal(ha, hr), form.__name__
        cen, r2 = 0.5 * (lo + hi), (0.25 * (hi[:, 0] - lo[:, 0])) ** 2
        l = o - cen
        c = ((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]) - r2  # what l0_rewrite leaves in a sphere slot
        for x, y in zip(sphere_slot(cen, r2, o, d, False), sphere_slot(l, c, o, d, True)):
            assert same(x, y)
        return int(ha.sum())


def test_the_rel_forms_give_the_absolute_forms_bits():
    lo, hi, o, d = triples(1 << 17, 5)
    hits = check_forms(lo, hi, o, d)
    assert len(lo) >= 100000 and 0.02 * len(lo) < hits < 0.98 * len(lo), hits
    # the edge-case rays, against boxes around and on their origins
    rays, fam = E.edge_rays((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), boxes=(((-1.0, -1.0, -1.0), (1.0, 0.0, 1.0)),), seed=3)
    assert len(set(fam.tolist())) >= 4
    rng = np.random.default_rng(9)
    for box_lo, box_hi in (((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)), ((-1.0, -1.0, -1.0), (1.0, 0.0, 1.0)), (None, None)):
        n = len(rays)
        blo = np.tile(np.array(box_lo), (n, 1)) if box_lo else rays[:, :3] - rng.integers(0, 2, (n, 3))  # a plane through the origin itself
        bhi = np.tile(np.array(box_hi), (n, 1)) if box_hi else blo + 1.0
        check_forms(blo, bhi, rays[:, :3].copy(), rays[:, 3:].copy())


def test_the_host_functions_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "l0_relative_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O0", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "l0_relative_host_check.cpp"),
                           os.path.join(ROOT, "lasgun_amd", "csrc", "host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "l0_relative_host_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    # the table it prints for the five walls and a sphere, camera at (0.25, 0.5, 6): the root sees the origin itself, every wall a point of its own
    rows = [list(map(float.fromhex, line.split()[3:])) for line in run.stdout.splitlines() if line.startswith("walls accel")]
    assert len(rows) == 11 and rows[0] == [0.25, 0.5, 6.0] and len({tuple(r) for r in rows}) == 6, rows
