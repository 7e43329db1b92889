"""Ray queries on the device against the CPU oracle (orc_intersect / orc_occluded, itself held to the witness by
tests/test_oracle_ray_query.py) on the edge-case rays of tests/edge_rays.py: every traversal form the accel accepts, the host and the
device entry points, the same rays in other lanes and other wave compositions.  No tolerance: t, p, ng and ns bit for bit (any NaN equals
any NaN), (kind, prim, instance) exact, the material's POD bits, the occlusion byte."""
import numpy as np
import pytest

import pyref
import edge_rays as E
import lasgun_amd as la
from lasgun_amd import scenes as S
from oracle_lib import oracle
from query_witness import Witness
from test_gpu_ray_query import big_batch

pytestmark = pytest.mark.gpu

G = la.api
NTHREADS = 16
if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference never reads it, camera.rs:142)
    pyref.Camera.set_aperture_radius = lambda self, radius: self

SCENES = [("kitchen_sink", lambda api: S.kitchen_sink_scene(api), {}),
          ("instanced", lambda api: S.instanced_scene(api), {}),
          ("tie_mesh", lambda api: S.tie_mesh_scene(api), {}),
          ("exotic_obj", lambda api: S.exotic_obj_scene(api), {}),
          ("random_2", lambda api: S.random_scene(api, 2), {}),
          ("spheres", lambda api: S.spheres_scene(api), {}),
          ("mesh", lambda api: S.mesh_scene(api, nu=64, nv=64, material="metal"), {}),
          ("mixed", lambda api: S.mixed_scene(api, nspheres=256, nu=64, nv=64), {}),
          ("f3", E.f3_scene, {}),
          ("f7", E.f7_scene, {"huge": True}),
          ("grid", E.grid_scene, {"mesh": True})]
BIG = ("spheres", "mesh", "mixed")


def forms(accel):
    """(name, setup) of every traversal form the accel accepts: reference, pruned, LDS-resident, LDS + pruned, fast."""
    def ref():
        G.set_mode(accel, False)
        G.set_prune(accel, False)
        G.set_lds_scene(accel, False)
    out = [("reference", ref), ("prune", lambda: (ref(), G.set_prune(accel, True)))]
    ref()
    if G.set_lds_scene(accel, True):
        out += [("lds", lambda: (ref(), G.set_lds_scene(accel, True))),
                ("lds+prune", lambda: (ref(), G.set_prune(accel, True), G.set_lds_scene(accel, True)))]
    ref()
    try:
        G.set_mode(accel, True)
    except la.LasgunError:
        pass  # (a scene the fast mode refuses)
    else:
        out.append(("fast", lambda: (ref(), G.set_mode(accel, True))))
    ref()
    return out


class Expect:
    """The oracle's answers for one scene, and the comparison of the device's against them."""

    def __init__(self, oaccel, rays, fam):
        self.rays, self.fam = rays, fam
        o = oracle()
        o.set_trig_mode(True)  # the sphere's trigonometry the device runs (its normals compare bit for bit)
        try:
            self.hits, self.mats = o.intersect(oaccel, rays, NTHREADS)
            self.occ = o.occluded(oaccel, rays, NTHREADS)
        finally:
            o.set_trig_mode(False)

    def check(self, accel, hits, occ, ctx, sel=None):
        want = self.hits if sel is None else self.hits[sel]
        wmat = self.mats if sel is None else self.mats[sel]
        wocc = self.occ if sel is None else self.occ[sel]
        fam = self.fam if sel is None else self.fam[sel]
        rays = self.rays if sel is None else self.rays[sel]
        bad = np.zeros(len(want), dtype=bool)
        for k in ("t", "p", "ng", "ns"):
            a, b = hits[k].reshape(len(want), -1), want[k].reshape(len(want), -1)
            same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
            bad |= ~same.all(axis=1)
        for k in ("kind", "prim", "instance"):
            bad |= hits[k] != want[k]
        hit = want["kind"] != 0
        bad |= (hits["material"] == -1) == hit
        table = {m: G.accel_material(accel, int(m)) for m in np.unique(hits["material"][hit & ~bad])}
        for i in np.where(hit & ~bad)[0]:
            m = table[hits["material"][i]]
            bad[i] = m["kind"] != wmat["kind"][i] or np.array(m["p"]).view(np.int64).tolist() != wmat["p"][i].view(np.int64).tolist()
        occ_bad = occ != wocc
        if bad.any() or occ_bad.any():
            i = int(np.where(bad | occ_bad)[0][0])
            raise AssertionError("%s: %d hit and %d occlusion mismatches; first: ray %d (%s) %r\n  device %r occluded %d\n  oracle %r occluded %d"
                                 % (ctx, int(bad.sum()), int(occ_bad.sum()), i, fam[i], rays[i].tolist(), hits[i], occ[i], want[i], wocc[i]))


def suite(name, builder, kw):
    gscene, pscene, oscene = builder(G), builder(pyref.Api), builder(oracle())
    lo, hi, boxes = E.scene_geometry(Witness(pscene), pscene)
    rays, fam = E.edge_rays(lo, hi, boxes=boxes, seed=len(name), **kw)
    return G.Accel.from_scene(gscene), oracle().Accel.from_scene(oscene), rays, fam, (gscene, oscene)


@pytest.mark.parametrize("name,builder,kw", SCENES, ids=[s[0] for s in SCENES])
def test_edge_rays_match_the_oracle_in_every_form(name, builder, kw):
    accel, oaccel, rays, fam, keep = suite(name, builder, kw)
    exp = Expect(oaccel, rays, fam)
    n = len(rays)
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    filler = rays[fam == "F1"]
    for form, setup in forms(accel):
        setup()
        exp.check(accel, G.intersect(accel, rays), G.occluded(accel, rays), (name, form))
        # other lanes, other wave compositions: shuffled, and shifted by filler rays
        exp.check(accel, G.intersect(accel, rays[perm]), G.occluded(accel, rays[perm]), (name, form, "shuffled"), sel=perm)
        for shift in (1, 17, 63):
            r = np.concatenate([filler[:shift], rays])
            h, o = G.intersect(accel, r), G.occluded(accel, r)
            exp.check(accel, h[shift:], o[shift:], (name, form, "shift", shift))
        for m in (1, 63, 64, 65):
            sel = perm[:m]
            exp.check(accel, G.intersect(accel, rays[sel]), G.occluded(accel, rays[sel]), (name, form, "n", m), sel=sel)
    # non-vacuous: per family, at least this many hits and misses (F3's twins all run along the grid's border lines: misses only there)
    hit = exp.hits["kind"] != 0
    least = {"F1": (64, 64), "F2": (256, 256), "F3": (0 if name == "grid" else 8, 24), "F4": (8, 8), "F5": (64, 64), "F6": (8, 8),
             "F7": (24, 0)}
    for f in sorted(set(fam)):
        assert (hit & (fam == f)).sum() >= least[f][0] and (~hit & (fam == f)).sum() >= least[f][1], (name, f)
    assert ("F5" in fam) == bool(kw.get("mesh")) and ("F7" in fam) == bool(kw.get("huge"))
    assert exp.occ.any() and not exp.occ.all()
    nonfinite = hit & ~np.isfinite(exp.hits["t"])
    assert nonfinite.sum() >= 4, name  # (winners at t = NaN / +inf: the rays the any-hit exit and the transform of non-finite origins must get right)
    if kw.get("huge"):
        nan = np.isnan(exp.hits["t"]) & (fam == "F7")
        assert nan.sum() >= 1 and exp.occ[nan].sum() == 0, name
        plain = oracle().Accel.from_scene(E.f7_scene(oracle(), with_sphere=False))
        h0, _ = oracle().intersect(plain, rays[nan])
        assert (h0["t"] < 1.0).any(), "no F7 ray has a finite t < 1 before its NaN winner"
    del keep


@pytest.mark.parametrize("name", BIG)
def test_a_million_rays_match_the_oracle(name):
    builder = dict((s[0], s[1]) for s in SCENES)[name]
    gscene, oscene = builder(G), builder(oracle())
    accel, oaccel = G.Accel.from_scene(gscene), oracle().Accel.from_scene(oscene)
    rays = big_batch(accel, 21)
    exp = Expect(oaccel, rays, np.array(["big"] * len(rays)))
    assert exp.occ.any() and not exp.occ.all()
    for form, setup in forms(accel):
        setup()
        exp.check(accel, G.intersect(accel, rays), G.occluded(accel, rays), (name, form))


def test_edge_rays_through_the_device_entry_points():
    torch = pytest.importorskip("torch")
    accel, oaccel, rays, fam, keep = suite("f7", E.f7_scene, {"huge": True})
    exp = Expect(oaccel, rays, fam)
    n = len(rays)
    dr = torch.from_numpy(rays.copy()).cuda()
    dh = torch.zeros((n * 96,), dtype=torch.uint8, device="cuda")
    do = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        s = torch.cuda.current_stream().cuda_stream
        G.intersect_device(accel, n, dr.data_ptr(), dh.data_ptr(), stream=s)
        G.occluded_device(accel, n, dr.data_ptr(), do.data_ptr(), stream=s)
    stream.synchronize()
    hits = np.frombuffer(dh.cpu().numpy().tobytes(), dtype=la.HIT_DTYPE)
    exp.check(accel, hits, do.cpu().numpy().astype(bool), ("f7", "device entry points"))
    del keep
