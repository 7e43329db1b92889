"""What tests/test_gpu_stream_contract.py is built from: a stream held by a kernel that ends by itself, device outputs between guard
words, one `Op` per *_device entry point (its reference from the synchronous host form of the same call, its host tables overwritten with
another valid table as soon as the call returns), and the seeded program of calls that is enqueued behind one blocker.

The blocker is torch.cuda._sleep, calibrated once with two events; nothing here waits for a word the host writes.  Every host table an
Op passes is a private copy, pageable or page-locked, that is overwritten with the OTHER valid table of its pair right after the call
and then dropped: a library that read the caller's memory late would read valid records (and give the other table's answer), never
garbage."""
import re
import os
import time

import numpy as np

import lasgun_amd as la
from lasgun_amd import scenes as S

G = la.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = 2.0 ** -36          # the shading offset (integrate.rs:40)
GUARD = 256               # bytes before and behind every output (keeps the 16-byte alignment of lg_hit and id planes)
FILL = 0xA5
SMALL, MID, LARGE = 65, 64 * 7 + 5, 64 * 64 + 37
SCENES = {"cornell_glass": lambda api: S.cornell_scene(api, "glass"),                          # resident in LDS
          "instanced": lambda api: S.instanced_scene(api),                                     # tables in L2, the reference walk
          "mesh_glass": lambda api: S.mesh_scene(api, nu=48, nv=48, material="glass")}         # the scene the fast mode is run on
FORMS = [("cornell_glass", "lds"), ("instanced", "reference"), ("mesh_glass", "fast")]
VIEW_DTYPE = np.dtype(la.View)
GROUP_DTYPE = np.dtype([("lights", np.uint32), ("flags", np.uint32)])  # lg_light_group
assert VIEW_DTYPE.itemsize == 120 and GROUP_DTYPE.itemsize == 8


def max_launch_ctxs():
    """MAX_LAUNCH_CTXS as csrc/internal.h states it."""
    text = open(os.path.join(ROOT, "lasgun_amd", "csrc", "internal.h")).read()
    m = re.search(r"constexpr\s+size_t\s+MAX_LAUNCH_CTXS\s*=\s*(\d+)\s*;", text)
    assert m, "internal.h no longer states MAX_LAUNCH_CTXS"
    return int(m.group(1))


def set_form(accel, form):
    G.set_mode(accel, False)
    G.set_prune(accel, form == "prune")
    fits = G.set_lds_scene(accel, form == "lds")
    if form == "lds":
        assert fits, "the scene is meant to sit in LDS"
    if form == "fast":
        G.set_mode(accel, True)


# ---- the blocker ---------------------------------------------------------------------------------------------------------------------------
class Blocker:
    """A kernel that holds a stream for a time and ends by itself."""
    FACTOR, FLOOR, CAP = 8.0, 0.25, 2.0
    _rate = None  # _sleep cycles per second, measured once per session

    @classmethod
    def rate(cls, torch):
        if cls._rate is None:
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            cycles = 2_000_000
            while True:
                a.record()
                torch.cuda._sleep(cycles)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                if ms >= 5.0 or cycles >= 1 << 34:
                    break
                cycles *= 4
            cls._rate = cycles / (ms * 1e-3)
            print("blocker: %d cycles slept %.2f ms: %.3g cycles a second" % (cycles, ms, cls._rate))
        return cls._rate

    @classmethod
    def seconds_for(cls, enqueue_seconds, what):
        t = max(cls.FACTOR * enqueue_seconds, cls.FLOOR)
        assert t <= cls.CAP, "%s: enqueueing took %.3f s on the idle stream; a blocker of %.2f s is over the cap of %.1f s" % (what, enqueue_seconds, t, cls.CAP)
        return t

    @classmethod
    def hold(cls, torch, stream, seconds):
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(seconds * cls.rate(torch)))


# ---- outputs between guard words -----------------------------------------------------------------------------------------------------------
class Out:
    """`nbytes` of device memory over a prefill, GUARD bytes of the prefill on either side."""

    def __init__(self, torch, nbytes):
        self.nbytes = int(nbytes)
        self.t = torch.full((GUARD + (self.nbytes + 15) // 16 * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def reset(self):
        self.t.fill_(FILL)

    def check(self, ref, ctx):
        """ref: the bytes expected, or None for a plane that was not asked for (it keeps the prefill)."""
        back = self.t.cpu().numpy()
        assert (back[:GUARD] == FILL).all() and (back[GUARD + self.nbytes:] == FILL).all(), (ctx, "the guard words")
        body = back[GUARD:GUARD + self.nbytes]
        if ref is None:
            assert (body == FILL).all(), (ctx, "a plane that was not asked for")
        else:
            assert len(ref) == self.nbytes, (ctx, len(ref), self.nbytes)
            want = np.frombuffer(ref, dtype=np.uint8)
            assert body.tobytes() == ref, (ctx, "bytes differ", int((body != want).sum()), "of", self.nbytes)


def prefilled(shape, dtype):
    """A host array of the prefill's bytes: what a device output holds where a call writes nothing."""
    a = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8)
    return a.view(dtype).reshape(shape)


def words_differing(a, b):
    """The share of the 32-bit words of two references (lists of byte strings) that differ."""
    x = np.frombuffer(b"".join(r + b"\0" * (-len(r) % 4) for r in a), dtype=np.uint32)
    y = np.frombuffer(b"".join(r + b"\0" * (-len(r) % 4) for r in b), dtype=np.uint32)
    assert x.shape == y.shape
    return float((x != y).mean())


class Op:
    """One device call: run(stream handle) enqueues it; outs = [(Out, reference bytes or None)]; alt = the references under the OTHER
    table of the pair (the one the caller's copy is overwritten with), in the order of the outs that have a reference."""

    def __init__(self, name, run, outs, keep=(), alt=None):
        self.name, self.run, self.outs, self.keep, self.alt = name, run, list(outs), keep, alt

    def refs(self):
        return [r for _, r in self.outs if r is not None]

    def check(self, ctx=None):
        for i, (o, ref) in enumerate(self.outs):
            o.check(ref, (ctx, self.name, i))

    def reset(self):
        for o, _ in self.outs:
            o.reset()

    def tables_matter(self):
        """The pair of tables changes the answer: at least 10 % of the output words differ."""
        assert self.alt is not None, self.name
        f = words_differing(self.refs(), self.alt)
        assert f >= 0.10, (self.name, "the two tables of the pair give nearly the same answer", f)
        return f


def pinned_like(torch, arr):
    """An array of arr's shape and dtype in PAGE-LOCKED host memory, what a torch pipeline hands over: a copy the library left to the
    runtime would be a DMA in stream order, reading the table after the caller has overwritten it (a pageable source the runtime reads
    before hipMemcpyAsync returns)."""
    raw = torch.empty(max(arr.nbytes, 1), dtype=torch.uint8, pin_memory=True)
    assert raw.is_pinned()
    return raw.numpy()[:arr.nbytes].view(arr.dtype).reshape(arr.shape)


def tabled(tab, other, call, torch=None):
    """run(s) for a call that takes a host table: a private copy of `tab` goes in and is overwritten with `other` on return.  The
    pageable copy (torch None) is then dropped; the page-locked one (torch given) is kept until the Op runs again, so that its block is
    not handed to a table of another kind while a late reader could still see it: valid for valid, always."""
    assert tab.dtype == other.dtype and tab.shape == other.shape and tab.tobytes() != other.tobytes()
    held = [None]

    def run(s):
        t = np.ascontiguousarray(tab).copy() if torch is None else pinned_like(torch, tab)
        t[...] = tab
        call(t, s)
        t[...] = other
        held[0] = t if torch is not None else None
        del t
    return run


def cviews(tab):
    return [la.View.from_buffer_copy(tab[i].tobytes()) for i in range(len(tab))]


# ---- a scene, its rays and points, and one Op per entry point ---------------------------------------------------------------------------------
class Env:
    def __init__(self, torch, name, form, seed=0):
        self.torch, self.name, self.form = torch, name, form
        self.acc = G.Accel.from_scene(SCENES[name](G))
        set_form(self.acc, form)
        G.set_streaming(self.acc, 2)  # the renders level by level: an organisation that is named is never measured (the one documented wait)
        assert G.camera_samples(self.acc) == 1
        self.rng = np.random.default_rng(seed)
        cam = G.camera_rays(self.acc, 96, 64)
        hits = G.intersect(self.acc, cam)
        hit = hits["kind"] != 0
        back = cam.copy()
        back[:, 3:] = -back[:, 3:]
        self.hit_rays = cam[hit]
        self.miss_rays = np.concatenate([cam[~hit], back[G.intersect(self.acc, back)["kind"] == 0]])
        assert len(self.hit_rays) >= 256 and len(self.miss_rays) >= 256, (name, len(self.hit_rays), len(self.miss_rays))
        self.reach = 2.0 * float(np.median(hits["t"][hit]))
        sel = hits[hit]
        self.points = np.ascontiguousarray(sel["p"] + sel["ng"] * ERR)
        self.normals = np.ascontiguousarray(sel["ng"])
        self.lo, self.hi = self.points.min(axis=0), self.points.max(axis=0)
        self.size = float(np.linalg.norm(self.hi - self.lo))
        self.nlights = G.light_count(self.acc)
        assert self.nlights >= 1

    # -- inputs
    def dev(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).cuda()

    def out(self, nbytes):
        return Out(self.torch, nbytes)

    def rays(self, n):
        """n rays in no order, about half of which hit: asserted on the host form's answer (hits and misses each at least 15 %)."""
        nh = n // 2
        r = np.concatenate([self.hit_rays[self.rng.integers(0, len(self.hit_rays), nh)], self.miss_rays[self.rng.integers(0, len(self.miss_rays), n - nh)]])
        r = np.ascontiguousarray(r[self.rng.permutation(n)])
        f = float((G.intersect(self.acc, r)["kind"] != 0).mean())
        assert 0.15 <= f <= 0.85, (self.name, "hits", f)
        return r

    def segments(self, n):
        r = self.rays(n)
        r[:, 3:] *= self.reach
        return r

    def pts(self, n):
        idx = self.rng.integers(0, len(self.points), n)
        return np.ascontiguousarray(self.points[idx]), np.ascontiguousarray(self.normals[idx])

    def lights(self, k):
        t = np.zeros(k, dtype=la.LIGHT_DTYPE)
        t["position"] = self.rng.uniform(self.lo - 0.1 * self.size, self.hi + 0.1 * self.size, (k, 3))
        t["intensity"] = self.rng.uniform(0.2, 1.0, (k, 3))
        t["falloff"] = (1.0, 0.0, 0.0)
        return t

    def views(self, k):
        tab = np.zeros(k, dtype=VIEW_DTYPE)
        base = G.accel_view(self.acc)
        for i in range(k):
            tab[i:i + 1] = np.frombuffer(bytes(base), dtype=VIEW_DTYPE)
            tab["origin"][i] += self.rng.normal(0.0, 0.05 * self.size, 3)
        return tab

    def rules(self, default, gain):
        return G.path_rules(self.acc, default=default, gain=gain)

    def groups(self, flip):
        full = (1 << self.nlights) - 1
        g = np.zeros(2, dtype=GROUP_DTYPE)
        g["lights"] = (0, full) if flip else (full, 0)
        g["flags"] = (la.GROUP_AMBIENT, 0)
        return g

    # -- plane helpers
    def _planes(self, ref, every):
        """(outs, ptrs): an Out per plane of `every`, those of `ref` with its bytes, the rest not asked for."""
        outs, ptrs = [], {}
        for p in every:
            if p in ref:
                o = self.out(ref[p].nbytes)
                outs.append((o, ref[p].tobytes()))
                ptrs[p + "_ptr"] = o.ptr
            else:
                outs.append((self.out(64), None))
        return outs, ptrs

    # -- ray queries
    def intersect(self, rays, d=None, o=None):
        n = len(rays)
        d = d if d is not None else self.dev(rays)
        o = o or self.out(n * 96)
        return Op("intersect", lambda s: G.intersect_device(self.acc, n, d.data_ptr(), o.ptr, stream=s), [(o, G.intersect(self.acc, rays).tobytes())], keep=(d,))

    def occluded(self, segs, d=None, o=None):
        n = len(segs)
        d = d if d is not None else self.dev(segs)
        o = o or self.out(n)
        ref = G.occluded(self.acc, segs).astype(np.uint8).tobytes()
        return Op("occluded", lambda s: G.occluded_device(self.acc, n, d.data_ptr(), o.ptr, stream=s), [(o, ref)], keep=(d,))

    def radiance(self, rays, d=None, o=None):
        n = len(rays)
        d = d if d is not None else self.dev(rays)
        o = o or self.out(n * 24)
        return Op("radiance", lambda s: G.radiance_device(self.acc, n, d.data_ptr(), o.ptr, stream=s), [(o, G.radiance(self.acc, rays).tobytes())], keep=(d,))

    def query_order(self, rays):
        n, d = len(rays), self.dev(rays)
        perm, keys = G.query_order(self.acc, rays)
        op, ok = self.out(n * 4), self.out(n * 4)
        return Op("query_order", lambda s: G.query_order_device(self.acc, n, d.data_ptr(), op.ptr, ok.ptr, stream=s), [(op, perm.tobytes()), (ok, keys.tobytes())], keep=(d,))

    def visibility(self, nf, nt):
        (f, _), (t, _) = self.pts(nf), self.pts(nt)
        df, dt = self.dev(f), self.dev(t)
        bits, blocked = G.visibility(self.acc, f, t, counts=True)
        ob, oc = self.out(bits.nbytes), self.out(blocked.nbytes)
        return Op("visibility", lambda s: G.visibility_device(self.acc, nf, df.data_ptr(), nt, dt.data_ptr(), ob.ptr, None, oc.ptr, stream=s),
                  [(ob, bits.tobytes()), (oc, blocked.tobytes())], keep=(df, dt))

    def open_directions(self, n, k):
        p, nrm = self.pts(n)
        dirs = la.sphere_directions(k, 0.5 * self.reach)
        dp, dn, dd = self.dev(p), self.dev(nrm), self.dev(dirs)
        bits, nopen, above = G.open_directions(self.acc, p, dirs, nrm, counts=True)
        outs = [(self.out(a.nbytes), a.tobytes()) for a in (bits, nopen, above)]
        return Op("open_directions", lambda s: G.open_directions_device(self.acc, n, dp.data_ptr(), dn.data_ptr(), k, dd.data_ptr(), outs[0][0].ptr, None, outs[1][0].ptr,
                                                                        outs[2][0].ptr, stream=s), outs, keep=(dp, dn, dd))

    def range_scan(self, n, k):
        o, _ = self.pts(n)
        beams = la.sphere_directions(k)
        do, db = self.dev(o), self.dev(beams)
        ref = G.range_scan(self.acc, o, beams, None, planes=("range", "point", "id", "hits", "nearest"))
        outs, ptrs = self._planes(ref, la.SCAN_PLANES)
        return Op("range_scan", lambda s: G.range_scan_device(self.acc, n, do.data_ptr(), None, k, db.data_ptr(), stream=s, **ptrs), outs, keep=(do, db))

    def hit_layers(self, rays, k=3):
        n, d = len(rays), self.dev(rays)
        ref = G.hit_layers(self.acc, rays, k, planes=("hits", "along", "count", "inside"))
        outs, ptrs = self._planes(ref, la.LAYER_PLANES)
        return Op("hit_layers", lambda s: G.hit_layers_device(self.acc, n, d.data_ptr(), k, stream=s, **ptrs), outs, keep=(d,))

    PATH_ASKED = ("point", "id", "count", "end", "gain")

    def trace_paths(self, rays, rules, other, k=3, d=None, pinned=False):
        n = len(rays)
        d = d if d is not None else self.dev(rays)
        ref = G.trace_paths(self.acc, rays, k, rules, planes=self.PATH_ASKED)
        alt = G.trace_paths(self.acc, rays, k, other, planes=self.PATH_ASKED)
        outs, ptrs = self._planes(ref, la.PATH_PLANES)
        run = tabled(rules, other, lambda t, s: G.trace_paths_device(self.acc, n, d.data_ptr(), k, t, stream=s, **ptrs), self.torch if pinned else None)
        return Op("trace_paths pinned" if pinned else "trace_paths", run, outs, keep=(d,), alt=[alt[p].tobytes() for p in la.PATH_PLANES if p in alt])

    def scatter(self, rays):
        n, d = len(rays), self.dev(rays)
        ref = G.scatter(self.acc, rays, planes=("hits", "direct", "flags", "reflect", "refract_weight"))
        outs, ptrs = self._planes(ref, la.SCATTER_PLANES)
        return Op("scatter", lambda s: G.scatter_device(self.acc, n, d.data_ptr(), stream=s, **ptrs), outs, keep=(d,))

    LIT_ASKED = ("direct", "flags", "terms", "visible")

    def scatter_lit(self, rays, lights, other, d=None, pinned=False):
        n = len(rays)
        d = d if d is not None else self.dev(rays)
        amb = (0.05, 0.04, 0.03)
        ref = G.scatter_lit(self.acc, rays, lights, amb, planes=self.LIT_ASKED)
        alt = G.scatter_lit(self.acc, rays, other, amb, planes=self.LIT_ASKED)
        outs, ptrs = self._planes(ref, la.LIT_PLANES)
        run = tabled(lights, other, lambda t, s: G.scatter_lit_device(self.acc, n, d.data_ptr(), lights=t, ambient=amb, stream=s, **ptrs),
                     self.torch if pinned else None)
        return Op("scatter_lit shared pinned" if pinned else "scatter_lit shared", run, outs, keep=(d,), alt=[alt[p].tobytes() for p in la.LIT_PLANES if p in alt])

    def scatter_lit_per_ray(self, rays, k):
        n, d = len(rays), self.dev(rays)
        tab = self.lights(n * k).reshape(n, k)
        dt = self.dev(tab)
        ref = G.scatter_lit(self.acc, rays, tab, (0.0, 0.0, 0.0), planes=self.LIT_ASKED)
        outs, ptrs = self._planes(ref, la.LIT_PLANES)
        return Op("scatter_lit per ray", lambda s: G.scatter_lit_device(self.acc, n, d.data_ptr(), per_ray_lights_ptr=dt.data_ptr(), count=k, stream=s, **ptrs), outs,
                  keep=(d, dt))

    def radiance_groups(self, rays, groups, other, d=None):
        n = len(rays)
        d = d if d is not None else self.dev(rays)
        pairs = lambda g: [(int(x["lights"]), int(x["flags"])) for x in g]  # noqa: E731
        ref = G.radiance_groups(self.acc, rays, pairs(groups))
        alt = G.radiance_groups(self.acc, rays, pairs(other))
        o = self.out(ref.nbytes)

        def call(t, s):
            if G.call("radiance_groups_device", self.acc.h, d.data_ptr(), n, t.ctypes.data, len(t), o.ptr, int(s)):
                raise la.LasgunError(G.last_error())
        return Op("radiance_groups", tabled(groups, other, call), [(o, ref.tobytes())], keep=(d,), alt=[alt.tobytes()])

    # -- films from rays and poses
    def capture_rays(self, rays, samples, w=64):
        slots = len(rays) // samples
        rays = np.ascontiguousarray(rays[:slots * samples])
        h = (slots + w - 1) // w + 1  # (the last rows keep the prefill: no slot names them)
        d = self.dev(rays)
        film, rgb = G.capture_rays(self.acc, rays, w, h, samples=samples, into=(prefilled((h, w, 4), np.uint8), prefilled((h, w, 3), np.float64)))
        of, od = self.out(film.nbytes), self.out(rgb.nbytes)
        return Op("capture_rays x%d" % samples, lambda s: G.capture_rays_device(self.acc, slots, d.data_ptr(), w, h, samples=samples, rgba_ptr=of.ptr, rgb_ptr=od.ptr, stream=s),
                  [(of, film.tobytes()), (od, rgb.tobytes())], keep=(d,))

    def radiance_gather(self, n, k, with_radiance):
        o, _ = self.pts(n)
        dirs = la.sphere_directions(k)
        wt = self.rng.uniform(-1.0, 1.0, (k, 2))
        do, dd, dw = self.dev(o), self.dev(dirs), self.dev(wt)
        asked = ("radiance", "sums") if with_radiance else ("sums",)
        ref = G.radiance_gather(self.acc, o, dirs, None, wt, planes=asked)
        outs, ptrs = self._planes(ref, la.GATHER_PLANES)
        return Op("radiance_gather " + "+".join(asked), lambda s: G.radiance_gather_device(self.acc, n, do.data_ptr(), None, k, dd.data_ptr(), dw.data_ptr(), 2, stream=s, **ptrs),
                  outs, keep=(do, dd, dw))

    # -- views
    def capture_views(self, tab, other, w=24, h=16):
        k = len(tab)
        ref = G.capture_views(self.acc, cviews(tab), w, h, rgba=True, rgb=True)
        alt = G.capture_views(self.acc, cviews(other), w, h, rgba=True, rgb=True)
        oa, od = self.out(ref[0].nbytes), self.out(ref[1].nbytes)

        def call(t, s):
            if G.call("capture_views_device", self.acc.h, t.ctypes.data, k, w, h, oa.ptr, od.ptr, int(s)):
                raise la.LasgunError(G.last_error())
        return Op("capture_views", tabled(tab, other, call), [(oa, ref[0].tobytes()), (od, ref[1].tobytes())], alt=[alt[0].tobytes(), alt[1].tobytes()])

    VF_ASKED = ("depth", "normal", "coverage", "id", "point")

    def capture_view_features(self, tab, other, w=24, h=16):
        k = len(tab)
        ref = G.capture_view_features(self.acc, cviews(tab), w, h, planes=self.VF_ASKED)
        alt = G.capture_view_features(self.acc, cviews(other), w, h, planes=self.VF_ASKED)
        outs, ptrs = self._planes(ref, la.VIEW_FEATURE_PLANES)
        f = la._capi.CViewFeatures(*[ptrs.get(p + "_ptr") for p in la.VIEW_FEATURE_PLANES])

        def call(t, s):
            if G.call("capture_view_features_device", self.acc.h, t.ctypes.data, k, w, h, la._C.addressof(f), None, int(s)):
                raise la.LasgunError(G.last_error())
        return Op("capture_view_features", tabled(tab, other, call), outs, keep=(f,), alt=[alt[p].tobytes() for p in la.VIEW_FEATURE_PLANES if p in alt])

    def capture_features(self, w=40, h=24):
        ref = G.capture_features(self.acc, w, h, planes=("depth", "normal", "coverage", "id"))
        outs, ptrs = self._planes(ref, la.FEATURE_PLANES)
        return Op("capture_features", lambda s: G.capture_features_device(self.acc, w, h, stream=s, **ptrs), outs)

    def camera_rays(self, w=40, h=24):
        ref = G.camera_rays(self.acc, w, h, 3, 2, w - 1, h - 3)
        o = self.out(ref.nbytes)
        return Op("camera_rays", lambda s: G.camera_rays_device(self.acc, w, h, 3, 2, w - 1, h - 3, o.ptr, stream=s), [(o, ref.tobytes())])

    def view_rays(self, tab, other, w=16, h=12, o=None):
        """tab, other: one view each."""
        ref = G.view_rays(self.acc, cviews(tab)[0], w, h)
        alt = G.view_rays(self.acc, cviews(other)[0], w, h)
        o = o or self.out(ref.nbytes)

        def call(t, s):
            if G.call("view_rays_device", self.acc.h, t.ctypes.data, w, h, 0, 0, w, h, o.ptr, int(s)):
                raise la.LasgunError(G.last_error())
        op = Op("view_rays", tabled(tab, other, call), [(o, ref.tobytes())], alt=[alt.tobytes()])
        op.rays = ref
        return op

    def lens_rays(self, w=20, h=10, root=2):
        def lens(fwd):
            return np.frombuffer(bytes(la.Lens(la.LENS_EQUIRECTANGULAR, tuple(0.5 * (self.lo + self.hi)), (1, 0, 0), (0, 1, 0), fwd)), dtype=np.uint8).copy()
        tab, other = lens((0, 0, -1)), lens((0, 0.6, -0.8))
        as_lens = lambda t: la._capi.CLens.from_buffer_copy(t.tobytes())  # noqa: E731
        ref, alt = G.lens_rays(as_lens(tab), w, h, root), G.lens_rays(as_lens(other), w, h, root)
        o = self.out(ref.nbytes)
        device = self.torch.cuda.current_device()

        def call(t, s):
            if G.call("lens_rays_device", device, t.ctypes.data, w, h, root, None, w * h, o.ptr, int(s)):
                raise la.LasgunError(G.last_error())
        return Op("lens_rays", tabled(tab, other, call), [(o, ref.tobytes())], alt=[alt.tobytes()])

    # -- renders
    def _frame(self, w, h):
        full = G.Film(w, h)
        G.capture_subset(0, 1, self.acc, full)
        return full.pixels().copy()

    def _subset_ref(self, ks, n, w, h):
        buf = prefilled((h, w, 4), np.uint8)
        film = G.Film.new_with_output(w, h, buf)
        for k in ks:
            G.capture_subset(int(k), n, self.acc, film)
        return buf

    def capture_subset(self, k, n, w=96, h=64):
        ref = self._subset_ref([k], n, w, h)
        o = self.out(ref.nbytes)
        return Op("capture_subset", lambda s: G.capture_subset_device(k, n, self.acc, w, h, o.ptr, stream=s), [(o, ref.tobytes())])

    def capture_subsets(self, ks, other, n, w=96, h=64):
        tab, oth = np.asarray(ks, dtype=np.uint64), np.asarray(other, dtype=np.uint64)  # (size_t)
        ref, alt = self._subset_ref(ks, n, w, h), self._subset_ref(other, n, w, h)
        o = self.out(ref.nbytes)

        def call(t, s):
            if G.call("capture_subsets_device", t.ctypes.data_as(la._C.POINTER(la._C.c_size_t)), len(t), n, self.acc.h, w, h, o.ptr, int(s)):
                raise la.LasgunError(G.last_error())
        return Op("capture_subsets", tabled(tab, oth, call), [(o, ref.tobytes())], alt=[alt.tobytes()])

    def capture_rows(self, w=96, h=64, y0=5, y1=47):
        ref = np.ascontiguousarray(self._frame(w, h)[y0:y1])
        o = self.out(ref.nbytes)
        return Op("capture_rows", lambda s: G.capture_rows_device(self.acc, w, h, y0, y1, o.ptr, stream=s), [(o, ref.tobytes())])

    def capture_interleaved(self, w=96, h=96, b=8, n=3, r=1):
        from lasgun_amd.distributed import interleaved_rows
        ref = np.ascontiguousarray(self._frame(w, h)[interleaved_rows(r, n, h, b)])
        o = self.out(ref.nbytes)
        return Op("capture_interleaved", lambda s: G.capture_interleaved_device(self.acc, w, h, b, n, r, o.ptr, stream=s), [(o, ref.tobytes())])


def both(make, a, b):
    """The call with table a (overwritten with b on return), then the same call with table b (overwritten with a): two calls of one
    family in flight with different tables."""
    return [make(a, b), make(b, a)]


# every *_device entry point of HipApi, by the name test_gpu_stream_contract.py parametrises over: an Op, or for a family that takes a
# host table the pair of Ops of both()
ENTRY_POINTS = {
    "intersect": lambda e: e.intersect(e.rays(MID)),
    "occluded": lambda e: e.occluded(e.segments(MID)),
    "visibility": lambda e: e.visibility(SMALL, 37),
    "open_directions": lambda e: e.open_directions(MID, 19),
    "range_scan": lambda e: e.range_scan(SMALL, 9),
    "hit_layers": lambda e: e.hit_layers(e.rays(MID)),
    "trace_paths": lambda e: both(lambda a, b, r=e.rays(MID): e.trace_paths(r, a, b), e.rules(la.PATH_ABSORB, 1.0), e.rules(la.PATH_REFLECT, 0.5)),
    # the same with the caller's table in page-locked memory (stage_rule_table is handed the caller's pointer as it is)
    "trace_paths_pinned": lambda e: both(lambda a, b, r=e.rays(MID): e.trace_paths(r, a, b, pinned=True), e.rules(la.PATH_ABSORB, 1.0), e.rules(la.PATH_REFLECT, 0.5)),
    "scatter_lit_shared_pinned": lambda e: both(lambda a, b, r=e.rays(MID): e.scatter_lit(r, a, b, pinned=True), e.lights(5), e.lights(5)),
    "scatter_lit_shared_1024_pinned": lambda e: both(lambda a, b, r=e.rays(SMALL): e.scatter_lit(r, a, b, pinned=True), e.lights(la.MAX_CALL_LIGHTS),
                                                     e.lights(la.MAX_CALL_LIGHTS)),
    "scatter": lambda e: e.scatter(e.rays(MID)),
    "scatter_lit_shared": lambda e: both(lambda a, b, r=e.rays(MID): e.scatter_lit(r, a, b), e.lights(5), e.lights(5)),
    # (the largest table a call takes, 72 KiB of lights: staging of more than a page, more than a small copy)
    "scatter_lit_shared_1024": lambda e: both(lambda a, b, r=e.rays(SMALL): e.scatter_lit(r, a, b), e.lights(la.MAX_CALL_LIGHTS), e.lights(la.MAX_CALL_LIGHTS)),
    "scatter_lit_per_ray": lambda e: e.scatter_lit_per_ray(e.rays(MID), 3),
    "radiance": lambda e: e.radiance(e.rays(MID)),
    "radiance_groups": lambda e: both(lambda a, b, r=e.rays(MID): e.radiance_groups(r, a, b), e.groups(False), e.groups(True)),
    "capture_rays_1": lambda e: e.capture_rays(e.rays(MID), 1),
    "capture_rays_4": lambda e: e.capture_rays(e.rays(MID), 4),
    "radiance_gather_sums": lambda e: e.radiance_gather(SMALL, 7, False),
    "radiance_gather_radiance": lambda e: e.radiance_gather(SMALL, 7, True),
    "capture_views": lambda e: both(e.capture_views, e.views(2), e.views(2)),
    "capture_view_features": lambda e: both(e.capture_view_features, e.views(2), e.views(2)),
    "capture_features": lambda e: e.capture_features(),
    "query_order": lambda e: e.query_order(e.rays(MID)),
    "camera_rays": lambda e: e.camera_rays(),
    "view_rays": lambda e: both(e.view_rays, e.views(1), e.views(1)),
    "lens_rays": lambda e: e.lens_rays(),
    "capture_subset": lambda e: e.capture_subset(2, 7),
    "capture_subsets": lambda e: both(lambda a, b: e.capture_subsets(a, b, 10), [0, 3, 9], [1, 4, 8]),
    "capture_rows": lambda e: e.capture_rows(),
    "capture_interleaved": lambda e: e.capture_interleaved(),
}


# ---- running steps on a stream ---------------------------------------------------------------------------------------------------------------
class Step:
    """Something of the program that is not a library call of its own: a torch operation on the stream, a setter."""

    def __init__(self, name, run):
        self.name, self.run = name, run


def enqueue(torch, stream, steps):
    """Every step on `stream`, no synchronise between them; returns the host's time for it."""
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        assert s != 0
        t0 = time.perf_counter()
        for st in steps:
            st.run(s)
        return time.perf_counter() - t0


def expected(steps):
    """{Out: (reference, writer)} after the steps in order: where two calls write one output the later wins."""
    last = {}
    for st in steps:
        if isinstance(st, Op):
            for i, (o, ref) in enumerate(st.outs):
                last[id(o)] = (o, ref, (st.name, i))
    return list(last.values())


def check_all(steps, ctx):
    for o, ref, who in expected(steps):
        o.check(ref, (ctx, who))


def reset_all(torch, stream, steps):
    with torch.cuda.stream(stream):
        for o, _, _ in expected(steps):
            o.reset()
    stream.synchronize()


def behind_a_blocker(torch, stream, steps, ctx, report=None):
    """The stream contract for `steps`: warmed up on the idle stream (buffers grown, references met), timed on the idle stream, then enqueued
    behind a blocker of 8 x that time (at least 0.25 s, at most 2 s): the stream is still busy when the last enqueue returns, and the
    bytes are the references' once it has drained."""
    torch.cuda.synchronize()  # (the prefills and uploads ran on the default stream, which does not order against this one)
    enqueue(torch, stream, steps)
    stream.synchronize()
    check_all(steps, (ctx, "warm-up"))
    reset_all(torch, stream, steps)
    t_enq = enqueue(torch, stream, steps)
    stream.synchronize()
    check_all(steps, (ctx, "idle"))
    reset_all(torch, stream, steps)
    t_block = Blocker.seconds_for(t_enq, ctx)
    torch.cuda.synchronize()
    Blocker.hold(torch, stream, t_block)
    t_behind = enqueue(torch, stream, steps)
    busy = not stream.query()
    print("%s: enqueue %.2f ms idle, %.2f ms behind a blocker of %.0f ms" % (ctx, 1e3 * t_enq, 1e3 * t_behind, 1e3 * t_block))
    if report is not None:
        report.append((str(ctx), t_enq, t_behind, t_block))
    stream.synchronize()
    assert busy, (ctx, "the stream had drained when the last enqueue returned: a call waited (%.0f ms against a blocker of %.0f ms)" % (1e3 * t_behind, 1e3 * t_block))
    check_all(steps, (ctx, "behind the blocker"))


# ---- the program -------------------------------------------------------------------------------------------------------------------------------
def small_mix(e):
    """The small mixed calls (also what each thread of the threads case runs): every family that takes a host table, and the plain ones."""
    r = e.rays(SMALL)
    d = e.dev(r)
    return [e.intersect(r, d=d), e.scatter_lit(r, e.lights(3), e.lights(3), d=d), e.trace_paths(r, e.rules(la.PATH_ABSORB, 1.0), e.rules(la.PATH_REFLECT, 0.5), d=d),
            e.radiance(r, d=d), e.capture_views(e.views(1), e.views(1), w=16, h=8), e.radiance_groups(r, e.groups(False), e.groups(True), d=d),
            e.occluded(e.segments(SMALL)), e.capture_subsets([0, 2], [1, 3], 5, w=32, h=16)]


def program(e, seed):
    """The seeded program: groups of calls whose order inside a group is what the group is about; the groups are shuffled by the seed.
    Returns (steps, pairs): pairs are the (Op, Op) of one family back to back with different host tables."""
    torch = e.torch
    e.rng = np.random.default_rng(seed)
    groups, pairs = [], []

    def pair(make, a, b):
        x, y = make(a, b), make(b, a)
        pairs.append((x, y))
        groups.append([x, y])

    rm = e.rays(MID)
    dm = e.dev(rm)
    pair(lambda a, b: e.capture_views(a, b), e.views(2), e.views(2))
    pair(lambda a, b: e.trace_paths(rm, a, b, d=dm), e.rules(la.PATH_ABSORB, 1.0), e.rules(la.PATH_REFLECT, 0.5))
    pair(lambda a, b: e.scatter_lit(rm, a, b, d=dm), e.lights(5), e.lights(5))
    pair(lambda a, b: e.trace_paths(rm, a, b, d=dm, pinned=True), e.rules(la.PATH_ABSORB, 1.0), e.rules(la.PATH_REFLECT, 0.5))  # page-locked tables
    pair(lambda a, b: e.scatter_lit(rm, a, b, d=dm, pinned=True), e.lights(5), e.lights(5))
    pair(lambda a, b: e.radiance_groups(rm, a, b, d=dm), e.groups(False), e.groups(True))
    pair(lambda a, b: e.capture_subsets([int(k) for k in a], [int(k) for k in b], 10), np.array([0, 3, 9]), np.array([1, 4, 8]))
    # sizes small, large, small: the context's carve changes between calls
    groups.append([e.radiance(e.rays(SMALL)), e.radiance(e.rays(LARGE)), e.radiance(e.rays(SMALL))])
    # true dependencies through the stream: the rays a view makes, read by two queries
    vr = e.view_rays(e.views(1), e.views(1))

    class Ptr:  # (what the queries below read: the view's rays where view_rays_device wrote them)
        @staticmethod
        def data_ptr():
            return vr.outs[0][0].ptr
    groups.append([vr, e.radiance(vr.rays, d=Ptr), e.intersect(vr.rays, d=Ptr)])
    # ... and the order of a query, read by a torch operation on the stream
    qo = e.query_order(rm)
    perm, keys = (np.frombuffer(qo.outs[i][1], dtype=np.uint32) for i in (0, 1))
    sorted_keys = e.out(len(rm) * 4)

    def gather(s):
        n = len(rm)
        p = qo.outs[0][0].t[GUARD:GUARD + 4 * n].view(torch.int32).to(torch.int64)
        k = qo.outs[1][0].t[GUARD:GUARD + 4 * n].view(torch.int32)
        sorted_keys.t[GUARD:GUARD + 4 * n].view(torch.int32).copy_(k[p])
    groups.append([qo, Op("keys[perm] on the stream", gather, [(sorted_keys, keys[perm].tobytes())])])
    # one output written by two calls: the later wins
    x = e.out(MID * 24)
    groups.append([e.radiance(e.rays(MID), o=x), e.radiance(e.rays(MID), o=x)])
    # one ray buffer overwritten on the stream behind a call that reads it
    first, second = e.rays(MID), e.segments(MID)
    buf, d1, d2 = e.dev(first), e.dev(first), e.dev(second)
    groups.append([Step("copy_", lambda s: buf.copy_(d1, non_blocking=True)), e.intersect(first, d=buf), Step("copy_", lambda s: buf.copy_(d2, non_blocking=True)),
                   e.occluded(second, d=buf)])
    # both query orders
    groups.append([Step("sorted", lambda s: G.set_query_order(e.acc, 1)), e.intersect(e.rays(MID)), e.occluded(e.segments(SMALL)), e.radiance(e.rays(MID)),
                   Step("as given", lambda s: G.set_query_order(e.acc, 0))])
    # a render between two queries: they share the level arrays
    groups.append([e.scatter(e.rays(MID)), e.capture_subset(1, 3), e.hit_layers(e.rays(SMALL))])
    groups.append([e.range_scan(SMALL, 9), e.open_directions(MID, 19)])
    groups.append([e.visibility(SMALL, 37), e.radiance_gather(SMALL, 7, False), e.capture_rays(e.rays(MID), 4)])
    order = np.random.default_rng(seed).permutation(len(groups))
    steps = [st for g in order for st in groups[g]]
    assert sum(isinstance(st, Op) for st in steps) >= 24
    return steps, pairs
