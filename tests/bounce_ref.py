"""Ray paths (include/lasgun_hip.h, lg_trace_paths*) restated in numpy: `bounce` is lasgun_amd/csrc/bounce.h word for word (every numpy
operation is one rounded f64 operation; nothing is fused), `chain` the header's loop over an `intersect` the caller supplies (lg_intersect
of an accel, or the CPU oracle's).  Shared by tests/test_bounce_host.py (the header compiled alone on the CPU) and
tests/test_gpu_ray_paths.py (the kernel).  A helper module, not a test file."""
import numpy as np

ABSORB, REFLECT, PASS, REFRACT = 0, 1, 2, 3
END_CUT, END_ESCAPED, END_ABSORBED, END_DEGENERATE = 0, 1, 2, 3
STEP = 2.0 ** -36
RULE_DTYPE = np.dtype([("action", np.uint32), ("reserved", np.uint32), ("ior", np.float64), ("gain", np.float64)])
HIT_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("ng", "<f8", (3,)), ("ns", "<f8", (3,)), ("kind", "<u4"), ("prim", "<u4"), ("instance", "<u4"),
                      ("material", "<i4")])
MISS = np.zeros(1, dtype=HIT_DTYPE)
MISS["t"], MISS["prim"], MISS["instance"], MISS["material"] = np.inf, 0xFFFFFFFF, 0xFFFFFFFF, -1
MISS_ID = np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
# what happened at a vertex that did not absorb (bounce's fourth result)
DID_REFLECT, DID_PASS, DID_REFRACT, DID_TIR = 0, 1, 2, 3


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def keep_nan(a, b):
    """b, but a where a is NaN: the contract's 'a NaN stays'."""
    return np.where(np.isnan(a), a, b)


def bounce(action, ior, d, p, ng, N, medium):
    """bounce_next of m vertices: (o' (m, 3), d' (m, 3), medium' (m,) uint32, what happened (m,)).  action: REFLECT, PASS or REFRACT."""
    action, medium = np.asarray(action), np.asarray(medium, dtype=np.uint32)
    col = lambda v: v[:, None]  # noqa: E731
    with np.errstate(all="ignore"):
        s = dot(d, N)
        flip = s > 0.0
        N = np.where(col(flip), -N, N)
        s = np.where(flip, -s, s)
        step = ng * STEP
        back, through = p + step, p - step
        k = 2.0 * s
        mirrored = d - col(k) * N
        L = np.sqrt(dot(d, d))
        q = 1.0 / L
        u = d * col(q)
        ci = -dot(u, N)
        eta = np.where((medium & 1) == 1, ior, 1.0 / ior)
        sin2 = (eta * eta) * np.fmax(1.0 - ci * ci, 0.0)
        ct = np.sqrt(1.0 - sin2)
        a = eta * ci - ct
        w = col(eta) * u + col(a) * N
        refracted = w * col(L)
    passes = action == PASS
    refracts = (action == REFRACT) & ~(sin2 >= 1.0)
    goes_through = passes | refracts
    o2 = np.where(col(goes_through), through, back)
    d2 = np.where(col(passes), d, np.where(col(refracts), refracted, mirrored))
    m2 = np.where(goes_through, medium ^ 1, medium).astype(np.uint32)
    did = np.where(passes, DID_PASS, np.where(refracts, DID_REFRACT, np.where(action == REFRACT, DID_TIR, DID_REFLECT)))
    return o2, d2, m2, did


def finite(o2, d2):
    return np.isfinite(o2).all(axis=1) & np.isfinite(d2).all(axis=1)


def id_words(h):
    return np.stack([h["kind"], h["prim"], h["instance"], h["material"].view(np.uint32)], axis=1).astype(np.uint32)


def table_rule(rules):
    """rule_of for `chain` from a rule table indexed by the record's material: (action, ior, gain) per hit; outside the table: ABSORB."""
    def rule_of(h):
        m = h["material"].astype(np.int64)
        ok = (m >= 0) & (m < len(rules))
        r = rules[np.where(ok, m, 0)] if len(rules) else np.zeros(len(m), dtype=RULE_DTYPE)
        return np.where(ok, r["action"], ABSORB), np.where(ok, r["ior"], 1.0), np.where(ok, r["gain"], 1.0)
    return rule_of


def chain(intersect, rays, K, rule_of, normal=0, start_medium=None):
    """The contract restated: the nine planes of K vertices of `rays` from K calls of `intersect` (an (m, 6) array -> m lg_hit records);
    rule_of(records of one call) -> (action, ior, gain) per record (table_rule makes one from a rule table).  Plus "did": per ray,
    whether it ever refracted inward, refracted outward, met total internal reflection (for the tests' conditions)."""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    n = len(rays)
    hits = np.repeat(MISS, K * n).reshape(K, n)
    point = np.zeros((K, n, 3))
    ident = np.tile(MISS_ID, (K, n, 1))
    along = np.full((K, n), np.inf)
    count, end, gain, T = np.zeros(n, dtype=np.uint32), np.full(n, END_CUT, dtype=np.uint32), np.ones(n), np.zeros(n)
    medium = np.zeros(n, dtype=np.uint32) if start_medium is None else (np.asarray(start_medium, dtype=np.uint32) & 1)
    last = rays.copy()
    inward, outward, tir = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    live, cur = np.arange(n), rays.copy()
    for j in range(K):
        if len(live) == 0:
            break
        h = intersect(cur)
        hit = h["kind"] != 0
        hits[j, live], ident[j, live] = h, id_words(h)
        end[live[~hit]] = END_ESCAPED  # (last: the segment that missed, already there)
        on, hh, seg = live[hit], h[hit], cur[hit]
        point[j, on] = hh["p"]
        with np.errstate(invalid="ignore", over="ignore"):
            T[on] = hh["t"] if j == 0 else keep_nan(T[on], T[on] + hh["t"])
        along[j, on] = T[on]
        count[on] += 1
        action, ior, rgain = (np.asarray(v)[hit] for v in rule_of(h))  # (asked about every record of the call, misses included)
        go = action != ABSORB
        end[on[~go]] = END_ABSORBED    # (last: the segment that found this vertex, already there)
        idx, hh, seg = on[go], hh[go], seg[go]
        with np.errstate(all="ignore"):
            gain[idx] = keep_nan(gain[idx], gain[idx] * rgain[go])
        before = medium[idx]
        o2, d2, m2, did = bounce(action[go], ior[go], seg[:, 3:], hh["p"], hh["ng"], hh["ns"] if normal else hh["ng"], before)
        medium[idx] = m2
        inward[idx] |= (did == DID_REFRACT) & (before == 0)
        outward[idx] |= (did == DID_REFRACT) & (before == 1)
        tir[idx] |= did == DID_TIR
        fin = finite(o2, d2)
        end[idx[~fin]] = END_DEGENERATE
        live, cur = idx[fin], np.ascontiguousarray(np.concatenate([o2, d2], axis=1)[fin])
        last[live] = cur               # the next ray: what a cut path resumes from
    out = {"hits": hits, "point": point, "id": ident, "along": along, "count": count, "end": end, "gain": gain, "last": last, "medium": medium,
           "did": {"inward": inward, "outward": outward, "tir": tir}}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
