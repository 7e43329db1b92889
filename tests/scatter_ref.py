"""What the tests of lg_scatter* (include/lasgun_hip.h) restate in numpy, all of it f64 with nothing fused (numpy's elementwise operations
are IEEE's, one rounding each):

  compose       the header's composition rule as a loop over ONE entry point: L(ray, d) level by level to a depth of the caller's choosing,
                finished as (0 + L) * 1.0 -- what must be lg_radiance's value on an accel of that depth, bit for bit;
  reflect_child the reflected child restated from a hit record: origin p + ng * (2^-52 * 2^16), direction -wo + 2 (wo . ns) ns with
                wo = -normalize(d) as vecmath.h normalises (d * (1 / |d|)) and dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
  refract_origin  the transmitted child's origin, p - ng * 2^-36.
The transmitted DIRECTION cannot be restated from a record (the shading frame's tangent ss is in none); it is pinned through compose and
by two closed forms, unit_error and snell_error, whose tolerance the test measures on the CPU witness's own directions (pyref)."""
import numpy as np

HIT, REFLECT, REFRACT = 1, 2, 4                 # LG_SCATTER_*
ERR = 2.220446049250313e-16 * 65536.0           # N::epsilon() * 2^16 == 2^-36: the step off a surface
assert ERR == 2.0 ** -36


def bits(a):
    """Bit patterns with every NaN canonicalised: NaN positions must coincide, a NaN's sign and payload are not part of the contract."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize(v):
    with np.errstate(all="ignore"):
        return v * (1.0 / np.sqrt(dot(v, v)))[:, None]


def compose(scatter, rays, depth, levels=None):
    """li() of `rays` to `depth` over scatter(rays) -> a dict with at least direct, flags, reflect, reflect_weight, refract, refract_weight.
    `levels`: a list that receives (d, rays, planes) of every call, top-down."""
    def L(r, d):
        out = scatter(r)
        if levels is not None:
            levels.append((d, r, out))
        direct, flags = out["direct"], out["flags"]
        hit = (flags & HIT) != 0
        R, T = np.zeros_like(direct), np.zeros_like(direct)  # +0.0: an absent child, and every child at the last depth
        if d < depth:
            has_r, has_t = (flags & REFLECT) != 0, (flags & REFRACT) != 0
            with np.errstate(all="ignore"):
                if has_r.any():
                    R[has_r] = out["reflect_weight"][has_r] * L(np.ascontiguousarray(out["reflect"][has_r]), d + 1)
                if has_t.any():
                    w = out["refract_weight"][has_t]
                    T[has_t] = ((w[:, :3] * L(np.ascontiguousarray(out["refract"][has_t]), d + 1)) * w[:, 3:4]) / w[:, 4:5]
        value = direct.copy()  # a miss: the background, as it is
        with np.errstate(all="ignore"):
            value[hit] = (direct[hit] + R[hit]) + T[hit]
        return value
    with np.errstate(all="ignore"):
        return (0.0 + L(np.ascontiguousarray(rays, dtype=np.float64), 0)) * 1.0


def classes(flags, inside=None):
    """How many rays of each class a level holds; `inside`: which hits were made from inside their surface (wo . ns < 0)."""
    hit, r, t = (flags & HIT) != 0, (flags & REFLECT) != 0, (flags & REFRACT) != 0
    out = {"miss": int((~hit).sum()), "no_child": int((hit & ~r & ~t).sum()), "reflect_only": int((r & ~t).sum()), "refract_only": int((t & ~r).sum()),
           "both": int((r & t).sum())}
    if inside is not None:
        out["tir"] = int((inside & r & ~t).sum())
    return out


def witness_level(pscene, rays):
    """One level of li()'s tree on the CPU witness (tests/pyref.py, the header of its li() restated: the frame, both sample_f calls, the
    presence tests): per ray its flags, whether the hit was made from inside (wo . ns < 0), both children's rays, and for a transmitted
    child (ns, wi, eta) -- the witness's own transmitted direction, which the closed-form tolerances are measured on."""
    import pyref as P
    n = len(rays)
    flags, inside = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=bool)
    reflect, refract = np.zeros((n, 6)), np.zeros((n, 6))
    ns_out, eta = np.zeros((n, 3)), np.zeros(n)
    for i, r in enumerate(rays):
        o, d = tuple(float(x) for x in r[:3]), tuple(float(x) for x in r[3:])
        hit = P.closest(pscene, o, d)
        if hit is None:
            continue
        flags[i] = HIT
        mat = hit["mat"]
        wo = P.neg(P.normalize(d))
        ng = P.normalize(P.cross(hit["g"][0], hit["g"][1]))
        if P.dot(ng, wo) < 0.0:
            ng = P.neg(ng)
        ns = P.normalize(hit["n"]) if hit["n"] is not None else P.normalize(P.cross(hit["s"][0], hit["s"][1]))
        p0, p_err = P.add(o, P.mul(d, hit["t"])), P.mul(ng, ERR)
        bsdf = P.BSDF(ng, ns, P.normalize(hit["s"][0]), P.scattering(mat))
        inside[i] = P.dot(wo, ns) < 0.0
        ns_out[i] = ns
        spectrum, wi, pdf = bsdf.sample_f(wo, P.TRANSMISSION | P.SPECULAR)
        if not (pdf <= 0.0 or spectrum == P.ZERO or abs(P.dot(wi, ns)) == 0.0):
            flags[i] |= REFRACT
            refract[i] = P.sub(p0, p_err) + tuple(wi)
            eta[i] = mat.p[2] if mat.kind == "glass" else 1.0
        spectrum, wi, pdf = bsdf.sample_f(wo, P.REFLECTION | P.SPECULAR)
        if not (pdf <= 0.0 or spectrum == P.ZERO or P.dot(wi, ns) <= 0.0):
            flags[i] |= REFLECT
            reflect[i] = P.add(p0, p_err) + tuple(P.reflect(wo, ns))
    return {"flags": flags, "inside": inside, "reflect": reflect, "refract": refract, "ns": ns_out, "eta": eta}


def witness_levels(pscene, rays, depth):
    """witness_level over the loop's levels 0 .. depth, breadth-first: a list of (rays, level) pairs."""
    out, rays = [], np.ascontiguousarray(rays, dtype=np.float64)
    for d in range(depth + 1):
        lv = witness_level(pscene, rays)
        out.append((rays, lv))
        f = lv["flags"]
        rays = np.concatenate([lv["reflect"][(f & REFLECT) != 0], lv["refract"][(f & REFRACT) != 0]])
        if not len(rays):
            break
    return out


def wo_of(rays):
    return -normalize(rays[:, 3:6])


def unpack(hits):
    """p, ng, ns of HIT_DTYPE records as (n, 3) arrays."""
    return np.ascontiguousarray(hits["p"]), np.ascontiguousarray(hits["ng"]), np.ascontiguousarray(hits["ns"])


def reflect_child(rays, hits):
    p, ng, ns = unpack(hits)
    wo = wo_of(rays)
    with np.errstate(all="ignore"):
        origin = p + ng * ERR
        d = -1.0 * wo + (2.0 * dot(wo, ns))[:, None] * ns
    return np.concatenate([origin, d], axis=1)


def refract_origin(hits):
    p, ng, _ = unpack(hits)
    with np.errstate(all="ignore"):
        return p - ng * ERR


def unit_error(wi):
    """| |wi| - 1 |"""
    return np.abs(np.sqrt(dot(wi, wi)) - 1.0)


def snell_error(rays, ns, wi, eta):
    """| sin(theta_t) - ratio * sin(theta_i) | against the shading normal, the sines from cross products; eta: the material's (inside
    over outside); ratio = 1 / eta for a hit from outside (wo . ns > 0), eta from inside."""
    wo = wo_of(rays)
    ratio = np.where(dot(wo, ns) > 0.0, 1.0 / eta, eta)
    c_i, c_t = np.cross(wo, ns), np.cross(wi, ns)
    return np.abs(np.sqrt(dot(c_t, c_t)) - ratio * np.sqrt(dot(c_i, c_i)))
