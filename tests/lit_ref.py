"""Numpy restatements for lit scatter (include/lasgun_hip.h, lg_scatter_lit*): the light pool of the tests, 'the same scene rebuilt with
exactly these lights and this ambient colour' for any binding, the shadow segments of the hits, the sequential sum, the bit tests."""
import numpy as np

import lasgun_amd as la
from light_subsets import subset_scene

POOL_N = 70
POOL_BOX = ((-2.5, 2.5), (0.5, 2.5), (-1.5, 3.5))
AMBIENT = (0.2, 0.15, 0.1)
ZERO_FALLOFF = 37  # the pool light whose falloff is (0, 0, 0): f_att == 0, its term is never added, its visibility bit is still its own
FALLOFFS = ((1.0, 0.0, 0.0), (0.5, 0.1, 0.02), (0.0, 1.0, 0.0), (0.2, 0.0, 0.3), (2.0, 0.05, 0.0))
EPS = 2.0 ** -36  # p_err: ng * (2^-52 * 2^16)


def pool():
    """70 point lights, fixed seed, uniform in POOL_BOX, varied intensities and falloffs: a LIGHT_DTYPE array."""
    rng = np.random.default_rng(2323)
    out = np.zeros(POOL_N, dtype=la.LIGHT_DTYPE)
    for a, (lo, hi) in enumerate(POOL_BOX):
        out["position"][:, a] = rng.uniform(lo, hi, POOL_N)
    out["intensity"] = rng.uniform(0.02, 0.6, (POOL_N, 3))
    out["falloff"] = np.array(FALLOFFS)[rng.integers(0, len(FALLOFFS), POOL_N)]
    out["falloff"][ZERO_FALLOFF] = (0.0, 0.0, 0.0)
    out.setflags(write=False)
    return out


def relit(builder, lights, ambient, depth=None):
    """scene_of(api): builder(api)'s scene with NONE of its own lights and exactly `lights` (a LIGHT_DTYPE array, in order) and `ambient` in
    their place; depth: max_recursion_depth where given."""
    def scene_of(api):
        scene = subset_scene(api, builder, 0, False)
        for rec in lights:
            scene.add_point_light(rec["position"].tolist(), rec["intensity"].tolist(), rec["falloff"].tolist())
        scene.set_ambient_light([float(x) for x in ambient])
        if depth is not None:
            scene.set_max_recursion_depth(depth)
        return scene
    return scene_of


def shadow_segments(hits, positions):
    """(n, K, 6): the segment from sh.p = p + ng * 2^-36 of hit i towards light k, direction position - sh.p (f64, nothing fused).
    positions: (K, 3) shared or (n, K, 3) per ray."""
    p = np.ascontiguousarray(hits["p"]) + np.ascontiguousarray(hits["ng"]) * EPS
    positions = np.asarray(positions, dtype=np.float64)
    if positions.ndim == 2:
        positions = np.broadcast_to(positions[None], (len(p),) + positions.shape)
    seg = np.empty(positions.shape[:2] + (6,), dtype=np.float64)
    seg[:, :, :3] = p[:, None, :]
    seg[:, :, 3:] = positions - p[:, None, :]
    return seg


def pack_bits(visible_bool):
    """(n, K) bool -> (n, ceil(K / 32)) uint32: bit k & 31 of word k >> 5."""
    n, k = visible_bool.shape
    words = np.zeros((n, (k + 31) // 32), dtype=np.uint32)
    for j in range(k):
        words[:, j >> 5] |= visible_bool[:, j].astype(np.uint32) << np.uint32(j & 31)
    return words


def unpack_bits(words, k):
    """(n, W) uint32 -> (n, K) bool."""
    return np.stack([(words[:, j >> 5] >> np.uint32(j & 31)) & 1 for j in range(k)], axis=1).astype(bool) if k else np.zeros((len(words), 0), dtype=bool)


def sequential_sum(terms, last):
    """((+0 + terms[:, 0]) + terms[:, 1]) + ... + last, in f64: `direct` of a hit from its terms and the K == 0 call's direct (the ambient
    term).  Adding the +0.0 of a term that was not added changes no bit of a sum that started at +0.0."""
    acc = np.zeros((terms.shape[0], 3), dtype=np.float64)
    for k in range(terms.shape[1]):
        acc = acc + terms[:, k, :]
    return acc + last
