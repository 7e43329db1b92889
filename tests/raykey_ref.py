"""The coherence key of a query ray, restated in numpy float64 (the layout documented in lasgun_amd/csrc/raykey.h and
include/lasgun_hip.h, lg_query_order*) -- TEST INFRASTRUCTURE, imports neither the HIP library nor anything that needs a GPU.

  bits 31..20  the origin's cell in a 16 x 16 x 16 grid over the scene's world bounds, Morton order (x lowest), clamped
  bits 19..0   the cell of d / |d|_1 on the octahedral map, a 1024 x 1024 grid over [-1, 1]^2, Morton order (u lowest), clamped

The key is f64 arithmetic without transcendentals and the library is built with -ffp-contract=off, so the restatement is demanded bit
for bit.  Two things are therefore kept exactly as the header has them: the order of the operations (the L1 norm is (|dx| + |dy|) + |dz|,
a cell is ((p * 0.5) + 0.5) * 1024) and the NaN rules (a clamp is fmin(fmax(x, 0), top), and fmax / fmin return the other operand of a
NaN).  The Morton codes are bit loops here, not the header's shift-and-mask ladder.

One input class is outside the bit-for-bit demand: a direction with an infinite x or y component and dz < 0.  There px (or py) is
inf / inf, the unfold takes copysign(1, NaN), and the sign of a generated NaN is the hardware's choice (x86 sets it, the GPU does not).
No ray set of the tests holds such a ray; every other f64 input has one key."""
import numpy as np

ORIGIN_BITS, DIR_BITS = 4, 10
ORIGIN_CELLS, DIR_CELLS = 1 << ORIGIN_BITS, 1 << DIR_BITS


def key_bounds(lo, hi):
    """(lo, scale) as the key uses them: scale = 1 / (hi - lo), 0 for a non-finite or non-positive extent or a non-finite lo (which is
    then taken as 0)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = hi - lo
        ok = np.isfinite(e) & (e > 0.0) & np.isfinite(lo)
        scale = np.where(ok, 1.0 / np.where(ok, e, 1.0), 0.0)
    return np.where(np.isfinite(lo), lo, 0.0), scale


def key_cell(x, cells):
    """trunc(x) clamped to 0 .. cells - 1, NaN -> 0 (np.fmax / np.fmin drop a NaN operand, as C's fmax / fmin do)."""
    return np.fmin(np.fmax(x, 0.0), float(cells - 1)).astype(np.int64).astype(np.uint32)


def spread(v, nbits, stride):
    """Bit i of v (i < nbits) moved to bit stride * i."""
    v = np.asarray(v, dtype=np.uint32)
    out = np.zeros_like(v)
    for i in range(nbits):
        out |= ((v >> np.uint32(i)) & np.uint32(1)) << np.uint32(stride * i)
    return out


def origin_cells(rays, bounds):
    """(n, 3) uint32: the origin's cell index on each axis."""
    lo, scale = bounds
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        f = (rays[:, :3] - lo) * scale
        return key_cell(f * float(ORIGIN_CELLS), ORIGIN_CELLS)


def octahedral(rays):
    """(px, py, lower): the direction's point on the octahedral map's square and whether the lower half was unfolded."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    dx, dy, dz = rays[:, 3], rays[:, 4], rays[:, 5]
    with np.errstate(all="ignore"):
        l1 = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, py = dx / l1, dy / l1
        lower = dz < 0.0  # (-0.0 and NaN stay on the upper half)
        qx = (1.0 - np.abs(py)) * np.copysign(1.0, px)
        qy = (1.0 - np.abs(px)) * np.copysign(1.0, py)
    return np.where(lower, qx, px), np.where(lower, qy, py), lower


def direction_cells(rays):
    """(n, 2) uint32: the direction's cell (u, v) on the octahedral map."""
    px, py, _ = octahedral(rays)
    with np.errstate(all="ignore"):
        u = key_cell((px * 0.5 + 0.5) * float(DIR_CELLS), DIR_CELLS)
        v = key_cell((py * 0.5 + 0.5) * float(DIR_CELLS), DIR_CELLS)
    return np.stack([u, v], axis=1)


def ray_key(rays, bounds):
    """uint32 keys of an (n, 6) array of rays (origin, direction); bounds = key_bounds(lo, hi)."""
    o, d = origin_cells(rays, bounds), direction_cells(rays)
    okey = spread(o[:, 0], ORIGIN_BITS, 3) | (spread(o[:, 1], ORIGIN_BITS, 3) << np.uint32(1)) | (spread(o[:, 2], ORIGIN_BITS, 3) << np.uint32(2))
    dkey = spread(d[:, 0], DIR_BITS, 2) | (spread(d[:, 1], DIR_BITS, 2) << np.uint32(1))
    return ((okey << np.uint32(2 * DIR_BITS)) | dkey).astype(np.uint32)


def world_bounds(root_lo, root_hi, root_matrix):
    """(lo, hi) of the 8 corners of the root's box taken through the root's transform (root_matrix[column][row], a point's image is
    ((c0 * x + c1 * y) + c2 * z) + c3), reduced corner by corner with fmin / fmax; a corner that is not finite counts as NaN and is
    stepped over."""
    m = np.asarray(root_matrix, dtype=np.float64)
    box = np.array([root_lo, root_hi], dtype=np.float64)
    corners = np.array([[box[c & 1, 0], box[c >> 1 & 1, 1], box[c >> 2 & 1, 2]] for c in range(8)])
    with np.errstate(all="ignore"):
        img = ((m[0, :3] * corners[:, 0:1] + m[1, :3] * corners[:, 1:2]) + m[2, :3] * corners[:, 2:3]) + m[3, :3] * 1.0
    img[~np.isfinite(corners).all(axis=1)] = np.nan
    lo, hi = img[0].copy(), img[0].copy()
    for c in range(1, 8):
        lo, hi = np.fmin(lo, img[c]), np.fmax(hi, img[c])
    return lo, hi


def witness_bounds(witness):
    """key_bounds of a query_witness.Witness: its root's own box (local space) and transform, never the library's."""
    box = witness.root.nodes[0][0]
    return key_bounds(*world_bounds(box[0], box[1], witness.root.m))
