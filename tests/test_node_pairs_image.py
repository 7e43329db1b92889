"""The pair form of the LDS image as the host makes it for real scenes, without a device (lg_scene_lds_image: the builder lg_accel_from runs;
DESIGN.md section 3.1).

Image against a restatement: the node form of the same scene's image holds every node record with its walk words, so the pair form is
restated from it in plain Python -- every tree's interior nodes in node order as 112-byte pair records, the root records behind them, the
primrefs, leaf records and accel records moved as they are, the accel records pointing at their root records -- and compared in all bytes.
Every interior node has exactly one pair record, every leaf is reachable with its slot range, the root records are there, and the image
grows by nothing but the root records (against the 56 payload bytes of a node record; against the 80-byte LDS records it shrinks).

Visit order: a numpy walk of every tree in the node form (bvh.rs:471-505 as walk.h's node step writes it) and one in the pair form (read
from the pair image's own bytes) over >= 1e5 rays a scene -- tests/edge_rays.py's rays and random ones, taken as the tree's local rays:
the same sequence of (leaf, slot range) visits, the same set of box tests with every box tested exactly once where the node form tests
it, a stack that never holds more; with the any-hit walk's early exit (the walk stops after its k-th leaf) the same leaves and a
superset of the box tests.  What the walks do not restate: the primitives inside the leaves and the transforms between levels (every
tree is walked with the same rays); those are the GPU tests' (tests/test_gpu_node_pairs.py, against the CPU oracle)."""
import numpy as np
import pytest

import edge_rays as E
import lasgun_amd as la
import level_door_scenes as D
from lasgun_amd import scenes as S
from test_gpu_l0_relative import nested3_scene

G = la.api
NODE_B, PAIR_B, ROOT_B, ACCEL_B = 80, 112, 64, 256
LEAF = 0x80000000
SCENES = {"headline": lambda api: S.spheres_scene(api, nspheres=1024), "nested3": nested3_scene, **D.SMALL}
N_RAYS = 100_000


class NodeImage:
    """The node form, parsed: per tree (in image order) its node records."""

    def __init__(self, words, info):
        self.raw = words.tobytes()
        self.info = info
        n_nodes = info["prim_off"] * 16 // NODE_B
        rec = np.frombuffer(self.raw[:n_nodes * NODE_B], dtype=np.uint8).reshape(n_nodes, NODE_B)
        self.box = rec[:, :48].copy().view(np.float64).reshape(n_nodes, 6)
        self.box_bytes = rec[:, :48].copy()
        w = rec[:, 64:80].copy().view(np.uint32).reshape(n_nodes, 4)
        self.link, self.meta, self.end = w[:, 0].astype(np.int64), w[:, 1].astype(np.int64), w[:, 2].astype(np.int64)
        self.leaf = (self.meta & LEAF) != 0
        acc = np.frombuffer(self.raw[info["accel_off"] * 16:info["accel_off"] * 16 + info["accels"] * ACCEL_B], dtype=np.uint32).reshape(info["accels"], ACCEL_B // 4)
        self.accel_root = acc[:, 24].astype(np.int64)  # byte offset of each accel's tree
        roots = sorted(set(int(r) for r in self.accel_root))
        assert all(r % NODE_B == 0 for r in roots)
        starts = [r // NODE_B for r in roots] + [n_nodes]
        self.trees = [(starts[k], starts[k + 1]) for k in range(len(roots))]  # [first node, end) of every tree, in image order
        self.n_nodes = n_nodes


def restate(nimg):
    """The pair form of the image, from the node form."""
    info = nimg.info
    interior = [[i for i in range(a, b) if not nimg.leaf[i]] for a, b in nimg.trees]
    pairs = sum(len(x) for x in interior)
    pair16, root16 = pairs * PAIR_B // 16, len(nimg.trees) * ROOT_B // 16
    shift = pair16 + root16 - info["prim_off"]
    out = bytearray((pair16 + root16) * 16) + bytearray(nimg.raw[info["prim_off"] * 16:])
    pair_of, root_of, first_pair = {}, {}, 0
    for t, (a, b) in enumerate(nimg.trees):
        for k, i in enumerate(interior[t]):
            pair_of[i] = (first_pair + k) * PAIR_B
        root_of[a] = pair16 * 16 + t * ROOT_B
        first_pair += len(interior[t])

    def word(i):
        if nimg.leaf[i]:
            first, count = int(nimg.link[i]), int(nimg.end[i] - nimg.link[i])
            assert 0 < count < 1 << 15 and first + count <= 1 << 16
            return LEAF | first | count << 16
        return pair_of[i]

    for t, (a, b) in enumerate(nimg.trees):
        for i in interior[t]:
            c0, c1 = i + 1, int(nimg.link[i]) // NODE_B
            assert a < c0 < c1 < b and int(nimg.link[i]) % NODE_B == 0
            axis_bit = int(nimg.meta[i]) & 7
            assert axis_bit in (1, 2, 4)
            o = pair_of[i]
            out[o:o + 48] = nimg.box_bytes[c0].tobytes()
            out[o + 48:o + 96] = nimg.box_bytes[c1].tobytes()
            out[o + 96:o + 112] = np.array([word(c0), word(c1), axis_bit, 0], dtype=np.uint32).tobytes()
        o = root_of[a]
        out[o:o + 48] = nimg.box_bytes[a].tobytes()
        out[o + 48:o + 52] = np.array([word(a)], dtype=np.uint32).tobytes()
    acc0 = (info["accel_off"] + shift) * 16
    for k, r in enumerate(nimg.accel_root):
        out[acc0 + k * ACCEL_B + 96:acc0 + k * ACCEL_B + 100] = np.array([root_of[int(r) // NODE_B]], dtype=np.uint32).tobytes()
    want_info = dict(info, units=len(out) // 16, prim_off=info["prim_off"] + shift, soup_off=info["soup_off"] + shift, accel_off=info["accel_off"] + shift, pairs=1)
    return bytes(out), want_info, interior, pair_of, root_of


def images(name):
    scene = SCENES[name](G)
    node, pair = G.scene_lds_image(scene, False), G.scene_lds_image(scene, True)
    assert node is not None and pair is not None, "the scene fits in LDS"
    assert node[1]["pairs"] == 0 and pair[1]["pairs"] == 1
    return NodeImage(*node), pair


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_image_is_the_restatement(name):
    nimg, (pwords, pinfo) = images(name)
    want, want_info, interior, pair_of, root_of = restate(nimg)
    assert pinfo == want_info
    got = pwords.tobytes()
    assert len(got) == len(want)
    assert got == want, [i for i in range(0, len(want), 16) if got[i:i + 16] != want[i:i + 16]][:8]
    pairs, trees = sum(len(x) for x in interior), len(nimg.trees)
    assert 2 * pairs + trees == nimg.n_nodes, "one pair record per interior node, two children each"
    assert pairs * PAIR_B == 56 * (nimg.n_nodes - trees) and pinfo["units"] * 16 <= nimg.info["units"] * 16 - nimg.n_nodes * (NODE_B - 56) + trees * ROOT_B
    # every leaf reachable from its tree's root record with its slot range, every pair record reached once
    reached_pairs, leaves = set(), []
    for a, b in nimg.trees:
        todo = [int(np.frombuffer(got[root_of[a] + 48:root_of[a] + 52], dtype=np.uint32)[0])]
        while todo:
            w = todo.pop()
            if w & LEAF:
                leaves.append((w & 0xFFFF, (w & 0xFFFF) + ((w >> 16) & 0x7FFF)))
                continue
            assert w not in reached_pairs
            reached_pairs.add(w)
            todo.extend(int(x) for x in np.frombuffer(got[w + 96:w + 104], dtype=np.uint32))
    assert len(reached_pairs) == pairs
    assert sorted(leaves) == sorted((int(nimg.link[i]), int(nimg.end[i])) for i in range(nimg.n_nodes) if nimg.leaf[i])


# ---- the walks -------------------------------------------------------------------------------------------------------------------------------
def rays_for(lo, hi, seed):
    rays, _ = E.edge_rays(lo, hi, seed=seed)
    rng = np.random.default_rng(seed)
    more = max(N_RAYS - len(rays), 0)
    o = rng.uniform(np.asarray(lo) - 3.0, np.asarray(hi) + 3.0, size=(more, 3))
    d = rng.normal(size=(more, 3))
    d[rng.random(more) < 0.02, rng.integers(0, 3)] = 0.0  # rays in an axis plane
    return np.concatenate([np.asarray(rays, dtype=np.float64), np.concatenate([o, d], axis=1)])


def slab(box, o, dinv):  # slab_intersects_nc: fmin / fmax ignore a NaN operand
    with np.errstate(all="ignore"):
        t1, t2 = (box[:, 0:3] - o) * dinv, (box[:, 3:6] - o) * dinv
        lo_, hi_ = np.fmin(t1, t2), np.fmax(t1, t2)
        tnear = np.fmax(np.fmax(lo_[:, 0], lo_[:, 1]), lo_[:, 2])
        tfar = np.fmin(np.fmin(hi_[:, 0], hi_[:, 1]), hi_[:, 2])
        return ~(tnear > tfar) & ~(tfar <= 0.0)


class Trace:
    def __init__(self, n, nodes):
        self.leaf_hash = np.zeros(n, dtype=np.uint64)
        self.leaves = np.zeros(n, dtype=np.int64)
        self.tests = np.zeros(n, dtype=np.int64)
        self.bits = np.zeros((n, (nodes + 63) // 64), dtype=np.uint64)
        self.max_sp = np.zeros(n, dtype=np.int64)

    def test(self, idx, node):
        self.tests[idx] += 1
        self.bits[idx, node >> 6] |= np.uint64(1) << (node & 63).astype(np.uint64)

    def visit(self, idx, first, end):
        with np.errstate(over="ignore"):
            self.leaf_hash[idx] = self.leaf_hash[idx] * np.uint64(0x9E3779B97F4A7C15) + (first.astype(np.uint64) << np.uint64(20)) + end.astype(np.uint64) + np.uint64(1)
        self.leaves[idx] += 1


def walk_nodes(nimg, a, b, o, dinv, neg, stop):
    n = len(o)
    tr = Trace(n, b - a)
    cur, sp, stack, done = np.full(n, a, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((n, 72), dtype=np.int64), np.zeros(n, dtype=bool)
    axis = np.where(nimg.meta & 1, 0, np.where(nimg.meta & 2, 1, 2))
    while not done.all():
        idx = np.nonzero(~done)[0]
        c = cur[idx]
        hit = slab(nimg.box[c], o[idx], dinv[idx])
        tr.test(idx, c - a)
        leaf_hit, inner = hit & nimg.leaf[c], hit & ~nimg.leaf[c]
        tr.visit(idx[leaf_hit], nimg.link[c[leaf_hit]], nimg.end[c[leaf_hit]])
        ii, ci = idx[inner], c[inner]
        ng = neg[ii, axis[ci]]
        first, second = ci + 1, nimg.link[ci] // NODE_B
        stack[ii, sp[ii]] = np.where(ng, first, second)
        sp[ii] += 1
        cur[ii] = np.where(ng, second, first)
        tr.max_sp[ii] = np.maximum(tr.max_sp[ii], sp[ii])
        pop = idx[~inner]
        stopped = tr.leaves[pop] >= stop[pop]
        empty = sp[pop] == 0
        done[pop[stopped | empty]] = True
        go = pop[~(stopped | empty)]
        sp[go] -= 1
        cur[go] = stack[go, sp[go]]
    return tr


def walk_pairs(pbytes, nimg, a, b, root_off, pair_of, o, dinv, neg, stop):
    n = len(o)
    tr = Trace(n, b - a)
    inner_nodes = np.array([i for i in range(a, b) if not nimg.leaf[i]], dtype=np.int64)
    k = len(inner_nodes)
    base = pair_of[int(inner_nodes[0])] if k else 0
    rec = np.frombuffer(pbytes[base:base + k * PAIR_B], dtype=np.uint8).reshape(k, PAIR_B)
    boxes = rec[:, :96].copy().view(np.float64).reshape(k, 12)
    words = rec[:, 96:112].copy().view(np.uint32).reshape(k, 4).astype(np.int64)
    axis = np.where(words[:, 2] == 1, 0, np.where(words[:, 2] == 2, 1, 2))
    c0, c1 = inner_nodes + 1 - a, nimg.link[inner_nodes] // NODE_B - a  # which boxes a record's two tests are
    root = np.frombuffer(pbytes[root_off:root_off + 48], dtype=np.float64).reshape(1, 6)
    w0 = int(np.frombuffer(pbytes[root_off + 48:root_off + 52], dtype=np.uint32)[0])
    word, sp, stack = np.full(n, w0, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((n, 72), dtype=np.int64)
    everyone = np.arange(n)
    tr.test(everyone, np.zeros(n, dtype=np.int64))
    done = ~slab(np.repeat(root, n, axis=0), o, dinv)
    while not done.all():
        idx = np.nonzero(~done)[0]
        w = word[idx]
        at_leaf = (w & LEAF) != 0
        li = idx[at_leaf]
        wl = w[at_leaf]
        tr.visit(li, wl & 0xFFFF, (wl & 0xFFFF) + ((wl >> 16) & 0x7FFF))
        ii = idx[~at_leaf]
        r = (w[~at_leaf] - base) // PAIR_B
        assert ((w[~at_leaf] - base) % PAIR_B == 0).all() and (r >= 0).all() and (r < max(k, 1)).all()
        tr.test(ii, c0[r]); tr.test(ii, c1[r])
        hit_a, hit_b = slab(boxes[r, 0:6], o[ii], dinv[ii]), slab(boxes[r, 6:12], o[ii], dinv[ii])
        ng = neg[ii, axis[r]]
        near_w, far_w = np.where(ng, words[r, 1], words[r, 0]), np.where(ng, words[r, 0], words[r, 1])
        near_hit, far_hit = np.where(ng, hit_b, hit_a), np.where(ng, hit_a, hit_b)
        both, none = near_hit & far_hit, ~near_hit & ~far_hit
        stack[ii[both], sp[ii[both]]] = far_w[both]
        sp[ii[both]] += 1
        tr.max_sp[ii] = np.maximum(tr.max_sp[ii], sp[ii])
        word[ii] = np.where(near_hit, near_w, far_w)
        pop = np.concatenate([li, ii[none]])
        stopped = np.zeros(len(pop), dtype=bool)
        stopped[:len(li)] = tr.leaves[li] >= stop[li]
        empty = sp[pop] == 0
        done[pop[stopped | empty]] = True
        go = pop[~(stopped | empty)]
        sp[go] -= 1
        word[go] = stack[go, sp[go]]
    return tr


@pytest.mark.parametrize("name", sorted(SCENES))
def test_both_walks_visit_the_same_leaves_and_test_the_same_boxes(name):
    nimg, (pwords, pinfo) = images(name)
    pbytes = pwords.tobytes()
    _, _, interior, pair_of, root_of = restate(nimg)
    lo, hi = nimg.box[:, 0:3].min(axis=0), nimg.box[:, 3:6].max(axis=0)
    rays = rays_for(lo, hi, seed=len(name))
    assert len(rays) >= N_RAYS
    o = rays[:, 0:3]
    with np.errstate(all="ignore"):
        dinv = 1.0 / rays[:, 3:6]
    neg = dinv < 0.0
    never = np.full(len(rays), 1 << 60, dtype=np.int64)
    biggest = max(nimg.trees, key=lambda t: t[1] - t[0])
    for a, b in nimg.trees:
        x = walk_nodes(nimg, a, b, o, dinv, neg, never)
        y = walk_pairs(pbytes, nimg, a, b, root_of[a], pair_of, o, dinv, neg, never)
        assert np.array_equal(x.leaves, y.leaves) and np.array_equal(x.leaf_hash, y.leaf_hash), "the sequence of (leaf, slot range) visits"
        assert np.array_equal(x.bits, y.bits) and np.array_equal(x.tests, y.tests), "the same box tests, each as often (once)"
        assert (y.max_sp <= x.max_sp).all(), "the stack never holds more"
        if (a, b) != biggest or x.leaves.max() < 2:
            continue
        stop = 1 + np.arange(len(rays), dtype=np.int64) % 3  # the any-hit walk's early exit after the k-th leaf
        x = walk_nodes(nimg, a, b, o, dinv, neg, stop)
        y = walk_pairs(pbytes, nimg, a, b, root_of[a], pair_of, o, dinv, neg, stop)
        assert np.array_equal(x.leaves, y.leaves) and np.array_equal(x.leaf_hash, y.leaf_hash)
        assert ((x.bits & ~y.bits) == 0).all(), "the pair form's box tests contain the node form's"
