"""The packet form of the plain exact walk without a device (lasgun_amd/csrc/packet.h, packet_host.h).

The walk: a numpy restatement of the packet walk over the pair image lg_scene_lds_image makes -- per packet of 64 rays the lanes are grouped
by (sign triple of dinv, plain or not), each group is walked with ONE word, ONE lane mask and ONE stack of (word, mask) entries, near and
far by the GROUP's signs -- against the per-lane pair walk of tests/test_node_pairs_image.py (walk_pairs, itself held to the node walk
there), over the root accel's tree of each scene and >= 1e4 packets: coherent tiles as a camera and a light make them, random incoherent
rays (the union of the lanes' visits is far bigger than any lane's: masks and pops), tests/edge_rays.py's rays (-0, +-inf and NaN
components, which must fall into groups that are not plain) and packets of 2 .. 8 octants.  Per lane: the same sequence of (leaf, slot
range) visits, the same box tests with every box tested at most once, with the any-hit walk's early exit (a lane leaves after its k-th
leaf) the same stopping point; the packet's stack never deeper than the tree's chain of interior nodes, which the gate holds to the
accel's stack_depth.

The gate: tools/packet_gate_check.cpp, a stand-alone program with its own main over exactly the text launch.cpp includes, under
AddressSanitizer and UBSan on the CPU: every refusing condition alone flips it.  And what it says for this repository's scenes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import edge_rays as E
import lasgun_amd as la
import level_door_scenes as D
from lasgun_amd import scenes as S
from test_gpu_l0_relative import nested3_scene
from test_node_pairs_image import LEAF, NODE_B, PAIR_B, NodeImage, Trace, restate, slab, walk_pairs

G = la.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PACKETS = 10_000


def one_sphere_scene(api):
    scene = D._base(api)
    scene.root.add_sphere([0.1, -0.2, 0.0], 0.8, D._mats(api)[0])
    return scene


def two_leaves_scene(api):
    scene = D._base(api)
    plastic, matte, _ = D._mats(api)
    scene.root.add_sphere([-1.2, 0.0, 0.0], 0.5, plastic)
    scene.root.add_sphere([1.2, 0.3, -0.2], 0.5, matte)
    return scene


SCENES = {"headline": lambda api: S.spheres_scene(api, nspheres=1024), "root_is_a_leaf": one_sphere_scene, "two_leaves": two_leaves_scene,
          "cornell_plastic": lambda api: S.cornell_scene(api, "plastic"), **D.SMALL}


# ---- rays ------------------------------------------------------------------------------------------------------------------------------------
def packets_for(lo, hi, seed):
    """(N_PACKETS * 64, 6) rays, packet p = rays [64 p, 64 p + 64), and the index of the first edge-ray packet."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    centre, size = (lo + hi) / 2, float(np.max(hi - lo)) + 1e-3
    edge, _ = E.edge_rays(tuple(lo), tuple(hi), seed=seed)
    edge = np.asarray(edge, dtype=np.float64)
    edge = np.concatenate([edge, edge[:(-len(edge)) % 64]])[:200 * 64]
    n_edge, n_rand, n_oct = len(edge) // 64, 600, 1200
    n_tile = N_PACKETS - n_edge - n_rand - n_oct
    gy, gx = np.meshgrid(np.arange(8) - 3.5, np.arange(8) - 3.5, indexing="ij")

    def tiles(n, pitch, shadow):
        eye = centre + rng.normal(size=(n, 1, 3)) * size * 1.5
        aim = centre + rng.uniform(-0.6, 0.6, size=(n, 1, 3)) * size
        fwd = aim - eye
        u = np.cross(fwd, rng.normal(size=(n, 1, 3)))
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        v = np.cross(fwd, u)
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        step = np.linalg.norm(fwd, axis=2, keepdims=True) * pitch
        d = fwd + (gx.reshape(1, 64, 1) * u + gy.reshape(1, 64, 1) * v) * step
        if shadow:  # 64 neighbouring points towards one light: origins differ, the directions meet
            o = eye + d
            return np.concatenate([o, (aim - o) * 2.0], axis=2)
        return np.concatenate([np.broadcast_to(eye, d.shape), d], axis=2)

    half = n_tile // 2
    coherent = np.concatenate([tiles(half, 1.0 / 4096, False), tiles(n_tile - half, 1.0 / 2048, True)])
    o = rng.uniform(lo - 3.0, hi + 3.0, size=(n_rand, 64, 3))
    random = np.concatenate([o, rng.normal(size=(n_rand, 64, 3))], axis=2)
    # 2 .. 8 octants: a tile whose lanes have the signs of their direction flipped, lane k taking pattern k mod (number of octants)
    octs = tiles(n_oct, 1.0 / 1024, False)
    n_octants = 2 + np.arange(n_oct) % 7
    pattern = (np.arange(64).reshape(1, 64) % n_octants.reshape(-1, 1))
    for axis in range(3):
        flip = (pattern >> axis) & 1
        octs[:, :, 3 + axis] *= np.where(flip, -1.0, 1.0)
    rays = np.concatenate([coherent.reshape(-1, 6), random.reshape(-1, 6), octs.reshape(-1, 6), edge])
    assert len(rays) == N_PACKETS * 64
    return rays, (n_tile + n_rand, n_tile + n_rand + n_oct), n_tile + n_rand + n_oct


def group_key(o, dinv):
    """neg_mask_x (walk.h): the sign triple of dinv, + 8 where the ray is not plain (dinv finite and not zero, origin finite)."""
    neg = (dinv < 0.0)
    key = neg[:, 0] * 1 + neg[:, 1] * 2 + neg[:, 2] * 4
    plain = np.isfinite(dinv).all(axis=1) & (dinv != 0.0).all(axis=1) & np.isfinite(o).all(axis=1)
    return key + np.where(plain, 0, 8)


# ---- the packet walk -------------------------------------------------------------------------------------------------------------------------
class OnceTrace(Trace):
    def test(self, idx, node):
        bit = np.uint64(1) << (node & 63).astype(np.uint64)
        assert not (self.bits[idx, node >> 6] & bit).any(), "a box tested twice for one ray"
        super().test(idx, node)


def walk_packets(pbytes, nimg, a, b, root_off, pair_of, o, dinv, key, stop, depth):
    """Every packet (64 consecutive rays), one group after the other.  Groups share nothing but the stack, which is empty between them: every
    (packet, key) is walked as a packet of its own under its initial mask.  Returns the per-ray trace and the deepest stack."""
    n = len(o)
    tr = OnceTrace(n, b - a)
    inner_nodes = np.array([i for i in range(a, b) if not nimg.leaf[i]], dtype=np.int64)
    k = len(inner_nodes)
    base = pair_of[int(inner_nodes[0])] if k else 0
    rec = np.frombuffer(pbytes[base:base + k * PAIR_B], dtype=np.uint8).reshape(k, PAIR_B)
    boxes = rec[:, :96].copy().view(np.float64).reshape(k, 12)
    words = rec[:, 96:112].copy().view(np.uint32).reshape(k, 4).astype(np.int64)
    c0, c1 = inner_nodes + 1 - a, nimg.link[inner_nodes] // NODE_B - a
    root = np.frombuffer(pbytes[root_off:root_off + 48], dtype=np.float64).reshape(1, 6)
    w0 = int(np.frombuffer(pbytes[root_off + 48:root_off + 52], dtype=np.uint32)[0])
    # the groups: (packet, key) pairs that have a lane
    pk = np.arange(n) // 64
    pairs = np.unique(pk * 16 + key)
    gp, gk = pairs // 16, pairs % 16
    s = len(pairs)
    rid = gp.reshape(-1, 1) * 64 + np.arange(64).reshape(1, 64)  # the ray in every lane
    m = key[rid] == gk.reshape(-1, 1)
    negbits = gk & 7
    tr.test(rid[m], np.zeros(int(m.sum()), dtype=np.int64))
    hit0 = slab(np.repeat(root, n, axis=0), o, dinv)
    m &= hit0[rid]
    word, sp = np.full(s, w0, dtype=np.int64), np.zeros(s, dtype=np.int64)
    stack_w, stack_m = np.zeros((s, depth), dtype=np.int64), np.zeros((s, depth, 64), dtype=bool)
    live = np.ones(n, dtype=bool)
    max_sp = 0
    active = m.any(axis=1)
    while active.any():
        idx = np.nonzero(active)[0]
        w = word[idx]
        at_leaf = (w & LEAF) != 0
        # a leaf: every lane of the mask visits it; a lane that has seen its k-th leaf leaves the packet (the any-hit walk's early exit)
        li = idx[at_leaf]
        rows, cols = np.nonzero(m[li])
        r_leaf = rid[li[rows], cols]
        wl = w[at_leaf][rows]
        tr.visit(r_leaf, wl & 0xFFFF, (wl & 0xFFFF) + ((wl >> 16) & 0x7FFF))
        live[r_leaf] = tr.leaves[r_leaf] < stop[r_leaf]
        # a pair record: both boxes for every lane of the mask, near and far by the GROUP's signs
        ii = idx[~at_leaf]
        r = (w[~at_leaf] - base) // PAIR_B
        assert ((w[~at_leaf] - base) % PAIR_B == 0).all() and (r >= 0).all() and (r < max(k, 1)).all()
        rows, cols = np.nonzero(m[ii])
        rr, rec_r = rid[ii[rows], cols], r[rows]
        tr.test(rr, c0[rec_r]); tr.test(rr, c1[rec_r])
        ma, mb = np.zeros((len(ii), 64), dtype=bool), np.zeros((len(ii), 64), dtype=bool)
        ma[rows, cols] = slab(boxes[rec_r, 0:6], o[rr], dinv[rr])
        mb[rows, cols] = slab(boxes[rec_r, 6:12], o[rr], dinv[rr])
        ng = (negbits[ii] & words[r, 2]) != 0
        near_w, far_w = np.where(ng, words[r, 1], words[r, 0]), np.where(ng, words[r, 0], words[r, 1])
        near_m, far_m = np.where(ng[:, None], mb, ma), np.where(ng[:, None], ma, mb)
        near_any, far_any = near_m.any(axis=1), far_m.any(axis=1)
        both = near_any & far_any
        pb = ii[both]
        stack_w[pb, sp[pb]] = far_w[both]
        stack_m[pb, sp[pb]] = far_m[both]
        sp[pb] += 1
        if len(pb):
            max_sp = max(max_sp, int(sp[pb].max()))
        word[ii] = np.where(near_any, near_w, far_w)
        m[ii] = np.where(near_any[:, None], near_m, far_m)
        # pop: the next entry with a live lane, or the group is done
        pop = np.concatenate([li, ii[~near_any & ~far_any]])
        while len(pop):
            empty = sp[pop] == 0
            active[pop[empty]] = False
            pop = pop[~empty]
            sp[pop] -= 1
            word[pop] = stack_w[pop, sp[pop]]
            mm = stack_m[pop, sp[pop]] & live[rid[pop]]
            m[pop] = mm
            pop = pop[~mm.any(axis=1)]
    return tr, max_sp


def interior_depth(nimg, a):
    """packet_stack_need (packet_host.h): the longest chain of interior nodes from the tree's node 0."""
    worst, todo = 0, [(a, 0)]
    while todo:
        i, d = todo.pop()
        if nimg.leaf[i]:
            continue
        worst = max(worst, d + 1)
        todo += [(i + 1, d + 1), (int(nimg.link[i]) // NODE_B, d + 1)]
    return worst


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_packet_walk_is_every_lanes_own_walk(name):
    scene = SCENES[name](G)
    node, pair = G.scene_lds_image(scene, False), G.scene_lds_image(scene, True)
    assert node is not None and pair is not None and pair[1]["pairs"] == 1, "the scene fits in LDS"
    nimg, pbytes = NodeImage(*node), pair[0].tobytes()
    _, _, interior, pair_of, root_of = restate(nimg)
    a = int(nimg.accel_root[0]) // NODE_B  # the root accel's tree: the one the packet walks with a cursor
    b = next(e for s, e in nimg.trees if s == a)
    lo, hi = nimg.box[a:b, 0:3].min(axis=0), nimg.box[a:b, 3:6].max(axis=0)
    rays, oct_range, first_edge = packets_for(lo, hi, seed=len(name))
    o = rays[:, 0:3]
    with np.errstate(all="ignore"):
        dinv = 1.0 / rays[:, 3:6]
    neg = dinv < 0.0
    key = group_key(o, dinv)
    # the edge rays with a -0, an infinity or a NaN in them fall into groups that are not plain
    odd = ~np.isfinite(rays).all(axis=1) | ((rays[:, 3:6] == 0.0).any(axis=1))
    assert odd[first_edge * 64:].sum() > 100 and (key[odd] >= 8).all()
    groups = np.array([len(np.unique(key[p * 64:p * 64 + 64])) for p in range(*oct_range)])
    assert groups.min() >= 2 and groups.max() == 8, "packets of 2 .. 8 octants"
    depth = interior_depth(nimg, a)
    for stop in (np.full(len(rays), 1 << 60, dtype=np.int64), 1 + np.arange(len(rays), dtype=np.int64) % 3):
        x = walk_pairs(pbytes, nimg, a, b, root_of[a], pair_of, o, dinv, neg, stop)
        y, max_sp = walk_packets(pbytes, nimg, a, b, root_of[a], pair_of, o, dinv, key, stop, depth + 1)
        assert np.array_equal(x.leaves, y.leaves) and np.array_equal(x.leaf_hash, y.leaf_hash), "the sequence of (leaf, slot range) visits, the stopping point"
        assert np.array_equal(x.bits, y.bits) and np.array_equal(x.tests, y.tests), "the same box tests, each at most once"
        assert max_sp <= depth, "the packet's stack: one pending far child per interior node of the current path"


# ---- the gate --------------------------------------------------------------------------------------------------------------------------------
def test_the_gate_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler: the library itself could not have been built")
    exe = str(tmp_path / "packet_gate_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "packet_gate_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and "packet_gate_check: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])


GATE = {  # packet_host.h, PacketRefusal
    "headline": (lambda api: S.spheres_scene(api, nspheres=1024), 0),
    "cornell_plastic": (lambda api: S.cornell_scene(api, "plastic"), 0),
    "cornell_glass": (lambda api: S.cornell_scene(api, "glass"), 0),
    "root_is_a_leaf": (one_sphere_scene, 0),
    "nested3": (nested3_scene, 6),          # groups in groups, trees of their own
    "srt_lone": (D.srt_lone_scene, 6),      # a mesh with interior nodes
    "nested": (D.nested_scene, 8),          # a group that holds a group
    "mesh_and_sphere": (D.mesh_and_sphere_scene, 8),
}


@pytest.mark.parametrize("name", sorted(GATE))
def test_what_the_gate_says_for_the_scenes(name):
    build, want = GATE[name]
    assert G.scene_packet_walk_gate(build(G)) == want
