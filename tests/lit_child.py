"""Child process of tests/test_gpu_scatter_lit.py: lg_scatter_lit calls in a fresh process, because the level-by-level pipeline's memory
budget (LASGUN_WF_BUDGET_MB) is read once per process.
usage: python lit_child.py OUT.txt -- one line per query order: the order and the SHA-256 of each plane of CHUNK_PLANES; with
LASGUN_DEBUG=1 the library says on stderr how many chunks it cut."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lasgun_amd as la
    from test_gpu_scatter_lit import AMB, CHUNK_K, CHUNK_PLANES, POOL, chunk_rays, chunk_scene, digests
    G = la.api
    G.set_device(0)
    accel = G.Accel.from_scene(chunk_scene(G))
    rays = chunk_rays(accel)
    with open(sys.argv[1], "w") as f:
        for order in (0, 1):
            G.set_query_order(accel, order)
            f.write("%d %s\n" % (order, " ".join(digests(G.scatter_lit(accel, rays, POOL[:CHUNK_K], AMB, CHUNK_PLANES)))))


if __name__ == "__main__":
    main()
