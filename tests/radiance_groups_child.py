"""Child process of tests/test_gpu_radiance_groups.py: one light-groups call in a fresh process, because the level-by-level pipeline's
memory budget (LASGUN_WF_BUDGET_MB) is read once per process.
usage: python radiance_groups_child.py SCENE RAYS.npy OUT.npy ORDER -- with LASGUN_DEBUG=1 the library says on stderr how many chunks it cut."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lasgun_amd as la
    from test_gpu_radiance_groups import EIGHT, SCENES, lg
    name, rays_path, out_path, order = sys.argv[1:5]
    G = la.api
    G.set_device(0)
    accel = G.Accel.from_scene(SCENES[name](G))
    G.set_query_order(accel, int(order))
    np.save(out_path, G.radiance_groups(accel, np.load(rays_path), lg(EIGHT)))


if __name__ == "__main__":
    main()
