"""Child process of tests/test_gpu_ray_film.py: one ray film in a fresh process, because the level-by-level pipeline's memory budget
(LASGUN_WF_BUDGET_MB) is read once per process.
usage: python ray_film_child.py SCENE RAYS.npy SAMPLES W H ORDER OUT.npz -- with LASGUN_DEBUG=1 the library says on stderr how many chunks it cut."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lasgun_amd as la
    from test_gpu_radiance_query import FORM_SCENES
    name, rays_path, samples, w, h, order, out_path = sys.argv[1:8]
    G = la.api
    G.set_device(0)
    accel = G.Accel.from_scene(dict(FORM_SCENES)[name](G))
    G.set_query_order(accel, int(order))
    rgba, rgb = G.capture_rays(accel, np.load(rays_path), int(w), int(h), samples=int(samples), rgb=True)
    np.savez(out_path, rgba=rgba, rgb=rgb)


if __name__ == "__main__":
    main()
