"""Child process of tests/test_gpu_views.py: one view batch in a fresh process, because the level-by-level pipeline's memory budget
(LASGUN_WF_BUDGET_MB) is read once per process.
usage: python views_child.py SCENE VIEWS.npy W H OUT.npz -- VIEWS.npy holds the K lg_view records as (K, 120) uint8; with LASGUN_DEBUG=1 the
library says on stderr how many chunks it cut."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lasgun_amd as la
    from test_gpu_radiance_query import FORM_SCENES
    name, views_path, w, h, out_path = sys.argv[1:6]
    G = la.api
    G.set_device(0)
    accel = G.Accel.from_scene(dict(FORM_SCENES)[name](G))
    raw = np.load(views_path)
    views = [la.View.from_buffer_copy(raw[k].tobytes()) for k in range(raw.shape[0])]
    assert ctypes.sizeof(la.View) == raw.shape[1]
    rgba, rgb = G.capture_views(accel, views, int(w), int(h), rgb=True)
    np.savez(out_path, rgba=rgba, rgb=rgb)


if __name__ == "__main__":
    main()
