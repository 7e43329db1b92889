"""Child process of tests/test_gpu_scene_limits.py: the dynamic-LDS limit of the 256-lane kernels is a per-process attribute of each kernel
(hipFuncSetAttribute), so the order in which accels are built is tested in a fresh process.
usage: python scene_limits_child.py MIDDLE -- builds and renders deep_a, then MIDDLE (deep_c or readme), then renders deep_a again in every
organisation and asks it one query of each of four families; everything against the oracle.  Prints a line per stage, "done" at the end."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import lasgun_amd as la
    import limit_scenes as L
    import test_gpu_scene_limits as T
    from lasgun_amd import scenes as S
    G = la.api
    G.set_device(0)
    middle = sys.argv[1]
    W, H = T.W, T.H

    def render(tag, accel, want_rgba, want_rad):
        for org, streaming, prune in T.ORGS:
            G.set_streaming(accel, streaming)
            G.set_prune(accel, prune)
            film = G.Film(W, H)
            G.capture_subset(0, 1, accel, film)
            assert np.array_equal(film.pixels(), want_rgba), (tag, org, prune, int((film.pixels() != want_rgba).sum()))
            assert T.same_f64(G.capture_radiance(accel, W, H), want_rad), (tag, org, prune)
        G.set_streaming(accel, 1)
        G.set_prune(accel, None)
        print(tag, "rendered in", len(T.ORGS), "organisations", flush=True)

    a = T.case("deep_a")
    deep_a = G.Accel(L.deep_a(G))
    need_a = L.lds_bytes_256(G.accel_info(deep_a)["max_stack"])
    render("deep_a", deep_a, a.rgba, a.rad)
    if middle == "deep_c":
        build = L.deep_c
    else:
        build = S.readme_scene
    other = G.Accel(build(G))
    need_m = L.lds_bytes_256(G.accel_info(other)["max_stack"])
    assert (64 * 1024 < need_m < need_a) if middle == "deep_c" else need_m <= 64 * 1024, (middle, need_m, need_a)
    rgba, rad, _ = T.oracle_film(build, W, H)
    render(middle, other, rgba, rad)
    render("deep_a again", deep_a, a.rgba, a.rad)
    for form in ("reference", "prune"):
        T.set_form(deep_a, form)
        a.exp130.check(deep_a, G.intersect(deep_a, a.edge130), G.occluded(deep_a, a.edge130), ("deep_a again", form))
        assert T.same_f64(G.radiance(deep_a, G.camera_rays(deep_a, W, H)).reshape(H, W, 3), a.rad), form
        for family in ("visibility", "range_scan", "hit_layers", "features"):
            T.FAMILIES[family]("deep_a again", deep_a, a)
        print("deep_a again: queries in the", form, "form", flush=True)
    print("done")


if __name__ == "__main__":
    main()
