"""The scenes, rays and classes of the hit-attribute tests (tests/test_hit_attributes_witness.py on the CPU, tests/test_gpu_hit_attributes.py
on the device), numpy and tests/pyref.py only.  The films are the first samples of 96 x 64 camera rays of kitchen_sink, exotic_obj_scene,
instanced_scene and cornell glass.  A pinhole camera outside the geometry sees no sphere from inside, at most three faces of a box, and none
of those scenes has a face whose texture coordinates are degenerate; so beside the films stand their CONTINUATION rays -- each hit's
p - ng * 2^-36 with the direction kept, the segment lg_hit_layers walks next: they leave spheres from inside and boxes by their far faces --
and one small scene of this file's own (extra_scene: a mesh with real, degenerate and no texture coordinates, a camera inside a sphere, a
flat box, a group that is scaled, rotated and swap_backface at once)."""
import numpy as np

import pyref

from lasgun_amd import scenes as S

if not hasattr(pyref.Camera, "set_aperture_radius"):  # (kitchen_sink_scene sets it; the reference accepts it and never reads it, camera.rs:142)
    pyref.Camera.set_aperture_radius = lambda self, radius: self

W, H = 96, 64
STEP = 2.0 ** -36  # shade_frame's p_err scale: the layers' step through a surface


def uv_obj():
    """Two quads' worth of triangles with vt and vn: real texture coordinates, a face whose three vt coincide and one whose vt are collinear
    (determinant 0: the reference falls back to coordinate_system for dpdu / dpdv, triangle.rs:270-276)."""
    return """o uv
v -1 -1 0
v 1 -1 0
v 1 1 0
v -1 1 0
v 3 -1 0
v 3 1 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 0.5
vt 0.25 0.25
vn 0 0 1
vn 0.2 0 1
vn 0 0.2 1
f 1/1/1 2/2/2 3/3/3
f 1/1/1 3/3/3 4/4/2
f 2/5/1 5/5/2 6/5/3
f 2/1/1 6/6/3 3/5/2
"""


def extra_scene(api):
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    cam = scene.set_perspective_camera(70.0)
    cam.look_at([0.3, 0.4, 6.0], [0.5, 0.0, 0.0], [0.0, 1.0, 0.0])
    M = api.Material
    matte = M.matte([0.7, 0.7, 0.7], 0.0)
    scene.add_point_light([0.0, 5.0, 5.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0])
    with_uv = scene.parse_obj(uv_obj())
    scene.set_mesh_smoothing(False)
    flat = scene.parse_obj(S.torus_obj(8, 6, normals=True))  # normals dropped: flat, and no vt: the default texture coordinates
    scene.set_mesh_smoothing(True)
    root = scene.root
    root.add_sphere([0.0, 0.0, 0.0], 20.0, matte)                      # the camera sits inside
    root.add_obj_of(with_uv, matte)
    root.add_box([-3.0, -2.0, -1.0], [-1.5, -0.5, -1.0], matte)        # flat in z
    g = api.Aggregate.new()
    g.scale(1.5, 0.6, 0.8).rotate(35.0, [0.6, 0.0, 0.8]).translate([0.5, 2.0, -1.0])
    g.add_obj_of(flat, matte)
    g.add_cube([-2.5, -0.5, -0.5], 1.0, matte)
    g.add_sphere([2.0, 0.0, 0.0], 0.7, matte)
    g.swap_backface()
    root.add_group(g)
    return scene


SCENES = [("kitchen_sink", lambda api: S.kitchen_sink_scene(api), (W, H)),
          ("exotic_obj", lambda api: S.exotic_obj_scene(api), (W, H)),
          ("instanced", lambda api: S.instanced_scene(api), (W, H)),
          ("cornell_glass", lambda api: S.cornell_scene(api, "glass"), (W, H)),
          ("extra", extra_scene, (32, 24))]
FILMS = [s[0] for s in SCENES[:4]]


def film_rays(pscene, w, h):
    """The first sample of every pixel of a w x h film, row-major: (w * h, 6)."""
    return np.array([np.concatenate(pscene.camera.sample(x, y, w, h)[0]) for y in range(h) for x in range(w)], dtype=np.float64)


def continuation(rays, hits):
    """The rays behind the hits: origin p - ng * 2^-36, the direction's bits kept -- rebuilt here as lg_hit_layers forms them; misses are dropped."""
    keep = hits["kind"] != 0
    return np.concatenate([hits["p"][keep] - hits["ng"][keep] * STEP, rays[keep, 3:]], axis=1)


def classes(cat, rays, hits):
    """Which of the classes the issue names occur among (rays, hits): a set of names."""
    found = set()
    for i in np.nonzero(hits["kind"] != 0)[0]:
        kind, prim, inst = int(hits[i]["kind"]), int(hits[i]["prim"]), int(hits[i]["instance"])
        chain = cat.accels[inst]["chain"]
        for m, _, swap in chain:
            if swap:
                found.add("swap_backface")
            if any(m[a][b] != 0.0 for a in range(3) for b in range(3) if a != b):
                found.add("rotated")
            if any(abs(sum(m[a][b] * m[a][b] for b in range(3)) - 1.0) > 1e-9 for a in range(3)):  # a column that is no unit vector
                found.add("scaled")
        o, d = tuple(rays[i, :3]), tuple(rays[i, 3:])
        for _, minv, _ in chain:
            o, d = pyref.transform_point(minv, o), pyref.transform_vector(minv, d)
        if kind == 3:
            obj, _ = cat.accels[inst]["mesh"]
            found.add("smooth" if obj.normal else "flat")
            if not obj.texture:
                found.add("uv_default")
            else:
                poly = obj.polys[prim]
                uv = [obj.texture[poly[q][1]] for q in range(3)]
                det = (uv[0][0] - uv[2][0]) * (uv[1][1] - uv[2][1]) - (uv[0][1] - uv[2][1]) * (uv[1][0] - uv[2][0])
                found.add("uv_degenerate" if det == 0.0 else "uv_real")
        elif kind == 1:
            cen, rad, _ = cat.spheres[prim]
            found.add("sphere_inside" if pyref.sphere_t(o, d, cen, rad)[1] else "sphere_outside")
        else:
            mn, mx, _ = cat.cuboids[prim]
            dinv = tuple(pyref._div(1.0, c) for c in d)
            r = pyref.cuboid_isect(o, d, dinv, mn, mx, float("inf"))
            if r is not None:
                axis = 3 - r[1].index(1.0) - r[2].index(1.0)
                local = o[axis] + d[axis] * r[0]
                found.add("box_face_%d%s" % (axis, "-" if abs(local - mn[axis]) <= abs(local - mx[axis]) else "+"))
    return found


WANTED = {"uv_real", "uv_default", "uv_degenerate", "smooth", "flat", "sphere_outside", "sphere_inside", "scaled", "rotated", "swap_backface"} | \
    {"box_face_%d%s" % (a, s) for a in range(3) for s in "-+"}
