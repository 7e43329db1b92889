"""Scenes of the frame-table tests (test_tri_frames_gate.py, test_gpu_tri_frames.py): flat meshes -- a strip of
triangles in the plane y = 0, with or without vt and vn lines -- one per group under the root, as the Cornell box holds its walls, so
that the packet walk's gate and the fused form's take the scene (one level, one light) and the closest pass's epilogue reads the table.
Built through any binding."""
from lasgun_amd import scenes as S


def strip_obj(ntri, uv=None, normals=False):
    """`ntri` triangles side by side over x in [-1, 1], z in [-1, 1] of the plane y = 0.  uv: None (no vt lines), "skew" (a vt per vertex:
    an affine map with shear, so dpdu and dpdv are not the edges), "flat" (every vt the same: the uv determinant is 0 and dpdu, dpdv come
    from coordinate_system).  normals: vn lines that lean, so the interpolated normal differs across a triangle."""
    cols = (ntri + 1) // 2
    lines = ["o strip"]
    for i in range(cols + 1):
        x = -1.0 + 2.0 * i / cols
        lines += ["v %r 0 -1" % x, "v %r 0 1" % x]
    if uv is not None:
        for i in range(cols + 1):
            x = -1.0 + 2.0 * i / cols
            for z in (-1.0, 1.0):
                lines.append("vt 0.25 0.75" if uv == "flat" else "vt %r %r" % (0.5 + 0.375 * x + 0.125 * z, 0.5 + 0.25 * z - 0.0625 * x))
    if normals:
        for i in range(cols + 1):
            lines += ["vn %r 1 0.1" % (0.3 * (i % 3 - 1)), "vn 0.05 1 %r" % (0.2 * (i % 2))]

    def corner(v):
        return "%d" % v if uv is None and not normals else "%d/%s/%s" % (v, v if uv is not None else "", v if normals else "")
    faces = []
    for i in range(cols):
        a, b, c, d = 2 * i + 1, 2 * i + 2, 2 * i + 3, 2 * i + 4  # (x_i, -1), (x_i, 1), (x_i+1, -1), (x_i+1, 1)
        faces += [(a, c, d), (a, d, b)]
    for f in faces[:ntri]:
        lines.append("f " + " ".join(corner(v) for v in f))
    return "\n".join(lines) + "\n"


def _base(api, origin=(0.0, 0.0, 5.0), at=(0.0, 0.0, 0.0), orthographic=None):
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    scene.set_radial_background([0.26, 0.78, 0.67], [0.1, 0.09, 0.33], 0.5)
    camera = scene.set_perspective_camera(60.0) if orthographic is None else scene.set_orthographic_camera(orthographic)
    camera.look_at(list(origin), list(at), [0.0, 1.0, 0.0])
    scene.add_point_light([0.3, 1.2, 1.5], [0.9, 0.9, 0.9], [1.0, 0.0, 0.05])
    return scene


def _mats(api):
    M = api.Material
    return (M.plastic([0.9, 0.5, 0.3], [0.5, 0.7, 0.5], 0.25), M.matte([0.3, 0.7, 0.9], 20.0), M.metal([0.2, 0.9, 1.1], [3.9, 2.4, 2.2], 0.15, 0.1))


def walls_scene(api, obj=None, origin=(0.0, 0.0, 5.0), at=(0.0, 0.0, 0.0), orthographic=None, backface=False):
    """Three instances of one flat mesh, each alone in a group with a transform of its own -- a non-uniform scale and rotations about two
    axes above the mesh, so that xf_normal (the inverse transpose) and xf_vector differ -- around two spheres and a cube."""
    scene = _base(api, origin, at, orthographic)
    plastic, matte, metal = _mats(api)
    mesh = scene.parse_obj(S.PLANE_OBJ if obj is None else obj)
    A = api.Aggregate
    floor = A.new(); floor.scale(2.5, 1.0, 1.5); floor.rotate_z(12.0); floor.rotate_x(-8.0); floor.translate([0.1, -1.4, 0.0]); floor.add_obj_of(mesh, plastic)
    back = A.new(); back.scale(1.2, 1.0, 2.6); back.rotate_x(80.0); back.rotate_y(-25.0); back.translate([-0.2, 0.1, -1.8]); back.add_obj_of(mesh, matte)
    side = A.new(); side.scale(2.0, 1.0, 0.7); side.rotate_z(95.0); side.rotate_y(15.0); side.translate([1.9, 0.2, -0.3]); side.add_obj(mesh)  # (no material: Material::default())
    if backface:
        side.swap_backface()
    for g in (floor, back, side):
        scene.root.add_group(g)
    scene.root.add_sphere([-0.8, -0.6, 0.2], 0.6, metal)
    scene.root.add_sphere([0.7, 0.4, -0.5], 0.45, plastic)
    scene.root.add_cube([-0.2, -1.2, 0.6], 0.5, matte)
    return scene


def along_wall_scene(api):
    """An orthographic view ALONG a wall's plane: the wall y = 0 seen from a camera at y = 0 looking down -z, so that the local ray's
    direction is orthogonal to the triangle's normal -- dot(c, -lr.d) == 0 exactly -- for every ray; a second wall stands across the view."""
    scene = _base(api, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0), orthographic=4.0)
    plastic, matte, _ = _mats(api)
    mesh = scene.parse_obj(S.PLANE_OBJ)
    A = api.Aggregate
    flat = A.new(); flat.scale(2.0, 1.0, 2.0); flat.add_obj_of(mesh, plastic)  # the plane y = 0, edge on
    across = A.new(); across.scale(2.0, 1.0, 2.0); across.rotate_x(90.0); across.translate([0.0, 0.0, -2.0]); across.add_obj_of(mesh, matte)
    scene.root.add_group(flat)
    scene.root.add_group(across)
    scene.root.add_sphere([0.9, 0.8, 0.0], 0.5, plastic)
    return scene


def capped_scene(api, ntri, instances=1, normals=False):
    """`instances` groups, each holding one instance of a strip of `ntri` triangles (with vn lines: `normals`), beside a sphere."""
    scene = _base(api)
    plastic, matte, _ = _mats(api)
    mesh = scene.parse_obj(strip_obj(ntri, normals=normals))
    for k in range(instances):
        g = api.Aggregate.new(); g.scale(2.0, 1.0, 1.0 + 0.1 * k); g.rotate_x(60.0 + 5.0 * k); g.translate([0.0, -1.0 + 0.3 * k, -1.0]); g.add_obj_of(mesh, matte if k % 2 else plastic)
        scene.root.add_group(g)
    scene.root.add_sphere([0.0, 0.5, 0.5], 0.5, plastic)
    return scene
