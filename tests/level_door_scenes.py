"""Scenes of the level-door tests (test_gpu_level_door.py, test_level_door_predicate.py): every way a ray can
reach a nested accel.  A lone mesh in a scaled, rotated, translated group; group -> group -> mesh; a group that holds a mesh AND a
sphere (not lone); an identity group with a lone mesh; a mesh straight in the root.  Small films (64 x 64), one light, a glass sphere in
some so that the deeper levels and the shadow rays reach the doors from every side.  Built through any of the three bindings (the
product's, the oracle's, pyref.Api)."""
from lasgun_amd import scenes as S

W = H = 64


def _base(api, ortho=None, recursion=2):
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    scene.set_radial_background([0.26, 0.78, 0.67], [0.1, 0.09, 0.33], 0.5)
    scene.set_max_recursion_depth(recursion)
    if ortho is None:
        camera = scene.set_perspective_camera(50.0)
        camera.look_at([0.3, 0.4, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    else:  # a view down an axis: local directions with exact zeros, of either sign, in two components
        camera = scene.set_orthographic_camera(4.5)
        camera.look_at(*ortho)
    scene.add_point_light([0.5, 3.0, 2.5], [0.9, 0.9, 0.9], [1.0, 0.0, 0.0])
    return scene


def _mats(api):
    M = api.Material
    return (M.plastic([0.2, 0.3, 1.0], [0.5, 0.7, 0.5], 0.25), M.matte([0.8, 0.6, 0.4], 0.0), M.glass([1.0, 0.7, 1.0], [0.7, 1.0, 0.7], 1.25))


def srt_lone_scene(api, ortho=None):
    """A lone mesh (a small torus) in a scaled, rotated, translated group; a plane in a second such group under it; a glass sphere."""
    scene = _base(api, ortho)
    plastic, matte, glass = _mats(api)
    torus = scene.parse_obj(S.torus_obj(12, 8, normals=True))
    plane = scene.parse_obj(S.PLANE_OBJ)
    A = api.Aggregate
    g = A.new(); g.scale(1.3, 0.7, 1.1); g.rotate_x(35.0); g.rotate_y(30.0); g.translate([-0.4, 0.3, 0.2]); g.add_obj_of(torus, plastic)
    scene.root.add_group(g)
    f = A.new(); f.scale(3.0, 1.0, 3.0); f.rotate_z(8.0); f.translate([0.0, -1.6, 0.0]); f.add_obj_of(plane, matte)
    scene.root.add_group(f)
    scene.root.add_sphere([1.4, -0.6, 0.8], 0.6, glass)
    return scene


def nested_scene(api, ortho=None):
    """group -> group -> mesh: the inner group is lone, the outer one holds a group (never lone); a sphere beside them."""
    scene = _base(api, ortho)
    plastic, matte, glass = _mats(api)
    torus = scene.parse_obj(S.torus_obj(10, 6, normals=False))
    A = api.Aggregate
    inner = A.new(); inner.rotate_z(40.0); inner.translate([0.5, 0.0, 0.0]); inner.add_obj_of(torus, plastic)
    outer = A.new(); outer.scale(1.0, 1.5, 0.8); outer.rotate_y(-25.0); outer.add_group(inner)
    scene.root.add_group(outer)
    scene.root.add_sphere([-0.6, 0.3, 2.2], 0.5, matte)  # in front of the group: rays that leave the group's slab behind still hit it
    scene.root.add_sphere([1.2, -1.0, 1.0], 0.45, glass)
    return scene


def mesh_and_sphere_scene(api, ortho=None):
    """A group that holds a mesh and a sphere: two slots under its root, so the group is not lone and its mesh is entered the old way."""
    scene = _base(api, ortho)
    plastic, matte, glass = _mats(api)
    torus = scene.parse_obj(S.torus_obj(10, 6, normals=True))
    A = api.Aggregate
    g = A.new(); g.scale(1.2, 1.2, 0.9); g.rotate_x(-20.0); g.translate([0.0, 0.2, 0.0])
    g.add_obj_of(torus, plastic)
    g.add_sphere([0.0, 0.0, 0.0], 0.4, glass)
    scene.root.add_group(g)
    scene.root.add_cube([-2.0, -2.0, -1.0], 0.8, matte)
    return scene


def identity_lone_scene(api, ortho=None):
    """An identity group with a lone mesh (its entry keeps a plain ray: one frame, the same ray all the way), a second mesh straight in the
    root (an identity accel the probe sees through the ray's own component), a plane in an identity group."""
    scene = _base(api, ortho)
    plastic, matte, glass = _mats(api)
    torus = scene.parse_obj(S.torus_obj(12, 8, normals=True))
    small = scene.parse_obj(S.torus_obj(8, 6, R=0.35, r=0.12, normals=False))
    plane = scene.parse_obj(S.PLANE_OBJ)
    A = api.Aggregate
    g = A.new(); g.add_obj_of(torus, plastic)
    scene.root.add_group(g)
    scene.root.add_obj_of(small, matte)
    p = A.new(); p.add_obj_of(plane, matte)  # y = 0 through the torus' hole: the door's slab has no thickness
    scene.root.add_group(p)
    scene.root.add_sphere([1.5, 0.9, 0.5], 0.4, glass)
    return scene


SMALL = {"srt_lone": srt_lone_scene, "nested": nested_scene, "mesh_and_sphere": mesh_and_sphere_scene, "identity_lone": identity_lone_scene}
# views down -z, -y and +x: the camera's rays carry exact zeros (of either sign) in two components
AXIS_VIEWS = {"down_z": ([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]),
              "down_y": ([0.0, 5.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0]),
              "along_x": ([-5.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])}
