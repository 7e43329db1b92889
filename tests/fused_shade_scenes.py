"""Scenes of the fused-shade tests (test_fused_shade_gate.py, test_gpu_fused_shade.py): shadow_skip_scenes.py's sphere that fills a 64 x 64
film -- tiles wholly lit, wholly on the unlit side, across the boundary, and corners that miss -- with the lights given as a list, and what
the fused form's two passes have to carry beside it: a sphere that shadows another (walked hits whose light is hidden), a small sphere in
front of the background (hits appended behind the dense part of the hit queue, holes in dense tiles).  Built through any binding."""
from shadow_skip_scenes import LIGHTS, SIDE_LIGHT, material

ONE = [SIDE_LIGHT]
# the guards of the shadow skip's argument with ONE light: an infinite intensity component; a falloff that is zero everywhere (f_att == 0)
INF_INTENSITY = list(LIGHTS["inf_intensity"])
ZERO_FALLOFF = [([6.0, 0.5, 1.0], [0.9, 0.9, 0.9], [0.0, 0.0, 0.0])]


def _base(api, lights, recursion=None):
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    scene.set_radial_background([0.26, 0.78, 0.67], [0.1, 0.09, 0.33], 0.5)
    if recursion is not None:
        scene.set_max_recursion_depth(recursion)
    camera = scene.set_perspective_camera(45.0)
    camera.look_at([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    for pos, intensity, falloff in lights:
        scene.add_point_light(pos, intensity, falloff)
    return scene


def sphere_scene(api, kind="plastic", lights=ONE, recursion=None):
    """terminator_scene with its lights as a list (none, one, two ...)."""
    specular = kind in ("mirror", "glass")
    scene = _base(api, lights, (2 if specular else None) if recursion is None else recursion)
    root = api.Aggregate.new()
    root.add_sphere([0.0, 0.0, 0.0], 2.2, material(api, kind))
    if specular:
        root.add_sphere([3.0, 2.5, -1.0], 1.0, material(api, "plastic"))
    scene.set_root(root)
    return scene


def shadowed_scene(api):
    """A sphere between the light and the big one: a disc of the big sphere's lit side is walked and found hidden."""
    scene = _base(api, ONE)
    root = api.Aggregate.new()
    root.add_sphere([0.0, 0.0, 0.0], 2.2, material(api, "plastic"))
    root.add_sphere([3.456, 0.332, 1.18], 0.5, material(api, "matte20"))  # on the way from the light to a point the camera sees; itself outside the view
    scene.set_root(root)
    return scene


def speck_scene(api):
    """A small sphere in front of the background: no tile reaches WF_FULL_MIN hits, every hit is appended; beside it a sphere of a few tiles
    whose rim tiles are dense with holes."""
    scene = _base(api, ONE)
    root = api.Aggregate.new()
    root.add_sphere([-1.3, 0.9, 0.0], 0.22, material(api, "metal"))
    root.add_sphere([0.7, -0.4, 0.0], 0.9, material(api, "plastic"))
    scene.set_root(root)
    return scene


def nested_group_scene(api):
    """A group inside a group: the packet walk's gate refuses the scene graph, so the fused form's does."""
    scene = _base(api, ONE)
    inner = api.Aggregate.new()
    inner.add_sphere([0.4, 0.0, 0.0], 0.5, material(api, "plastic"))
    inner.add_sphere([-0.6, 0.3, 0.2], 0.4, material(api, "matte0"))
    mid = api.Aggregate.new()
    mid.add_sphere([0.0, -0.9, 0.0], 0.4, material(api, "metal"))
    mid.add_group(inner)
    root = api.Aggregate.new()
    root.add_sphere([1.5, 0.8, -0.5], 0.6, material(api, "matte20"))
    root.add_group(mid)
    scene.set_root(root)
    return scene
