"""Scenes of the shadow-skip tests (test_gpu_shadow_skip.py, test_shadow_skip_predicate.py): one sphere that fills a 64 x 64 film and point
lights to its side, so that the boundary between the hits a light can contribute to and those it cannot crosses the film's 8 x 8 tiles --
some tiles lie wholly on one side, some wholly on the other, some across it.  The film's corners miss the sphere (holes in dense blocks).
Built through any of the three bindings (the product's, the oracle's, pyref.Api)."""
W = H = 64
SIDE_LIGHT = ([6.0, 0.5, 1.0], [0.9, 0.9, 0.9], [1.0, 0.0, 0.0])
LIGHTS = {
    "one": [SIDE_LIGHT],
    "two": [SIDE_LIGHT, ([-5.0, 3.0, 2.0], [0.7, 0.2, 0.7], [1.0, 0.01, 0.0])],
    "three": [SIDE_LIGHT, ([-5.0, 3.0, 2.0], [0.7, 0.2, 0.7], [1.0, 0.01, 0.0]), ([0.5, -7.0, 0.5], [0.1, 0.8, 0.3], [0.5, 0.0, 0.02])],
    # more lights than the visibility word has bits: the flag is never set
    "many": [([6.0 * (1 if i % 2 else -1), -3.0 + 0.2 * i, 1.0 + 0.1 * i], [0.04, 0.03, 0.05], [1.0, 0.0, 0.0]) for i in range(33)],
    # guards: an infinite intensity component (0 * inf), a falloff of zero everywhere (the light is skipped by f_att == 0)
    "inf_intensity": [([6.0, 0.5, 1.0], [0.9, float("inf"), 0.9], [1.0, 0.0, 0.0])],
    "zero_falloff": [([6.0, 0.5, 1.0], [0.9, 0.9, 0.9], [0.0, 0.0, 0.0]), ([-5.0, 3.0, 2.0], [0.7, 0.2, 0.7], [1.0, 0.0, 0.0])],
}


def material(api, kind):
    M = api.Material
    return {"plastic": lambda: M.plastic([0.7, 1.0, 0.7], [0.5, 0.7, 0.5], 0.25),
            "matte0": lambda: M.matte([0.8, 0.6, 0.4], 0.0),
            "matte20": lambda: M.matte([0.8, 0.6, 0.4], 20.0),
            "metal": lambda: M.metal([0.2, 0.9, 1.1], [3.9, 2.4, 2.2], 0.1, 0.3),
            "mirror": lambda: M.mirror([0.9, 0.9, 0.9]),
            "glass": lambda: M.glass([1.0, 0.7, 1.0], [0.7, 1.0, 0.7], 1.25)}[kind]()


def terminator_scene(api, kind="plastic", lights="one", extra_lights=()):
    scene = api.Scene.new()
    scene.set_ambient_light([0.2, 0.2, 0.2])
    scene.set_radial_background([0.26, 0.78, 0.67], [0.1, 0.09, 0.33], 0.5)
    if kind in ("mirror", "glass"):
        scene.set_max_recursion_depth(2)
    camera = scene.set_perspective_camera(45.0)
    camera.look_at([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    for pos, intensity, falloff in list(LIGHTS[lights]) + list(extra_lights):
        scene.add_point_light(pos, intensity, falloff)
    root = api.Aggregate.new()
    root.add_sphere([0.0, 0.0, 0.0], 2.2, material(api, kind))
    if kind in ("mirror", "glass"):  # something for the secondary rays to hit: the deeper levels carry flags too
        root.add_sphere([3.0, 2.5, -1.0], 1.0, material(api, "plastic"))
    scene.set_root(root)
    return scene
