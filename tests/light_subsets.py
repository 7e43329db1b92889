"""'The same scene with a subset of its lights', for any binding (la.api or the oracle): what plane g of lg_radiance_groups is defined
against (include/lasgun_hip.h).  The scene builders of lasgun_amd.scenes add their lights themselves, so the builder runs with the
binding's `call` wrapped: a scene_add_point_light whose index (in add order) is outside the mask is dropped, and without the ambient
flag scene_set_ambient_light is dropped and the ambient colour set to (+0, +0, +0) afterwards.  Everything else -- the aggregate, the
camera, the background, the recursion depth, the order of the lights that stay -- is the builder's."""
import contextlib


@contextlib.contextmanager
def _light_filter(api, lights, ambient, seen):
    real = api.call  # (the bound method: the wrapper below shadows it as an instance attribute while the builder runs)

    def call(name, *args):
        if name == "scene_add_point_light":
            index = seen[0]
            seen[0] += 1
            if not (lights >> index) & 1:
                return None
        if name == "scene_set_ambient_light" and not ambient:
            return None
        return real(name, *args)

    api.call = call
    try:
        yield
    finally:
        del api.call


def subset_scene(api, builder, lights, ambient):
    """builder(api)'s scene with only the lights of the mask `lights`, in their order, and the ambient colour zero unless `ambient`."""
    seen = [0]
    with _light_filter(api, int(lights), bool(ambient), seen):
        scene = builder(api)
    assert seen[0] <= 32 and not int(lights) >> seen[0], "the mask names a light the builder never adds"
    if not ambient:
        scene.set_ambient_light([0.0, 0.0, 0.0])
    return scene


def light_count(api, builder):
    """The lights builder(api) adds."""
    seen = [0]
    with _light_filter(api, ~0, True, seen):
        builder(api)
    return seen[0]


def group_pairs(n_lights):
    """The groups of the oracle test: per_light_groups' (base, ambient, each light), all lights with and without ambient, {0, 1} without:
    (lights, ambient) pairs."""
    every = (1 << n_lights) - 1
    groups = [(0, False), (0, True)] + [(1 << l, False) for l in range(n_lights)] + [(every, True), (every, False)]
    if n_lights >= 2:
        groups.append((0b11, False))
    return groups


