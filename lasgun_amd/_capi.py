"""ctypes binding over a lasgun C ABI (include/lasgun_hip.h).

Host-side mirror of the reference's public surface for the render path, with the
reference's own names and argument meaning:

  Scene      /root/reference/src/scene.rs:49-143
  Aggregate  /root/reference/src/scene/node.rs:35-115
  Material   /root/reference/src/material/mod.rs:15-46
  Camera     /root/reference/src/camera.rs:75-102
  Film       /root/reference/src/film.rs:22-45
  Accel / capture / capture_subset / render   /root/reference/src/lib.rs:42-56,110

The binding is parametrised by (shared library, symbol prefix): every function
`<prefix>name` must have the signature declared in include/lasgun_hip.h.  The
product instantiates it once, for liblasgun_hip.so with prefix "lg_"
(lasgun_amd/__init__.py).  Nothing here computes anything: every call goes
straight to the C ABI, and a missing library is an ImportError, never a fallback.
"""
import ctypes as C
import numpy as np

_D3 = C.c_double * 3


class CMaterial(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p", C.c_double * 10)]


class CStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "primary_rays", "shadow_rays", "secondary_rays", "nodes_tested", "spheres_tested",
        "cuboids_tested", "triangles_tested", "accel_entries", "hits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class LasgunError(RuntimeError):
    pass


class ObjError(LasgunError):
    """Mirrors obj::ObjError: the one `Result` on the reference's path (scene.rs:120-130)."""


def _v3(v):
    v = list(v)
    if len(v) != 3:
        raise ValueError("expected 3 components")
    return _D3(float(v[0]), float(v[1]), float(v[2]))


# name -> (restype, argtypes).  These are exactly the entry points of include/lasgun_hip.h
# that have a counterpart in the reference's API (the core ABI).
CORE_SIGNATURES = {
    "last_error": (C.c_char_p, []),
    "material_default": (CMaterial, []),
    "material_matte": (CMaterial, [_D3, C.c_double]),
    "material_plastic": (CMaterial, [_D3, _D3, C.c_double]),
    "material_metal": (CMaterial, [_D3, _D3, C.c_double, C.c_double]),
    "material_glass": (CMaterial, [_D3, _D3, C.c_double]),
    "material_mirror": (CMaterial, [_D3]),
    "scene_new": (C.c_void_p, []),
    "scene_free": (None, [C.c_void_p]),
    "scene_set_perspective_camera": (None, [C.c_void_p, C.c_double]),
    "scene_set_orthographic_camera": (None, [C.c_void_p, C.c_double]),
    "camera_look_at": (None, [C.c_void_p, _D3, _D3, _D3]),
    "camera_set_supersampling": (None, [C.c_void_p, C.c_uint8]),
    "camera_set_aperture_radius": (None, [C.c_void_p, C.c_double]),
    "scene_set_solid_background": (None, [C.c_void_p, _D3]),
    "scene_set_radial_background": (None, [C.c_void_p, _D3, _D3, C.c_double]),
    "scene_set_ambient_light": (None, [C.c_void_p, _D3]),
    "scene_set_mesh_smoothing": (None, [C.c_void_p, C.c_int]),
    "scene_set_max_recursion_depth": (None, [C.c_void_p, C.c_uint32]),
    "scene_set_threads": (None, [C.c_void_p, C.c_size_t]),
    "scene_add_point_light": (None, [C.c_void_p, _D3, _D3, _D3]),
    "scene_parse_obj": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "scene_load_obj": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    "scene_root": (C.c_void_p, [C.c_void_p]),
    "scene_set_root": (None, [C.c_void_p, C.c_void_p]),
    "aggregate_new": (C.c_void_p, []),
    "aggregate_free": (None, [C.c_void_p]),
    "aggregate_add_group": (None, [C.c_void_p, C.c_void_p]),
    "aggregate_add_sphere": (None, [C.c_void_p, _D3, C.c_double, C.POINTER(CMaterial)]),
    "aggregate_add_cube": (None, [C.c_void_p, _D3, C.c_double, C.POINTER(CMaterial)]),
    "aggregate_add_box": (None, [C.c_void_p, _D3, _D3, C.POINTER(CMaterial)]),
    "aggregate_add_obj": (None, [C.c_void_p, C.c_uint32]),
    "aggregate_add_obj_of": (None, [C.c_void_p, C.c_uint32, C.POINTER(CMaterial)]),
    "aggregate_swap_backface": (None, [C.c_void_p]),
    "aggregate_translate": (None, [C.c_void_p, _D3]),
    "aggregate_scale": (None, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "aggregate_rotate_x": (None, [C.c_void_p, C.c_double]),
    "aggregate_rotate_y": (None, [C.c_void_p, C.c_double]),
    "aggregate_rotate_z": (None, [C.c_void_p, C.c_double]),
    "aggregate_rotate": (None, [C.c_void_p, C.c_double, _D3]),
    "aggregate_get_transform": (None, [C.c_void_p, C.c_double * 16, C.c_double * 16]),
    "film_new": (C.c_void_p, [C.c_uint32, C.c_uint32]),
    "film_wrap": (C.c_void_p, [C.c_uint32, C.c_uint32, C.c_void_p]),
    "film_pixels": (C.c_void_p, [C.c_void_p]),
    "film_width": (C.c_uint32, [C.c_void_p]),
    "film_height": (C.c_uint32, [C.c_void_p]),
    "film_free": (None, [C.c_void_p]),
    "accel_from": (C.c_void_p, [C.c_void_p]),
    "accel_free": (None, [C.c_void_p]),
    "capture": (C.c_int, [C.c_void_p, C.c_void_p]),
    "capture_subset": (C.c_int, [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "render": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_uint32]),
    # build-only extras shared by both sides (no reference counterpart)
    "capture_radiance": None,  # signature differs per side; bound by the owner
    "accel_dump": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_size_t),
                             C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.c_size_t)]),
    "kat_intersect": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_size_t, _D3, _D3, C.c_double * 8]),
    "kat_surface_interaction": (C.c_int, [_D3, _D3, C.c_double, _D3, _D3, _D3]),
    "math_eval": (C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The opt-in ray order of ray queries (include/lasgun_hip.h, lg_accel_set_query_order .. lg_query_order_device): entry points of the
# GPU library alone -- no counterpart in the reference, none in the oracle -- which its owner adds to what it binds (lasgun_amd/__init__.py).
QUERY_ORDER_SIGNATURES = {
    "accel_set_query_order": (C.c_int, [C.c_void_p, C.c_int]),
    "accel_get_query_order": (C.c_int, [C.c_void_p]),
    "query_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "query_order_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# Radiance queries (include/lasgun_hip.h, lg_radiance / lg_radiance_device): li() of the caller's rays; the GPU library's alone, as above.
RADIANCE_SIGNATURES = {
    "radiance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "radiance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

# Ray films and lens rays (include/lasgun_hip.h, lg_capture_rays* / lg_lens_rays*): a film from the caller's rays; the GPU library's alone.
RAY_FILM_SIGNATURES = {
    "capture_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "capture_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "lens_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lens_rays_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

# Visibility matrices (include/lasgun_hip.h, lg_visibility / lg_visibility_device): occlusion between two point sets, bit-packed; the GPU
# library's alone.
VISIBILITY_SIGNATURES = {
    "visibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "visibility_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

# Direction sets (include/lasgun_hip.h, lg_open_directions / lg_open_directions_device): which of K shared directions are open above each of
# N points, bit-packed and counted; the GPU library's alone.
DIRECTIONS_SIGNATURES = {
    "open_directions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "open_directions_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
}

# Range scans (include/lasgun_hip.h, lg_range_scan / lg_range_scan_device / lg_range_scan_lanes): the first hits along K shared beams from N
# sensor poses, as planes and per-pose reductions; the GPU library's alone.
RANGE_SCAN_SIGNATURES = {
    "range_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "range_scan_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "range_scan_lanes": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int]),
}

# Hit layers (include/lasgun_hip.h, lg_hit_layers / lg_hit_layers_device): the first K surfaces along each ray in one call, as layer-major
# planes; the GPU library's alone.
HIT_LAYERS_SIGNATURES = {
    "hit_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "hit_layers_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]),
}

# Light groups (include/lasgun_hip.h, lg_radiance_groups / lg_radiance_groups_device / lg_accel_light_count): li() of each ray split by
# subsets of the scene's lights, group-major planes from one call; the GPU library's alone.
LIGHT_GROUPS_SIGNATURES = {
    "radiance_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "radiance_groups_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "accel_light_count": (C.c_int, [C.c_void_p]),
}
GROUP_AMBIENT = 1  # LG_GROUP_AMBIENT
MAX_LIGHT_GROUPS = 64  # LG_MAX_LIGHT_GROUPS

# Ray paths (include/lasgun_hip.h, lg_trace_paths / lg_trace_paths_device): each ray followed through K specular bounces in one call, the
# rule per material the caller's; vertex-major and per-ray planes; the GPU library's alone.
PATHS_SIGNATURES = {
    "trace_paths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "trace_paths_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# Surface scatter (include/lasgun_hip.h, lg_scatter / lg_scatter_device): one level of li()'s tree, opened -- the hit, the light and ambient
# sum at it and the two specular children with their weights, as planes indexed by the ray; the GPU library's alone.
SCATTER_SIGNATURES = {
    "scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "scatter_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}
SCATTER_HIT, SCATTER_REFLECT, SCATTER_REFRACT = 1, 2, 4  # LG_SCATTER_*: lg_scatter_out::flags

# Hit attributes (include/lasgun_hip.h, lg_hit_attributes* / lg_hit_attributes_of*): barycentrics, uv, the local point, the BSDF's tangents
# and the geometric dpdu / dpdv of each ray's hit -- found by the walk, or named by a record --, as planes indexed by the ray; the GPU
# library's alone.
ATTRIBUTES_SIGNATURES = {
    "hit_attributes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hit_attributes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "hit_attributes_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hit_attributes_of_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}
ATTR_HIT, ATTR_NO_HIT, ATTR_BAD_RECORD = 1, 2, 4  # LG_ATTR_*: lg_attr_out::flags

# Closest points (include/lasgun_hip.h, lg_closest_points / lg_closest_points_device / lg_scene_closest_gate / lg_scene_closest_depth): for each point the nearest
# surface point of the scene, its distance and the primitive it lies on, as planes indexed by the point; the GPU library's alone.
CLOSEST_SIGNATURES = {
    "closest_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p]),
    "closest_points_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p]),
    "scene_closest_gate": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "scene_closest_depth": (C.c_int, [C.c_void_p]),
}

# Proximity queries (include/lasgun_hip.h, lg_nearest / lg_nearest_device / lg_scene_nearest_lds): for each point, under a radius of its own, the
# k nearest primitives in order as slot-major planes, the count of those within the radius and whether any is; the GPU library's alone.
NEAREST_SIGNATURES = {
    "nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.c_void_p]),
    "nearest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p]),
    "scene_nearest_lds": (C.c_size_t, [C.c_void_p, C.c_uint32]),
}

# Segment proximity (include/lasgun_hip.h, lg_closest_segments / lg_closest_segments_device): for each segment p0 .. p1, under a radius of its
# own, the nearest surface point of the scene to the segment, the segment's parameter, the distance and the primitive; the GPU library's alone.
SEGMENTS_SIGNATURES = {
    "closest_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p]),
    "closest_segments_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p]),
}

# Lit scatter (include/lasgun_hip.h, lg_scatter_lit / lg_scatter_lit_device): surface scatter under lights that come with the call -- the
# seven planes of lg_scatter, every light's own term and the visibility bits; the GPU library's alone.
LIT_SIGNATURES = {
    "scatter_lit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "scatter_lit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
}
MAX_CALL_LIGHTS = 1024  # LG_MAX_CALL_LIGHTS

# Radiance gathers (include/lasgun_hip.h, lg_radiance_gather / lg_radiance_gather_device / lg_radiance_gather_lanes): li() along K shared
# directions from N poses, as a plane and / or reduced per pose by the caller's weights; the GPU library's alone.
GATHER_SIGNATURES = {
    "radiance_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "radiance_gather_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "radiance_gather_lanes": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int]),
}

# Feature buffers (include/lasgun_hip.h, lg_capture_features* / lg_accel_material_count): depth, normal, albedo, coverage and ids of the
# camera's primary hits; the GPU library's alone.
FEATURES_SIGNATURES = {
    "capture_features": (C.c_int, [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p]),
    "capture_features_device": (C.c_int, [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "accel_material_count": (C.c_size_t, [C.c_void_p]),
}

# Views (include/lasgun_hip.h, lg_view_look_at .. lg_capture_views_device): one accel from K cameras into K films in one call; the GPU
# library's alone.
VIEWS_SIGNATURES = {
    "view_look_at": (C.c_int, [C.c_void_p, C.c_int, C.c_double, _D3, _D3, _D3, C.c_uint8]),
    "scene_view": (C.c_int, [C.c_void_p, C.c_void_p]),
    "accel_view": (C.c_int, [C.c_void_p, C.c_void_p]),
    "view_rays": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p]),
    "view_rays_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p]),
    "capture_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "capture_views_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# View features (include/lasgun_hip.h, lg_capture_view_features*): lg_capture_features' planes and the hit point for the K cameras of a
# view batch in one call; the GPU library's alone.
VIEW_FEATURES_SIGNATURES = {
    "capture_view_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "capture_view_features_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
}


class CView(C.Structure):  # lg_view: 120 bytes, no padding
    _fields_ = [("origin", _D3), ("view", _D3), ("up", _D3), ("aux", _D3), ("image_plane_height", C.c_double), ("pixel_separation", C.c_double),
                ("samples_root", C.c_uint32), ("reserved", C.c_uint32)]


class CFeatures(C.Structure):  # lg_features: five plane pointers, 40 bytes; NULL = not asked for
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("coverage", C.c_void_p), ("id", C.c_void_p)]


class CViewFeatures(C.Structure):  # lg_view_features: six plane pointers, 48 bytes; NULL = not asked for
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("coverage", C.c_void_p), ("id", C.c_void_p), ("point", C.c_void_p)]


class CScanOut(C.Structure):  # lg_scan_out: six pointers, 48 bytes; NULL = not asked for
    _fields_ = [("range", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("id", C.c_void_p), ("hits", C.c_void_p), ("nearest", C.c_void_p)]


class CLayersOut(C.Structure):  # lg_layers_out: five pointers, 40 bytes; NULL = not asked for
    _fields_ = [("hits", C.c_void_p), ("along", C.c_void_p), ("id", C.c_void_p), ("count", C.c_void_p), ("inside", C.c_void_p)]


class CLightGroup(C.Structure):  # lg_light_group: 8 bytes; bit l of `lights` = light l in add order, flags = GROUP_AMBIENT or 0
    _fields_ = [("lights", C.c_uint32), ("flags", C.c_uint32)]


class CPathRule(C.Structure):  # lg_path_rule: 24 bytes; action = LG_PATH_*, reserved = 0
    _fields_ = [("action", C.c_uint32), ("reserved", C.c_uint32), ("ior", C.c_double), ("gain", C.c_double)]


class CPathsOut(C.Structure):  # lg_paths_out: nine pointers, 72 bytes; NULL = not asked for
    _fields_ = [("hits", C.c_void_p), ("point", C.c_void_p), ("id", C.c_void_p), ("along", C.c_void_p), ("count", C.c_void_p), ("end", C.c_void_p),
                ("gain", C.c_void_p), ("last", C.c_void_p), ("medium", C.c_void_p)]


class CScatterOut(C.Structure):  # lg_scatter_out: seven pointers, 56 bytes; NULL = not asked for
    _fields_ = [("hits", C.c_void_p), ("direct", C.c_void_p), ("flags", C.c_void_p), ("reflect", C.c_void_p), ("reflect_weight", C.c_void_p),
                ("refract", C.c_void_p), ("refract_weight", C.c_void_p)]


class CAttrOut(C.Structure):  # lg_attr_out: seven pointers, 56 bytes; NULL = not asked for
    _fields_ = [("hits", C.c_void_p), ("flags", C.c_void_p), ("bary", C.c_void_p), ("uv", C.c_void_p), ("local", C.c_void_p), ("frame", C.c_void_p),
                ("dp", C.c_void_p)]


class CClosestOut(C.Structure):  # lg_closest_out: three pointers, 24 bytes; NULL = not asked for
    _fields_ = [("distance", C.c_void_p), ("point", C.c_void_p), ("id", C.c_void_p)]


class CNearestOut(C.Structure):  # lg_nearest_out: five pointers, 40 bytes; NULL = not asked for
    _fields_ = [("touch", C.c_void_p), ("count", C.c_void_p), ("distance", C.c_void_p), ("point", C.c_void_p), ("id", C.c_void_p)]


class CSegmentsOut(C.Structure):  # lg_segments_out: five pointers, 40 bytes; NULL = not asked for
    _fields_ = [("touch", C.c_void_p), ("distance", C.c_void_p), ("param", C.c_void_p), ("point", C.c_void_p), ("id", C.c_void_p)]


class CLight(C.Structure):  # lg_light: lg_scene_add_point_light's arguments, 72 bytes
    _fields_ = [("position", C.c_double * 3), ("intensity", C.c_double * 3), ("falloff", C.c_double * 3)]


class CLightSet(C.Structure):  # lg_light_set: the call's lights, 40 bytes
    _fields_ = [("lights", C.c_void_p), ("count", C.c_uint32), ("per_ray", C.c_uint32), ("ambient", C.c_double * 3)]


class CLitOut(C.Structure):  # lg_lit_out: lg_scatter_out, then terms and visible; nine pointers, 72 bytes; NULL = not asked for
    _fields_ = [("scatter", CScatterOut), ("terms", C.c_void_p), ("visible", C.c_void_p)]


class CGatherOut(C.Structure):  # lg_gather_out: two pointers, 16 bytes; NULL = not asked for
    _fields_ = [("radiance", C.c_void_p), ("sums", C.c_void_p)]


class CLens(C.Structure):  # lg_lens: 112 bytes, no padding
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("origin", _D3), ("right", _D3), ("up", _D3), ("forward", _D3),
                ("fov_deg", C.c_double)]


class Api:
    """One bound C ABI: `Api(ctypes.CDLL(path), "lg_")`."""

    def __init__(self, lib, prefix, extra_signatures=None):
        self.lib = lib
        self.prefix = prefix
        sigs = dict(CORE_SIGNATURES)
        if extra_signatures:
            sigs.update(extra_signatures)
        self._fn = {}
        for name, sig in sigs.items():
            if sig is None:
                continue
            fn = getattr(lib, prefix + name)  # AttributeError if the symbol is missing: fail loudly
            fn.restype, fn.argtypes = sig
            self._fn[name] = fn
        api = self

        # ------------------------------------------------------------------
        class Material:
            """material/mod.rs:15-46 -- a Copy POD (tag + parameters)."""

            def __init__(self, c):
                self.c = c

            @staticmethod
            def default():
                return Material(api.call("material_default"))

            @staticmethod
            def matte(kd, sigma):
                return Material(api.call("material_matte", _v3(kd), float(sigma)))

            @staticmethod
            def plastic(kd, ks, roughness):
                return Material(api.call("material_plastic", _v3(kd), _v3(ks), float(roughness)))

            @staticmethod
            def metal(eta, k, u_roughness, v_roughness):
                return Material(api.call("material_metal", _v3(eta), _v3(k), float(u_roughness), float(v_roughness)))

            @staticmethod
            def glass(kr, kt, eta):
                return Material(api.call("material_glass", _v3(kr), _v3(kt), float(eta)))

            @staticmethod
            def mirror(kr):
                return Material(api.call("material_mirror", _v3(kr)))

        # ------------------------------------------------------------------
        class Aggregate:
            """scene/node.rs:35-115.  add_group MOVES the child (as in Rust)."""

            def __init__(self, handle=None, owned=True):
                self.h = handle if handle is not None else api.call("aggregate_new")
                self.owned = owned

            @staticmethod
            def new():
                return Aggregate()

            def _alive(self):
                if self.h is None:
                    raise LasgunError("use of a moved Aggregate")
                return self.h

            def __del__(self):
                if getattr(self, "owned", False) and self.h is not None:
                    api.call("aggregate_free", self.h)
                    self.h = None

            def add_group(self, aggregate):
                child = aggregate._alive()
                if not aggregate.owned:
                    raise LasgunError("cannot move a borrowed Aggregate")
                api.call("aggregate_add_group", self._alive(), child)
                aggregate.h = None

            def add_sphere(self, center, radius, material):
                api.call("aggregate_add_sphere", self._alive(), _v3(center), float(radius), C.byref(material.c))

            def add_cube(self, origin, dim, material):
                api.call("aggregate_add_cube", self._alive(), _v3(origin), float(dim), C.byref(material.c))

            def add_box(self, minbound, maxbound, material):
                api.call("aggregate_add_box", self._alive(), _v3(minbound), _v3(maxbound), C.byref(material.c))

            def add_obj(self, mesh):
                api.call("aggregate_add_obj", self._alive(), int(mesh))

            def add_obj_of(self, mesh, material):
                api.call("aggregate_add_obj_of", self._alive(), int(mesh), C.byref(material.c))

            def swap_backface(self):
                api.call("aggregate_swap_backface", self._alive())

            def translate(self, delta):
                api.call("aggregate_translate", self._alive(), _v3(delta)); return self

            def scale(self, x, y, z):
                api.call("aggregate_scale", self._alive(), float(x), float(y), float(z)); return self

            def rotate_x(self, theta):
                api.call("aggregate_rotate_x", self._alive(), float(theta)); return self

            def rotate_y(self, theta):
                api.call("aggregate_rotate_y", self._alive(), float(theta)); return self

            def rotate_z(self, theta):
                api.call("aggregate_rotate_z", self._alive(), float(theta)); return self

            def rotate(self, theta, axis):
                api.call("aggregate_rotate", self._alive(), float(theta), _v3(axis)); return self

            def transform(self):
                """(m, minv) as 4x4 column-major numpy arrays [col][row] (test hook)."""
                m = (C.c_double * 16)(); mi = (C.c_double * 16)()
                api.call("aggregate_get_transform", self._alive(), m, mi)
                return np.array(m).reshape(4, 4), np.array(mi).reshape(4, 4)

        # ------------------------------------------------------------------
        class Camera:
            """camera.rs:75-102; a view of scene.camera (Rust hands out &mut Camera)."""

            def __init__(self, scene):
                self.scene = scene

            def look_at(self, origin, look, up):
                api.call("camera_look_at", self.scene.h, _v3(origin), _v3(look), _v3(up))

            def set_supersampling(self, base):
                api.call("camera_set_supersampling", self.scene.h, int(base))

            def set_aperture_radius(self, radius):
                api.call("camera_set_aperture_radius", self.scene.h, float(radius))

        # ------------------------------------------------------------------
        class Scene:
            """scene.rs:49-143."""

            def __init__(self):
                self.h = api.call("scene_new")

            @staticmethod
            def new():
                return Scene()

            def __del__(self):
                if getattr(self, "h", None) is not None:
                    api.call("scene_free", self.h)
                    self.h = None

            @property
            def root(self):
                return Aggregate(api.call("scene_root", self.h), owned=False)

            @property
            def camera(self):
                return Camera(self)

            def set_perspective_camera(self, fov):
                api.call("scene_set_perspective_camera", self.h, float(fov)); return Camera(self)

            def set_orthographic_camera(self, scale):
                api.call("scene_set_orthographic_camera", self.h, float(scale)); return Camera(self)

            def set_solid_background(self, color):
                api.call("scene_set_solid_background", self.h, _v3(color))

            def set_radial_background(self, inner, outer, scale):
                api.call("scene_set_radial_background", self.h, _v3(inner), _v3(outer), float(scale))

            def set_ambient_light(self, color):
                api.call("scene_set_ambient_light", self.h, _v3(color))

            def set_mesh_smoothing(self, enabled):
                api.call("scene_set_mesh_smoothing", self.h, 1 if enabled else 0)

            def set_max_recursion_depth(self, max_depth):
                api.call("scene_set_max_recursion_depth", self.h, int(max_depth))

            def set_threads(self, threads):
                api.call("scene_set_threads", self.h, int(threads))

            def add_point_light(self, position, intensity, falloff):
                api.call("scene_add_point_light", self.h, _v3(position), _v3(intensity), _v3(falloff))

            def parse_obj(self, text):
                data = text.encode() if isinstance(text, str) else bytes(text)
                ref = C.c_uint32()
                if api.call("scene_parse_obj", self.h, data, len(data), C.byref(ref)):
                    raise ObjError(api.last_error())
                return ref.value

            def load_obj(self, path):
                ref = C.c_uint32()
                if api.call("scene_load_obj", self.h, str(path).encode(), C.byref(ref)):
                    raise ObjError(api.last_error())
                return ref.value

            def set_root(self, node):
                if not node.owned:
                    raise LasgunError("cannot move a borrowed Aggregate")
                api.call("scene_set_root", self.h, node._alive())
                node.h = None

        # ------------------------------------------------------------------
        class Film:
            """film.rs:22-45: w*h RGBA8, row-major, top-left origin, zero-filled."""

            def __init__(self, width, height, handle=None, keep=None):
                self.h = handle if handle is not None else api.call("film_new", int(width), int(height))
                if not self.h:
                    raise LasgunError(api.last_error())
                self.w, self.h_px = int(width), int(height)
                self._keep = keep

            @staticmethod
            def new(width, height):
                return Film(width, height)

            @staticmethod
            def new_with_output(width, height, array):
                """Wrap an externally owned (h, w, 4) uint8 buffer (film.rs:36)."""
                a = np.ascontiguousarray(array, dtype=np.uint8)
                if a.size != width * height * 4 or a is not array and not np.shares_memory(a, array):
                    raise ValueError("need a C-contiguous uint8 buffer of w*h*4 bytes")
                h = api.call("film_wrap", int(width), int(height), a.ctypes.data)
                return Film(width, height, handle=h, keep=a)

            def __del__(self):
                if getattr(self, "h", None):
                    api.call("film_free", self.h)
                    self.h = None

            def pixels(self):
                """(h, w, 4) uint8 numpy copy of the film's buffer."""
                ptr = api.call("film_pixels", self.h)
                buf = (C.c_uint8 * (self.w * self.h_px * 4)).from_address(ptr)
                return np.frombuffer(buf, dtype=np.uint8).reshape(self.h_px, self.w, 4).copy()

        # ------------------------------------------------------------------
        class Accel:
            """lib.rs:42 `Accel::from(&scene)`: borrows the scene for its lifetime."""

            def __init__(self, scene):
                self.scene = scene  # keep the borrow alive
                self.h = api.call("accel_from", scene.h)
                if not self.h:
                    raise LasgunError(api.last_error())

            @staticmethod
            def from_scene(scene):
                return Accel(scene)

            def __del__(self):
                if getattr(self, "h", None):
                    api.call("accel_free", self.h)
                    self.h = None

            def dump(self):
                """(floats, ints) flattening of every BVH in the scene graph (build-parity tests)."""
                pf = C.POINTER(C.c_double)(); nf = C.c_size_t(); pi = C.POINTER(C.c_int64)(); ni = C.c_size_t()
                if api.call("accel_dump", self.h, C.byref(pf), C.byref(nf), C.byref(pi), C.byref(ni)):
                    raise LasgunError(api.last_error())
                f = np.ctypeslib.as_array(pf, shape=(nf.value,)).copy() if nf.value else np.zeros(0)
                i = np.ctypeslib.as_array(pi, shape=(ni.value,)).copy() if ni.value else np.zeros(0, dtype=np.int64)
                return f, i

        self.Material, self.Aggregate, self.Camera, self.Scene, self.Film, self.Accel = (
            Material, Aggregate, Camera, Scene, Film, Accel)

    # -- plumbing ----------------------------------------------------------
    def call(self, name, *args):
        return self._fn[name](*args)

    def last_error(self):
        e = self.call("last_error")
        return e.decode() if e else ""

    # -- lib.rs entry points -------------------------------------------------
    def capture(self, scene, film):
        """lib.rs:55 -- synchronous; on return every pixel of `film` is written.  On the HIP library: split over the devices of
        set_devices / set_device; a process that named none gets EVERY visible GPU for films of 2^18 pixels and more (an accel per
        device, one RCCL gather) and the HIP current device for smaller ones (include/lasgun_hip.h, lg_capture)."""
        if self.call("capture", scene.h, film.h):
            raise LasgunError(self.last_error())

    def capture_subset(self, k, n, accel, film):
        """lib.rs:110 -- writes exactly pixel indices {k + i*n < w*h}."""
        if self.call("capture_subset", int(k), int(n), accel.h, film.h):
            raise LasgunError(self.last_error())

    def render(self, scene, resolution):
        """lib.rs:46 -- Film::new + capture."""
        w, h = resolution
        fh = self.call("render", scene.h, int(w), int(h))
        if not fh:
            raise LasgunError(self.last_error())
        return self.Film(w, h, handle=fh)

    # -- known-answer / math hooks ---------------------------------------------
    def kat_intersect(self, kind, params=None, obj_text=None, origin=(0, 0, 0), d=(0, 0, 1)):
        p = (C.c_double * 8)(*([float(v) for v in (params or [])] + [0.0] * (8 - len(params or []))))
        text = (obj_text or "").encode()
        out = (C.c_double * 8)()
        if self.call("kat_intersect", int(kind), p, text, len(text), _v3(origin), _v3(d), out):
            raise LasgunError(self.last_error())
        o = list(out)
        return {"hit": o[0] != 0.0, "t": o[1], "ng": tuple(o[2:5]), "ns": tuple(o[5:8])}

    def kat_surface_interaction(self, origin, d, t, dpdu, dpdv):
        out = _D3()
        if self.call("kat_surface_interaction", _v3(origin), _v3(d), float(t), _v3(dpdu), _v3(dpdv), out):
            raise LasgunError(self.last_error())
        return tuple(out)

    def math_eval(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float64)
        out = np.empty_like(a)
        if self.call("math_eval", int(op), a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data):
            raise LasgunError(self.last_error() or "math_eval failed")
        return out
