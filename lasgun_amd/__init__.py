"""lasgun_amd -- MI355X-native drop-in for nfrasser/lasgun's per-pixel ray-trace path.

The package is a thin host-side mirror of the reference's `Scene` / `Aggregate` / `Material` /
`Film` / `Accel` / `capture` / `capture_subset` / `render` surface (see `_capi.py`) over the C ABI
of `liblasgun_hip.so` (include/lasgun_hip.h), whose render entry points run hand-written HIP
kernels for gfx950.  There is no CPU render path: importing this package without the built
library raises ImportError, and every render call fails without a HIP device.
"""
import ctypes as _C
import os as _os

import numpy as _np

from ._capi import Api, CStats, LasgunError, ObjError, QUERY_ORDER_SIGNATURES, RADIANCE_SIGNATURES, RAY_FILM_SIGNATURES, VISIBILITY_SIGNATURES, DIRECTIONS_SIGNATURES, RANGE_SCAN_SIGNATURES, HIT_LAYERS_SIGNATURES, PATHS_SIGNATURES, LIGHT_GROUPS_SIGNATURES, GATHER_SIGNATURES, FEATURES_SIGNATURES, VIEWS_SIGNATURES, VIEW_FEATURES_SIGNATURES, CView, CLens, CFeatures, CViewFeatures, CScanOut, CLayersOut, CPathRule, CPathsOut, CGatherOut, CLightGroup, GROUP_AMBIENT, MAX_LIGHT_GROUPS, SCATTER_SIGNATURES, CScatterOut, SCATTER_HIT, SCATTER_REFLECT, SCATTER_REFRACT, LIT_SIGNATURES, CLight, CLightSet, CLitOut, MAX_CALL_LIGHTS, ATTRIBUTES_SIGNATURES, CAttrOut, ATTR_HIT, ATTR_NO_HIT, ATTR_BAD_RECORD, CLOSEST_SIGNATURES, NEAREST_SIGNATURES, SEGMENTS_SIGNATURES, CClosestOut, CNearestOut, CSegmentsOut  # noqa: F401
from . import scenes  # noqa: F401

_HERE = _os.path.dirname(_os.path.abspath(__file__))
LIB_PATH = _os.environ.get("LASGUN_HIP_LIB") or _os.path.join(_HERE, "liblasgun_hip.so")  # env override: A/B builds

if not _os.path.exists(LIB_PATH):
    raise ImportError(
        "lasgun_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C lasgun_amd/csrc` (there is no CPU fallback)" % LIB_PATH)

_EXTRA = {
    "set_device": (_C.c_int, [_C.c_int]),
    "device_count": (_C.c_int, []),
    "trim_pool": (_C.c_uint64, [_C.c_int]),
    "set_devices": (_C.c_int, [_C.POINTER(_C.c_int), _C.c_int]),
    "capture_rows_device": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32,
                                       _C.c_void_p, _C.c_void_p]),
    "capture_subset_device": (_C.c_int, [_C.c_size_t, _C.c_size_t, _C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_void_p,
                                         _C.c_void_p]),
    "capture_subsets": (_C.c_int, [_C.POINTER(_C.c_size_t), _C.c_size_t, _C.c_size_t, _C.c_void_p, _C.c_void_p]),
    "capture_subsets_device": (_C.c_int, [_C.POINTER(_C.c_size_t), _C.c_size_t, _C.c_size_t, _C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_void_p,
                                          _C.c_void_p]),
    "capture_interleaved_device": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32,
                                              _C.c_void_p, _C.c_void_p]),
    "accel_stream": (_C.c_void_p, [_C.c_void_p]),
    "accel_set_mode": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_prune": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_shadow_skip": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_level_door": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_l0_relative": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_last_l0_relative": (_C.c_int, [_C.c_void_p]),
    "scene_l0_relative_origins": (_C.c_int, [_C.c_void_p, _C.POINTER(_C.c_double), _C.c_int]),
    "accel_set_node_pairs": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_last_node_pairs": (_C.c_int, [_C.c_void_p]),
    "accel_set_packet_walk": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_last_packet_walk": (_C.c_int, [_C.c_void_p]),
    "scene_packet_walk_gate": (_C.c_int, [_C.c_void_p]),
    "accel_set_fused_shade": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_last_fused_shade": (_C.c_int, [_C.c_void_p]),
    "scene_fused_shade_gate": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_tri_frames": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_last_tri_frames": (_C.c_int, [_C.c_void_p]),
    "scene_tri_frames_gate": (_C.c_int, [_C.c_void_p, _C.POINTER(_C.c_uint32), _C.c_int]),
    "accel_read_tri_frames": (_C.c_int, [_C.c_void_p, _C.c_void_p, _C.c_int]),
    "scene_lds_image": (_C.c_longlong, [_C.c_void_p, _C.c_int, _C.POINTER(_C.c_uint32), _C.c_size_t, _C.POINTER(_C.c_uint32)]),
    "accel_set_streaming": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_get_prune": (_C.c_int, [_C.c_void_p]),
    "accel_last_organisation": (_C.c_int, [_C.c_void_p]),
    "accel_set_tile_order": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_sample_order": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_tile_parts": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_lds_scene": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_set_wf_split": (_C.c_int, [_C.c_void_p, _C.c_int]),
    "accel_synchronize": (_C.c_int, [_C.c_void_p]),
    "capture_radiance": (_C.c_int, [_C.c_size_t, _C.c_size_t, _C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_void_p]),
    "capture_pixels": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_void_p, _C.c_size_t, _C.c_void_p, _C.c_void_p]),
    "capture_rect": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_void_p, _C.c_void_p]),
    "audit_prune": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_void_p]),
    "audit_fast": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_void_p]),
    "capture_stats": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.POINTER(CStats)]),
    "profile_enable": (None, [_C.c_void_p, _C.c_int]),
    "profile_read_kinds": (_C.c_int, [_C.c_void_p, _C.c_double * 5, _C.c_uint64 * 5]),
    "capture_stats_kind": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_int, _C.POINTER(CStats)]),
    "profile_read": (_C.c_int, [_C.c_void_p, _C.POINTER(_C.c_double), _C.POINTER(_C.c_uint64)]),
    "probe_rate": (_C.c_int, [_C.c_int, _C.POINTER(_C.c_double)]),
    "accel_from_on": (_C.c_void_p, [_C.c_void_p, _C.c_int]),
    "tune_export": (_C.c_size_t, [_C.c_void_p, _C.c_size_t]),
    "tune_import": (_C.c_int, [_C.c_void_p, _C.c_size_t]),
    "tune_clear": (None, []),
    "multi_create": (_C.c_void_p, [_C.c_void_p, _C.POINTER(_C.c_int), _C.c_int, _C.c_uint32]),
    "multi_free": (None, [_C.c_void_p]),
    "multi_capture_device": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_void_p]),
    "multi_capture": (_C.c_int, [_C.c_void_p, _C.c_void_p]),
    "multi_capture_device_all": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.POINTER(_C.c_void_p)]),
    "multi_rank_count": (_C.c_int, [_C.c_void_p]),
    "multi_accel": (_C.c_void_p, [_C.c_void_p, _C.c_int]),
    "multi_uses_rccl": (_C.c_int, [_C.c_void_p]),
    "accel_info": (_C.c_int, [_C.c_void_p, _C.c_uint64 * 8]),
    "trace_pixel": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_uint32, _C.c_int, _C.POINTER(_C.c_double), _C.c_size_t]),
    "host_build_dump": (_C.c_int, [_C.c_void_p, _C.POINTER(_C.POINTER(_C.c_double)), _C.POINTER(_C.c_size_t),
                                   _C.POINTER(_C.POINTER(_C.c_int64)), _C.POINTER(_C.c_size_t), _C.c_uint64 * 8]),
    "host_check_wide_records": (_C.c_int, [_C.c_void_p, _C.c_uint64 * 8]),
    "host_check_strips": (_C.c_int, [_C.c_void_p, _C.c_uint64 * 8]),
    "intersect": (_C.c_int, [_C.c_void_p, _C.c_void_p, _C.c_size_t, _C.c_void_p]),
    "occluded": (_C.c_int, [_C.c_void_p, _C.c_void_p, _C.c_size_t, _C.c_void_p]),
    "intersect_device": (_C.c_int, [_C.c_void_p, _C.c_void_p, _C.c_size_t, _C.c_void_p, _C.c_void_p]),
    "occluded_device": (_C.c_int, [_C.c_void_p, _C.c_void_p, _C.c_size_t, _C.c_void_p, _C.c_void_p]),
    "camera_rays": (_C.c_int, [_C.c_void_p] + [_C.c_uint32] * 6 + [_C.c_void_p]),
    "camera_rays_device": (_C.c_int, [_C.c_void_p] + [_C.c_uint32] * 6 + [_C.c_void_p, _C.c_void_p]),
    "camera_samples": (_C.c_uint32, [_C.c_void_p]),
    "accel_material": (_C.c_int, [_C.c_void_p, _C.c_int32, _C.c_void_p]),
    "accel_instance": (_C.c_int, [_C.c_void_p, _C.c_uint32, _C.POINTER(_C.c_int32), _C.POINTER(_C.c_int64)]),
    **QUERY_ORDER_SIGNATURES,
    **RADIANCE_SIGNATURES,
    **RAY_FILM_SIGNATURES,
    **VISIBILITY_SIGNATURES,
    **DIRECTIONS_SIGNATURES,
    **RANGE_SCAN_SIGNATURES,
    **HIT_LAYERS_SIGNATURES,
    **PATHS_SIGNATURES,
    **SCATTER_SIGNATURES,
    **LIT_SIGNATURES,
    **ATTRIBUTES_SIGNATURES,
    **CLOSEST_SIGNATURES,
    **NEAREST_SIGNATURES,
    **SEGMENTS_SIGNATURES,
    **LIGHT_GROUPS_SIGNATURES,
    **GATHER_SIGNATURES,
    **FEATURES_SIGNATURES,
    **VIEWS_SIGNATURES,
    **VIEW_FEATURES_SIGNATURES,
}


class Hit(_C.Structure):  # lg_hit (include/lasgun_hip.h): one closest hit of a ray query
    _fields_ = [("t", _C.c_double), ("p", _C.c_double * 3), ("ng", _C.c_double * 3), ("ns", _C.c_double * 3),
                ("kind", _C.c_uint32), ("prim", _C.c_uint32), ("instance", _C.c_uint32), ("material", _C.c_int32)]


HIT_DTYPE = _np.dtype(Hit)  # the numpy mirror of lg_hit: what HipApi.intersect returns
assert _C.sizeof(Hit) == 96 and HIT_DTYPE.itemsize == 96, "lg_hit is 96 bytes"
# a record of the frame table (include/lasgun_hip.h, lg_accel_read_tri_frames): 176 bytes
TRI_FRAME_DTYPE = _np.dtype([("c", "<f8", (3,)), ("ng0", "<f8", (3,)), ("ss", "<f8", (3,)), ("ns", "<f8", (2, 3)), ("ts", "<f8", (2, 3)), ("mat", "<i4"), ("pad", "<u4")])
assert TRI_FRAME_DTYPE.itemsize == 176, "a frame record is 176 bytes"
LENS_EQUIRECTANGULAR, LENS_FISHEYE = 0, 1  # lg_lens::kind
assert _C.sizeof(CLens) == 112, "lg_lens is 112 bytes"
assert _C.sizeof(CFeatures) == 40, "lg_features is 40 bytes"
FEATURE_PLANES = ("depth", "normal", "albedo", "coverage", "id")  # lg_features' members, in its order
assert _C.sizeof(CScanOut) == 48, "lg_scan_out is 48 bytes"
SCAN_PLANES = ("range", "point", "normal", "id", "hits", "nearest")  # lg_scan_out's members, in its order
_SCAN_SHAPE = {"range": ((), _np.float32, True), "point": ((3,), _np.float32, True), "normal": ((3,), _np.float32, True), "id": ((4,), _np.uint32, True),
               "hits": ((), _np.uint32, False), "nearest": ((), _np.float32, False)}  # (trailing shape, dtype, per pair -- else per pose)
SCAN_LANES = {"auto": 0, "beam": 1, "pose": 2}
assert _C.sizeof(CLayersOut) == 40, "lg_layers_out is 40 bytes"
LAYER_PLANES = ("hits", "along", "id", "count", "inside")  # lg_layers_out's members, in its order
_LAYER_SHAPE = {"hits": ((), HIT_DTYPE, True), "along": ((), _np.float64, True), "id": ((4,), _np.uint32, True), "count": ((), _np.uint32, False),
                "inside": ((), _np.float64, False)}  # (trailing shape, dtype, per layer and ray -- else per ray)
assert _C.sizeof(CPathRule) == 24 and _C.sizeof(CPathsOut) == 72, "lg_path_rule is 24 bytes, lg_paths_out 72"
PATH_PLANES = ("hits", "point", "id", "along", "count", "end", "gain", "last", "medium")  # lg_paths_out's members, in its order
_PATH_SHAPE = {"hits": ((), HIT_DTYPE, True), "point": ((3,), _np.float64, True), "id": ((4,), _np.uint32, True), "along": ((), _np.float64, True),
               "count": ((), _np.uint32, False), "end": ((), _np.uint32, False), "gain": ((), _np.float64, False), "last": ((6,), _np.float64, False),
               "medium": ((), _np.uint32, False)}  # (trailing shape, dtype, per vertex and ray -- else per ray)
PATH_ABSORB, PATH_REFLECT, PATH_PASS, PATH_REFRACT = 0, 1, 2, 3                   # LG_PATH_*: lg_path_rule::action
PATH_END_CUT, PATH_END_ESCAPED, PATH_END_ABSORBED, PATH_END_DEGENERATE = 0, 1, 2, 3  # LG_PATH_END_*: lg_paths_out::end
PATH_RULE_DTYPE = _np.dtype([("action", _np.uint32), ("reserved", _np.uint32), ("ior", _np.float64), ("gain", _np.float64)])  # lg_path_rule
assert PATH_RULE_DTYPE.itemsize == 24
assert _C.sizeof(CScatterOut) == 56, "lg_scatter_out is 56 bytes"
SCATTER_PLANES = ("hits", "direct", "flags", "reflect", "reflect_weight", "refract", "refract_weight")  # lg_scatter_out's members, in its order
_SCATTER_SHAPE = {"hits": ((), HIT_DTYPE), "direct": ((3,), _np.float64), "flags": ((), _np.uint32), "reflect": ((6,), _np.float64),
                  "reflect_weight": ((3,), _np.float64), "refract": ((6,), _np.float64), "refract_weight": ((5,), _np.float64)}  # (trailing shape, dtype) per ray
assert _C.sizeof(CLight) == 72 and _C.sizeof(CLightSet) == 40 and _C.sizeof(CLitOut) == 72, "lg_light is 72 bytes, lg_light_set 40, lg_lit_out 72"
LIT_PLANES = SCATTER_PLANES + ("terms", "visible")  # lg_lit_out's members, in its order
assert _C.sizeof(CAttrOut) == 56, "lg_attr_out is 56 bytes"
ATTR_PLANES = ("hits", "flags", "bary", "uv", "local", "frame", "dp")  # lg_attr_out's members, in its order
_ATTR_SHAPE = {"hits": ((), HIT_DTYPE), "flags": ((), _np.uint32), "bary": ((3,), _np.float64), "uv": ((2,), _np.float64), "local": ((3,), _np.float64),
               "frame": ((6,), _np.float64), "dp": ((6,), _np.float64)}  # (trailing shape, dtype) per ray
assert _C.sizeof(CClosestOut) == 24, "lg_closest_out is 24 bytes"
CLOSEST_PLANES = ("distance", "point", "id")  # lg_closest_out's members, in its order
_CLOSEST_SHAPE = {"distance": ((), _np.float64), "point": ((3,), _np.float64), "id": ((4,), _np.uint32)}  # (trailing shape, dtype) per point
assert _C.sizeof(CNearestOut) == 40, "lg_nearest_out is 40 bytes"
NEAREST_PLANES = ("touch", "count", "distance", "point", "id")  # lg_nearest_out's members, in its order
NEAREST_SLOT_PLANES = NEAREST_PLANES[2:]  # slot-major (k, n, ...): only these make k play a part
NEAREST_MAX_K = 8  # LG_NEAREST_MAX_K
_NEAREST_SHAPE = {"touch": ((), _np.uint8), "count": ((), _np.uint32), **_CLOSEST_SHAPE}  # (trailing shape, dtype) per point (per slot and point for a slot plane)
assert _C.sizeof(CSegmentsOut) == 40, "lg_segments_out is 40 bytes"
SEGMENT_PLANES = ("touch", "distance", "param", "point", "id")  # lg_segments_out's members, in its order
_SEGMENT_SHAPE = {"touch": ((), _np.uint8), "param": ((), _np.float64), **_CLOSEST_SHAPE}  # (trailing shape, dtype) per segment
LIGHT_DTYPE = _np.dtype([("position", _np.float64, (3,)), ("intensity", _np.float64, (3,)), ("falloff", _np.float64, (3,))])  # lg_light
assert LIGHT_DTYPE.itemsize == 72


def Light(position, intensity, falloff=(1.0, 0.0, 0.0)):
    """One point light of a scatter_lit call: lg_scene_add_point_light's arguments (falloff: constant, linear, quadratic)."""
    return (tuple(float(x) for x in position), tuple(float(x) for x in intensity), tuple(float(x) for x in falloff))


def lights_array(lights):
    """The light table of a scatter_lit call as a C-contiguous LIGHT_DTYPE array: from a sequence of Light()s (K,), from an array of
    that dtype of any shape, or from a float64 array whose last axis is the nine doubles of a record."""
    if isinstance(lights, _np.ndarray) and lights.dtype == LIGHT_DTYPE:
        return _np.ascontiguousarray(lights)
    if isinstance(lights, _np.ndarray):
        a = _np.ascontiguousarray(lights, dtype=_np.float64)
        if a.ndim < 1 or a.shape[-1] != 9:
            raise ValueError("lights: the last axis holds position, intensity and falloff, nine doubles")
        return a.view(LIGHT_DTYPE).reshape(a.shape[:-1])
    out = _np.zeros(len(lights), dtype=LIGHT_DTYPE)
    for k, (p, i, f) in enumerate(lights):
        out[k] = (p, i, f)
    return out


assert _C.sizeof(CGatherOut) == 16, "lg_gather_out is 16 bytes"
GATHER_PLANES = ("radiance", "sums")  # lg_gather_out's members, in its order
GATHER_LANES = {"auto": 0, "direction": 1, "pose": 2}
_FEATURE_SHAPE = {"depth": ((), _np.float32), "normal": ((3,), _np.float32), "albedo": ((3,), _np.float32), "coverage": ((), _np.float32),
                  "id": ((4,), _np.uint32)}
assert _C.sizeof(CViewFeatures) == 48, "lg_view_features is 48 bytes"
VIEW_FEATURE_PLANES = FEATURE_PLANES + ("point",)  # lg_view_features' members, in its order
_VIEW_FEATURE_SHAPE = dict(_FEATURE_SHAPE, point=((3,), _np.float32))


def Lens(kind, origin, right, up, forward, fov_deg=180.0):
    """An lg_lens: kind LENS_EQUIRECTANGULAR or LENS_FISHEYE, a basis used as given, and (fisheye) the full angle across the shorter side."""
    three = lambda v: (_C.c_double * 3)(*[float(c) for c in v])  # noqa: E731
    return CLens(int(kind), 0, three(origin), three(right), three(up), three(forward), float(fov_deg))


View = CView  # lg_view (include/lasgun_hip.h): a camera as the kernels read it, 120 bytes -- view_look_at / api.scene_view / api.accel_view make them


def _views(views):
    """A sequence of View (or one View) as a contiguous ctypes array of them."""
    vs = [views] if isinstance(views, CView) else list(views)
    for v in vs:
        if not isinstance(v, CView):
            raise TypeError("views: View records (lasgun_amd.View)")
    return (CView * len(vs))(*vs)


def tile_order_offsets(w, h, tile=8):
    """The film offsets y*w + x of every pixel of a w x h film in tile x tile-tile order (tiles row-major, pixels row-major inside a tile):
    the order in which neighbouring rays share a wave (uint64, w*h of them)."""
    ys, xs = _np.meshgrid(_np.arange(h, dtype=_np.uint64), _np.arange(w, dtype=_np.uint64), indexing="ij")
    t = _np.uint64(tile)
    key = ((ys // t) * _np.uint64((w + tile - 1) // tile) + xs // t) * (t * t) + (ys % t) * t + xs % t
    return (ys * _np.uint64(w) + xs).ravel()[_np.argsort(key.ravel(), kind="stable")].astype(_np.uint64)


HIT_NONE, HIT_SPHERE, HIT_BOX, HIT_TRIANGLE = 0, 1, 2, 3  # lg_hit::kind


class TuneEntry(_C.Structure):  # lg_tune_entry (include/lasgun_hip.h)
    _fields_ = [("key", _C.c_uint64 * 12), ("choice", _C.c_int32), ("reserved", _C.c_int32)]


class HipApi(Api):
    """The product's binding: core surface + the GPU-only extras of include/lasgun_hip.h."""

    def _stream(self, accel, stream):
        """hipStream_t to enqueue on: an explicit handle (0 = HIP's default stream, e.g. torch's
        `current_stream().cuda_stream`) or, when None, the accel's own stream."""
        if stream is None:
            return _C.c_void_p(self.call("accel_stream", accel.h))
        return _C.c_void_p(int(stream))

    def set_mode(self, accel, fast):
        """False = the reference traversal (parity path, default); True = the opt-in fast mode."""
        if self.call("accel_set_mode", accel.h, 1 if fast else 0):
            raise LasgunError(self.last_error())

    def set_prune(self, accel, enabled):
        """Pruned form of the reference traversal: None / -1 = the accel's default (on for scenes with a mesh of >= 4096
        triangles), False / True = off / on (include/lasgun_hip.h, lg_accel_set_prune)."""
        if self.call("accel_set_prune", accel.h, -1 if enabled is None or enabled == -1 else (1 if enabled else 0)):
            raise LasgunError(self.last_error())

    def set_shadow_skip(self, accel, enabled):
        """Level-by-level pipeline: skip the shadow walks of hits at which no light's term depends on its visibility (default on; same bytes
        either way; include/lasgun_hip.h, lg_accel_set_shadow_skip)."""
        if self.call("accel_set_shadow_skip", accel.h, 1 if enabled else 0):
            raise LasgunError(self.last_error())

    def set_level_door(self, accel, mask):
        """Exact walk, entering a nested accel: bit 0 = the one-axis probe at its door, bit 1 = a lone mesh and its group as one level
        (default 3; same results with every mask; include/lasgun_hip.h, lg_accel_set_level_door)."""
        if self.call("accel_set_level_door", accel.h, int(mask)):
            raise LasgunError(self.last_error())

    def set_l0_relative(self, accel, enabled):
        """Level-by-level pipeline, level 0's closest pass over an LDS-resident scene: node boxes and sphere slots held relative to the camera's
        origin where every ray of the launch shares it (default on; same bytes either way; include/lasgun_hip.h, lg_accel_set_l0_relative)."""
        if self.call("accel_set_l0_relative", accel.h, 1 if enabled else 0):
            raise LasgunError(self.last_error())

    def last_l0_relative(self, accel):
        """The form the last level-0 closest launch of the level-by-level pipeline took: True origin-relative, False absolute; None before the first."""
        v = self.call("accel_last_l0_relative", accel.h)
        return None if v < 0 else bool(v)

    def set_node_pairs(self, accel, enabled):
        """The exact walk from LDS over pair records, two boxes a trip (default on; same bytes either way; include/lasgun_hip.h,
        lg_accel_set_node_pairs)."""
        if self.call("accel_set_node_pairs", accel.h, 1 if enabled else 0):
            raise LasgunError(self.last_error())

    def last_node_pairs(self, accel):
        """The records the last launch over the LDS-resident scene read: True pair records, False node records, None before the first."""
        v = self.call("accel_last_node_pairs", accel.h)
        return None if v < 0 else bool(v)

    def set_packet_walk(self, accel, enabled):
        """Level 0's closest pass of the level-by-level pipeline in the packet form: one cursor and one stack per wave
        (default on; same bytes either way; include/lasgun_hip.h, lg_accel_set_packet_walk)."""
        if self.call("accel_set_packet_walk", accel.h, 1 if enabled else 0):
            raise LasgunError(self.last_error())

    def last_packet_walk(self, accel):
        """The form the last level-0 closest launch of the level-by-level pipeline took: True the packet form, False the per-lane walk,
        None before the first."""
        v = self.call("accel_last_packet_walk", accel.h)
        return None if v < 0 else bool(v)

    def scene_lds_image(self, scene, pairs):
        """The LDS image lg_accel_from would make for this scene, without a device: (uint32 words, info dict), or None where the tables
        do not fit in LDS (include/lasgun_hip.h, lg_scene_lds_image)."""
        info = (_C.c_uint32 * 8)()
        n = self.call("scene_lds_image", scene.h, 1 if pairs else 0, None, 0, info)
        if n < 0:
            raise LasgunError(self.last_error())
        if n == 0:
            return None
        words = _np.zeros(n, dtype=_np.uint32)
        self.call("scene_lds_image", scene.h, 1 if pairs else 0, words.ctypes.data_as(_C.POINTER(_C.c_uint32)), n, info)
        keys = ("units", "node_off", "prim_off", "soup_off", "accel_off", "pairs", "accels", "nodes")
        return words, {k: int(info[i]) for i, k in enumerate(keys)}

    def l0_relative_origins(self, scene):
        """The device-free part of that form's gate for a scene and its camera: the camera's origin in every accel's local space, (accels, 3)
        float64, or None where the gate says no (include/lasgun_hip.h, lg_scene_l0_relative_origins)."""
        import numpy as np
        out = np.zeros((64, 3), dtype=np.float64)
        n = self.call("scene_l0_relative_origins", scene.h, out.ctypes.data_as(_C.POINTER(_C.c_double)), 64)
        if n < 0:
            raise LasgunError(self.last_error())
        return out[:n].copy() if n else None

    def scene_packet_walk_gate(self, scene):
        """The scene graph's part of the packet walk's gate, without a device: 0 where the form may take the scene, otherwise the reason it
        may not (include/lasgun_hip.h, lg_scene_packet_walk_gate)."""
        v = self.call("scene_packet_walk_gate", scene.h)
        if v < 0:
            raise LasgunError(self.last_error())
        return int(v)

    def set_fused_shade(self, accel, enabled):
        """The camera's level 0 of the level-by-level pipeline in its fused form: the closest and shadow passes shade between them, no
        shade pass (default on; same bytes either way; include/lasgun_hip.h, lg_accel_set_fused_shade)."""
        if self.call("accel_set_fused_shade", accel.h, 1 if enabled else 0):
            raise LasgunError(self.last_error())

    def last_fused_shade(self, accel):
        """The form level 0 of the last chain of the level-by-level pipeline took: True fused (two passes), False the three kernels,
        None before the first."""
        v = self.call("accel_last_fused_shade", accel.h)
        return None if v < 0 else bool(v)

    def scene_fused_shade_gate(self, scene, camera_level0=True):
        """The fused form's gate for a scene, without a device: 0 where a render by the scene's own camera takes the form, otherwise the
        reason it does not (include/lasgun_hip.h, lg_scene_fused_shade_gate)."""
        v = self.call("scene_fused_shade_gate", scene.h, 1 if camera_level0 else 0)
        if v < 0:
            raise LasgunError(self.last_error())
        return int(v)

    def set_tri_frames(self, accel, enabled):
        """The frame table of flat triangles in the fused form's closest pass: a hit on a triangle with a record reads there what no ray
        enters (default on; same bytes either way; include/lasgun_hip.h, lg_accel_set_tri_frames)."""
        if self.call("accel_set_tri_frames", accel.h, 1 if enabled else 0):
            raise LasgunError(self.last_error())

    def last_tri_frames(self, accel):
        """Whether the level-0 closest launch of the last chain of the level-by-level pipeline read the frame table: True, False, None
        before the first."""
        v = self.call("accel_last_tri_frames", accel.h)
        return None if v < 0 else bool(v)

    def read_tri_frames(self, accel):
        """The accel's frame table as its device made it: a structured array of TRI_FRAME_DTYPE, one record per (mesh instance, triangle)
        in the plan's order (include/lasgun_hip.h, lg_accel_read_tri_frames)."""
        n = self.call("accel_read_tri_frames", accel.h, None, 0)
        if n < 0:
            raise LasgunError(self.last_error())
        rows = _np.zeros(n, dtype=TRI_FRAME_DTYPE)
        if n and self.call("accel_read_tri_frames", accel.h, rows.ctypes.data, n) != n:
            raise LasgunError(self.last_error())
        return rows

    def scene_tri_frames_gate(self, scene, cap=4096):
        """The frame table's plan for a scene, without a device: (records, base) -- the records an accel of the scene would hold (0: no
        table) and, per accel (the first `cap` of them), its first record or None (include/lasgun_hip.h, lg_scene_tri_frames_gate)."""
        base = (_C.c_uint32 * cap)(*([0xFFFFFFFE] * cap))
        v = self.call("scene_tri_frames_gate", scene.h, base, cap)
        if v < 0:
            raise LasgunError(self.last_error())
        return int(v), [None if b == 0xFFFFFFFF else int(b) for b in base if b != 0xFFFFFFFE]

    def last_organisation(self, accel):
        """What the accel's last launch ran as: "megakernel", "wavefront" (level by level), "queue"; None before the first."""
        v = self.call("accel_last_organisation", accel.h)
        name = {0: "megakernel", 1: "wavefront", 2: "queue"}.get(v & 15) if v >= 0 else None
        if name and (v & 16):
            name += ", bottom-up"
        if name and (v & 64):
            name += ", middle-out"
        if name and (v & 32):
            name += ", samples in a row"
        if name and (v & 128):
            name += ", tiles in parts"
        return name

    def set_tile_order(self, accel, order):
        """The direction the megakernel and the queue organisation claim a launch's tiles in: 0 top-down, 1 bottom-up, 2 from the middle row outwards, None / -1 = middle-out unless measured otherwise
        (include/lasgun_hip.h, lg_accel_set_tile_order).  Same bytes either way."""
        if self.call("accel_set_tile_order", accel.h, -1 if order is None else int(order)):
            raise LasgunError(self.last_error())

    def set_tile_parts(self, accel, parts):
        """The work item of the megakernel and of the queue organisation's level 0: a whole tile per wave (1) or a tile in 2 / 4 / 8 parts; None / -1 = whole unless measured otherwise for
        a small launch (include/lasgun_hip.h, lg_accel_set_tile_parts).  Same bytes either way."""
        if self.call("accel_set_tile_parts", accel.h, -1 if parts is None else int(parts)):
            raise LasgunError(self.last_error())

    def set_sample_order(self, accel, order):
        """A supersampled pixel's samples: 0 side by side in one launch chain, 1 one after the other, None / -1 = the default (side by side;
        the megakernel's form measured) (include/lasgun_hip.h, lg_accel_set_sample_order).  Same bytes either way."""
        if self.call("accel_set_sample_order", accel.h, -1 if order is None else int(order)):
            raise LasgunError(self.last_error())

    def get_prune(self, accel):
        """Whether a render of this accel uses the pruned reference walk right now (accel default, LASGUN_PRUNE, set_prune, fast mode)."""
        return bool(self.call("accel_get_prune", accel.h))

    def set_streaming(self, accel, enabled):
        """Kernel organisation (include/lasgun_hip.h, lg_accel_set_streaming): 1 / True = the accel's defaults, 0 / False = the
        megakernel only, 2 = the level-by-level wavefront pipeline wherever possible, 3 = the queue organisation (every recursion
        level in one persistent launch) wherever possible.  Same bytes out in every organisation."""
        if self.call("accel_set_streaming", accel.h, int(enabled) if enabled in (0, 1, 2, 3) else (1 if enabled else 0)):
            raise LasgunError(self.last_error())

    def set_wf_split(self, accel, bands):
        """Bands of a big wavefront launch on internal streams (0 = default; include/lasgun_hip.h, lg_accel_set_wf_split)."""
        self.call("accel_set_wf_split", accel.h, int(bands))

    def set_lds_scene(self, accel, enabled):
        """Scene tables resident in LDS for the streaming traversal kernels (default on); returns
        whether this accel's scene is small enough for that variant to exist."""
        return bool(self.call("accel_set_lds_scene", accel.h, 1 if enabled else 0))

    def set_device(self, device):
        if self.call("set_device", int(device)):
            raise LasgunError(self.last_error())

    def trace_pixel_log(self, accel, w, h, x, y, fast=False, nlights=1):
        """trace_pixel plus the event log of the PRIMARY ray's walk: rows of (code, a, b, c) -- 1.xy fast node pair
        (x/y = child boxes hit; a = accel*1e5 + node, b/c = tnear of the children), 2.x reference node, 3.x primitive
        test (a = primref, b = t, c = accel; .1 = accepted), 4 / 4.5 accel entry, 5 return, 6 triangle accepted, 9 end."""
        need = 7 + 2 * nlights
        n = need + 1 + 4 * 4000
        out = (_C.c_double * n)()
        if self.call("trace_pixel", accel.h, int(w), int(h), int(x), int(y), 1 if fast else 0, out, n):
            raise LasgunError(self.last_error())
        cnt = int(out[need])
        return [tuple(out[need + 1 + 4 * i + k] for k in range(4)) for i in range(cnt)]

    def trace_pixel(self, accel, w, h, x, y, fast=False, max_lights=64):
        """{"t", "ref", "accel", "shadow": [(t, ref), ...]} of pixel (x, y), sample 0 (debugging / test hook)."""
        n = 7 + 2 * max_lights
        out = (_C.c_double * n)()
        if self.call("trace_pixel", accel.h, int(w), int(h), int(x), int(y), 1 if fast else 0, out, n):
            raise LasgunError(self.last_error())
        nl = int(out[3])
        return {"t": out[0], "ref": int(out[1]), "accel": int(out[2]), "shadow": [(out[4 + 2 * l], int(out[5 + 2 * l])) for l in range(nl)],
                "shadow_origin": [out[4 + 2 * nl], out[5 + 2 * nl], out[6 + 2 * nl]]}

    def set_devices(self, ids=None):
        """Devices a host-film `capture` / `render` is split over (None or [] = every visible device)."""
        ids = list(ids or [])
        arr = (_C.c_int * max(len(ids), 1))(*ids)
        if self.call("set_devices", arr, len(ids)):
            raise LasgunError(self.last_error())

    def trim_pool(self, device=-1):
        """Give the device buffers parked in the library's pool back to the driver; returns the bytes freed."""
        return int(self.call("trim_pool", int(device)))

    def device_count(self):
        return int(self.call("device_count"))

    def capture_rows_device(self, accel, width, height, y0, y1, dev_ptr, row0=None, stream=None):
        """Enqueue rows [y0, y1) into device memory at `dev_ptr` (pixel (0,row0) first). No host copy."""
        if self.call("capture_rows_device", accel.h, width, height, y0, y1, y0 if row0 is None else row0,
                     _C.c_void_p(int(dev_ptr)), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def capture_interleaved_device(self, accel, width, height, block_rows, n, r, dev_ptr, stream=None):
        """Enqueue the rows {y : (y // block_rows) % n == r} into a compact (height/n)-row device tile."""
        if self.call("capture_interleaved_device", accel.h, width, height, block_rows, n, r, _C.c_void_p(int(dev_ptr)),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def capture_subset_device(self, k, n, accel, width, height, dev_ptr, stream=None):
        if self.call("capture_subset_device", k, n, accel.h, width, height, _C.c_void_p(int(dev_ptr)),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def capture_subsets(self, ks, n, accel, film):
        """Several subsets of one n as ONE render: writes exactly the pixels of the calls capture_subset(k, n, ...) for k in ks (no
        counterpart in the reference, whose progressive caller makes those calls one by one: www/renderer.ts:103-120)."""
        ks = [int(k) for k in ks]
        arr = (_C.c_size_t * max(len(ks), 1))(*ks)
        if self.call("capture_subsets", arr, len(ks), int(n), accel.h, film.h):
            raise LasgunError(self.last_error())

    def capture_subsets_device(self, ks, n, accel, width, height, dev_ptr, stream=None):
        """Enqueue the subsets {k + i*n}, k in ks, as one render into a full width*height device film."""
        ks = [int(k) for k in ks]
        arr = (_C.c_size_t * max(len(ks), 1))(*ks)
        if self.call("capture_subsets_device", arr, len(ks), int(n), accel.h, width, height, _C.c_void_p(int(dev_ptr)),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def synchronize(self, accel):
        if self.call("accel_synchronize", accel.h):
            raise LasgunError(self.last_error())

    def capture_radiance(self, accel, w, h, k=0, n=1, **_):
        rgb = _np.full((h, w, 3), _np.nan, dtype=_np.float64)
        if self.call("capture_radiance", k, n, accel.h, w, h, rgb.ctypes.data):
            raise LasgunError(self.last_error())
        return rgb

    def capture_pixels(self, accel, w, h, offsets, radiance=True):
        """(rgba (n, 4) uint8, radiance (n, 3) float64 or None) of the pixels `offsets` (y * w + x), in list order."""
        off = _np.ascontiguousarray(offsets, dtype=_np.uint64)
        rgba = _np.zeros((off.size, 4), dtype=_np.uint8)
        rad = _np.full((off.size, 3), _np.nan, dtype=_np.float64) if radiance else None
        if self.call("capture_pixels", accel.h, w, h, off.ctypes.data, off.size, rgba.ctypes.data, rad.ctypes.data if radiance else None):
            raise LasgunError(self.last_error())
        return rgba, rad

    def capture_rect(self, accel, w, h, x0, y0, x1, y1, radiance=True):
        """(rgba (y1-y0, x1-x0, 4) uint8, radiance (y1-y0, x1-x0, 3) float64 or None) of a crop of the w x h film."""
        rgba = _np.zeros((y1 - y0, x1 - x0, 4), dtype=_np.uint8)
        rad = _np.full((y1 - y0, x1 - x0, 3), _np.nan, dtype=_np.float64) if radiance else None
        if self.call("capture_rect", accel.h, w, h, x0, y0, x1, y1, rgba.ctypes.data, rad.ctypes.data if radiance else None):
            raise LasgunError(self.last_error())
        return rgba, rad

    def capture_stats(self, accel, w, h, y0=0, y1=None):
        s = CStats()
        if self.call("capture_stats", accel.h, w, h, y0, h if y1 is None else y1, _C.byref(s)):
            raise LasgunError(self.last_error())
        return s.as_dict()

    def audit_prune(self, accel, w, h, y0=0, y1=None):
        """Audit of the pruned reference walk on rows [y0, y1) (include/lasgun_hip.h, lg_audit_prune): every node / run it skips
        is also walked the reference's way; `violations` (skipped primitives the reference would have accepted) must be 0."""
        class _A(_C.Structure):
            _fields_ = [("skipped_nodes", _C.c_uint64), ("skipped_runs", _C.c_uint64), ("primitives", _C.c_uint64), ("violations", _C.c_uint64),
                        ("min_slack_nodes", _C.c_double), ("min_slack_runs", _C.c_double), ("max_margin_used_nodes", _C.c_double)]
        r = _A()
        if self.call("audit_prune", accel.h, w, h, y0, h if y1 is None else y1, _C.byref(r)):
            raise LasgunError(self.last_error())
        return {k: getattr(r, k) for k, _ in _A._fields_}

    def audit_fast(self, accel, w, h, y0=0, y1=None):
        """Audit of the opt-in FAST mode on rows [y0, y1) (lg_audit_fast): every ray also walked the reference's way on the device;
        {"rays", "fallbacks", "violations"} -- `violations` (rays whose answer is not the reference's) must be 0."""
        class _A(_C.Structure):
            _fields_ = [("rays", _C.c_uint64), ("fallbacks", _C.c_uint64), ("violations", _C.c_uint64)]
        r = _A()
        if self.call("audit_fast", accel.h, w, h, y0, h if y1 is None else y1, _C.byref(r)):
            raise LasgunError(self.last_error())
        return {k: int(getattr(r, k)) for k, _ in _A._fields_}

    def capture_stats_kind(self, accel, w, h, kind, y0=0, y1=None):
        """Work counters of one kind of traversal: 1 = closest-hit (primary/secondary), 2 = shadow."""
        s = CStats()
        if self.call("capture_stats_kind", accel.h, w, h, y0, h if y1 is None else y1, int(kind), _C.byref(s)):
            raise LasgunError(self.last_error())
        return s.as_dict()

    def profile_read_kinds(self, accel):
        """Streaming pipeline: {kernel: (total ms, launches)} from HIP events around each kernel."""
        ms = (_C.c_double * 5)(); n = (_C.c_uint64 * 5)()
        if self.call("profile_read_kinds", accel.h, ms, n):
            raise LasgunError(self.last_error())
        names = ("trace<closest>", "combine", "trace<shadow>", "shade", "trace_kernel")
        return {names[i]: (ms[i], int(n[i])) for i in range(5)}

    def profile_enable(self, accel, enabled=True):
        self.call("profile_enable", accel.h, 1 if enabled else 0)

    def profile_read(self, accel):
        ms = _C.c_double(); n = _C.c_uint64()
        if self.call("profile_read", accel.h, _C.byref(ms), _C.byref(n)):
            raise LasgunError(self.last_error())
        return ms.value, int(n.value)

    def host_build_dump(self, scene):
        """Host-only BVH build + flatten (no GPU needed): (floats, ints, info dict)."""
        pf = _C.POINTER(_C.c_double)(); nf = _C.c_size_t(); pi = _C.POINTER(_C.c_int64)(); ni = _C.c_size_t()
        info = (_C.c_uint64 * 8)()
        if self.call("host_build_dump", scene.h, _C.byref(pf), _C.byref(nf), _C.byref(pi), _C.byref(ni), info):
            raise LasgunError(self.last_error())
        f = _np.ctypeslib.as_array(pf, shape=(nf.value,)).copy()
        i = _np.ctypeslib.as_array(pi, shape=(ni.value,)).copy()
        keys = ("nodes", "primrefs", "spheres", "cuboids", "triangles", "accels", "max_stack", "has_specular")
        return f, i, dict(zip(keys, [int(v) for v in info]))

    def host_check_strips(self, scene):
        """Host-only self-check of the triangle strips of the mesh leaves (include/lasgun_hip.h, lg_host_check_strips)."""
        out = (_C.c_uint64 * 8)()
        if self.call("host_check_strips", scene.h, out):
            raise LasgunError(self.last_error())
        return dict(zip(("leaves", "runs", "triangles", "entries", "violations", "records_hash", "strips_hash"), [int(v) for v in out]))

    def host_check_wide_records(self, scene):
        """Host-only self-check of the fast mode's wide node records (no GPU needed): dict of counts; `violations` must be 0."""
        out = (_C.c_uint64 * 8)()
        if self.call("host_check_wide_records", scene.h, out):
            raise LasgunError(self.last_error())
        keys = ("records", "children", "leaves", "deepest_stack", "violations", "reserved_stack")
        return dict(zip(keys, [int(v) for v in out]))

    # ---- the table of measured organisation choices (lg_tune_*): entries are (twelve key words, choice) tuples
    def tune_export(self):
        n = int(self.call("tune_export", None, 0))
        buf = (TuneEntry * max(n, 1))()
        m = int(self.call("tune_export", _C.cast(buf, _C.c_void_p), n))
        return [(tuple(int(x) for x in buf[i].key), int(buf[i].choice)) for i in range(min(n, m))]

    def tune_import(self, entries):
        entries = list(entries)
        buf = (TuneEntry * max(len(entries), 1))()
        for i, (key, choice) in enumerate(entries):
            for j in range(12):
                buf[i].key[j] = int(key[j])
            buf[i].choice = int(choice)
        if self.call("tune_import", _C.cast(buf, _C.c_void_p), len(entries)):
            raise LasgunError(self.last_error())

    def tune_clear(self):
        self.call("tune_clear")

    def Multi(self, scene, devices, block_rows=64):
        """One film on several GPUs of this process, gathered on devices[0] over xGMI with one grouped RCCL exchange
        (lg_multi_*): `.capture_device(w, h, dev_ptr)`, `.capture(film)`, `.accel(rank)`, `.uses_rccl`."""
        api = self

        class _Multi:
            def __init__(self):
                ids = list(devices)
                arr = (_C.c_int * max(len(ids), 1))(*ids)
                self.scene = scene  # borrowed by the C side: keep it alive
                self.h = api.call("multi_create", scene.h, arr, len(ids), int(block_rows))
                if not self.h:
                    raise LasgunError(api.last_error())

            @property
            def uses_rccl(self):
                return bool(api.call("multi_uses_rccl", self.h))

            @property
            def ranks(self):
                return int(api.call("multi_rank_count", self.h))

            def accel(self, rank):
                class _Borrowed:  # the multi owns it
                    pass
                a = _Borrowed()
                a.h = api.call("multi_accel", self.h, int(rank))
                return a

            def capture_device(self, w, h, dev_ptr):
                if api.call("multi_capture_device", self.h, int(w), int(h), _C.c_void_p(int(dev_ptr))):
                    raise LasgunError(api.last_error())

            def capture_device_all(self, w, h, dev_ptrs):
                """All-gather form: dev_ptrs[r] = a w*h*4-byte buffer on rank r's device; every one receives the whole film."""
                arr = (_C.c_void_p * len(dev_ptrs))(*[int(p) for p in dev_ptrs])
                if api.call("multi_capture_device_all", self.h, int(w), int(h), arr):
                    raise LasgunError(api.last_error())

            def capture(self, film):
                if api.call("multi_capture", self.h, film.h):
                    raise LasgunError(api.last_error())

            def close(self):
                if self.h:
                    api.call("multi_free", self.h)
                    self.h = None

            def __del__(self):
                try:
                    self.close()
                except Exception:  # noqa: BLE001
                    pass
        return _Multi()

    def probe_rate(self, what):
        """Measured GB/s of the current device: "hbm_copy" (read + written bytes) or "lds_read"."""
        v = _C.c_double()
        if self.call("probe_rate", {"hbm_copy": 0, "lds_read": 1}[what], _C.byref(v)):
            raise LasgunError(self.last_error())
        return v.value

    # ---- ray queries (include/lasgun_hip.h, lg_intersect*): the caller's own rays through the render's walk, in the accel's traversal mode
    @staticmethod
    def _rays(rays):
        r = _np.ascontiguousarray(rays, dtype=_np.float64)
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("rays: an (n, 6) array of origin xyz, direction xyz")
        return r

    def intersect(self, accel, rays):
        """Closest hit of every ray of an (n, 6) float64 array (origin, direction): a structured array of HIT_DTYPE (lg_hit)."""
        r = self._rays(rays)
        hits = _np.zeros(r.shape[0], dtype=HIT_DTYPE)
        if self.call("intersect", accel.h, r.ctypes.data, r.shape[0], hits.ctypes.data):
            raise LasgunError(self.last_error())
        return hits

    def occluded(self, accel, rays):
        """Whether each segment o -> o + d of an (n, 6) float64 array is blocked (closest hit t < 1, point.rs:49): a bool array."""
        r = self._rays(rays)
        occ = _np.zeros(r.shape[0], dtype=_np.uint8)
        if self.call("occluded", accel.h, r.ctypes.data, r.shape[0], occ.ctypes.data):
            raise LasgunError(self.last_error())
        return occ.astype(bool)

    def intersect_device(self, accel, n, rays_ptr, hits_ptr, stream=None):
        """Enqueue the closest hits of n rays (device memory, 6 doubles each) into n lg_hit records at hits_ptr (16-byte aligned)."""
        if self.call("intersect_device", accel.h, _C.c_void_p(int(rays_ptr)), int(n), _C.c_void_p(int(hits_ptr)), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def occluded_device(self, accel, n, rays_ptr, occluded_ptr, stream=None):
        """Enqueue the occlusion bytes (1 = blocked) of n segments (device memory, 6 doubles each) into occluded_ptr."""
        if self.call("occluded_device", accel.h, _C.c_void_p(int(rays_ptr)), int(n), _C.c_void_p(int(occluded_ptr)), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- visibility matrices (include/lasgun_hip.h, lg_visibility*): occlusion between two point sets, the segments made on the device
    @staticmethod
    def _points(pts, what):
        p = _np.ascontiguousarray(pts, dtype=_np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("%s: an (n, 3) array of points" % what)
        return p

    def visibility(self, accel, from_pts, to_pts, counts=False, row_bytes=None, into=None):
        """Which segments from_pts[i] -> to_pts[j] are blocked: an (n_from, ceil(n_to / 8)) uint8 array, bit j of row i
        ((bits[i, j >> 3] >> (j & 7)) & 1, numpy's packbits(bitorder="little") per row) set iff lg_occluded answers 1 for the ray
        (from_pts[i], to_pts[j] - from_pts[i]).  counts=True: (bits, blocked), blocked[i] the uint32 number of set bits of row i;
        counts="only": blocked alone (no bit matrix is made).  row_bytes: a wider row stride (the array returned is then (n_from, row_bytes));
        into = (bits array or None, blocked array or None): C-contiguous buffers written in place -- bytes behind a row's used part keep their value.
        Also `accel.visibility(from_pts, to_pts, counts=False)`."""
        f, t = self._points(from_pts, "from_pts"), self._points(to_pts, "to_pts")
        used = (t.shape[0] + 7) // 8
        stride = used if row_bytes is None else int(row_bytes)
        if into is not None:
            bits, blocked = into
        else:
            bits = None if counts == "only" else _np.zeros((f.shape[0], stride), dtype=_np.uint8)
            blocked = _np.zeros(f.shape[0], dtype=_np.uint32) if counts else None
        for arr, dt in ((bits, _np.uint8), (blocked, _np.uint32)):
            if arr is not None and (arr.dtype != dt or not arr.flags["C_CONTIGUOUS"]):
                raise ValueError("into: C-contiguous uint8 bits and uint32 blocked")
        if self.call("visibility", accel.h, f.ctypes.data if f.size else None, f.shape[0], t.ctypes.data if t.size else None, t.shape[0],
                     bits.ctypes.data if bits is not None and bits.size else None, stride,
                     blocked.ctypes.data if blocked is not None and blocked.size else None):
            raise LasgunError(self.last_error())
        if bits is not None and blocked is not None:
            return bits, blocked
        return bits if bits is not None else blocked

    def visibility_device(self, accel, n_from, from_ptr, n_to, to_ptr, bits_ptr=None, row_bytes=None, blocked_ptr=None, stream=None):
        """Enqueue the visibility matrix of n_from x n_to points (device memory, 3 doubles each) into n_from rows of row_bytes bytes at bits_ptr
        (default ceil(n_to / 8)) and / or n_from uint32 row counts at blocked_ptr."""
        ptr = lambda p: _C.c_void_p(int(p)) if p is not None else None  # noqa: E731
        stride = (int(n_to) + 7) // 8 if row_bytes is None else int(row_bytes)
        if self.call("visibility_device", accel.h, ptr(from_ptr), int(n_from), ptr(to_ptr), int(n_to), ptr(bits_ptr), stride, ptr(blocked_ptr),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- direction sets (include/lasgun_hip.h, lg_open_directions*): which of K shared directions are open above each of N points
    def open_directions(self, accel, points, dirs, normals=None, counts=False, row_bytes=None, into=None):
        """Which directions dirs[k] are open at points[i]: an (n_points, ceil(n_dirs / 8)) uint8 array, bit k of row i
        ((bits[i, k >> 3] >> (k & 7)) & 1, numpy's packbits(bitorder="little") per row) set iff the direction is above the point's horizon
        ((n.x*d.x + n.y*d.y) + n.z*d.z > 0.0; every direction when normals is None) and lg_occluded answers 0 for the ray (points[i], dirs[k]).
        The direction's length is the reach; the origin is used as given.  counts=True: (bits, open, above), the uint32 numbers of open
        directions and of directions above per point; counts="only": (open, above) alone (no bit matrix is made).  row_bytes: a wider row
        stride (the array returned is then (n_points, row_bytes)); into = (bits array or None, open array or None, above array or None):
        C-contiguous buffers of those shapes written in place -- bytes behind a row's used part keep their value; the outputs are then the
        arrays given, whatever `counts` says.
        Also `accel.open_directions(points, dirs, normals=None, counts=False)`."""
        p, d = self._points(points, "points"), self._points(dirs, "dirs")
        n = None if normals is None else self._points(normals, "normals")
        if n is not None and n.shape != p.shape:
            raise ValueError("normals: one per point")
        used = (d.shape[0] + 7) // 8
        stride = used if row_bytes is None else int(row_bytes)
        if into is not None:
            bits, nopen, above = into
        else:
            bits = None if counts == "only" else _np.zeros((p.shape[0], stride), dtype=_np.uint8)
            nopen = _np.zeros(p.shape[0], dtype=_np.uint32) if counts else None
            above = _np.zeros(p.shape[0], dtype=_np.uint32) if counts else None
        for arr, dt in ((bits, _np.uint8), (nopen, _np.uint32), (above, _np.uint32)):
            if arr is not None and (arr.dtype != dt or not arr.flags["C_CONTIGUOUS"]):
                raise ValueError("into: C-contiguous uint8 bits, uint32 open and above")
        if bits is not None and (bits.ndim != 2 or bits.shape[0] != p.shape[0] or bits.shape[1] != stride):
            raise ValueError("into: bits of shape (n_points, row_bytes)")
        for arr in (nopen, above):
            if arr is not None and arr.shape != (p.shape[0],):
                raise ValueError("into: open and above of shape (n_points,)")
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        if self.call("open_directions", accel.h, data(p), data(n), p.shape[0], data(d), d.shape[0], data(bits), stride, data(nopen), data(above)):
            raise LasgunError(self.last_error())
        out = tuple(a for a in (bits, nopen, above) if a is not None)
        return out[0] if len(out) == 1 else out

    def open_directions_device(self, accel, n_points, points_ptr, normals_ptr, n_dirs, dirs_ptr, bits_ptr=None, row_bytes=None, open_ptr=None, above_ptr=None,
                               stream=None):
        """Enqueue the open directions of n_points points (device memory, 3 doubles each; normals_ptr may be None) against n_dirs directions
        into n_points rows of row_bytes bytes at bits_ptr (default ceil(n_dirs / 8)) and / or n_points uint32 counts at open_ptr and above_ptr."""
        ptr = lambda p: _C.c_void_p(int(p)) if p is not None else None  # noqa: E731
        stride = (int(n_dirs) + 7) // 8 if row_bytes is None else int(row_bytes)
        if self.call("open_directions_device", accel.h, ptr(points_ptr), ptr(normals_ptr), int(n_points), ptr(dirs_ptr), int(n_dirs), ptr(bits_ptr), stride,
                     ptr(open_ptr), ptr(above_ptr), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def ambient_occlusion(self, accel, points, normals, k=64, radius=1.0):
        """open / max(above, 1) per point, float64, for `k` Fibonacci directions (sphere_directions) of length `radius`: the share of the
        hemisphere above each point that is unblocked within `radius`.  A convention of this WRAPPER, not of the C contract."""
        nopen, above = self.open_directions(accel, points, sphere_directions(k, radius), normals, counts="only")
        return nopen.astype(_np.float64) / _np.maximum(above, 1).astype(_np.float64)

    # ---- range scans (include/lasgun_hip.h, lg_range_scan*): the first hits along K shared beams from N sensor poses
    @staticmethod
    def _scan_lanes(lanes):
        return SCAN_LANES[lanes] if isinstance(lanes, str) else int(lanes)

    def range_scan_lanes(self, n_poses, n_beams, lanes=0):
        """The work item a scan of these counts would use: 1 beam lanes (one pose x 64 beams a wave), 2 pose lanes (64 poses x 8 beams);
        -1 for a bad `lanes`.  lanes: 0 / "auto" (pose lanes iff n_poses >= n_beams), 1 / "beam", 2 / "pose".  No device is touched."""
        return int(self.call("range_scan_lanes", int(n_poses), int(n_beams), self._scan_lanes(lanes)))

    def range_scan(self, accel, origins, beams, frames=None, planes=("range",), lanes=0, into=None):
        """The first hits along beams[k] from origins[i]: a dict of the planes asked for (any of "range", "point", "normal", "id", "hits",
        "nearest") -- float32 (n_poses, n_beams) range = the hit's t (+inf: a miss), float32 (n_poses, n_beams, 3) point and normal (the
        geometric normal faced toward the sensor; zeros on a miss), uint32 (n_poses, n_beams, 4) id = kind, prim, instance, material (0, ~0,
        ~0, -1 on a miss), uint32 (n_poses,) hits = the beams that hit, float32 (n_poses,) nearest = the smallest non-negative finite range
        (+inf: none).  frames: (n_poses, 3, 3) or (n_poses, 9) float64, row-major matrices whose columns are the sensor's axes in world space,
        d[c] = (M[c,0]*b.x + M[c,1]*b.y) + M[c,2]*b.z; None: the beams are the directions, bit for bit.  The directions are not normalised.
        lanes: range_scan_lanes' (the outputs do not depend on it).  `into`: a dict of C-contiguous arrays of those shapes, written in place.
        Also `accel.range_scan(origins, beams, frames=None, planes=("range",), lanes=0)`."""
        o, b = self._points(origins, "origins"), self._points(beams, "beams")
        m = None
        if frames is not None:
            m = _np.ascontiguousarray(frames, dtype=_np.float64)
            if m.shape not in ((o.shape[0], 3, 3), (o.shape[0], 9)):
                raise ValueError("frames: one 3 x 3 matrix per pose")
        planes = tuple(planes)
        if any(p not in SCAN_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (SCAN_PLANES,))
        out = {}
        for p in planes:
            tail, dt, per_pair = _SCAN_SHAPE[p]
            shape = ((o.shape[0], b.shape[0]) if per_pair else (o.shape[0],)) + tail
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CScanOut(*[data(out.get(p)) for p in SCAN_PLANES])
        if self.call("range_scan", accel.h, data(o), data(m), o.shape[0], data(b), b.shape[0], self._scan_lanes(lanes), _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def range_scan_device(self, accel, n_poses, origins_ptr, frames_ptr, n_beams, beams_ptr, range_ptr=None, point_ptr=None, normal_ptr=None, id_ptr=None,
                          hits_ptr=None, nearest_ptr=None, lanes=0, stream=None):
        """Enqueue the scan of n_poses poses (device memory, 3 doubles an origin; frames_ptr 9 doubles a pose or None) along n_beams beams
        (3 doubles each) into device memory: n_poses * n_beams elements at range_ptr (f32), point_ptr and normal_ptr (3 f32), id_ptr (4 u32,
        16-byte aligned), n_poses elements at hits_ptr (u32) and nearest_ptr (f32); each may be None, not all."""
        ptr = lambda p: _C.c_void_p(int(p)) if p is not None else None  # noqa: E731
        f = CScanOut(*[int(p) if p is not None else None for p in (range_ptr, point_ptr, normal_ptr, id_ptr, hits_ptr, nearest_ptr)])
        if self.call("range_scan_device", accel.h, ptr(origins_ptr), ptr(frames_ptr), int(n_poses), ptr(beams_ptr), int(n_beams), self._scan_lanes(lanes),
                     _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- hit layers (include/lasgun_hip.h, lg_hit_layers*): the first K surfaces along each ray in one call
    def hit_layers(self, accel, rays, max_layers, planes=("along", "id", "count"), into=None):
        """The first max_layers surfaces along every ray of an (n, 6) float64 array: a dict of the planes asked for (any of "hits", "along",
        "id", "count", "inside"), LAYER-MAJOR -- HIT_DTYPE (K, n) hits = lg_intersect's record of layer j of ray i at [j, i] (the miss record
        behind a ray's last layer), float64 (K, n) along = t_0 + .. + t_j (+inf behind the last layer), uint32 (K, n, 4) id = kind, prim,
        instance, material (0, ~0, ~0, -1 behind the last layer), uint32 (n,) count = the layers found (== K: the ray may have been cut
        short), float64 (n,) inside = t_1 + t_3 + ..: the length inside material of a ray that starts outside every closed solid.  Segment
        j + 1 starts at layer j's p - ng * 2**-36 and keeps the ray's direction.  `into`: a dict of C-contiguous arrays of those shapes,
        written in place.  Also `accel.hit_layers(rays, max_layers, planes=...)`."""
        r = self._rays(rays)
        n, k = r.shape[0], int(max_layers)
        planes = tuple(planes)
        if any(p not in LAYER_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (LAYER_PLANES,))
        if not 0 <= k <= 0xFFFFFFFF:
            raise ValueError("max_layers: 0 .. 2^32 - 1")
        out = {}
        for p in planes:
            tail, dt, per_layer = _LAYER_SHAPE[p]
            shape = ((k, n) if per_layer else (n,)) + tail
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        # (an array without elements is not named: with k == 0 the library sees no plane and n > 0 rays, and says so)
        f = CLayersOut(*[data(out.get(p)) for p in LAYER_PLANES])
        if self.call("hit_layers", accel.h, data(r), n, k, _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def hit_layers_device(self, accel, n, rays_ptr, max_layers, hits_ptr=None, along_ptr=None, id_ptr=None, count_ptr=None, inside_ptr=None, stream=None):
        """Enqueue the hit layers of n rays (device memory, 6 doubles each) into device memory, layer-major: max_layers * n elements at
        hits_ptr (lg_hit, 16-byte aligned), along_ptr (f64) and id_ptr (4 u32, 16-byte aligned), n elements at count_ptr (u32) and inside_ptr
        (f64); each may be None, not all.  The pointers are integers (torch: tensor.data_ptr()) or objects with a data_ptr()."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        f = CLayersOut(*[ptr(p) for p in (hits_ptr, along_ptr, id_ptr, count_ptr, inside_ptr)])
        rays = ptr(rays_ptr)
        if self.call("hit_layers_device", accel.h, _C.c_void_p(rays) if rays is not None else None, int(n), int(max_layers), _C.addressof(f),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- ray paths (include/lasgun_hip.h, lg_trace_paths*): each ray followed through K specular bounces in one call
    def path_rules(self, accel, default=PATH_ABSORB, gain=1.0):
        """A rule table for trace_paths, one PATH_RULE_DTYPE record per material of the accel: glass -> PATH_REFRACT with the material's eta,
        mirror and metal -> PATH_REFLECT, the rest -> `default`; every gain = `gain`.  A convention of this WRAPPER, not of the C contract
        (lg_trace_paths takes whatever table the caller passes)."""
        rules = _np.zeros(self.material_count(accel), dtype=PATH_RULE_DTYPE)
        rules["action"], rules["ior"], rules["gain"] = int(default), 1.0, float(gain)
        for i in range(len(rules)):
            m = self.accel_material(accel, i)
            if m["kind"] == 3:            # glass: p[6] = eta
                rules[i]["action"], rules[i]["ior"] = PATH_REFRACT, m["p"][6]
            elif m["kind"] in (2, 4):     # metal, mirror
                rules[i]["action"] = PATH_REFLECT
        return rules

    @staticmethod
    def _path_rules(rules):
        r = _np.ascontiguousarray(rules)
        if r.dtype != PATH_RULE_DTYPE or r.ndim != 1:
            raise ValueError("rules: a 1-D array of PATH_RULE_DTYPE (la.path_rules(accel) makes one)")
        return r

    def trace_paths(self, accel, rays, max_bounces, rules, normal=0, start_medium=None, planes=("point", "id", "count", "end"), into=None):
        """Every ray of an (n, 6) float64 array followed through up to max_bounces vertices: a dict of the planes asked for (any of
        PATH_PLANES).  VERTEX-MAJOR: HIT_DTYPE (K, n) hits = lg_intersect's record of vertex j of ray i at [j, i] (the miss record behind a
        path's last vertex), float64 (K, n, 3) point, uint32 (K, n, 4) id = kind, prim, instance, material, float64 (K, n) along = the
        running sum of t (+inf behind the last vertex).  Per ray: uint32 (n,) count, end (PATH_END_*) and medium, float64 (n,) gain and
        (n, 6) last = the ray to resume a cut path from (or the segment the path ended on).  rules: PATH_RULE_DTYPE, one per material
        (path_rules(accel) is one convention); normal: 0 the geometric, 1 the shading normal; start_medium: (n,) uint32, bit 0 = the ray
        starts inside (None: all outside).  `into`: a dict of C-contiguous arrays of those shapes, written in place."""
        r = self._rays(rays)
        n, k = r.shape[0], int(max_bounces)
        planes = tuple(planes)
        if any(p not in PATH_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (PATH_PLANES,))
        if not 0 <= k <= 0xFFFFFFFF:
            raise ValueError("max_bounces: 0 .. 2^32 - 1")
        table = self._path_rules(rules)
        sm = None
        if start_medium is not None:
            sm = _np.ascontiguousarray(start_medium, dtype=_np.uint32)
            if sm.shape != (n,):
                raise ValueError("start_medium: (n,) uint32")
        out = {}
        for p in planes:
            tail, dt, per_vertex = _PATH_SHAPE[p]
            shape = ((k, n) if per_vertex else (n,)) + tail
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CPathsOut(*[data(out.get(p)) for p in PATH_PLANES])
        if self.call("trace_paths", accel.h, data(r), n, k, table.ctypes.data, len(table), int(normal), data(sm), _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def trace_paths_device(self, accel, n, rays_ptr, max_bounces, rules, normal=0, start_medium_ptr=None, hits_ptr=None, point_ptr=None, id_ptr=None, along_ptr=None,
                           count_ptr=None, end_ptr=None, gain_ptr=None, last_ptr=None, medium_ptr=None, stream=None):
        """Enqueue the paths of n rays (device memory, 6 doubles each) into device memory, vertex-major: max_bounces * n elements at hits_ptr
        (lg_hit, 16-byte aligned), point_ptr (3 f64), id_ptr (4 u32, 16-byte aligned) and along_ptr (f64), n elements at count_ptr, end_ptr,
        medium_ptr (u32), gain_ptr (f64) and last_ptr (6 f64); each may be None, not all.  rules is a HOST table (PATH_RULE_DTYPE), copied
        before the call returns; start_medium_ptr: n u32 in device memory or None.  The pointers are integers (torch: tensor.data_ptr()) or
        objects with a data_ptr()."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        f = CPathsOut(*[ptr(p) for p in (hits_ptr, point_ptr, id_ptr, along_ptr, count_ptr, end_ptr, gain_ptr, last_ptr, medium_ptr)])
        table = self._path_rules(rules)
        rays, sm = ptr(rays_ptr), ptr(start_medium_ptr)
        if self.call("trace_paths_device", accel.h, _C.c_void_p(rays) if rays is not None else None, int(n), int(max_bounces), table.ctypes.data, len(table),
                     int(normal), _C.c_void_p(sm) if sm is not None else None, _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- surface scatter (include/lasgun_hip.h, lg_scatter*): one level of li()'s tree, opened
    def scatter(self, accel, rays, planes=SCATTER_PLANES, into=None):
        """One level of li()'s tree for every ray of an (n, 6) float64 array: a dict of the planes asked for (any of SCATTER_PLANES), each
        indexed by the ray -- HIT_DTYPE (n,) hits = lg_intersect's record, float64 (n, 3) direct = the lights in order + ambient at a hit,
        the background li() returns at a miss, uint32 (n,) flags = SCATTER_HIT | SCATTER_REFLECT | SCATTER_REFRACT, float64 (n, 6) reflect
        and refract = the specular children's rays, (n, 3) reflect_weight = the reflected child's spectrum, (n, 5) refract_weight =
        spectrum[3], |wi . ns|, pdf.  An absent child's elements are +0.0.  li() to depth D is
        (direct + reflect_weight * L(reflect)) + (refract_weight[:3] * L(refract)) * cos / pdf, bottomed out by direct alone; the scene's
        own max_recursion_depth plays no part.  `into`: a dict of C-contiguous arrays of those shapes, written in place.  Also
        `accel.scatter(rays, planes=...)`."""
        r = self._rays(rays)
        n = r.shape[0]
        planes = tuple(planes)
        if any(p not in SCATTER_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (SCATTER_PLANES,))
        out = {}
        for p in planes:
            tail, dt = _SCATTER_SHAPE[p]
            shape = (n,) + tail
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CScatterOut(*[data(out.get(p)) for p in SCATTER_PLANES])
        if self.call("scatter", accel.h, data(r), n, _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def scatter_device(self, accel, n, rays_ptr, hits_ptr=None, direct_ptr=None, flags_ptr=None, reflect_ptr=None, reflect_weight_ptr=None, refract_ptr=None,
                       refract_weight_ptr=None, stream=None):
        """Enqueue the scatter of n rays (device memory, 6 doubles each) into device memory, n rows each: hits_ptr (lg_hit, 16-byte aligned),
        direct_ptr (3 f64), flags_ptr (u32), reflect_ptr and refract_ptr (6 f64), reflect_weight_ptr (3 f64), refract_weight_ptr (5 f64); each
        may be None, not all.  The pointers are integers (torch: tensor.data_ptr()) or objects with a data_ptr()."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        f = CScatterOut(*[ptr(p) for p in (hits_ptr, direct_ptr, flags_ptr, reflect_ptr, reflect_weight_ptr, refract_ptr, refract_weight_ptr)])
        rays = ptr(rays_ptr)
        if self.call("scatter_device", accel.h, _C.c_void_p(rays) if rays is not None else None, int(n), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- hit attributes (include/lasgun_hip.h, lg_hit_attributes* / lg_hit_attributes_of*): where on its primitive a hit lies, and its frame
    def _attr_out(self, n, planes, into, allowed):
        planes = tuple(planes)
        if any(p not in allowed for p in planes):
            raise ValueError("planes: any of %s" % (allowed,))
        out = {}
        for p in planes:
            tail, dt = _ATTR_SHAPE[p]
            shape = (n,) + tail
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        return out, CAttrOut(*[data(out.get(p)) for p in ATTR_PLANES]), data

    def hit_attributes(self, accel, rays, planes=ATTR_PLANES, into=None):
        """The closest hit of every ray of an (n, 6) float64 array with its surface attributes: a dict of the planes asked for (any of
        ATTR_PLANES), each indexed by the ray -- HIT_DTYPE (n,) hits = lg_intersect's record, uint32 (n,) flags = ATTR_HIT or 0 (a miss),
        float64 (n, 3) bary = a triangle hit's barycentrics (the weights of the face's three vertices; +0.0 otherwise), (n, 2) uv = the
        surface parameter (a triangle's interpolated texture coordinates, a sphere's phi / 2 pi and theta / pi, a box face's unit square),
        (n, 3) local = the hit point in the primitive's own space, (n, 6) frame = the BSDF's tangents ss, ts, (n, 6) dp = the world-space
        geometric dpdu, dpdv.  A miss's rows are +0.0.  `into`: a dict of C-contiguous arrays of those shapes, written in place.  Also
        `accel.hit_attributes(rays, planes=...)`."""
        r = self._rays(rays)
        n = r.shape[0]
        out, f, data = self._attr_out(n, planes, into, ATTR_PLANES)
        if self.call("hit_attributes", accel.h, data(r), n, _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def hit_attributes_of(self, accel, rays, hits, planes=ATTR_PLANES[1:], into=None):
        """The attributes of the primitives that records NAME, without a walk: `hits` is a HIT_DTYPE (n,) array (of intersect, of a layer of
        hit_layers, a compacted subset ...) of which kind, prim and instance are read, `rays` the (n, 6) rays they belong to.  The planes of
        hit_attributes but "hits"; flags = ATTR_HIT, 0 for a record of kind 0, ATTR_NO_HIT where the named primitive's own test rejects
        the ray, ATTR_BAD_RECORD where the record names no primitive of this accel (the rows are +0.0 for all three)."""
        r = self._rays(rays)
        n = r.shape[0]
        h = _np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if h.shape != (n,):
            raise ValueError("hits: a HIT_DTYPE array of shape (%d,)" % n)
        out, f, data = self._attr_out(n, planes, into, ATTR_PLANES[1:])
        if self.call("hit_attributes_of", accel.h, data(r), data(h), n, _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    # ---- closest points (include/lasgun_hip.h, lg_closest_points*): the nearest surface point of the scene for each of a batch of points
    def closest_points(self, accel, points, radius=float("inf"), planes=None, into=None):
        """The nearest surface point of the scene for every point of an (n, 3) float64 array (world space): a dict of the planes asked
        for (any of CLOSEST_PLANES; None: all three), each indexed by the point -- float64 (n,) distance, +inf where no surface lies
        within `radius`; float64 (n, 3) point, the closest point in world space (+0.0 for a miss); uint32 (n, 4) id = kind, prim,
        instance, material as in lg_hit (0, ~0, ~0, -1 for a miss).  The answer is the header's arithmetic over every primitive of the
        scene, bit for bit, in every traversal mode; exact ties go to the smallest (instance, kind, prim).  A point inside a sphere or
        a box gets the distance to its surface; a point with a non-finite coordinate the miss record.  A scene that holds a sphere
        under a non-uniform scale is refused (scene_closest_gate).  `into`: a dict of C-contiguous arrays of those shapes, written in
        place.  Also `accel.closest_points(points, radius=..., planes=...)`."""
        q = _np.ascontiguousarray(points, dtype=_np.float64)
        if q.ndim != 2 or q.shape[1] != 3:
            raise ValueError("points: an (n, 3) float64 array")
        n = q.shape[0]
        planes = CLOSEST_PLANES if planes is None else tuple(planes)
        if any(p not in CLOSEST_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (CLOSEST_PLANES,))
        out = {}
        for p in planes:
            tail, dt = _CLOSEST_SHAPE[p]
            shape = (n,) + tail
            if into is not None and p not in into:
                raise ValueError("into: no array for the plane %r that is asked for" % (p,))
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CClosestOut(*[data(out.get(p)) for p in CLOSEST_PLANES])
        if self.call("closest_points", accel.h, data(q), n, float(radius), _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def closest_points_device(self, accel, n, points_ptr, radius=float("inf"), distance_ptr=None, point_ptr=None, id_ptr=None, stream=None):
        """Enqueue closest_points of n points (device memory, 3 doubles each) into device memory, n rows each: distance_ptr (f64),
        point_ptr (3 f64), id_ptr (4 u32, 16-byte aligned); each may be None, not all.  The pointers are integers (torch:
        tensor.data_ptr()) or objects with a data_ptr().  An accel's first call also builds the query's own tables."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        f = CClosestOut(*[ptr(p) for p in (distance_ptr, point_ptr, id_ptr)])
        pts = ptr(points_ptr)
        if self.call("closest_points_device", accel.h, _C.c_void_p(pts) if pts is not None else None, int(n), float(radius), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def scene_closest_gate(self, scene):
        """closest_points' gate for a scene, without a device: (verdict, shrink) -- verdict -1 where every accel that holds a sphere sits
        under a similarity (uniform scale, rotations, translations), otherwise the first instance that does not, which closest_points
        names when it refuses the scene; shrink: float64 (instances,), one entry for EVERY instance of the scene: a proven lower bound of
        the smallest singular value of each accel's local -> world linear part, 0 where nothing is proven (include/lasgun_hip.h,
        lg_scene_closest_gate)."""
        cap = 4096
        while True:  # the C entry point writes min(cap, instances) entries and does not say how many there are: grow until one stays unwritten
            shrink = _np.full(cap, _np.nan, dtype=_np.float64)
            v = self.call("scene_closest_gate", scene.h, shrink.ctypes.data_as(_C.POINTER(_C.c_double)), cap)
            if v < -1:
                raise LasgunError(self.last_error())
            if _np.isnan(shrink[-1]):
                return int(v), shrink[~_np.isnan(shrink)].copy()
            cap *= 8

    CLOSEST_MAX_DEPTH = 64  # LG_CLOSEST_MAX_DEPTH

    def scene_closest_depth(self, scene):
        """The entries of the kernel's per-lane stack that closest_points needs for a scene, without a device: up to 32 fit the default
        64 KiB of dynamic LDS, up to CLOSEST_MAX_DEPTH the 128 KiB the call raises the kernel's limit to; a scene that needs more is
        refused (include/lasgun_hip.h, lg_scene_closest_depth)."""
        v = self.call("scene_closest_depth", scene.h)
        if v < 0:
            raise LasgunError(self.last_error())
        return int(v)

    # ---- proximity queries (include/lasgun_hip.h, lg_nearest*): the k nearest primitives of each point under a radius of its own
    def nearest(self, accel, points, radii=None, radius=float("inf"), k=1, planes=None, into=None):
        """The k nearest primitives of the scene for every point of an (n, 3) float64 array (world space), each point under its own
        radius: `radii` (an (n,) float64 array; a NaN or negative entry makes that point a miss) or, with radii None, the shared
        `radius`.  A dict of the planes asked for (any of NEAREST_PLANES; None: all five): uint8 (n,) touch, 1 where any primitive lies
        within the radius; uint32 (n,) count, how many do -- all of them, not capped at k; and slot-major float64 (k, n) distance,
        float64 (k, n, 3) point, uint32 (k, n, 4) id: slot j is the j-th candidate in ascending (squared distance, key = instance, kind,
        prim) order, an empty slot the miss row (+inf, +0.0, (0, ~0, ~0, -1)).  One candidate per primitive, closest_points' own, so slot 0
        under a shared radius is closest_points' answer byte for byte.  k is 0 .. NEAREST_MAX_K and plays a part only with a slot plane.
        What it costs follows from the planes: touch alone stops at the first contact; slot planes without count prune by the k-th best;
        count has to meet every primitive within the radius (at radius +inf: every primitive, for every point).  `into`: a dict of
        C-contiguous arrays of those shapes, written in place.  Also `accel.nearest(points, radii=..., k=...)`."""
        q = _np.ascontiguousarray(points, dtype=_np.float64)
        if q.ndim != 2 or q.shape[1] != 3:
            raise ValueError("points: an (n, 3) float64 array")
        n = q.shape[0]
        r = None
        if radii is not None:
            r = _np.ascontiguousarray(radii, dtype=_np.float64)
            if r.shape != (n,):
                raise ValueError("radii: an (n,) float64 array, one radius per point")
        planes = NEAREST_PLANES if planes is None else tuple(planes)
        if any(p not in NEAREST_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (NEAREST_PLANES,))
        k = int(k)
        if not 0 <= k <= NEAREST_MAX_K:
            raise ValueError("k: 0 .. %d" % NEAREST_MAX_K)
        out = {}
        for p in planes:
            tail, dt = _NEAREST_SHAPE[p]
            shape = ((k, n) if p in NEAREST_SLOT_PLANES else (n,)) + tail
            if into is not None and p not in into:
                raise ValueError("into: no array for the plane %r that is asked for" % (p,))
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        if k == 0 and n and any(p in NEAREST_SLOT_PLANES for p in planes):
            raise ValueError("k: 0 with a slot plane (distance, point, id) asked for")
        f = CNearestOut(*[data(out.get(p)) for p in NEAREST_PLANES])
        if self.call("nearest", accel.h, data(q), data(r), n, float(radius), k, _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def nearest_device(self, accel, n, points_ptr, radii_ptr=None, radius=float("inf"), k=1, touch_ptr=None, count_ptr=None, distance_ptr=None, point_ptr=None, id_ptr=None,
                       stream=None):
        """Enqueue nearest of n points (device memory, 3 doubles each; radii_ptr: n doubles or None for the shared radius) into device
        memory: touch_ptr (n u8), count_ptr (n u32), and slot-major distance_ptr (k x n f64), point_ptr (k x n x 3 f64), id_ptr (k x n x
        4 u32, 16-byte aligned); each may be None, not all.  The pointers are integers (torch: tensor.data_ptr()) or objects with a
        data_ptr().  An accel's first call also builds the query's own tables."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        void = lambda p: _C.c_void_p(p) if p is not None else None  # noqa: E731
        f = CNearestOut(*[ptr(p) for p in (touch_ptr, count_ptr, distance_ptr, point_ptr, id_ptr)])
        if self.call("nearest_device", accel.h, void(ptr(points_ptr)), void(ptr(radii_ptr)), int(n), float(radius), int(k), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def scene_nearest_lds(self, scene, k):
        """The dynamic LDS a workgroup of nearest needs for a scene and k, without a device: 256 * (8 * scene_closest_depth + 20 * k)
        bytes; a call is refused exactly where this exceeds 160 KiB (include/lasgun_hip.h, lg_scene_nearest_lds)."""
        v = self.call("scene_nearest_lds", scene.h, int(k))
        if v == 0:
            raise LasgunError(self.last_error())
        return int(v)

    def touching(self, accel, centres, radii):
        """A CONVENIENCE of this wrapper over nearest's touch plane: for spheres (centres (n, 3), radii (n,) or one number) a bool (n,)
        array, True where the scene's SURFACE comes within the sphere's radius of its centre -- the collision test of a sphere set.  A
        sphere wholly inside a solid, farther from its surface than its radius, does not touch it; a NaN or negative radius never
        touches.  The walk of a sphere ends at its first contact."""
        q = _np.ascontiguousarray(centres, dtype=_np.float64)
        r = _np.ascontiguousarray(_np.broadcast_to(_np.asarray(radii, dtype=_np.float64), q.shape[:1]))
        return self.nearest(accel, q, radii=r, k=0, planes=("touch",))["touch"].astype(bool)

    # ---- segment proximity (include/lasgun_hip.h, lg_closest_segments*): capsules and swept spheres against the scene
    def closest_segments(self, accel, segments, radii=None, radius=float("inf"), planes=None, into=None):
        """The nearest surface point of the scene to every segment of an (n, 6) float64 array (world space: p0, then p1), each segment
        under its own radius: `radii` (an (n,) float64 array; a NaN or negative entry makes that segment a miss) or, with radii None,
        the shared `radius`.  A dict of the planes asked for (any of SEGMENT_PLANES; None: all five): uint8 (n,) touch, 1 where the
        scene's surface comes within the radius of the segment; float64 (n,) distance (+inf: a miss); float64 (n,) param, s in [0, 1]:
        the segment's own closest point is p0 + (p1 - p0) * s; float64 (n, 3) point, ON THE SURFACE; uint32 (n, 4) id = kind, prim,
        instance, material (a miss: 0, ~0, ~0, -1).  A segment with p0 == p1 answers as nearest(k=1) does for that point.  touch alone
        stops at the first contact.  `into`: a dict of C-contiguous arrays of those shapes, written in place.  Also
        `accel.closest_segments(segments, radii=...)`."""
        q = _np.ascontiguousarray(segments, dtype=_np.float64)
        if q.ndim != 2 or q.shape[1] != 6:
            raise ValueError("segments: an (n, 6) float64 array: p0, then p1")
        n = q.shape[0]
        r = None
        if radii is not None:
            r = _np.ascontiguousarray(radii, dtype=_np.float64)
            if r.shape != (n,):
                raise ValueError("radii: an (n,) float64 array, one radius per segment")
        planes = SEGMENT_PLANES if planes is None else tuple(planes)
        if any(p not in SEGMENT_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (SEGMENT_PLANES,))
        out = {}
        for p in planes:
            tail, dt = _SEGMENT_SHAPE[p]
            shape = (n,) + tail
            if into is not None and p not in into:
                raise ValueError("into: no array for the plane %r that is asked for" % (p,))
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CSegmentsOut(*[data(out.get(p)) for p in SEGMENT_PLANES])
        if self.call("closest_segments", accel.h, data(q), data(r), n, float(radius), _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def closest_segments_device(self, accel, n, segments_ptr, radii_ptr=None, radius=float("inf"), touch_ptr=None, distance_ptr=None, param_ptr=None, point_ptr=None,
                                id_ptr=None, stream=None):
        """Enqueue closest_segments of n segments (device memory, 6 doubles each; radii_ptr: n doubles or None for the shared radius) into
        device memory: touch_ptr (n u8), distance_ptr and param_ptr (n f64), point_ptr (n x 3 f64), id_ptr (n x 4 u32, 16-byte aligned);
        each may be None, not all.  The pointers are integers (torch: tensor.data_ptr()) or objects with a data_ptr().  An accel's first
        call also builds the query's own tables."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        void = lambda p: _C.c_void_p(p) if p is not None else None  # noqa: E731
        f = CSegmentsOut(*[ptr(p) for p in (touch_ptr, distance_ptr, param_ptr, point_ptr, id_ptr)])
        if self.call("closest_segments_device", accel.h, void(ptr(segments_ptr)), void(ptr(radii_ptr)), int(n), float(radius), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def capsules_touching(self, accel, p0, p1, radii):
        """A CONVENIENCE of this wrapper over closest_segments' touch plane: for capsules (axes p0 .. p1, each (n, 3); radii (n,) or one
        number) a bool (n,) array, True where the scene's SURFACE comes within the capsule's radius of its axis -- a robot's links
        against the world.  A capsule wholly inside a solid, farther from its surface than its radius, does not touch it; a NaN or
        negative radius never touches.  The walk of a capsule ends at its first contact."""
        a, b = _np.ascontiguousarray(p0, dtype=_np.float64), _np.ascontiguousarray(p1, dtype=_np.float64)
        if a.ndim != 2 or a.shape[1] != 3 or b.shape != a.shape:
            raise ValueError("p0, p1: two (n, 3) float64 arrays")
        r = _np.ascontiguousarray(_np.broadcast_to(_np.asarray(radii, dtype=_np.float64), a.shape[:1]))
        return self.closest_segments(accel, _np.concatenate([a, b], axis=1), radii=r, planes=("touch",))["touch"].astype(bool)

    def sweep_touching(self, accel, centres_from, centres_to, radii):
        """capsules_touching under the swept-sphere reading: did a sphere of radius radii[i] touch the scene's surface anywhere on its
        straight way from centres_from[i] to centres_to[i] -- the step check of continuous collision detection.  No time of impact."""
        return self.capsules_touching(accel, centres_from, centres_to, radii)

    def signed_distance(self, accel, points, max_layers=32):
        """A CONVENTION of this wrapper over closest_points and hit_layers, for scenes made of CLOSED solids only (spheres, boxes,
        watertight meshes that do not intersect one another's surfaces at the point): closest_points' distance, negated where the ray
        from the point along +x crosses an odd number of surfaces (hit_layers' count), and NaN where that count reached max_layers (the
        parity is then unknown) or the point is not finite.  An open mesh, a point exactly on a surface or a +x ray that grazes an edge
        gives a parity that means nothing; the magnitude is closest_points' whatever the sign."""
        q = _np.ascontiguousarray(points, dtype=_np.float64)
        d = self.closest_points(accel, q, planes=("distance",))["distance"]
        rays = _np.concatenate([q, _np.broadcast_to(_np.array([1.0, 0.0, 0.0]), q.shape)], axis=1)
        finite = _np.isfinite(q).all(axis=1)
        rays[~finite, :3] = 0.0
        count = self.hit_layers(accel, rays, int(max_layers), ("count",))["count"] if len(q) else _np.zeros(0, dtype=_np.uint32)
        out = _np.where(count % 2 == 1, -d, d)
        out[(count >= int(max_layers)) | ~finite] = _np.nan
        return out

    def hit_attributes_device(self, accel, n, rays_ptr, hits_ptr=None, flags_ptr=None, bary_ptr=None, uv_ptr=None, local_ptr=None, frame_ptr=None, dp_ptr=None,
                              stream=None):
        """Enqueue hit_attributes of n rays (device memory, 6 doubles each) into device memory, n rows each: hits_ptr (lg_hit, 16-byte
        aligned), flags_ptr (u32), bary_ptr and local_ptr (3 f64), uv_ptr (2 f64), frame_ptr and dp_ptr (6 f64); each may be None, not all.
        The pointers are integers (torch: tensor.data_ptr()) or objects with a data_ptr()."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        f = CAttrOut(*[ptr(p) for p in (hits_ptr, flags_ptr, bary_ptr, uv_ptr, local_ptr, frame_ptr, dp_ptr)])
        rays = ptr(rays_ptr)
        if self.call("hit_attributes_device", accel.h, _C.c_void_p(rays) if rays is not None else None, int(n), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def hit_attributes_of_device(self, accel, n, rays_ptr, records_ptr, flags_ptr=None, bary_ptr=None, uv_ptr=None, local_ptr=None, frame_ptr=None, dp_ptr=None,
                                 stream=None):
        """Enqueue hit_attributes_of of n rays and n records (device memory: 6 doubles and one 16-byte aligned lg_hit each) into device
        memory; the planes as for hit_attributes_device, without hits."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        f = CAttrOut(None, *[ptr(p) for p in (flags_ptr, bary_ptr, uv_ptr, local_ptr, frame_ptr, dp_ptr)])
        rays, recs = ptr(rays_ptr), ptr(records_ptr)
        if self.call("hit_attributes_of_device", accel.h, _C.c_void_p(rays) if rays is not None else None, _C.c_void_p(recs) if recs is not None else None, int(n),
                     _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- lit scatter (include/lasgun_hip.h, lg_scatter_lit*): surface scatter under lights that come with the call
    @staticmethod
    def _light_set(lights, n, ambient, ptr=None):
        """(CLightSet, K, per_ray, what keeps the table alive): lights (K,) are shared, (n, K) are per ray; `ptr`: the table's address where
        it is not the array's own (a per-ray table on the device)."""
        amb = (_C.c_double * 3)(*[float(x) for x in ambient])
        if ptr is not None:
            count, per_ray = lights
            return CLightSet(int(ptr) or None, int(count), int(per_ray), amb), int(count), int(per_ray), None
        tab = lights_array(lights)
        if tab.ndim == 2 and tab.shape[0] != n:
            raise ValueError("lights: (K,) shared by every ray, or (n, K) with a row per ray")
        if tab.ndim not in (1, 2):
            raise ValueError("lights: (K,) shared by every ray, or (n, K) with a row per ray")
        count = tab.shape[-1]
        return CLightSet(tab.ctypes.data if tab.size else None, count, 1 if tab.ndim == 2 else 0, amb), count, tab.ndim == 2, tab

    def scatter_lit(self, accel, rays, lights, ambient=(0.0, 0.0, 0.0), planes=LIT_PLANES, into=None):
        """scatter() under lights that come with the call, for every ray of an (n, 6) float64 array.  `lights`: a sequence of Light()s or a
        lights_array of shape (K,), shared by every ray, or of shape (n, K), ray i's own lights in row i; K is 0 .. MAX_CALL_LIGHTS, and the
        scene's own lights and ambient colour play no part.  A dict of the planes asked for (any of LIT_PLANES): the seven of scatter() --
        `direct` is the sum of the visible lights' terms in order, then the ambient term under `ambient` -- and float64 (n, K, 3) terms =
        every light's own term (+0.0 where it is not added), uint32 (n, ceil(K / 32)) visible = bit k & 31 of word k >> 5 is set iff light k
        is visible from the hit.  `into`: a dict of C-contiguous arrays of those shapes, written in place.  Also `accel.scatter_lit(...)`."""
        r = self._rays(rays)
        n = r.shape[0]
        planes = tuple(planes)
        if any(p not in LIT_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (LIT_PLANES,))
        ls, count, _, keep = self._light_set(lights, n, ambient)
        shapes = dict(_SCATTER_SHAPE, terms=((count, 3), _np.float64), visible=(((count + 31) // 32,), _np.uint32))
        out = {}
        for p in planes:
            tail, dt = shapes[p]
            shape = (n,) + tail
            arr = into[p] if into is not None else _np.zeros(shape, dtype=dt)
            if arr.dtype != dt or arr.shape != shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, shape))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CLitOut(CScatterOut(*[data(out.get(p)) for p in SCATTER_PLANES]), data(out.get("terms")), data(out.get("visible")))
        if self.call("scatter_lit", accel.h, data(r), n, _C.addressof(ls), _C.addressof(f)):
            raise LasgunError(self.last_error())
        del keep
        return out

    def scatter_lit_device(self, accel, n, rays_ptr, lights=None, ambient=(0.0, 0.0, 0.0), per_ray_lights_ptr=None, count=None, hits_ptr=None, direct_ptr=None,
                           flags_ptr=None, reflect_ptr=None, reflect_weight_ptr=None, refract_ptr=None, refract_weight_ptr=None, terms_ptr=None, visible_ptr=None,
                           stream=None):
        """Enqueue scatter_lit of n rays (device memory, 6 doubles each) into device memory.  Shared lights: `lights`, a HOST table (a sequence
        of Light()s or a lights_array of shape (K,)), staged by the call -- it may be dropped on return.  Per-ray lights:
        `per_ray_lights_ptr`, DEVICE memory of n x count records of 72 bytes, ray i's at row i, and `count`.  The planes as for
        scatter_device, and terms_ptr (n x K x 3 f64), visible_ptr (n x ceil(K / 32) u32); each may be None, not all.  The pointers are
        integers (torch: tensor.data_ptr()) or objects with a data_ptr()."""
        ptr = lambda p: None if p is None else int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)  # noqa: E731
        if per_ray_lights_ptr is not None:
            ls, _, _, keep = self._light_set((count, 1), n, ambient, ptr=ptr(per_ray_lights_ptr))
        else:
            tab = lights_array(lights if lights is not None else [])
            if tab.ndim != 1:
                raise ValueError("lights: a host table of shape (K,); per-ray lights are device memory (per_ray_lights_ptr, count)")
            ls, _, _, keep = self._light_set(tab, n, ambient)
        f = CLitOut(CScatterOut(*[ptr(p) for p in (hits_ptr, direct_ptr, flags_ptr, reflect_ptr, reflect_weight_ptr, refract_ptr, refract_weight_ptr)]),
                    ptr(terms_ptr), ptr(visible_ptr))
        rays = ptr(rays_ptr)
        if self.call("scatter_lit_device", accel.h, _C.c_void_p(rays) if rays is not None else None, int(n), _C.addressof(ls), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())
        del keep

    # ---- radiance gathers (include/lasgun_hip.h, lg_radiance_gather*): li() along K shared directions from N poses, reduced per pose
    @staticmethod
    def _gather_lanes(lanes):
        return GATHER_LANES[lanes] if isinstance(lanes, str) else int(lanes)

    def radiance_gather_lanes(self, n_poses, n_dirs, lanes=0):
        """The work item a gather of these counts would use: 1 direction lanes (one pose x 64 directions a wave), 2 pose lanes (64 poses x
        one direction); -1 for a bad `lanes`.  lanes: 0 / "auto" (pose lanes iff n_poses >= n_dirs), 1 / "direction", 2 / "pose".  No device
        is touched."""
        return int(self.call("radiance_gather_lanes", int(n_poses), int(n_dirs), self._gather_lanes(lanes)))

    def radiance_gather(self, accel, origins, dirs, frames=None, weights=None, planes=("sums",), lanes=0, into=None):
        """li() along dirs[k] from origins[i], what `radiance` returns for that ray: a dict of the planes asked for (any of "radiance",
        "sums") -- float64 (n_poses, n_dirs, 3) radiance, and float64 (n_poses, n_weights, 3) sums[i, c] = the sum over k, in order from
        +0.0, of radiance[i, k] * weights[k, c] (one product, one sum a step).  weights: (n_dirs, n_weights) float64, or (n_dirs,) for one
        column; needed for "sums" alone.  frames: (n_poses, 3, 3) or (n_poses, 9) float64, row-major, d[c] = (M[c,0]*b.x + M[c,1]*b.y) +
        M[c,2]*b.z; None: the directions are used bit for bit.  The directions are not normalised.  lanes: radiance_gather_lanes' (the
        outputs do not depend on it).  `into`: a dict of C-contiguous arrays of those shapes, written in place.
        Also `accel.radiance_gather(origins, dirs, frames=None, weights=None, planes=("sums",), lanes=0)`."""
        o, b = self._points(origins, "origins"), self._points(dirs, "dirs")
        m = None
        if frames is not None:
            m = _np.ascontiguousarray(frames, dtype=_np.float64)
            if m.shape not in ((o.shape[0], 3, 3), (o.shape[0], 9)):
                raise ValueError("frames: one 3 x 3 matrix per pose")
        planes = tuple(planes)
        if any(p not in GATHER_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (GATHER_PLANES,))
        wt, n_weights = None, 0
        if weights is not None:
            wt = _np.ascontiguousarray(weights, dtype=_np.float64)
            if wt.ndim == 1:
                wt = wt.reshape(-1, 1)
            if wt.ndim != 2 or wt.shape[0] != b.shape[0]:
                raise ValueError("weights: (n_dirs, n_weights), one row per direction")
            n_weights = wt.shape[1]
        shapes = {"radiance": (o.shape[0], b.shape[0], 3), "sums": (o.shape[0], n_weights, 3)}
        out = {}
        for p in planes:
            arr = into[p] if into is not None else _np.zeros(shapes[p], dtype=_np.float64)
            if arr.dtype != _np.float64 or arr.shape != shapes[p] or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous float64 array of shape %s" % (p, shapes[p]))
            out[p] = arr
        data = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        f = CGatherOut(*[data(out.get(p)) for p in GATHER_PLANES])
        if self.call("radiance_gather", accel.h, data(o), data(m), o.shape[0], data(b), b.shape[0], data(wt), n_weights, self._gather_lanes(lanes), _C.addressof(f)):
            raise LasgunError(self.last_error())
        return out

    def radiance_gather_device(self, accel, n_poses, origins_ptr, frames_ptr, n_dirs, dirs_ptr, weights_ptr=None, n_weights=0, radiance_ptr=None, sums_ptr=None,
                               lanes=0, stream=None):
        """Enqueue the gather of n_poses poses (device memory, 3 doubles an origin; frames_ptr 9 doubles a pose or None) along n_dirs
        directions (3 doubles each) into device memory: n_poses * n_dirs * 3 doubles at radiance_ptr and / or, with n_dirs * n_weights
        doubles at weights_ptr, n_poses * n_weights * 3 doubles at sums_ptr; each output may be None, not both."""
        ptr = lambda p: _C.c_void_p(int(p)) if p is not None else None  # noqa: E731
        f = CGatherOut(*[int(p) if p is not None else None for p in (radiance_ptr, sums_ptr)])
        if self.call("radiance_gather_device", accel.h, ptr(origins_ptr), ptr(frames_ptr), int(n_poses), ptr(dirs_ptr), int(n_dirs), ptr(weights_ptr), int(n_weights),
                     self._gather_lanes(lanes), _C.addressof(f), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- feature buffers (include/lasgun_hip.h, lg_capture_features*): depth, normal, albedo, coverage and ids of the camera's primary hits
    def material_count(self, accel):
        """The number of materials of the accel's tables: indices 0 .. count-1 are valid for accel_material and name the rows of material_rgb."""
        return int(self.call("accel_material_count", accel.h))

    def default_albedo_table(self, accel):
        """(material_count, 3) float64: per material kd for matte and plastic, kr for mirror, kt for glass and (1, 1, 1) for metal -- the
        material_rgb capture_features uses when none is given.  A convention of this WRAPPER, not of the C contract (lg_capture_features
        takes whatever colours the caller passes)."""
        out = _np.ones((self.material_count(accel), 3), dtype=_np.float64)
        for i in range(out.shape[0]):
            m = self.accel_material(accel, i)
            if m["kind"] in (0, 1, 4):    # matte / plastic: kd; mirror: kr
                out[i] = m["p"][0:3]
            elif m["kind"] == 3:          # glass: kt
                out[i] = m["p"][3:6]
        return out

    def capture_features(self, accel, w, h, rect=None, planes=FEATURE_PLANES, material_rgb=None, into=None):
        """The feature buffers of the pixels rect = (x0, y0, x1, y1) (default: the whole film) of the accel's own camera view of a w x h film:
        a dict of the planes asked for (any of "depth", "normal", "albedo", "coverage", "id"), each addressed like the film -- float32
        (h, w) depth and coverage, float32 (h, w, 3) normal and albedo, uint32 (h, w, 4) id = kind, prim, instance, material of sample 0.
        Normal and albedo are means over ALL the pixel's samples (premultiplied by coverage), depth the mean over those that hit (+inf: none).
        material_rgb: (material_count, 3) float64, the colour summed per hit material; default default_albedo_table(accel).
        `into`: a dict of C-contiguous arrays of those shapes, written in place -- pixels outside rect keep their bytes; new arrays are zero there."""
        x0, y0, x1, y1 = (0, 0, w, h) if rect is None else rect
        planes = tuple(planes)
        if any(p not in FEATURE_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (FEATURE_PLANES,))
        out = {}
        for p in planes:
            shape, dt = _FEATURE_SHAPE[p]
            arr = into[p] if into is not None else _np.zeros((h, w) + shape, dtype=dt)
            if arr.dtype != dt or arr.shape != (h, w) + shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, (h, w) + shape))
            out[p] = arr
        table = None
        if "albedo" in out:
            table = _np.ascontiguousarray(self.default_albedo_table(accel) if material_rgb is None else material_rgb, dtype=_np.float64)
            if table.shape != (self.material_count(accel), 3):
                raise ValueError("material_rgb: a (material_count, 3) array")
        f = CFeatures(*[out[p].ctypes.data if p in out and out[p].size else None for p in FEATURE_PLANES])
        if self.call("capture_features", accel.h, int(w), int(h), int(x0), int(y0), int(x1), int(y1), _C.addressof(f),
                     table.ctypes.data if table is not None and table.size else None):
            raise LasgunError(self.last_error())
        return out

    def capture_features_device(self, accel, w, h, rect=None, depth_ptr=None, normal_ptr=None, albedo_ptr=None, coverage_ptr=None, id_ptr=None,
                                material_rgb_ptr=None, stream=None):
        """Enqueue the same planes into device memory: each pointer w*h elements of its plane, addressed like the film (id 16-byte aligned),
        or None; material_rgb_ptr: material_count * 3 doubles in device memory, required with albedo_ptr."""
        x0, y0, x1, y1 = (0, 0, w, h) if rect is None else rect
        f = CFeatures(*[int(p) if p is not None else None for p in (depth_ptr, normal_ptr, albedo_ptr, coverage_ptr, id_ptr)])
        if self.call("capture_features_device", accel.h, int(w), int(h), int(x0), int(y0), int(x1), int(y1), _C.addressof(f),
                     _C.c_void_p(int(material_rgb_ptr)) if material_rgb_ptr is not None else None, self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def radiance(self, accel, rays):
        """Radiance along every ray of an (n, 6) float64 array (origin, direction): (n, 3) float64 RGB, li() as the render computes it
        -- lights, shadows, ambient, specular recursion, background on a miss -- before quantisation (include/lasgun_hip.h, lg_radiance)."""
        r = self._rays(rays)
        out = _np.zeros((r.shape[0], 3), dtype=_np.float64)
        if self.call("radiance", accel.h, r.ctypes.data, r.shape[0], out.ctypes.data):
            raise LasgunError(self.last_error())
        return out

    def radiance_device(self, accel, n, rays_ptr, out_ptr, stream=None):
        """Enqueue the radiance of n rays (device memory, 6 doubles each) into 3 n doubles at out_ptr (both 8-byte aligned)."""
        if self.call("radiance_device", accel.h, _C.c_void_p(int(rays_ptr)), int(n), _C.c_void_p(int(out_ptr)), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- light groups (include/lasgun_hip.h, lg_radiance_groups*): li() of each ray split by subsets of the scene's lights
    def light_count(self, accel):
        """The scene's point lights: the mask bits a LightGroup may use (include/lasgun_hip.h, lg_accel_light_count)."""
        return int(self.call("accel_light_count", accel.h))

    @staticmethod
    def _groups(groups):
        """The groups as a C array of lg_light_group: LightGroup records or (lights, flags) pairs."""
        items = [g if isinstance(g, CLightGroup) else LightGroup(*g) for g in groups]
        return (CLightGroup * max(len(items), 1))(*items), len(items)

    def radiance_groups(self, accel, rays, groups, into=None):
        """Radiance along every ray of an (n, 6) float64 array split by light groups: (G, n, 3) float64, plane g what `radiance` returns on
        an accel rebuilt with the lights of groups[g].lights alone (bit l: light l in add order) and, without GROUP_AMBIENT in its flags,
        no ambient term -- bit for bit, from ONE chain of walks.  The background belongs to every group.  groups: LightGroup records or
        (lights, flags) pairs, at most MAX_LIGHT_GROUPS.  `into`: a C-contiguous (G, n, 3) float64 array written in place.  Also
        `accel.radiance_groups(rays, groups)`."""
        r = self._rays(rays)
        table, k = self._groups(groups)
        shape = (k, r.shape[0], 3)
        out = into if into is not None else _np.zeros(shape, dtype=_np.float64)
        if out.dtype != _np.float64 or out.shape != shape or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("into: a C-contiguous float64 array of shape %s" % (shape,))
        if self.call("radiance_groups", accel.h, r.ctypes.data, r.shape[0], _C.addressof(table), k, out.ctypes.data if out.size else None):
            raise LasgunError(self.last_error())
        return out

    def radiance_groups_device(self, accel, n, rays_ptr, groups, out_ptr, stream=None):
        """Enqueue the light groups of n rays (device memory, 6 doubles each) into G * n * 3 doubles at out_ptr, group-major (both 8-byte
        aligned).  groups: a host sequence, as for radiance_groups; it may be dropped when the call returns.  The pointers are integers
        (torch: tensor.data_ptr()) or objects with a data_ptr()."""
        ptr = lambda p: None if p is None else _C.c_void_p(int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p))  # noqa: E731
        table, k = self._groups(groups)
        if self.call("radiance_groups_device", accel.h, ptr(rays_ptr), int(n), _C.addressof(table), k, ptr(out_ptr), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- ray films (include/lasgun_hip.h, lg_capture_rays* / lg_lens_rays*): a film from the caller's rays
    def capture_rays(self, accel, rays, w, h, samples=1, offsets=None, rgba=True, rgb=False, into=None):
        """The film of (slots * samples, 6) float64 rays, slot-major: slot g's rays are summed in order, scaled by 1 / samples and written at
        film offset offsets[g] (or g).  Returns the (h, w, 4) uint8 film and / or the (h, w, 3) float64 radiance asked for (both: a pair).
        `into` = (film array or None, rgb array or None): C-contiguous buffers written in place -- pixels no slot names keep their bytes."""
        r = self._rays(rays)
        samples = int(samples)
        if samples <= 0 or r.shape[0] % samples:
            raise ValueError("rays: slots * samples of them")
        slots = r.shape[0] // samples
        off = None if offsets is None else _np.ascontiguousarray(offsets, dtype=_np.uint64)
        if off is not None and off.shape != (slots,):
            raise ValueError("offsets: one per pixel slot")
        out_a, out_d = into if into is not None else (_np.zeros((h, w, 4), dtype=_np.uint8) if rgba else None,
                                                      _np.zeros((h, w, 3), dtype=_np.float64) if rgb else None)
        film = self.Film.new_with_output(w, h, out_a) if out_a is not None else None
        if self.call("capture_rays", accel.h, r.ctypes.data, slots, samples, off.ctypes.data if off is not None else None, film.h if film else None,
                     out_d.ctypes.data if out_d is not None else None, int(w), int(h)):
            raise LasgunError(self.last_error())
        if out_a is not None and out_d is not None:
            return out_a, out_d
        return out_a if out_a is not None else out_d

    def capture_rays_device(self, accel, slots, rays_ptr, w, h, samples=1, offsets_ptr=None, rgba_ptr=None, rgb_ptr=None, stream=None):
        """Enqueue the film of slots * samples rays (device memory) into w*h RGBA8 words at rgba_ptr and / or w*h*3 doubles at rgb_ptr;
        offsets_ptr: slots uint64 film offsets in device memory, or None."""
        ptr = lambda p: _C.c_void_p(int(p)) if p is not None else None  # noqa: E731
        if self.call("capture_rays_device", accel.h, ptr(rays_ptr), int(slots), int(samples), ptr(offsets_ptr), int(w), int(h), ptr(rgba_ptr), ptr(rgb_ptr),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def lens_rays(self, lens, w, h, samples_root=1, offsets=None):
        """The rays of a Lens over a w x h film (or over the pixel slots `offsets` names): (slots * samples_root^2, 6) float64, slot-major."""
        off = None if offsets is None else _np.ascontiguousarray(offsets, dtype=_np.uint64)
        slots = w * h if off is None else off.shape[0]
        out = _np.zeros((slots * samples_root * samples_root, 6), dtype=_np.float64)
        if self.call("lens_rays", _C.addressof(lens), int(w), int(h), int(samples_root), off.ctypes.data if off is not None else None, slots,
                     out.ctypes.data if out.size else None):
            raise LasgunError(self.last_error())
        return out

    def lens_rays_device(self, device, lens, w, h, samples_root, slots, rays_ptr, offsets_ptr=None, stream=0):
        """Enqueue the same rays into device memory of `device` on `stream` (0 = HIP's default stream)."""
        if self.call("lens_rays_device", int(device), _C.addressof(lens), int(w), int(h), int(samples_root),
                     _C.c_void_p(int(offsets_ptr)) if offsets_ptr is not None else None, int(slots), _C.c_void_p(int(rays_ptr)), _C.c_void_p(int(stream))):
            raise LasgunError(self.last_error())

    def capture_lens(self, accel, lens, w, h, samples_root=1, tile_order=True):
        """A Lens's picture of the accel's scene: its rays generated on the device into a torch buffer (8 x 8-tile order by default: the order
        in which a wave's rays are neighbours) and rendered by capture_rays_device.  Returns the (h, w, 4) uint8 film."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        slots, S = w * h, samples_root * samples_root
        offs = torch.from_numpy(tile_order_offsets(w, h).view(_np.int64)).to(dev) if tile_order else None
        rays = torch.empty(slots * S * 6, dtype=torch.float64, device=dev)
        film = torch.zeros(slots * 4, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        optr = offs.data_ptr() if offs is not None else None
        self.lens_rays_device(dev.index, lens, w, h, samples_root, slots, rays.data_ptr(), optr, stream=stream)
        self.capture_rays_device(accel, slots, rays.data_ptr(), w, h, samples=S, offsets_ptr=optr, rgba_ptr=film.data_ptr(), stream=stream)
        torch.cuda.current_stream().synchronize()
        return film.cpu().numpy().reshape(h, w, 4)

    def set_query_order(self, accel, order):
        """The order a query's rays are walked in: 0 as given (default), 1 sorted on the device by a coherence key -- for rays that arrive
        in no particular order; the sort is part of every call's time (include/lasgun_hip.h, lg_accel_set_query_order).  Same bytes either way."""
        if self.call("accel_set_query_order", accel.h, int(order)):
            raise LasgunError(self.last_error())

    def get_query_order(self, accel):
        return int(self.call("accel_get_query_order", accel.h))

    def query_order(self, accel, rays):
        """The order set_query_order(accel, 1) walks an (n, 6) float64 array of rays in: (perm, keys), two uint32 arrays -- perm[s] the ray
        walked in slot s, keys[i] ray i's key; perm is the stable ascending sort of keys."""
        r = self._rays(rays)
        perm = _np.zeros(r.shape[0], dtype=_np.uint32)
        keys = _np.zeros(r.shape[0], dtype=_np.uint32)
        if self.call("query_order", accel.h, r.ctypes.data, r.shape[0], perm.ctypes.data, keys.ctypes.data):
            raise LasgunError(self.last_error())
        return perm, keys

    def query_order_device(self, accel, n, rays_ptr, perm_ptr, keys_ptr=None, stream=None):
        """Enqueue the order of n rays (device memory, 6 doubles each) into n uint32 at perm_ptr and, unless None, their keys at keys_ptr."""
        keys = _C.c_void_p(int(keys_ptr)) if keys_ptr is not None else None
        if self.call("query_order_device", accel.h, _C.c_void_p(int(rays_ptr)), int(n), _C.c_void_p(int(perm_ptr)), keys, self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def camera_rays(self, accel, w, h, x0=0, y0=0, x1=None, y1=None):
        """The rays a capture traces for the pixels [x0,x1) x [y0,y1) of a w x h film: ((y1-y0) * (x1-x0) * samples, 6) float64,
        row-major pixels, each pixel's samples in camera.rs order."""
        x1 = w if x1 is None else x1
        y1 = h if y1 is None else y1
        n = max(x1 - x0, 0) * max(y1 - y0, 0) * self.camera_samples(accel)
        out = _np.zeros((n, 6), dtype=_np.float64)
        if self.call("camera_rays", accel.h, w, h, x0, y0, x1, y1, out.ctypes.data if n else None):
            raise LasgunError(self.last_error())
        return out

    def camera_rays_device(self, accel, w, h, x0, y0, x1, y1, rays_ptr, stream=None):
        if self.call("camera_rays_device", accel.h, w, h, x0, y0, x1, y1, _C.c_void_p(int(rays_ptr)), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- views (include/lasgun_hip.h, lg_view_look_at .. lg_capture_views_device): one accel from K cameras into K films in one call
    def view_look_at(self, origin, look, up, fov=None, scale=None, supersampling=0):
        """The View of a perspective camera of `fov` degrees (or an orthographic one of `scale`) at `origin` looking at `look`: what a scene's
        own camera holds after set_perspective_camera(fov) / set_orthographic_camera(scale), look_at and set_supersampling, byte for byte."""
        if (fov is None) == (scale is None):
            raise ValueError("view_look_at: fov (perspective) or scale (orthographic), one of them")
        from ._capi import _v3
        v = CView()
        if self.call("view_look_at", _C.addressof(v), 1 if fov is not None else 0, float(fov if fov is not None else scale), _v3(origin), _v3(look), _v3(up),
                     int(supersampling)):
            raise LasgunError(self.last_error())
        return v

    def scene_view(self, scene):
        """The scene's own camera as a View (no device is touched)."""
        v = CView()
        if self.call("scene_view", scene.h, _C.addressof(v)):
            raise LasgunError(self.last_error())
        return v

    def accel_view(self, accel):
        """The camera of the scene the accel was built from, as a View: capture_views(accel, [accel_view(accel)], w, h) is capture's film."""
        v = CView()
        if self.call("accel_view", accel.h, _C.addressof(v)):
            raise LasgunError(self.last_error())
        return v

    def view_rays(self, accel, view, w, h, x0=0, y0=0, x1=None, y1=None):
        """camera_rays with `view` in the camera's place: ((y1-y0) * (x1-x0) * samples_root^2, 6) float64, the same pixel and sample order."""
        x1 = w if x1 is None else x1
        y1 = h if y1 is None else y1
        n = max(x1 - x0, 0) * max(y1 - y0, 0) * int(view.samples_root) ** 2
        out = _np.zeros((n, 6), dtype=_np.float64)
        if self.call("view_rays", accel.h, _C.addressof(view), w, h, x0, y0, x1, y1, out.ctypes.data if n else None):
            raise LasgunError(self.last_error())
        return out

    def view_rays_device(self, accel, view, w, h, x0, y0, x1, y1, rays_ptr, stream=None):
        if self.call("view_rays_device", accel.h, _C.addressof(view), w, h, x0, y0, x1, y1, _C.c_void_p(int(rays_ptr)), self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def capture_views(self, accel, views, w, h, rgba=True, rgb=False, into=None):
        """The accel's scene from K Views into K w x h films in ONE call: the (K, h, w, 4) uint8 films and / or the (K, h, w, 3) float64
        radiance before quantisation (both: a pair).  The views share samples_root.  `into` = (films array or None, rgb array or None):
        C-contiguous buffers of those shapes, written in place."""
        tab = _views(views)
        k = len(tab)
        out_a, out_d = into if into is not None else (_np.zeros((k, h, w, 4), dtype=_np.uint8) if rgba else None,
                                                      _np.zeros((k, h, w, 3), dtype=_np.float64) if rgb else None)
        for o, dt, c in ((out_a, _np.uint8, 4), (out_d, _np.float64, 3)):
            if o is not None and (o.dtype != dt or o.size != k * h * w * c or not o.flags["C_CONTIGUOUS"]):
                raise ValueError("into: C-contiguous (K, h, w, 4) uint8 / (K, h, w, 3) float64")
        if self.call("capture_views", accel.h, _C.addressof(tab) if k else None, k, int(w), int(h), out_a.ctypes.data if out_a is not None else None,
                     out_d.ctypes.data if out_d is not None else None):
            raise LasgunError(self.last_error())
        if out_a is not None and out_d is not None:
            return out_a, out_d
        return out_a if out_a is not None else out_d

    def capture_views_device(self, accel, views, w, h, rgba_ptr=None, rgb_ptr=None, stream=None):
        """Enqueue the same K films into K*w*h RGBA8 words at rgba_ptr and / or K*w*h*3 doubles at rgb_ptr (device memory); `views` stays a
        host sequence of View and is copied before the call returns."""
        tab = _views(views)
        ptr = lambda p: _C.c_void_p(int(p)) if p is not None else None  # noqa: E731
        if self.call("capture_views_device", accel.h, _C.addressof(tab) if len(tab) else None, len(tab), int(w), int(h), ptr(rgba_ptr), ptr(rgb_ptr),
                     self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    # ---- view features (include/lasgun_hip.h, lg_capture_view_features*): the feature planes and the hit point for K views in one call
    def capture_view_features(self, accel, views, w, h, planes=VIEW_FEATURE_PLANES, material_rgb=None, into=None):
        """The feature planes of the accel's scene seen from K Views, K whole w x h films in ONE call: a dict of the planes asked for (any of
        "depth", "normal", "albedo", "coverage", "id", "point"), plane p of view v at out[p][v] -- float32 (K, h, w) depth and coverage,
        float32 (K, h, w, 3) normal, albedo and point, uint32 (K, h, w, 4) id = kind, prim, instance, material of sample 0.  Normal and
        albedo are means over ALL the pixel's samples (premultiplied by coverage); depth and the world-space point are means over those
        that hit (+inf and (0, 0, 0): none).  The views share samples_root.
        material_rgb: (material_count, 3) float64, the colour summed per hit material; default default_albedo_table(accel).
        `into`: a dict of C-contiguous arrays of those shapes, written in place."""
        tab = _views(views)
        k = len(tab)
        planes = tuple(planes)
        if any(p not in VIEW_FEATURE_PLANES for p in planes):
            raise ValueError("planes: any of %s" % (VIEW_FEATURE_PLANES,))
        out = {}
        for p in planes:
            shape, dt = _VIEW_FEATURE_SHAPE[p]
            arr = into[p] if into is not None else _np.zeros((k, h, w) + shape, dtype=dt)
            if arr.dtype != dt or arr.shape != (k, h, w) + shape or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("into[%r]: a C-contiguous %s array of shape %s" % (p, _np.dtype(dt).name, (k, h, w) + shape))
            out[p] = arr
        table = None
        if "albedo" in out:
            table = _np.ascontiguousarray(self.default_albedo_table(accel) if material_rgb is None else material_rgb, dtype=_np.float64)
            if table.shape != (self.material_count(accel), 3):
                raise ValueError("material_rgb: a (material_count, 3) array")
        f = CViewFeatures(*[out[p].ctypes.data if p in out and out[p].size else None for p in VIEW_FEATURE_PLANES])
        if self.call("capture_view_features", accel.h, _C.addressof(tab) if k else None, k, int(w), int(h), _C.addressof(f),
                     table.ctypes.data if table is not None and table.size else None):
            raise LasgunError(self.last_error())
        return out

    def capture_view_features_device(self, accel, views, w, h, depth_ptr=None, normal_ptr=None, albedo_ptr=None, coverage_ptr=None, id_ptr=None,
                                     point_ptr=None, material_rgb_ptr=None, stream=None):
        """Enqueue the same planes into device memory: each pointer K*w*h elements of its plane, film after film (id 16-byte aligned), or
        None; material_rgb_ptr: material_count * 3 doubles in device memory, required with albedo_ptr.  `views` stays a host sequence of
        View and is copied before the call returns."""
        tab = _views(views)
        f = CViewFeatures(*[int(p) if p is not None else None for p in (depth_ptr, normal_ptr, albedo_ptr, coverage_ptr, id_ptr, point_ptr)])
        if self.call("capture_view_features_device", accel.h, _C.addressof(tab) if len(tab) else None, len(tab), int(w), int(h), _C.addressof(f),
                     _C.c_void_p(int(material_rgb_ptr)) if material_rgb_ptr is not None else None, self._stream(accel, stream)):
            raise LasgunError(self.last_error())

    def camera_samples(self, accel):
        """Rays per pixel of lg_camera_rays (the camera's supersamples)."""
        return int(self.call("camera_samples", accel.h))

    def accel_material(self, accel, index):
        """The material behind lg_hit::material: a Material as the caller passed it ({"kind", "p"} of the POD)."""
        from ._capi import CMaterial
        m = CMaterial()
        if self.call("accel_material", accel.h, int(index), _C.byref(m)):
            raise LasgunError(self.last_error())
        return {"kind": int(m.kind), "p": tuple(m.p)}

    def accel_instance(self, accel, instance):
        """(parent, obj_ref) of the accel behind lg_hit::instance: parent -1 for the root, obj_ref -1 for a group."""
        parent, obj = _C.c_int32(), _C.c_int64()
        if self.call("accel_instance", accel.h, int(instance), _C.byref(parent), _C.byref(obj)):
            raise LasgunError(self.last_error())
        return int(parent.value), int(obj.value)

    def accel_info(self, accel):
        out = (_C.c_uint64 * 8)()
        self.call("accel_info", accel.h, out)
        keys = ("nodes", "primrefs", "spheres", "cuboids", "triangles", "accels", "max_stack", "device_bytes")
        return dict(zip(keys, [int(v) for v in out]))


def device_source_sha16():
    """First 16 hex digits of the SHA-256 over the device sources (csrc/*.h, csrc/k_*.hip, in name order): the provenance
    stamp of profiler counters -- bench.py reports a committed PMC figure only while the sources it was collected on are unchanged."""
    import glob
    import hashlib
    src = _os.path.join(_HERE, "csrc")
    h = hashlib.sha256()
    for path in sorted(glob.glob(_os.path.join(src, "*.h")) + glob.glob(_os.path.join(src, "k_*.hip"))):
        if _os.path.basename(path) in ("host.h", "internal.h", "tune.h", "choice.h"):  # host-side headers: no kernel is compiled from them
            continue
        h.update(_os.path.basename(path).encode() + b"\0")
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so and load it by
    file name; liblasgun_hip.so asks for the soname libamdhip64.so.7.  If this library is loaded first it
    binds to the system runtime and a later `import torch` brings a SECOND runtime into the process, which
    then finds no GPU.  Loading torch's copy first (when a torch wheel with a bundled runtime is installed;
    torch itself is not imported) makes both resolve to the same object, whichever is imported first."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    bundled = _os.path.join(_os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if _os.path.exists(bundled):
        _C.CDLL(bundled, mode=_C.RTLD_GLOBAL)


def sphere_directions(k, length=1.0):
    """(k, 3) float64: a Fibonacci lattice of k directions spread evenly over the sphere, each of length `length` (the reach of
    open_directions).  A convention of this WRAPPER, not of the C contract."""
    i = _np.arange(int(k), dtype=_np.float64) + 0.5
    z = 1.0 - 2.0 * i / max(int(k), 1)
    phi = i * (_np.pi * (3.0 - _np.sqrt(5.0)))
    d = _np.stack([_np.sqrt(1.0 - z * z) * _np.cos(phi), _np.sqrt(1.0 - z * z) * _np.sin(phi), z], axis=1)
    return _np.ascontiguousarray(d * (float(length) / _np.linalg.norm(d, axis=1))[:, None])


def spinning_lidar_beams(rings, azimuths, elev_lo_deg, elev_hi_deg):
    """(rings * azimuths, 3) float64 unit beams of a spinning lidar in the sensor's frame (x forward, y left, z up): `rings` elevations
    spread evenly over [elev_lo_deg, elev_hi_deg] (one ring: their mean), `azimuths` steps of a full turn.  RING-MAJOR -- beam
    r * azimuths + a -- so that 64 consecutive beams are neighbours: a stretch of one ring.  A convention of this WRAPPER, not of the C
    contract."""
    rings, azimuths = int(rings), int(azimuths)
    elev = _np.deg2rad(_np.linspace(float(elev_lo_deg), float(elev_hi_deg), rings) if rings > 1 else _np.array([0.5 * (float(elev_lo_deg) + float(elev_hi_deg))]))
    az = _np.arange(azimuths, dtype=_np.float64) * (2.0 * _np.pi / max(azimuths, 1))
    e, a = _np.meshgrid(elev, az, indexing="ij")
    d = _np.stack([_np.cos(e) * _np.cos(a), _np.cos(e) * _np.sin(a), _np.sin(e)], axis=-1).reshape(-1, 3)
    return _np.ascontiguousarray(d / _np.linalg.norm(d, axis=1)[:, None])


def cosine_directions(k):
    """(k, 3) float64: k unit directions about +z whose density is proportional to the cosine of the angle to +z (a Fibonacci spiral on the
    unit disk, lifted to the hemisphere), so that the mean of li over them estimates irradiance / pi.  For j = 0 .. k-1: u = (j + 0.5) / k,
    r = sqrt(u), phi = j * pi * (3 - sqrt(5)), d = (r cos phi, r sin phi, sqrt(1 - u)).  A convention of this WRAPPER, not of the C contract."""
    j = _np.arange(int(k), dtype=_np.float64)
    u = (j + 0.5) / max(int(k), 1)
    r, phi = _np.sqrt(u), j * (_np.pi * (3.0 - _np.sqrt(5.0)))
    return _np.ascontiguousarray(_np.stack([r * _np.cos(phi), r * _np.sin(phi), _np.sqrt(1.0 - u)], axis=1))


def sh_weights(dirs, bands=3):
    """(K, bands^2) float64 weights for radiance_gather that project a pose's radiance onto the real spherical harmonics: column l*l + l + m
    of row k is Y_lm(d_k / |d_k|) * 4 pi / K, the Monte-Carlo weight of K directions spread evenly over the sphere (sphere_directions).
    bands 1 .. 3, with (x, y, z) = d / |d|:  Y_00 = 0.28209479177387814;  Y_1,-1 = 0.4886025119029199 y,  Y_10 = 0.4886025119029199 z,
    Y_11 = 0.4886025119029199 x;  Y_2,-2 = 1.0925484305920792 x y,  Y_2,-1 = 1.0925484305920792 y z,  Y_20 = 0.31539156525252005 (3 z z - 1),
    Y_21 = 1.0925484305920792 x z,  Y_22 = 0.5462742152960396 (x x - y y).  No Condon-Shortley sign.  A convention of this WRAPPER, not of
    the C contract."""
    bands = int(bands)
    if not 1 <= bands <= 3:
        raise ValueError("bands: 1, 2 or 3")
    d = _np.ascontiguousarray(dirs, dtype=_np.float64).reshape(-1, 3)
    n = d / _np.linalg.norm(d, axis=1)[:, None]
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    cols = [_np.full(d.shape[0], 0.28209479177387814)]
    if bands >= 2:
        cols += [0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x]
    if bands >= 3:
        cols += [1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0), 1.0925484305920792 * (x * z),
                 0.5462742152960396 * (x * x - y * y)]
    return _np.ascontiguousarray(_np.stack(cols, axis=1) * (4.0 * _np.pi / max(d.shape[0], 1)))


def frames_from_normals(normals):
    """(N, 3, 3) float64 frames for radiance_gather / range_scan: per point a row-major matrix whose columns t, s, n are an orthonormal
    basis with n = normal / |normal| as the THIRD column, so that a direction (0, 0, 1) leaves along the normal.  Branch-free (Duff et al.,
    "Building an Orthonormal Basis, Revisited", 2017): sg = copysign(1, n.z), a = -1 / (sg + n.z), b = n.x * n.y * a,
    t = (1 + sg * n.x * n.x * a, sg * b, -sg * n.x), s = (b, sg + n.y * n.y * a, -n.y).  A convention of this WRAPPER, not of the C contract."""
    v = _np.ascontiguousarray(normals, dtype=_np.float64).reshape(-1, 3)
    n = v / _np.linalg.norm(v, axis=1)[:, None]
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    sg = _np.copysign(1.0, z)
    a = -1.0 / (sg + z)
    b = x * y * a
    t = _np.stack([1.0 + sg * x * x * a, sg * b, -sg * x], axis=1)
    s = _np.stack([b, sg + y * y * a, -y], axis=1)
    return _np.ascontiguousarray(_np.stack([t, s, n], axis=2))


def LightGroup(lights=0, ambient=False, flags=None):
    """lg_light_group (include/lasgun_hip.h): `lights` a mask (bit l: light l in add order) or an iterable of light indices; `ambient`:
    the scene's ambient term is part of the group (GROUP_AMBIENT); `flags`: the raw word instead."""
    if not isinstance(lights, int):
        mask = 0
        for l in lights:
            if not 0 <= int(l) < 32:
                raise ValueError("a light index is 0 .. 31")
            mask |= 1 << int(l)
        lights = mask
    return CLightGroup(int(lights), int(flags) if flags is not None else (GROUP_AMBIENT if ambient else 0))


def per_light_groups(n_lights):
    """The groups a re-lit frame needs: [base (no lights, no ambient), the ambient term alone, light 0, light 1, ...] -- 2 + n_lights
    groups for radiance_groups; relight() takes its planes.  A convention of this WRAPPER, not of the C contract."""
    n = int(n_lights)
    if not 0 <= n <= 32:
        raise ValueError("n_lights: 0 .. 32")
    return [LightGroup(0), LightGroup(0, ambient=True)] + [LightGroup(1 << l) for l in range(n)]


def relight(planes, ambient_scale=1.0, light_scales=None):
    """A frame re-lit from per_light_groups' planes without tracing again: base + a * (amb - base) + sum_i s_i * (L_i - base), with
    planes[0] the base, planes[1] the ambient plane and planes[2 + i] light i's; a = ambient_scale, s_i = light_scales[i] (a scalar, or
    3 values per light to change its colour; None: all 1).  li() is linear in the intensities, so this is the frame the scaled scene
    renders up to rounding -- it is NOT bit-exact against a rebuilt render: the render sums the lights' terms in one running sum at every
    hit, this sums whole planes.  Evaluated left to right in float64.  A convention of this WRAPPER."""
    p = _np.asarray(planes, dtype=_np.float64)
    if p.ndim < 2 or p.shape[0] < 2 or p.shape[-1] != 3:
        raise ValueError("planes: (2 + n_lights, ..., 3), as radiance_groups returns for per_light_groups")
    n = p.shape[0] - 2
    scales = [1.0] * n if light_scales is None else list(light_scales)
    if len(scales) != n:
        raise ValueError("light_scales: one scalar or 3 values per light, %d lights" % n)
    s = [_np.broadcast_to(_np.asarray(x, dtype=_np.float64), (3,)) for x in scales]
    a = _np.broadcast_to(_np.asarray(ambient_scale, dtype=_np.float64), (3,))
    base = p[0]
    out = base + a * (p[1] - base)
    for i in range(n):
        out = out + s[i] * (p[2 + i] - base)
    return out


def view_look_at(origin, look, up, fov=None, scale=None, supersampling=0):
    """api.view_look_at at package level: a View from a look-at camera (perspective `fov` degrees, or orthographic `scale`)."""
    return api.view_look_at(origin, look, up, fov=fov, scale=scale, supersampling=supersampling)


CUBE_FACES = (((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, -1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, -1)), ((0, 0, 1), (0, -1, 0)), ((0, 0, -1), (0, -1, 0)))


def cube_map_views(origin, supersampling=0):
    """The six faces of a cube map around `origin`, in the order +X -X +Y -Y +Z -Z: face f is the perspective view of fov 90 degrees
    view_look_at(origin, look=origin + axis_f, up=up_f), with the axes (1,0,0) (-1,0,0) (0,1,0) (0,-1,0) (0,0,1) (0,0,-1) and the ups
    (0,-1,0) (0,-1,0) (0,0,1) (0,0,-1) (0,-1,0) (0,-1,0).  A convention of this WRAPPER, not of the C contract."""
    o = [float(c) for c in origin]
    return [view_look_at(o, [o[c] + float(axis[c]) for c in range(3)], up, fov=90.0, supersampling=supersampling) for axis, up in CUBE_FACES]


def orbit_views(center, radius, elevation_deg, n, fov, up=(0, 1, 0), supersampling=0):
    """n perspective views of `fov` degrees looking at `center` from eyes on a circle about the axis `up` through it: with u = up / |up|,
    (t, s) = the first two columns of frames_from_normals(u) (so t, s, u is an orthonormal basis), e = radians(elevation_deg) and
    a_k = 2 pi k / n, eye_k = center + radius * (cos(e) * (cos(a_k) * t + sin(a_k) * s) + sin(e) * u) and view k is
    view_look_at(eye_k, center, up, fov=fov).  A convention of this WRAPPER, not of the C contract."""
    c = _np.asarray(center, dtype=_np.float64).reshape(3)
    u = _np.asarray(up, dtype=_np.float64).reshape(3)
    u = u / _np.linalg.norm(u)
    f = frames_from_normals(u)[0]
    t, s = f[:, 0], f[:, 1]
    e = _np.radians(float(elevation_deg))
    views = []
    for k in range(int(n)):
        a = 2.0 * _np.pi * k / int(n)
        eye = c + float(radius) * (_np.cos(e) * (_np.cos(a) * t + _np.sin(a) * s) + _np.sin(e) * u)
        views.append(view_look_at(eye, c, up, fov=float(fov), supersampling=supersampling))
    return views


_share_torch_hip_runtime()
api = HipApi(_C.CDLL(LIB_PATH), "lg_", _EXTRA)
api.Accel.features = lambda self, w, h, rect=None, planes=FEATURE_PLANES, material_rgb=None: api.capture_features(self, w, h, rect, planes, material_rgb)  # accel.features(w, h)
api.Accel.visibility = lambda self, from_pts, to_pts, counts=False: api.visibility(self, from_pts, to_pts, counts)  # accel.visibility(from_pts, to_pts)
api.Accel.open_directions = lambda self, points, dirs, normals=None, counts=False: api.open_directions(self, points, dirs, normals, counts)  # accel.open_directions(points, dirs)
api.Accel.range_scan = lambda self, origins, beams, frames=None, planes=("range",), lanes=0: api.range_scan(self, origins, beams, frames, planes, lanes)  # accel.range_scan(origins, beams)
api.Accel.hit_layers = lambda self, rays, max_layers, planes=("along", "id", "count"): api.hit_layers(self, rays, max_layers, planes)  # accel.hit_layers(rays, 8)
api.Accel.radiance_groups = lambda self, rays, groups: api.radiance_groups(self, rays, groups)  # accel.radiance_groups(rays, per_light_groups(n))
api.Accel.scatter = lambda self, rays, planes=SCATTER_PLANES: api.scatter(self, rays, planes)  # accel.scatter(rays)
api.Accel.hit_attributes = lambda self, rays, planes=ATTR_PLANES: api.hit_attributes(self, rays, planes)  # accel.hit_attributes(rays, ("uv", "bary"))
api.Accel.closest_points = lambda self, points, radius=float("inf"), planes=None: api.closest_points(self, points, radius, planes)  # accel.closest_points(points, radius=0.5)
api.Accel.nearest = lambda self, points, radii=None, radius=float("inf"), k=1, planes=None: api.nearest(self, points, radii, radius, k, planes)  # accel.nearest(points, radii=r, k=4)
api.Accel.touching = lambda self, centres, radii: api.touching(self, centres, radii)  # accel.touching(centres, radii): a bool per sphere
api.Accel.closest_segments = lambda self, segments, radii=None, radius=float("inf"), planes=None: api.closest_segments(self, segments, radii, radius, planes)  # accel.closest_segments(segments, radii=r)
api.Accel.capsules_touching = lambda self, p0, p1, radii: api.capsules_touching(self, p0, p1, radii)  # accel.capsules_touching(p0, p1, radii): a bool per capsule
api.Accel.sweep_touching = lambda self, centres_from, centres_to, radii: api.sweep_touching(self, centres_from, centres_to, radii)  # accel.sweep_touching(a, b, radii): a bool per swept sphere
api.Accel.signed_distance = lambda self, points, max_layers=32: api.signed_distance(self, points, max_layers)  # accel.signed_distance(points): closed solids only
api.Accel.scatter_lit = lambda self, rays, lights, ambient=(0.0, 0.0, 0.0), planes=LIT_PLANES: api.scatter_lit(self, rays, lights, ambient, planes)  # accel.scatter_lit(rays, [la.Light(p, i)])
def path_rules(accel, default=PATH_ABSORB, gain=1.0):
    """The wrapper's one convention of a rule table for trace_paths: glass refracts with its eta, mirror and metal reflect, the rest `default`."""
    return api.path_rules(accel, default, gain)


api.Accel.trace_paths = lambda self, rays, max_bounces, rules=None, normal=0, start_medium=None, planes=("point", "id", "count", "end"): api.trace_paths(self, rays, max_bounces, api.path_rules(self) if rules is None else rules, normal, start_medium, planes)  # accel.trace_paths(rays, 8)
api.Accel.radiance_gather = lambda self, origins, dirs, frames=None, weights=None, planes=("sums",), lanes=0: api.radiance_gather(self, origins, dirs, frames, weights, planes, lanes)  # accel.radiance_gather(origins, dirs, weights=w)
api.Accel.views = lambda self, views, w, h, rgba=True, rgb=False: api.capture_views(self, views, w, h, rgba, rgb)  # accel.views(views, w, h)
api.Accel.view_features = lambda self, views, w, h, planes=VIEW_FEATURE_PLANES, material_rgb=None: api.capture_view_features(self, views, w, h, planes, material_rgb)  # accel.view_features(views, w, h)

# reference-shaped names at package level: `from lasgun_amd import Scene, Material, capture`
Scene, Aggregate, Material, Camera, Film, Accel = api.Scene, api.Aggregate, api.Material, api.Camera, api.Film, api.Accel
capture, capture_subset, render = api.capture, api.capture_subset, api.render
