"""ctypes binding of libcapsaicin_hip.so (include/capsaicin_hip.h, include/capsaicin_scene.h).

No rendering happens in Python and nothing here falls back to a CPU path: every call goes through the C ABI and
raises CapError with cap_last_error() when the library reports a failure (e.g. no HIP device).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, "libcapsaicin_hip.so")
# A/B and diagnostic builds made by tools/build_variant.sh (compile-time switches measured against the product build in one GPU call)
if os.environ.get("CAP_LIB_VARIANT"):
    LIB_PATH = os.path.join(_PKG, "variants", "libcapsaicin_hip_%s.so" % os.environ["CAP_LIB_VARIANT"])

RENDER_AOV = 1
RENDER_EXT_MATERIALS = 2
RENDER_STAGE_TIMERS = 4
RENDER_GBUFFER_FEEDBACK = 8
RENDER_LOWRES_INDIRECT = 16

BUF_GBUFFER_GEO, BUF_DIRECT, BUF_ALBEDO, BUF_NORMAL_DEPTH, BUF_INDIRECT, BUF_COMBINED, BUF_ACCUM_SUM, BUF_ACCUM_MEAN, BUF_INDIRECT_LOWRES = range(9)


class CapError(RuntimeError):
    pass


class CameraData(C.Structure):
    """CameraData, reference src/systems/camera_system.h:16-31 (72 bytes)."""
    _fields_ = [("position", C.c_float * 3), ("focal_length", C.c_float), ("right", C.c_float * 3), ("znear", C.c_float),
                ("forward", C.c_float * 3), ("focus_distance", C.c_float), ("up", C.c_float * 3), ("aperture", C.c_float),
                ("sensor_size", C.c_float * 2)]


class Stats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_extension", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("shaded_vertices", C.c_uint64), ("frames", C.c_uint64), ("ms_total", C.c_double), ("ms_primary", C.c_double),
                ("ms_trace_closest", C.c_double), ("ms_trace_any", C.c_double), ("ms_shade", C.c_double),
                ("ms_resolve", C.c_double), ("launches_trace_closest", C.c_uint64), ("launches_trace_any", C.c_uint64),
                ("launches_shade", C.c_uint64), ("rays_extension_bounce0", C.c_uint64), ("rays_shadow_bounce0", C.c_uint64),
                ("guard_shade", C.c_uint64), ("guard_trace_any", C.c_uint64), ("guard_last", C.c_uint64), ("ms_post", C.c_double),
                ("post_frames", C.c_uint64), ("ms_direct", C.c_double), ("ms_post_pass", C.c_double * 5), ("shadow_entries", C.c_uint64),
                ("shadow_entries_bounce0", C.c_uint64), ("guard_append", C.c_uint64), ("lane1_dropped", C.c_uint64)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "ms_post_pass" else getattr(self, n)) for n, _ in self._fields_}


class BvhInfo(C.Structure):
    _fields_ = [("triangle_count", C.c_uint32), ("node_count", C.c_uint32), ("max_depth", C.c_uint32),
                ("stack_entries", C.c_uint32), ("bounds_lo", C.c_float * 3), ("bounds_hi", C.c_float * 3),
                ("build_ms", C.c_double)]


class RefitInfo(C.Structure):
    """CapRefitInfo: what cap_bvh_refit reports (the ratio of the two metrics tells when a rebuild pays)."""
    _fields_ = [("ms", C.c_double), ("expected_node_visits", C.c_double), ("expected_node_visits_built", C.c_double)]


class PseudonormalsInfo(C.Structure):
    """CapPseudonormalsInfo: what the weld of cap_pseudonormals_build found; the sign of signed_distance means inside / outside only
    when closed == 1."""
    _fields_ = [("vertices", C.c_uint32), ("edges", C.c_uint32), ("boundary_edges", C.c_uint32), ("nonmanifold_edges", C.c_uint32),
                ("inconsistent_edges", C.c_uint32), ("degenerate_triangles", C.c_uint32), ("closed", C.c_uint32), ("reserved", C.c_uint32),
                ("ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class WindingInfo(C.Structure):
    """CapWindingInfo: what cap_winding_build summed: the records of the dipole table, the triangles that contribute nothing, and the
    whole tree's area, area-weighted normal sum (0 for a closed mesh, up to rounding) and area-weighted centroid."""
    _fields_ = [("inner_nodes", C.c_uint32), ("degenerate_triangles", C.c_uint32), ("total_area", C.c_double), ("root_n", C.c_float * 3),
                ("root_p", C.c_float * 3), ("ms", C.c_double)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n in ("root_n", "root_p") else getattr(self, n)) for n, _ in self._fields_}


class WindingInstancesInfo(C.Structure):
    """CapWindingInstancesInfo: the derived tables of cap_winding_instances: whether current ones exist (built), the instances and how
    many of them contribute, the top-level tree's levels with their entry counts (padding included; host_top's layout), the forest's
    dipole records, and the whole table's normal sum, weight and centroid.  Only instances, levels, entries and level_entries are
    filled while built == 0."""
    _fields_ = [("instances", C.c_uint32), ("contributing", C.c_uint32), ("levels", C.c_uint32), ("entries", C.c_uint32),
                ("forest_records", C.c_uint32), ("built", C.c_uint32), ("level_entries", C.c_uint32 * 25), ("reserved", C.c_uint32),
                ("total_weight", C.c_double), ("root_n", C.c_float * 3), ("root_p", C.c_float * 3)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n in ("root_n", "root_p", "level_entries") else getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


VERTICES_DEVICE = 1  # CAP_VERTICES_DEVICE


def vertex_update_args(vertex_count, positions=None, normals=None, texcoords=None):
    """Checks the arrays of Renderer.update_vertices and returns (pointers, flags, keep-alive).  numpy arrays are host arrays; torch
    tensors must be contiguous float32 on a GPU (device pointers, CAP_VERTICES_DEVICE); one call takes one kind.  Shapes (V, 3) /
    (V, 3) / (V, 2) or flat."""
    arrays = (("positions", positions, 3), ("normals", normals, 3), ("texcoords", texcoords, 2))
    kinds = {("numpy" if isinstance(a, np.ndarray) else "torch" if hasattr(a, "data_ptr") else type(a).__name__)
             for _, a, _ in arrays if a is not None}
    if kinds - {"numpy", "torch"}:
        raise CapError("update_vertices takes numpy arrays or torch tensors, got %s" % ", ".join(sorted(kinds - {"numpy", "torch"})))
    if len(kinds) > 1:
        raise CapError("update_vertices: mixing host (numpy) and device (torch) arrays in one call")
    device = kinds == {"torch"}
    ptrs, keep = [], []
    for name, a, width in arrays:
        if a is None:
            ptrs.append(None)
            continue
        shape = tuple(a.shape)
        if shape not in ((vertex_count, width), (vertex_count * width,)):
            raise CapError("update_vertices: %s has shape %s, expected (%d, %d) or (%d,)" % (name, shape, vertex_count, width, vertex_count * width))
        if device:
            import torch
            if a.dtype != torch.float32 or not a.is_contiguous() or a.device.type != "cuda":
                raise CapError("update_vertices: %s must be a contiguous float32 tensor on the GPU, got %s on %s" % (name, a.dtype, a.device))
            ptrs.append(C.c_void_p(a.data_ptr()))
        else:
            if a.dtype != np.float32:
                raise CapError("update_vertices: %s must be float32, got %s" % (name, a.dtype))
            a = np.ascontiguousarray(a)
            ptrs.append(_p(a))
        keep.append(a)
    return ptrs, (VERTICES_DEVICE if device else 0), keep


class RayDesc(C.Structure):
    """CapRayDesc: DXR RayDesc layout (32 bytes)."""
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class Hit(C.Structure):
    """CapHit (16 bytes): closest hit of a ray query; a miss is (tmax, 0, 0, MISS)."""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_uint32)]


MISS = 0xFFFFFFFF  # CapHit::triangle of a miss (and the ids CAP_BUF_GBUFFER_GEO stores for one)


def hit_triangles(hits):
    """Global triangle ids of (N, 4) hit records (column 3 holds the id's bits) as int64; a miss reads MISS.  torch in, torch out."""
    if isinstance(hits, np.ndarray):
        return np.ascontiguousarray(hits, np.float32).reshape(-1, 4)[:, 3].view(np.uint32).astype(np.int64)
    import torch
    return hits[:, 3].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


class PointDesc(C.Structure):
    """CapPointDesc (16 bytes): a query point and its search radius (+inf: unbounded)."""
    _fields_ = [("point", C.c_float * 3), ("radius", C.c_float)]


class Closest(C.Structure):
    """CapClosest (32 bytes): the closest point, its squared distance, the weights of v1 and v2, the triangle (MISS: none within the
    radius) and the feature the point lies on."""
    _fields_ = [("point", C.c_float * 3), ("dist2", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_uint32),
                ("feature", C.c_uint32)]


class SweepDesc(C.Structure):
    """CapSweepDesc (32 bytes): a sphere of `radius` whose centre moves from origin along direction for t in [0, tmax]."""
    _fields_ = [("origin", C.c_float * 3), ("radius", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class SweepHit(C.Structure):
    """CapSweepHit (32 bytes): Closest's layout with the time of first contact where dist2 is (tmax and MISS on a miss)."""
    _fields_ = [("point", C.c_float * 3), ("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_uint32), ("feature", C.c_uint32)]


class BoxDesc(C.Structure):
    """CapBoxDesc (32 bytes): an axis-aligned box, lo and hi corner; the pad words are not read."""
    _fields_ = [("lo", C.c_float * 3), ("pad0", C.c_float), ("hi", C.c_float * 3), ("pad1", C.c_float)]


class TriangleDesc(C.Structure):
    """CapTriangleDesc (48 bytes): a query triangle a, b, c and the global id of the scene triangle that is no candidate
    (0xFFFFFFFF: none); the pad words are not read."""
    _fields_ = [("a", C.c_float * 3), ("skip", C.c_uint32), ("b", C.c_float * 3), ("pad0", C.c_uint32), ("c", C.c_float * 3), ("pad1", C.c_uint32)]


FEATURE_FACE, FEATURE_EDGE_V0V1, FEATURE_EDGE_V1V2, FEATURE_EDGE_V2V0, FEATURE_V0, FEATURE_V1, FEATURE_V2 = range(7)  # CAP_FEATURE_*


def closest_triangles(records):
    """(triangle ids, features) of (N, 8) closest-point records (columns 6 and 7 hold their bits) as int64; a miss reads MISS.  torch
    in, torch out.  The (N, k, 8) pages of closest_points_multi give (N, k) ids and features."""
    if isinstance(records, np.ndarray):
        if records.ndim == 3:
            w = np.ascontiguousarray(records, np.float32)[..., 6:8].view(np.uint32).astype(np.int64)
            return w[..., 0], w[..., 1]
        w = np.ascontiguousarray(records, np.float32).reshape(-1, 8)[:, 6:8].view(np.uint32).astype(np.int64)
        return w[:, 0], w[:, 1]
    import torch
    w = records[..., 6:8].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return w[..., 0], w[..., 1]


OUTPUT_COMBINED, OUTPUT_DIRECT, OUTPUT_INDIRECT, OUTPUT_VARIANCE = range(4)  # SettingsComponent::output, gui_system.h:11-17


class PostSettings(C.Structure):
    """SettingsComponent fields read by the reconstruction chain, reference src/systems/gui_system.h:20-37.  Every field behind
    lowres_indirect reads 0 as the reference default (so `use_variance`, default true, travels as disable_variance)."""
    _fields_ = [("gather", C.c_int32), ("denoise", C.c_int32), ("eaw5", C.c_int32), ("eaw_normal_sigma", C.c_float),
                ("eaw_depth_sigma", C.c_float), ("eaw_luma_sigma", C.c_float), ("gather_normal_sigma", C.c_float),
                ("gather_depth_sigma", C.c_float), ("gather_luma_sigma", C.c_float), ("temporal_upscale_feedback", C.c_float),
                ("taa_feedback", C.c_float), ("lowres_indirect", C.c_int32), ("disable_variance", C.c_int32), ("fast_weights", C.c_int32),
                ("output", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().cap_post_settings_default(C.byref(self))  # the reference's defaults, from the library itself
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def use_variance(self):  # RaytracingOptions::use_variance, raytracing_system.h:25
        return 0 if self.disable_variance else 1

    @use_variance.setter
    def use_variance(self, v):
        self.disable_variance = 0 if v else 1


class GeometryView(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("indices", C.POINTER(C.c_uint32)), ("meshes", C.POINTER(C.c_uint32)), ("vertex_count", C.c_uint32),
                ("index_count", C.c_uint32), ("mesh_count", C.c_uint32), ("texture_count", C.c_uint32),
                ("material_count", C.c_uint32)]


class TraceOptions(C.Structure):  # CapTraceOptions
    _fields_ = [("ray_flags", C.c_uint32), ("instance_mask", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class InstanceDesc(C.Structure):  # CapInstanceDesc, 64 B
    _fields_ = [("transform", C.c_float * 12), ("mask", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class InstancesInfo(C.Structure):  # CapInstancesInfo
    _fields_ = [("count", C.c_uint32), ("inert", C.c_uint32), ("tlas_nodes", C.c_uint32), ("tlas_depth", C.c_uint32), ("ms", C.c_double)]


class ObjectRange(C.Structure):  # CapObjectRange
    _fields_ = [("first_mesh", C.c_uint32), ("mesh_count", C.c_uint32)]


class ObjectInfo(C.Structure):  # CapObjectInfo, 48 B
    _fields_ = [("first_triangle", C.c_uint32), ("triangle_count", C.c_uint32), ("node_count", C.c_uint32), ("max_depth", C.c_uint32),
                ("bounds_lo", C.c_float * 3), ("bounds_hi", C.c_float * 3), ("builder", C.c_uint32), ("reserved", C.c_uint32)]


class ObjectsInfo(C.Structure):  # CapObjectsInfo
    _fields_ = [("count", C.c_uint32), ("triangles", C.c_uint32), ("nodes", C.c_uint32), ("max_depth", C.c_uint32), ("ms", C.c_double)]


INSTANCES_DEVICE = 1  # CAP_INSTANCES_DEVICE
OBJECT_MAX_COUNT = 4096  # CAP_OBJECT_MAX_COUNT
OBJECT_RANGE_DTYPE = np.dtype([("first_mesh", np.uint32), ("mesh_count", np.uint32)])
OBJECT_INFO_DTYPE = np.dtype([("first_triangle", np.uint32), ("triangle_count", np.uint32), ("node_count", np.uint32), ("max_depth", np.uint32),
                              ("bounds_lo", np.float32, (3,)), ("bounds_hi", np.float32, (3,)), ("builder", np.uint32), ("reserved", np.uint32)])
INSTANCE_MAX_CONDITION = 4096.0  # CAP_INSTANCE_MAX_CONDITION
INSTANCE_DESC_DTYPE = np.dtype([("transform", np.float32, (12,)), ("mask", np.uint32), ("reserved", np.uint32, (3,))])

# every symbol include/capsaicin_hip.h and include/capsaicin_scene.h declare: (restype, argtypes)
_vp, _u32, _u64, _i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
SYMBOLS = {
    "cap_last_error": (C.c_char_p, []),
    "cap_device_count": (_i, []),
    "cap_ctx_create": (_i, [_i, _vp, C.POINTER(_vp)]),
    "cap_ctx_destroy": (None, [_vp]),
    "cap_scene_upload": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "cap_texture_upload": (_i, [_vp, _u32, _vp, _u32, _u32]),
    "cap_bluenoise_upload": (_i, [_vp, _vp]),
    "cap_materials_upload": (_i, [_vp, _vp, _u32]),
    "cap_bvh_build": (_i, [_vp]),
    "cap_set_bvh_build": (_i, [_vp, _u32]),
    "cap_bvh_info": (_i, [_vp, C.POINTER(BvhInfo)]),
    "cap_bvh_readback": (_i, [_vp, _vp, _vp]),
    "cap_bvh_wide_readback": (_i, [_vp, _vp, _vp, _vp]),
    "cap_scene_update_vertices": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "cap_bvh_refit": (_i, [_vp, C.POINTER(RefitInfo)]),
    "cap_camera_set": (_i, [_vp, C.POINTER(CameraData)]),
    "cap_prev_camera_set": (_i, [_vp, C.POINTER(CameraData)]),
    "cap_set_resolution": (_i, [_vp, _u32, _u32]),
    "cap_set_shard": (_i, [_vp, _u32, _u32]),
    "cap_set_batch_paths": (_i, [_vp, _u64]),
    "cap_set_traversal": (_i, [_vp, _u32]),
    "cap_debug_set": (_i, [_vp, _u32, _u64]),
    "cap_debug_get": (_i, [_vp, _u32, C.POINTER(_u64)]),
    "cap_debug_switch_index": (_i, [C.c_char_p]),
    "cap_debug_pair_ids_dense": (_i, [_vp, _u32, _u32, _u32]),
    "cap_debug_head_chunk": (_i, [_u32, _u32, _vp, _u32, _vp, _u64, _vp, _vp]),
    "cap_debug_query_ranges": (_i, [_u64, _u32, _vp, _vp, _vp]),
    "cap_debug_closest_instance_bound": (_i, [_vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    "cap_debug_overlap_instance_prune": (_i, [_vp] * 17),
    "cap_debug_overlap_world_node": (_i, [_vp] * 12),
    "cap_debug_sweep_instance_prune": (_i, [_vp] * 6 + [C.c_float] + [_vp] * 7),
    "cap_render": (_i, [_vp, _u32, _u32, _u32, _u32]),
    "cap_accum_reset": (_i, [_vp]),
    "cap_accum_import": (_i, [_vp, _vp, _u64]),
    "cap_sync": (_i, [_vp]),
    "cap_readback": (_i, [_vp, _i, _vp]),
    "cap_stats_get": (_i, [_vp, C.POINTER(Stats)]),
    "cap_stats_reset": (_i, [_vp]),
    "cap_tile_buffer_floats": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "cap_resolve_tiles": (_i, [_vp, _vp]),
    "cap_trace_rays": (_i, [_vp, _vp, _u64, _vp, _u32]),
    "cap_trace_occlusion": (_i, [_vp, _vp, _u64, _vp, _u32]),
    "cap_trace_rays_multi": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _u32]),
    "cap_scene_set_instance_masks": (_i, [_vp, _vp, _u32]),
    "cap_trace_rays_ex": (_i, [_vp, _vp, _u64, _vp, C.POINTER(TraceOptions)]),
    "cap_trace_occlusion_ex": (_i, [_vp, _vp, _u64, _vp, C.POINTER(TraceOptions)]),
    "cap_trace_rays_multi_ex": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_instances_set": (_i, [_vp, _vp, _u32, _u32, C.POINTER(InstancesInfo)]),
    "cap_instances_set_ex": (_i, [_vp, _vp, _vp, _u32, _u32, C.POINTER(InstancesInfo)]),
    "cap_objects_set": (_i, [_vp, _vp, _u32, C.POINTER(ObjectsInfo)]),
    "cap_objects_info": (_i, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "cap_instances_readback": (_i, [_vp, _vp, _vp]),
    "cap_trace_instances": (_i, [_vp, _vp, _u64, _vp, _vp, C.POINTER(TraceOptions)]),
    "cap_trace_instances_occlusion": (_i, [_vp, _vp, _u64, _vp, C.POINTER(TraceOptions)]),
    "cap_trace_instances_multi": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_closest_points": (_i, [_vp, _vp, _u64, _vp, C.POINTER(TraceOptions)]),
    "cap_sweep_spheres": (_i, [_vp, _vp, _u64, _vp, C.POINTER(TraceOptions)]),
    "cap_sweep_instances": (_i, [_vp, _vp, _u64, _vp, _vp, C.POINTER(TraceOptions)]),
    "cap_closest_points_multi": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_overlap_boxes": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_overlap_instances": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_overlap_triangles": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_overlap_triangles_instances": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_pseudonormals_build": (_i, [_vp, C.POINTER(PseudonormalsInfo)]),
    "cap_pseudonormals_drop": (_i, [_vp]),
    "cap_pseudonormals_readback": (_i, [_vp, _vp]),
    "cap_signed_distance": (_i, [_vp, _vp, _u64, _vp, _vp, C.POINTER(TraceOptions)]),
    "cap_winding_build": (_i, [_vp, C.POINTER(WindingInfo)]),
    "cap_winding_drop": (_i, [_vp]),
    "cap_winding_readback": (_i, [_vp, _vp]),
    "cap_winding_numbers": (_i, [_vp, _vp, _u64, C.c_float, _vp, _vp]),
    "cap_winding_instances": (_i, [_vp, _vp, _u64, C.c_float, _vp, _vp]),
    "cap_winding_instances_info": (_i, [_vp, C.POINTER(WindingInstancesInfo)]),
    "cap_winding_instances_readback": (_i, [_vp, _vp, _vp, _vp]),
    "cap_objects_readback": (_i, [_vp, _vp, _vp]),
    "cap_closest_instances": (_i, [_vp, _vp, _u64, _vp, _vp, C.POINTER(TraceOptions)]),
    "cap_signed_distance_instances": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(TraceOptions)]),
    "cap_closest_instances_multi": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, C.POINTER(TraceOptions)]),
    "cap_assemble_tiles": (_i, [_vp, _vp, _u32, _vp]),
    "cap_post_settings_default": (None, [C.POINTER(PostSettings)]),
    "cap_post_frame": (_i, [_vp, C.POINTER(PostSettings), _u32, C.POINTER(CameraData)]),
    "cap_aov_tile_buffer_floats": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "cap_resolve_aov_tiles": (_i, [_vp, _vp]),
    "cap_post_frame_gathered": (_i, [_vp, C.POINTER(PostSettings), _u32, C.POINTER(CameraData), _vp, _u32]),
    "cap_feedback_buffer_floats": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "cap_feedback_export": (_i, [_vp, _vp]),
    "cap_feedback_import": (_i, [_vp, _vp, _u32]),
    "cap_post_reset": (_i, [_vp]),
    "cap_post_readback": (_i, [_vp, _vp]),
    "cap_obj_load": (_i, [C.c_char_p, C.c_char_p, C.POINTER(_vp)]),
    "cap_geometry_free": (None, [_vp]),
    "cap_obj_set_threads": (None, [C.c_int]),
    "cap_geometry_view": (_i, [_vp, C.POINTER(GeometryView)]),
    "cap_geometry_texture_name": (C.c_char_p, [_vp, _u32]),
    "cap_geometry_warning": (C.c_char_p, [_vp]),
    "cap_geometry_materials": (_i, [_vp, _vp]),
    "cap_scene_upload_geometry": (_i, [_vp, _vp]),
    "cap_comm_unique_id": (_i, [_vp]),
    "cap_comm_init_rank": (_i, [_vp, _vp, _u32, _u32]),
    "cap_comm_gather_frame": (_i, [_vp]),
    "cap_comm_init_all": (_i, [_vp, _u32]),
    "cap_comm_gather_frame_all": (_i, [_vp, _u32]),
    "cap_comm_image": (_i, [_vp, C.POINTER(C.c_void_p)]),
    "cap_comm_readback": (_i, [_vp, _vp]),
    "cap_comm_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "cap_comm_destroy": (_i, [_vp]),
    "cap_comm_abort": (_i, [_vp]),
    "cap_image_decode": (_i, [_vp, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(_u32), C.POINTER(_u32)]),
    "cap_image_free": (None, [_vp]),
    "cap_host_sah_build": (_i, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "cap_host_wide_build": (_i, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp]),
}

_LIB = None


def build_native(force=False):
    """Compile the HIP library in-tree with hipcc for gfx950 (capsaicin_amd/csrc/Makefile)."""
    args = ["make", "-C", os.path.join(_PKG, "csrc"), "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise CapError("native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
        # PyTorch-ROCm bundles its own copy of the HIP runtime (same SONAME).  A process must hold exactly one runtime: if torch
        # is going to be used next to this library (device buffers for the tile gather, torch.distributed), its copy has to be
        # the one already loaded when libcapsaicin_hip.so resolves libamdhip64.so.7; the other order leaves torch with
        # "No HIP GPUs are available".  torch is plumbing only; nothing below needs it.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch-less host: the system runtime is used
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB


def _check(rc, what):
    if rc != 0:
        raise CapError("%s failed (status %d): %s" % (what, rc, lib().cap_last_error().decode()))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    return int(lib().cap_device_count())


def load_bluenoise(path=None):
    """assets/bluenoise256.rgba: raw RGBA8 texels of the reference's blue-noise texture (the sampler's RNG)."""
    path = path or os.path.join(_ROOT, "assets", "bluenoise256.rgba")
    return np.fromfile(path, np.uint8).reshape(256, 256, 4)


_SCENE_CONFIG = None


def scene_config():
    """assets/scene_config.json: the scene constants of the benchmark workloads that the reference does not fix."""
    global _SCENE_CONFIG
    if _SCENE_CONFIG is None:
        import json
        cfg = json.load(open(os.path.join(os.path.dirname(_PKG), "assets", "scene_config.json")))
        cfg["cornell_ggx"] = {k: v for k, v in cfg["cornell_ggx"].items() if not k.startswith("_")}
        _SCENE_CONFIG = cfg
    return _SCENE_CONFIG


def camera_from_config(c, width, height):
    """CameraData from a config entry; right / up by the reference's own formulas when absent (input_system.cpp:134-141)."""
    cam = CameraData()
    f = np.float64(c["forward"])
    f /= np.linalg.norm(f)
    right = np.float64(c["right"]) if "right" in c else -np.cross(f, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.float64(c["up"]) if "up" in c else np.cross(f, right)
    cam.position[:] = c["position"]
    cam.forward[:] = f
    cam.right[:] = right
    cam.up[:] = up
    cam.focal_length = c["focal_length"]
    cam.sensor_size[0] = c["sensor_x"]
    cam.sensor_size[1] = np.float32(c["sensor_x"]) * (np.float32(height) / np.float32(width))  # camera_system.cpp:10-17
    return cam


def cornell_camera(width, height):
    """The Cornell-box view fixed by SURVEY.md 8d (assets/scene_config.json)."""
    return camera_from_config(scene_config()["cornell_camera"], width, height)


class Geometry:
    """Host-side GeometryStorage produced by the native OBJ loader (cap_obj_load)."""

    def __init__(self, obj_path, mtl_dir=None):
        self.h = C.c_void_p()
        _check(lib().cap_obj_load(obj_path.encode(), (mtl_dir or "").encode(), C.byref(self.h)), "cap_obj_load")
        v = GeometryView()
        _check(lib().cap_geometry_view(self.h, C.byref(v)), "cap_geometry_view")
        self.view = v
        nv, ni, nm = v.vertex_count, v.index_count, v.mesh_count
        self.positions = np.ctypeslib.as_array(v.positions, (3 * nv,)).copy() if nv else np.zeros(0, np.float32)
        self.normals = np.ctypeslib.as_array(v.normals, (3 * nv,)).copy() if nv else np.zeros(0, np.float32)
        self.texcoords = np.ctypeslib.as_array(v.texcoords, (2 * nv,)).copy() if nv else np.zeros(0, np.float32)
        self.indices = np.ctypeslib.as_array(v.indices, (ni,)).copy() if ni else np.zeros(0, np.uint32)
        self.meshes = np.ctypeslib.as_array(v.meshes, (nm * 8,)).copy().reshape(-1, 8) if nm else np.zeros((0, 8), np.uint32)
        self.texture_names = [lib().cap_geometry_texture_name(self.h, i).decode() for i in range(v.texture_count)]
        self.material_count = v.material_count
        self.warning = lib().cap_geometry_warning(self.h).decode()

    def materials(self):
        m = np.zeros((self.meshes.shape[0], 12), np.float32)
        _check(lib().cap_geometry_materials(self.h, _p(m)), "cap_geometry_materials")
        return m

    def __del__(self):
        if getattr(self, "h", None):
            lib().cap_geometry_free(self.h)
            self.h = None


def host_sah_build(tri_lo, tri_hi):
    """The host-side SAH tree over triangle boxes (no GPU): (nodes [n-1, 16] float32, order [n] uint32, depth)."""
    lo, hi = np.asarray(tri_lo, np.float32), np.asarray(tri_hi, np.float32)
    n = len(lo)
    boxes = np.zeros((n, 8), np.float32)
    boxes[:, 0:3], boxes[:, 4:7] = lo, hi
    nodes = np.zeros((max(n - 1, 1), 16), np.float32)
    order = np.zeros(n, np.uint32)
    depth = C.c_uint32()
    _check(lib().cap_host_sah_build(_p(boxes), n, _p(nodes), _p(order), C.byref(depth)), "cap_host_sah_build")
    return nodes[:max(n - 1, 0)], order, int(depth.value)


def image_decode(data, name=None):
    """Texture file bytes -> [h, w, 4] uint8 (PNG / TGA / binary PPM), as TextureSystem's stbi_load(..., 4) would hand over."""
    buf = np.frombuffer(bytes(data), np.uint8)
    px, w, h = C.c_void_p(), _u32(), _u32()
    _check(lib().cap_image_decode(_p(buf), buf.size, name.encode() if name else None, C.byref(px), C.byref(w), C.byref(h)), "cap_image_decode")
    out = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint8)), (h.value, w.value, 4)).copy()
    lib().cap_image_free(px)
    return out


def host_wide_build(nodes, n, scene_lo, scene_hi):
    """Binary tree (host_sah_build's nodes) -> compressed 8-wide view: (wide nodes [count, 20] uint32, tri_src, depth, top)."""
    nodes = np.ascontiguousarray(nodes, np.float32)
    lo, hi = np.ascontiguousarray(scene_lo, np.float32), np.ascontiguousarray(scene_hi, np.float32)
    wide = np.zeros((max(n, 1), 20), np.uint32)
    src = np.zeros(max(n, 1), np.uint32)
    info = np.zeros(3, np.uint32)
    _check(lib().cap_host_wide_build(_p(nodes) if n > 1 else None, n, _p(lo), _p(hi), _p(wide), wide.shape[0], _p(src), _p(info)),
           "cap_host_wide_build")
    return wide[:int(info[0])], src[:n], int(info[1]), int(info[2])


def comm_unique_id():
    """128-byte RCCL id made by rank 0; the caller carries it to the other ranks."""
    buf = (C.c_uint8 * 128)()
    _check(lib().cap_comm_unique_id(C.cast(buf, C.c_void_p)), "cap_comm_unique_id")
    return bytes(buf)


def comm_init_all(renderers):
    arr = (C.c_void_p * len(renderers))(*[r.ctx for r in renderers])
    _check(lib().cap_comm_init_all(C.cast(arr, C.c_void_p), len(renderers)), "cap_comm_init_all")


def comm_gather_frame_all(renderers):
    arr = (C.c_void_p * len(renderers))(*[r.ctx for r in renderers])
    _check(lib().cap_comm_gather_frame_all(C.cast(arr, C.c_void_p), len(renderers)), "cap_comm_gather_frame_all")


class Renderer:
    """One CapContext (= one GPU).  Mirrors what RaytracingSystem::Run consumes and produces."""

    def __init__(self, device=0, stream=None):
        self.ctx = C.c_void_p()
        _check(lib().cap_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.ctx)), "cap_ctx_create")
        self.width = self.height = 0
        self.device = device
        self._tri_end = np.zeros(0, np.int64)  # inclusive prefix sums of the uploaded mesh table's triangle counts
        self._vertex_count = 0
        self._scene_host = None  # (positions (V, 3) float32 or the device tensor of the last update, indices, meshes (M, 8)): scene_triangle_queries

    def close(self):
        if getattr(self, "ctx", None):
            lib().cap_ctx_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    # ---- scene ----
    def upload_scene(self, positions, normals, texcoords, indices, meshes):
        a = [np.ascontiguousarray(positions, np.float32).ravel(), np.ascontiguousarray(normals, np.float32).ravel(),
             np.ascontiguousarray(texcoords, np.float32).ravel(), np.ascontiguousarray(indices, np.uint32).ravel(),
             np.ascontiguousarray(meshes, np.uint32).reshape(-1, 8)]
        _check(lib().cap_scene_upload(self.ctx, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), a[0].size // 3, a[3].size,
                                      a[4].shape[0]), "cap_scene_upload")
        self._set_mesh_table(a[4])
        self._vertex_count = a[0].size // 3
        self._scene_host = (a[0].reshape(-1, 3).copy(), a[3].copy(), a[4].copy())

    def upload_geometry(self, geo):
        _check(lib().cap_scene_upload_geometry(self.ctx, geo.h), "cap_scene_upload_geometry")
        self._set_mesh_table(geo.meshes)
        self._vertex_count = int(geo.view.vertex_count)
        self._scene_host = (geo.positions.reshape(-1, 3).copy(), geo.indices.copy(), np.array(geo.meshes, np.uint32).reshape(-1, 8))

    def _set_mesh_table(self, meshes):
        self._tri_end = np.cumsum(np.asarray(meshes, np.uint32).reshape(-1, 8)[:, 2].astype(np.int64) // 3)

    def upload_texture(self, index, rgba8):
        if rgba8 is None:
            _check(lib().cap_texture_upload(self.ctx, index, None, 0, 0), "cap_texture_upload")
            return
        t = np.ascontiguousarray(rgba8, np.uint8)
        _check(lib().cap_texture_upload(self.ctx, index, _p(t), t.shape[1], t.shape[0]), "cap_texture_upload")

    def upload_bluenoise(self, rgba8):
        t = np.ascontiguousarray(rgba8, np.uint8)
        assert t.size == 256 * 256 * 4
        _check(lib().cap_bluenoise_upload(self.ctx, _p(t)), "cap_bluenoise_upload")

    def upload_materials(self, materials):
        m = np.ascontiguousarray(materials, np.float32).reshape(-1, 12)
        _check(lib().cap_materials_upload(self.ctx, _p(m), m.shape[0]), "cap_materials_upload")

    BVH_BUILD_AUTO, BVH_BUILD_LBVH, BVH_BUILD_SAH, BVH_BUILD_PLOC, BVH_BUILD_SAH_DEVICE = 0, 1, 2, 3, 4  # CapBvhBuild

    def set_bvh_build(self, mode):
        """0 auto (Morton hierarchy up to 64 triangles, clustering build above, device SAH from 4096 on), 1 Morton hierarchy on the device, 2 SAH on the host, 3 clustering,
        4 SAH on the device (surface-area splits down to small segments, clustering inside)."""
        _check(lib().cap_set_bvh_build(self.ctx, mode), "cap_set_bvh_build")

    def build_bvh(self):
        _check(lib().cap_bvh_build(self.ctx), "cap_bvh_build")
        return self.bvh_info()

    def update_vertices(self, positions=None, normals=None, texcoords=None):
        """Replace vertex attributes of the uploaded scene (same topology); None keeps an array.  numpy arrays go in as host arrays,
        contiguous float32 torch tensors on this context's device as device pointers (after torch's current stream is synchronised).
        The trees are stale until refit_bvh() or build_bvh()."""
        ptrs, flags, keep = vertex_update_args(self._vertex_count, positions, normals, texcoords)
        if flags:
            import torch
            dev = torch.device("cuda", self.device)
            for a in keep:
                if a.device != dev:
                    raise CapError("update_vertices: tensors must be on %s, got %s" % (dev, a.device))
            torch.cuda.current_stream(dev).synchronize()  # the arrays were written on torch's stream
        _check(lib().cap_scene_update_vertices(self.ctx, ptrs[0], ptrs[1], ptrs[2], flags), "cap_scene_update_vertices")
        if positions is not None and self._scene_host is not None:
            kept = positions.reshape(-1, 3).copy() if isinstance(positions, np.ndarray) else positions.detach().reshape(-1, 3).clone()
            self._scene_host = (kept,) + self._scene_host[1:]

    def refit_bvh(self):
        """Refit the trees of the last build_bvh() to the current vertices; returns RefitInfo (ms, expected_node_visits,
        expected_node_visits_built)."""
        info = RefitInfo()
        _check(lib().cap_bvh_refit(self.ctx, C.byref(info)), "cap_bvh_refit")
        return info

    def bvh_info(self):
        bi = BvhInfo()
        _check(lib().cap_bvh_info(self.ctx, C.byref(bi)), "cap_bvh_info")
        return bi

    def bvh_readback(self):
        bi = self.bvh_info()
        nodes = np.zeros((bi.node_count, 16), np.float32)
        leaves = np.zeros(bi.triangle_count, np.uint32)
        _check(lib().cap_bvh_readback(self.ctx, _p(nodes), _p(leaves)), "cap_bvh_readback")
        return nodes, leaves

    # ---- view ----
    def bvh_wide_readback(self):
        """(wide nodes [count, 20] uint32, tri_src [triangles] uint32, depth, top) of the compressed 8-wide view."""
        info = np.zeros(3, np.uint32)
        _check(lib().cap_bvh_wide_readback(self.ctx, None, None, _p(info)), "cap_bvh_wide_readback")
        nodes = np.zeros((int(info[0]), 20), np.uint32)
        src = np.zeros(max(1, self.bvh_info().triangle_count), np.uint32)
        _check(lib().cap_bvh_wide_readback(self.ctx, _p(nodes), _p(src), _p(info)), "cap_bvh_wide_readback")
        return nodes, src[:self.bvh_info().triangle_count], int(info[1]), int(info[2])

    def bvh_wide_info(self):
        """(wide nodes, depth, leading top-level nodes) of the compressed 8-wide view, without reading it back."""
        info = np.zeros(3, np.uint32)
        _check(lib().cap_bvh_wide_readback(self.ctx, None, None, _p(info)), "cap_bvh_wide_readback")
        return int(info[0]), int(info[1]), int(info[2])

    def set_camera(self, cam):
        _check(lib().cap_camera_set(self.ctx, C.byref(cam)), "cap_camera_set")

    def set_prev_camera(self, cam):
        _check(lib().cap_prev_camera_set(self.ctx, C.byref(cam)), "cap_prev_camera_set")

    def set_resolution(self, width, height):
        _check(lib().cap_set_resolution(self.ctx, width, height), "cap_set_resolution")
        self.width, self.height = width, height

    def set_shard(self, index, count):
        _check(lib().cap_set_shard(self.ctx, index, count), "cap_set_shard")

    def set_traversal(self, mode):
        """0 auto, 1 LBVH + LDS stack, 2 exhaustive (small scenes)."""
        _check(lib().cap_set_traversal(self.ctx, mode), "cap_set_traversal")

    DEBUG_QUEUE_CAPACITY_DIV, DEBUG_WIDE_DEPTH_LIMIT, DEBUG_WIDE_IN_USE, DEBUG_FAIL_LANE1, DEBUG_LANES_USED = 1, 2, 3, 4, 5
    DEBUG_QUEUE_CANARY_FILL, DEBUG_QUEUE_CANARY_BEHIND, DEBUG_QUEUE_CANARY_USED, DEBUG_SELFTEST_DIV, DEBUG_NEE_PAIRS = 6, 7, 8, 9, 10
    DEBUG_SELFTEST_SHADE_UNARY, DEBUG_SELFTEST_SHADE_DIV2, DEBUG_SHADE_TAME = 11, 12, 13
    DEBUG_CAMERA_CULL = 14
    DEBUG_MARK_FORM = 15  # form << 8 | dense; form 0 none, 1 by id, 2 carry chain, 3 carry chain over two words
    DEBUG_SAMPLE_TABLE = 16  # 1: the last render's fused launches took the direction-sample terms from the per-batch table
    DEBUG_SELFTEST_SAMPLE_TABLE = 17  # mismatching entries << 32 | (bounce, slot) rows of the last batch's table compared
    DEBUG_CAMERA_TABLE = 18  # 1: the last render ran bounce 0 inside bounce 1's launch, from the per-batch table of camera vertices
    DEBUG_SELFTEST_CAMERA_TABLE = 19  # mismatching entries << 32 | jitter groups << 16 | frame slots of the last batch compared
    DEBUG_GRAY_ENTRIES = 20  # 1: the last render's fused launches used 32-byte extension entries (one throughput word)
    DEBUG_GROUP_WALK = 22  # slots per jitter group if the last batch's head kernel walked bounce 0's chunks group by group, 0: slot-major
    DEBUG_CAMERA_TABLE_REUSED = 23  # 1: the last batch found its camera-vertex table built from the same inputs and launched no builder
    DEBUG_SKY_PLANE = 24  # 1: the last render's fused launches stored the sky term into the sky plane and the resolve added it
    DEBUG_SKY_PLANE_NONZERO = 25  # after such a render: entries of the last batch's sky plane that are not +0 (its escapes at bounce >= 1)
    DEBUG_SELFTEST_GRAY = 21  # after a 48-byte render: entries with unequal throughput words << 32 | entries of the last batch's queues looked at

    def debug_set(self, key, value):
        _check(lib().cap_debug_set(self.ctx, key, value), "cap_debug_set")

    DEBUG_SWITCH_BASE = 64

    def debug_switch(self, name, value):
        """Sets one of the A/B switches of the context's table by its (environment-variable) name; value None = the product's choice."""
        i = lib().cap_debug_switch_index(name.encode())
        if i < 0:
            raise CapError("unknown switch %s" % name)
        self.debug_set(self.DEBUG_SWITCH_BASE + i, 0xFFFFFFFFFFFFFFFF if value is None else int(value))

    def debug_get(self, key):
        v = _u64()
        _check(lib().cap_debug_get(self.ctx, key, C.byref(v)), "cap_debug_get")
        return int(v.value)

    def set_batch_paths(self, n):
        _check(lib().cap_set_batch_paths(self.ctx, n), "cap_set_batch_paths")

    # ---- render ----
    def render(self, frame_begin, n_frames, num_bounces, flags=0):
        _check(lib().cap_render(self.ctx, frame_begin, n_frames, num_bounces, flags), "cap_render")

    def accum_reset(self):
        _check(lib().cap_accum_reset(self.ctx), "cap_accum_reset")

    def accum_import(self, sum_rgba, frames):
        """Continues a dumped accumulation: sum_rgba = readback(BUF_ACCUM_SUM) of the interrupted render, frames = its frame count."""
        a = np.ascontiguousarray(sum_rgba, np.float32)
        assert a.shape == (self.height, self.width, 4)
        _check(lib().cap_accum_import(self.ctx, _p(a), int(frames)), "cap_accum_import")

    def sync(self):
        _check(lib().cap_sync(self.ctx), "cap_sync")

    def readback(self, kind):
        if kind == BUF_INDIRECT_LOWRES:
            out = np.zeros((self.height // 2, self.width // 2, 4), np.float32)
        else:
            out = np.zeros((self.height, self.width, 4), np.float32)
        _check(lib().cap_readback(self.ctx, kind, _p(out)), "cap_readback")
        return out

    def stats(self):
        s = Stats()
        _check(lib().cap_stats_get(self.ctx, C.byref(s)), "cap_stats_get")
        return s

    def stats_reset(self):
        _check(lib().cap_stats_reset(self.ctx), "cap_stats_reset")

    # ---- ray flags and instance masks (CapTraceOptions: DXR RayFlags / InstanceInclusionMask) ----
    RAY_FLAG_ACCEPT_FIRST_HIT, RAY_FLAG_CULL_BACK_FACING, RAY_FLAG_CULL_FRONT_FACING = 0x04, 0x10, 0x20  # CAP_RAY_FLAG_*

    def set_instance_masks(self, masks):
        """One mask byte per mesh of the uploaded scene (cap_scene_set_instance_masks); None restores all 0xFF.  A triangle of mesh m
        is a candidate of a query iff masks[m] & mask != 0 (mask= of the trace_* calls, default 0xFF)."""
        if masks is None:
            _check(lib().cap_scene_set_instance_masks(self.ctx, None, len(self._tri_end)), "cap_scene_set_instance_masks")
            return
        m = np.ascontiguousarray(masks, np.uint8).reshape(-1)
        _check(lib().cap_scene_set_instance_masks(self.ctx, _p(m), m.size), "cap_scene_set_instance_masks")

    def trace_options(self, cull=None, mask=None, first_hit=False):
        """The CapTraceOptions of cull=None | "back" | "front", mask=None | 1..0xFF, first_hit; None when every argument is the
        default (the trace_* calls then take the plain entry points)."""
        if cull not in (None, "back", "front"):
            raise CapError('cull must be None, "back" or "front", got %r' % (cull,))
        if cull is None and mask is None and not first_hit:
            return None
        flags = {None: 0, "back": self.RAY_FLAG_CULL_BACK_FACING, "front": self.RAY_FLAG_CULL_FRONT_FACING}[cull]
        if first_hit:
            flags |= self.RAY_FLAG_ACCEPT_FIRST_HIT
        return TraceOptions(flags, 0 if mask is None else int(mask))

    # ---- queries: what the twelve wrappers below share ----
    MULTI_MAX_K, MULTI_CONTINUE = 16, 1  # CAP_MULTI_MAX_K, CAP_MULTI_CONTINUE

    def _stage_records(self, records, width, what):
        """(device, records on it, N) of a query's rays (width 8) or points (width 4), `what` the argument's name: a contiguous
        (N, width) float32 tensor as it is, a numpy array staged through torch"""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(records, np.ndarray):
            records = torch.from_numpy(np.ascontiguousarray(records, np.float32).reshape(-1, width)).to(dev)
        if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != width or not records.is_contiguous() or records.device != dev:
            raise CapError("%s must be a contiguous (N, %d) float32 tensor on %s, got %s %s on %s"
                           % (what, width, dev, records.dtype, tuple(records.shape), records.device))
        return dev, records, records.shape[0]

    def _out(self, out, shape, dtype, dev):
        """(the tensor of that shape and dtype a query writes, the caller's numpy array or None) of out=: a tensor is checked, a numpy
        array or None gets a new one"""
        host_out = None
        if isinstance(out, np.ndarray):
            host_out, out = out, None
        if out is None:
            import torch
            out = torch.empty(shape, dtype=dtype, device=dev)
        elif out.dtype != dtype or out.shape != shape or not out.is_contiguous() or out.device != dev:
            raise CapError("out must be a contiguous %s %s tensor on %s, got %s %s on %s" % (shape, dtype, dev, out.dtype, tuple(out.shape), out.device))
        return out, host_out

    def _resume_page(self, page, shape, dtype, dev, what):
        """(one page of a multi query on the device, the caller's numpy page or None): a new one without a page to resume from, a numpy
        page of the right size staged through torch, a tensor checked; `what` names the argument"""
        if page is None or isinstance(page, np.ndarray):
            import torch
            if page is None:
                return torch.empty(shape, dtype=dtype, device=dev), None
            if page.size == int(np.prod(shape)):
                return torch.from_numpy(np.ascontiguousarray(page, np.float32 if dtype == torch.float32 else np.int32).reshape(shape)).to(dev), page
        elif page.dtype == dtype and page.shape == shape and page.is_contiguous() and page.device == dev:
            return page, None
        raise CapError("%s must be the %s %s page of the previous call, a contiguous tensor on %s or a numpy array of its size, got %s %s"
                       % (what, shape, dtype, dev, page.dtype, tuple(page.shape)))

    def _page_size(self, k, counts, resuming):
        k = int(k)
        if not 0 <= k <= self.MULTI_MAX_K:
            raise CapError("k must be in 0 .. %d (page with resume=), got %d" % (self.MULTI_MAX_K, k))
        if k == 0 and (not counts or resuming):
            raise CapError("k = 0 counts only: pass counts=True and no resume")
        return k

    def _run(self, name, args, dev, sync, host, outputs, host_outputs):
        """The one path of every query.  With sync, waits for torch's stream; calls the entry point `name` on this context with args --
        a tensor goes as its pointer, a TraceOptions by reference, None as NULL, an integer or a C.c_float as it is --; waits for the context's
        stream with sync, and always before a read-back.  Returns the outputs as the caller gets them: the device tensors, or with
        host numpy copies, written into the caller's own array where host_outputs holds one"""
        if sync:
            import torch
            torch.cuda.current_stream(dev).synchronize()  # the inputs (and the outputs' allocations) were made on torch's stream
        _check(getattr(lib(), name)(self.ctx, *[a if a is None or type(a) in (int, C.c_float) else C.byref(a) if type(a) is TraceOptions
                                                else C.c_void_p(a.data_ptr()) for a in args]), name)
        if sync or host:
            self.sync()
        if not host:
            return outputs
        res = []
        for out, mine in zip(outputs, host_outputs):
            h = out.cpu().numpy()
            if mine is not None:
                mine[...] = h.reshape(mine.shape)
                h = mine
            res.append(h)
        return res

    def _single(self, name, records, width, what, out, cols, dtype, sync, tail, second=()):
        """One result per ray or point through the entry point `name`: out= is the (N, cols) array of `dtype` it writes ((N,) with
        cols = 0), `second` the dtypes of the (N,) arrays it fills behind that, `tail` its arguments behind those.  Returns the first
        array alone without `second`, else the tuple of all"""
        host = isinstance(records, np.ndarray)  # then the results are read back to the host, which needs the sync
        dev, records, n = self._stage_records(records, width, what)
        out, host_out = self._out(out, (n, cols) if cols else (n,), dtype, dev)
        extra = [out.new_empty((n,), dtype=t) for t in second]
        res = self._run(name, (records, n, out, *extra, *tail), dev, sync or host, host or host_out is not None,
                        [out] + extra, [host_out] + [None] * len(extra))
        return tuple(res) if second else res[0]

    def _multi(self, name, records, width, what, cols, instanced, k, counts, resume, sync, tail):
        """Up to k results per ray, point or box through the entry point `name`: a page of (N, k, cols) float32 records (cols = 0: of
        (N, k) int32 ids) and, instanced, one of (N, k) int32 instances -- resume= is the previous call's page or, instanced, pair of
        pages --, then the (N,) int32 counts with counts=True; `tail` is what the entry point takes behind the multi flags.  Returns
        the page alone where there is nothing else, else the tuple"""
        import torch
        if not instanced:
            given, names = [resume], ("resume",)
        elif resume is None or (isinstance(resume, (tuple, list)) and len(resume) == 2):
            given, names = [None, None] if resume is None else list(resume), ("resume[0]", "resume[1]")
        else:
            raise CapError("resume must be the (records, instances) pair of pages of the previous call")
        host = isinstance(records, np.ndarray)  # numpy rays or points, or a numpy page: read back to the host, which needs the sync
        dev, records, n = self._stage_records(records, width, what)
        k = self._page_size(k, counts, resume is not None)
        pages, host_pages = [], []
        first = ((n, k, cols), torch.float32) if cols else ((n, k), torch.int32)
        for page, page_name, (shape, dtype) in zip(given, names, (first, ((n, k), torch.int32))):
            page, mine = self._resume_page(page, shape, dtype, dev, page_name)
            pages.append(page)
            host_pages.append(mine)
            host = host or mine is not None
        cnt = [torch.empty((n,), dtype=torch.int32, device=dev)] if counts else []
        res = self._run(name, (records, n, k, *(pages if k else [None] * len(pages)), cnt[0] if counts else None,
                               self.MULTI_CONTINUE if resume is not None else 0, *tail),
                        dev, sync or host, host, pages + cnt, host_pages + [None])
        return tuple(res) if instanced or counts else res[0]

    @staticmethod
    def _plain_or_ex(name, options, plain_tail):
        """(entry point, its last arguments) of the three ray queries that have a plain form: that form with plain_tail when every
        option is at its default, else the _ex form with the options"""
        return (name, plain_tail) if options is None else (name + "_ex", (options,))

    # ---- ray queries (cap_trace_rays / cap_trace_occlusion) ----
    def trace_rays(self, rays, out=None, sync=True, cull=None, mask=None, first_hit=False):
        """Closest hit of each ray.  rays: (N, 8) float32 = CapRayDesc rows (origin, tmin, direction, tmax), a contiguous torch tensor
        on this context's device or a numpy array (staged through torch; the hits come back as numpy).  Returns (N, 4) float32 hit
        records (t, u, v, triangle id bits: hit_triangles() reads them).  sync=True orders the call against torch's current stream
        (waits for it before the launch) and waits for the context's stream before returning: right for a renderer on a stream of its
        own.  sync=False only enqueues, on the context's stream: for a renderer created on torch's stream (as bench.py creates it).
        cull="back" | "front" drops the triangles facing away from / towards the ray, mask= is the instance inclusion mask
        (set_instance_masks), first_hit=True returns some hit instead of the closest (cap_trace_rays_ex)."""
        import torch
        name, tail = self._plain_or_ex("cap_trace_rays", self.trace_options(cull, mask, first_hit), (0,))
        return self._single(name, rays, 8, "rays", out, 4, torch.float32, sync, tail)

    def trace_occlusion(self, rays, out=None, sync=True, cull=None, mask=None):
        """1 where some triangle occludes the ray's open interval (tmin, tmax), else 0: (N,) int32.  Arguments as trace_rays."""
        import torch
        name, tail = self._plain_or_ex("cap_trace_occlusion", self.trace_options(cull, mask), (0,))
        return self._single(name, rays, 8, "rays", out, 0, torch.int32, sync, tail)

    # ---- closest-point queries (cap_closest_points) ----
    def _closest_single(self, name, points, out, sync, mask, second=()):
        """One (N, 8) float32 record per point through the entry point `name`, and an (N,) array of each dtype in `second` behind it"""
        import torch
        return self._single(name, points, 4, "points", out, 8, torch.float32, sync, (self.trace_options(None, mask),), second)

    def closest_points(self, points, out=None, sync=True, mask=None):
        """The triangle nearest to each point within its radius.  points: (N, 4) float32 = CapPointDesc rows (x, y, z, radius; +inf:
        unbounded), a contiguous torch tensor on this context's device or a numpy array (staged through torch; the records come back as
        numpy).  Returns (N, 8) float32 CapClosest records (closest point, dist2, u, v, triangle and feature bits: closest_triangles()
        reads those); a miss is (0, 0, 0, radius^2, 0, 0, MISS, 0).  mask= is the instance inclusion mask (set_instance_masks).  sync as
        trace_rays."""
        return self._closest_single("cap_closest_points", points, out, sync, mask)

    # ---- sphere sweep queries (cap_sweep_spheres) ----
    def sweep_spheres(self, sweeps, out=None, sync=True, mask=None):
        """The first contact of each moving sphere with the scene.  sweeps: (N, 8) float32 = CapSweepDesc rows (origin, radius,
        direction, tmax; sweep_queries() packs them), a contiguous torch tensor on this context's device or a numpy array (staged
        through torch; the records come back as numpy).  Returns (N, 8) float32 CapSweepHit records: the contact point on the triangle,
        the time t of first contact in units of the direction, u, v, and the triangle and feature bits -- CapClosest's layout, so
        closest_triangles() reads those; a miss is (0, 0, 0, tmax, 0, 0, MISS, 0).  The centre at contact is origin + t * direction,
        the contact normal points from the contact point to it.  mask= is the instance inclusion mask (set_instance_masks).  sync as
        trace_rays."""
        import torch
        return self._single("cap_sweep_spheres", sweeps, 8, "sweeps", out, 8, torch.float32, sync, (self.trace_options(None, mask),))

    def sweep_instances(self, sweeps, out=None, sync=True, mask=None):
        """The first contact of each moving sphere with the instance table, in WORLD space (cap_sweep_instances): (records (N, 8)
        float32, instances (N,) int32, -1 on a miss).  The records are sweep_spheres' -- world-space contact point, the time t, (u, v),
        the scene's triangle id and the feature: closest_triangles() reads those; the winner is minimal in (t, instance, triangle).
        Needs set_instances().  sweeps, out, sync and mask= as sweep_spheres; numpy sweeps give numpy results."""
        import torch
        return self._single("cap_sweep_instances", sweeps, 8, "sweeps", out, 8, torch.float32, sync, (self.trace_options(None, mask),), (torch.int32,))

    @staticmethod
    def sweep_queries(origin, radius, direction, tmax=np.inf):
        """(N, 8) float32 CapSweepDesc rows of (N, 3) origins and directions; radius and tmax are scalars or N values"""
        o = np.asarray(origin, np.float32).reshape(-1, 3)
        q = np.zeros((len(o), 8), np.float32)
        q[:, 0:3], q[:, 3], q[:, 4:7], q[:, 7] = o, radius, np.asarray(direction, np.float32).reshape(-1, 3), tmax
        return q

    # ---- signed distance (cap_pseudonormals_*, cap_signed_distance) ----
    def build_pseudonormals(self):
        """Build the angle-weighted pseudonormal table of the scene (cap_pseudonormals_build) and return its PseudonormalsInfo.  Needs
        a built tree; build_bvh() and refit_bvh() keep an existing table current."""
        info = PseudonormalsInfo()
        _check(lib().cap_pseudonormals_build(self.ctx, C.byref(info)), "cap_pseudonormals_build")
        return info

    def drop_pseudonormals(self):
        _check(lib().cap_pseudonormals_drop(self.ctx), "cap_pseudonormals_drop")

    def pseudonormals(self):
        """The table as a (T, 7, 3) float32 array: per global triangle id the unnormalised pseudonormals of the face, the edges v0v1,
        v1v2, v2v0 and the vertices v0, v1, v2 (the FEATURE_* order)."""
        table = np.zeros((int(self._tri_end[-1]) if len(self._tri_end) else 0, 7, 3), np.float32)
        _check(lib().cap_pseudonormals_readback(self.ctx, _p(table)), "cap_pseudonormals_readback")
        return table

    def signed_distance(self, points, out=None, sync=True, mask=None, sign="pseudonormal", beta=2.0):
        """closest_points with the signed distance (cap_signed_distance): (records (N, 8) float32, signed (N,) float32).  The records
        are closest_points', bit for bit; signed is -sqrt(dist2) where the point lies behind the pseudonormal of the feature the record
        reports, +sqrt(dist2) otherwise, +inf on a miss.  Needs build_pseudonormals().  points, out, sync and mask= as closest_points;
        numpy points give numpy results.
        sign="winding" takes the sign from the winding number instead, for meshes that are not closed: the same two arrays, signed
        negative exactly where winding_numbers(points, beta) >= 1/2, composed on the device from the two calls.  Needs build_winding()
        as well, and takes no mask= (the winding number covers every triangle)."""
        import torch
        if sign == "pseudonormal":
            return self._closest_single("cap_signed_distance", points, out, sync, mask, (torch.float32,))
        if sign != "winding":
            raise CapError('sign must be "pseudonormal" or "winding", got %r' % (sign,))
        if mask is not None:
            raise CapError('sign="winding" takes no mask=: the winding number covers every triangle')
        host = isinstance(points, np.ndarray)
        dev, pts, n = self._stage_records(points, 4, "points")
        rec, host_out = self._out(out, (n, 8), torch.float32, dev)
        rec, signed = self._closest_single("cap_signed_distance", pts, rec, sync or host, None, (torch.float32,))
        w = self.winding_numbers(pts, beta=beta, sync=sync or host)
        signed = torch.where(w >= 0.5, -signed.abs(), signed.abs())
        if not (host or host_out is not None):
            return rec, signed
        h = rec.cpu().numpy()
        if host_out is not None:
            host_out[...] = h.reshape(host_out.shape)
            h = host_out
        return h, signed.cpu().numpy()

    # ---- winding numbers (cap_winding_*, cap_winding_numbers) ----
    def build_winding(self):
        """Build the dipole table of the scene's binary tree (cap_winding_build) and return its WindingInfo.  Needs a built tree;
        build_bvh() and refit_bvh() keep an existing table current."""
        info = WindingInfo()
        _check(lib().cap_winding_build(self.ctx, C.byref(info)), "cap_winding_build")
        return info

    def drop_winding(self):
        _check(lib().cap_winding_drop(self.ctx), "cap_winding_drop")

    def winding_table(self):
        """The table as an (inner nodes, 2, 8) float32 array, indexed as bvh_readback()'s nodes: per child slot the centroid p~, the
        radius r, the normal sum N and the child's traversal code (bits: view as uint32)."""
        table = np.zeros((max(self.bvh_info().triangle_count, 1) - 1, 2, 8), np.float32)
        _check(lib().cap_winding_readback(self.ctx, _p(table)), "cap_winding_readback")
        return table

    def winding_numbers(self, points, beta=2.0, out=None, visits=False, sync=True):
        """The generalised winding number of the scene about each point (cap_winding_numbers): (N,) float32, 1 inside and 0 outside a
        closed mesh wound outwards, in between near holes; w >= 1/2 is the robust inside test.  Subtrees farther than beta x their
        radius are replaced by their dipole: beta >= 1, larger is more exact and slower, inf sums every triangle exactly.
        visits=True also returns an (N, 2) int32 array: the dipole terms and the exact triangle terms each walk added.  Needs
        build_winding().  points (the radius column is not read), out and sync as closest_points; numpy points give numpy results."""
        return self._winding("cap_winding_numbers", 2, points, beta, out, visits, sync)

    def _winding(self, name, width, points, beta, out, visits, sync):
        """winding_numbers and winding_instances: (N,) float32 through the entry point `name`, with an (N, width) int32 visits array"""
        import torch
        host = isinstance(points, np.ndarray)  # then the results are read back to the host, which needs the sync
        dev, points, n = self._stage_records(points, 4, "points")
        out, host_out = self._out(out, (n,), torch.float32, dev)
        vis = [torch.empty((n, width), dtype=torch.int32, device=dev)] if visits else []
        res = self._run(name, (points, n, C.c_float(beta), out, vis[0] if visits else None), dev, sync or host,
                        host or host_out is not None, [out] + vis, [host_out, None])
        return tuple(res) if visits else res[0]

    def winding_instances(self, points, beta=2.0, out=None, visits=False, sync=True):
        """The generalised winding number of the instanced scene about each WORLD point (cap_winding_instances): (N,) float32, the
        winding number of the scene flattened through the instance transforms -- 1 inside a closed part, a mirrored one included, 2
        where two parts overlap, in between near holes; w >= 1/2 is the robust inside test.  An instance with mask 0 is switched off.
        beta as winding_numbers.  visits=True also returns an (N, 4) int32 array: the dipole terms taken at the top level, the
        instances entered, the dipole terms below instances and the exact triangle terms.  Needs set_instances() and build_winding();
        the tables it derives from them are rebuilt on the stream when either changed.  points, out and sync as winding_numbers."""
        return self._winding("cap_winding_instances", 4, points, beta, out, visits, sync)

    def winding_instances_info(self):
        """The WindingInstancesInfo of the derived tables (cap_winding_instances_info); never builds them."""
        info = WindingInstancesInfo()
        _check(lib().cap_winding_instances_info(self.ctx, C.byref(info)), "cap_winding_instances_info")
        return info

    def winding_instances_tables(self):
        """(top (entries, 8), inst (N, 12), forest (forest nodes, 2, 8)) float32 of cap_winding_instances_readback, built first when
        they are not current: per top-level entry (p~_w, r, N_w, word 7: the instance at level 0; r = -1: empty), in the tree's
        layout (winding_instances_info().level_entries); per instance L row-major, |det L|, sigma, s; and with an object table the
        forest's dipole table, indexed as objects_readback()'s nodes (without one the objects' table is winding_table())."""
        info = self.winding_instances_info()
        nodes = sum(int(o["triangle_count"]) - 1 for o in self.objects_info())
        top, inst, forest = np.zeros((info.entries, 8), np.float32), np.zeros((info.instances, 12), np.float32), np.zeros((nodes, 2, 8), np.float32)
        _check(lib().cap_winding_instances_readback(self.ctx, _p(top), _p(inst), _p(forest) if nodes else None), "cap_winding_instances_readback")
        return top, inst, forest

    def objects_readback(self):
        """(nodes (forest nodes, 16) float32, leaf triangles (forest records,) uint32) of the object table's forest (cap_objects_readback),
        as bvh_readback() gives the scene's tree: object k's nodes and records follow object k - 1's, child codes number the forest."""
        info = self.objects_info()
        nodes = np.zeros((sum(int(o["triangle_count"]) - 1 for o in info), 16), np.float32)
        leaves = np.zeros(sum(int(o["triangle_count"]) for o in info), np.uint32)
        _check(lib().cap_objects_readback(self.ctx, _p(nodes) if len(nodes) else None, _p(leaves) if len(leaves) else None), "cap_objects_readback")
        return nodes, leaves

    def closest_instances(self, points, out=None, sync=True, mask=None):
        """The (instance, triangle) nearest to each point in WORLD space over the instance table (cap_closest_instances): (records
        (N, 8) float32, instances (N,) int32, -1 on a miss).  The records are closest_points' -- world-space closest point and dist2,
        (u, v), the scene's triangle id and the feature: closest_triangles() reads those.  points, out, sync and mask= as
        closest_points; numpy points give numpy results."""
        import torch
        return self._closest_single("cap_closest_instances", points, out, sync, mask, (torch.int32,))

    def signed_distance_instances(self, points, out=None, sync=True, mask=None, sign="pseudonormal", beta=2.0):
        """closest_instances with the signed distance (cap_signed_distance_instances): (records (N, 8) float32, instances (N,) int32,
        -1 on a miss, signed (N,) float32).  Records and instances are closest_instances', bit for bit; signed is the WORLD distance
        sqrt(dist2), negative where the point's object-space image W p lies behind the pseudonormal of the feature nearest to it on
        the winning instance's object, +inf on a miss.  Needs set_instances() and build_pseudonormals().  points, out, sync and mask=
        as closest_instances; numpy points give numpy results.
        sign="winding" takes the sign from the winding number over the instances instead, for parts that are not closed or are
        mirrored: the same three arrays, signed negative exactly where winding_instances(points, beta) >= 1/2, composed on the device
        from the two calls.  Needs build_winding() as well, and takes no mask=."""
        import torch
        if sign == "pseudonormal":
            return self._closest_single("cap_signed_distance_instances", points, out, sync, mask, (torch.int32, torch.float32))
        if sign != "winding":
            raise CapError('sign must be "pseudonormal" or "winding", got %r' % (sign,))
        if mask is not None:
            raise CapError('sign="winding" takes no mask=: the winding number covers every triangle')
        host = isinstance(points, np.ndarray)
        dev, pts, n = self._stage_records(points, 4, "points")
        rec, host_out = self._out(out, (n, 8), torch.float32, dev)
        rec, inst, signed = self._closest_single("cap_signed_distance_instances", pts, rec, sync or host, None, (torch.int32, torch.float32))
        w = self.winding_instances(pts, beta=beta, sync=sync or host)
        signed = torch.where(w >= 0.5, -signed.abs(), signed.abs())
        if not (host or host_out is not None):
            return rec, inst, signed
        h = rec.cpu().numpy()
        if host_out is not None:
            host_out[...] = h.reshape(host_out.shape)
            h = host_out
        return h, inst.cpu().numpy(), signed.cpu().numpy()

    def closest_points_multi(self, points, k, counts=False, resume=None, sync=True, mask=None):
        """The k triangles nearest to each point within its radius, in (dist2, triangle) order (cap_closest_points_multi): (N, k, 8)
        float32 records as closest_points writes them, miss records (0, 0, 0, radius^2, 0, 0, MISS, 0) after a point's last candidate;
        closest_triangles() reads the (N, k) ids and features.  counts=True also returns the number of ALL candidates per point, (N,)
        int32, and turns off pruning by the k-th distance (k = 0: counts only, the records are (N, 0, 8)).  resume=<previous page> (the
        (N, k, 8) result of a call with the same points) continues after it with CAP_MULTI_CONTINUE, writes the next page over it and
        returns it.  points, sync and mask= as closest_points; numpy points (or a numpy resume page) give numpy results."""
        return self._multi("cap_closest_points_multi", points, 4, "points", 8, False, k, counts, resume, sync, (self.trace_options(None, mask),))

    def closest_instances_multi(self, points, k, counts=False, resume=None, sync=True, mask=None):
        """The k (instance, triangle) pairs nearest to each point in WORLD space within its radius, in (dist2, instance, triangle) order
        (cap_closest_instances_multi): (records (N, k, 8) float32 as closest_instances writes them, instances (N, k) int32, -1 in the
        miss slots after a point's last pair[, counts (N,) int32 = the number of ALL candidate pairs per point with counts=True, which
        turns off pruning by the k-th distance]).  k = 0: counts only, the records are (N, 0, 8) and the instances (N, 0).
        resume=(records, instances) of the previous call with the same points continues after it with CAP_MULTI_CONTINUE and writes the
        next pages over both.  closest_triangles() reads the (N, k) ids and features.  points, sync and mask= as closest_points; numpy
        points (or numpy resume pages) give numpy results."""
        return self._multi("cap_closest_instances_multi", points, 4, "points", 8, True, k, counts, resume, sync, (self.trace_options(None, mask),))

    # ---- box overlap queries (cap_overlap_boxes) ----
    def overlap_boxes(self, boxes, k, counts=False, resume=None, sync=True, mask=None):
        """The triangles that meet each closed axis-aligned box, the first k by triangle id (cap_overlap_boxes).  boxes: (N, 8) float32
        = CapBoxDesc rows (lo, -, hi, -; columns 3 and 7 are not read), a contiguous torch tensor on this context's device or a numpy
        array (staged through torch; the results come back as numpy).  Returns (N, k) int32 ids, -1 in the slots after a box's last
        triangle.  counts=True also returns the number of ALL triangles that meet each box, (N,) int32 (k = 0: counts only, the ids are
        (N, 0)).  resume=<previous page> (the (N, k) result of a call with the same boxes) continues after it with CAP_MULTI_CONTINUE,
        writes the next page over it and returns it.  sync and mask= as closest_points."""
        return self._multi("cap_overlap_boxes", boxes, 8, "boxes", 0, False, k, counts, resume, sync, (self.trace_options(None, mask),))

    def overlap_instances(self, boxes, k, counts=False, resume=None, sync=True, mask=None):
        """The (instance, triangle) pairs whose world-space triangle meets each closed axis-aligned WORLD-space box, the first k in
        (instance, triangle) order (cap_overlap_instances): (triangles (N, k) int32, instances (N, k) int32[, counts (N,) int32 = the
        number of ALL pairs of each box with counts=True]), -1 in the slots after a box's last pair.  k = 0: counts only, both pages
        are (N, 0).  resume=(triangles, instances) of the previous call with the same boxes continues after it with
        CAP_MULTI_CONTINUE and writes the next pages over both.  Needs set_instances().  boxes, sync and mask= as overlap_boxes."""
        return self._multi("cap_overlap_instances", boxes, 8, "boxes", 0, True, k, counts, resume, sync, (self.trace_options(None, mask),))

    # ---- triangle overlap queries (cap_overlap_triangles) ----
    def overlap_triangles(self, tris, k, counts=False, resume=None, sync=True, mask=None):
        """The scene triangles that meet each query triangle, the first k by triangle id (cap_overlap_triangles).  tris: (N, 12) float32
        = CapTriangleDesc rows (a, skip, b, -, c, -): column 3 carries the BITS of `skip`, the global id of a scene triangle that is no
        candidate (0xFFFFFFFF: none); columns 7 and 11 are not read.  triangle_queries() packs them, scene_triangle_queries() makes
        them of the scene's own triangles.  A contiguous torch tensor on this context's device or a numpy array (staged through torch;
        the results come back as numpy).  The return value, counts=, resume=, sync and mask= are overlap_boxes'."""
        return self._multi("cap_overlap_triangles", tris, 12, "tris", 0, False, k, counts, resume, sync, (self.trace_options(None, mask),))

    def overlap_triangles_instances(self, tris, k, counts=False, resume=None, sync=True, mask=None):
        """The (instance, triangle) pairs whose world-space triangle meets each WORLD-space query triangle, the first k in (instance,
        triangle) order (cap_overlap_triangles_instances).  tris: (N, 12) float32 CapTriangleDesc rows as overlap_triangles', with
        column 7 carrying the BITS of `skip_instance`: the pair (skip_instance, skip) is no candidate (skip = 0xFFFFFFFF: nothing is
        skipped).  triangle_queries() packs them, instance_triangle_queries() makes them of the placed scene's own triangles.  The
        return value, counts=, resume=, sync and mask= are overlap_instances'.  Needs set_instances()."""
        return self._multi("cap_overlap_triangles_instances", tris, 12, "tris", 0, True, k, counts, resume, sync, (self.trace_options(None, mask),))

    @staticmethod
    def triangle_queries(a, b, c, skip=None, skip_instance=None):
        """(N, 12) float32 CapTriangleDesc rows of (N, 3) vertices a, b, c; skip: None (0xFFFFFFFF: nothing is skipped) or N global
        triangle ids, whose bits go into column 3; skip_instance: None (column 7 stays 0) or N instance indices, whose bits go into
        column 7 -- read by overlap_triangles_instances alone.  The last pad column holds 0."""
        a, b, c = (np.asarray(x, np.float32).reshape(-1, 3) for x in (a, b, c))
        if not len(a) == len(b) == len(c):
            raise CapError("triangle_queries: a, b and c must have one row per triangle, got %d, %d and %d" % (len(a), len(b), len(c)))
        q = np.zeros((len(a), 12), np.float32)
        q[:, 0:3], q[:, 4:7], q[:, 8:11] = a, b, c
        ids = np.full(len(a), 0xFFFFFFFF, np.uint32) if skip is None else np.asarray(skip, np.int64).astype(np.uint32).reshape(-1)
        if len(ids) != len(a):
            raise CapError("triangle_queries: skip must hold one id per triangle, got %d for %d" % (len(ids), len(a)))
        q.view(np.uint32)[:, 3] = ids
        if skip_instance is not None:
            inst = np.asarray(skip_instance, np.int64).astype(np.uint32).reshape(-1)
            if len(inst) != len(a):
                raise CapError("triangle_queries: skip_instance must hold one index per triangle, got %d for %d" % (len(inst), len(a)))
            q.view(np.uint32)[:, 7] = inst
        return q

    def instance_triangle_queries(self, transforms, instances, ids):
        """The (N, 12) float32 query rows of the scene's triangles `ids` (global ids) as placed by transforms[instances] ((I, 3, 4)
        object-to-world, as given to set_instances): the vertices of the WORLD record of cap_closest_instances -- v0w,
        fl(v0w + e1w), fl(v0w + e2w), in float32 by the contract's arithmetic -- with the skip pair set to (instance, id): the
        starting point of a self-contact test of an assembly with overlap_triangles_instances."""
        f32 = np.float32
        M = np.asarray(transforms, f32).reshape(-1, 3, 4)
        inst = np.asarray(instances, np.int64).reshape(-1)
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(inst) != len(ids):
            raise CapError("instance_triangle_queries: one instance per id, got %d for %d" % (len(inst), len(ids)))
        if len(inst) and (inst.min() < 0 or inst.max() >= len(M)):
            raise CapError("instance_triangle_queries: instances must be in 0 .. %d" % (len(M) - 1))
        q = self.scene_triangle_queries(ids)
        v0, e1, e2 = q[:, 0:3], q[:, 4:7] - q[:, 0:3], q[:, 8:11] - q[:, 0:3]  # the stored record: e = fl(v - v0)
        m = M[inst]
        with np.errstate(all="ignore"):
            dot = lambda r, v: (m[:, r, 0] * v[:, 0] + m[:, r, 1] * v[:, 1]) + m[:, r, 2] * v[:, 2]
            v0w = np.stack([dot(r, v0) + m[:, r, 3] for r in range(3)], -1)
            e1w, e2w = np.stack([dot(r, e1) for r in range(3)], -1), np.stack([dot(r, e2) for r in range(3)], -1)
            assert v0w.dtype == f32 and e1w.dtype == f32
            return self.triangle_queries(v0w, v0w + e1w, v0w + e2w, ids, inst)

    def scene_triangle_queries(self, ids):
        """The (N, 12) float32 query rows of the scene's own triangles `ids` (global ids): the vertices as uploaded (or as last
        updated), with `skip` set to the triangle's own id -- the starting point of a self-intersection test.  A triangle that shares
        a vertex or an edge with the query touches it and is listed: filtering adjacency out is the caller's job."""
        if self._scene_host is None:
            raise CapError("scene_triangle_queries: no scene uploaded")
        pos, idx, meshes = self._scene_host
        if not isinstance(pos, np.ndarray):  # the device tensor of the last update_vertices
            pos = pos.cpu().numpy()
        ids = np.asarray(ids, np.int64).reshape(-1)
        total = int(self._tri_end[-1]) if len(self._tri_end) else 0
        if len(ids) and (ids.min() < 0 or ids.max() >= total):
            raise CapError("scene_triangle_queries: ids must be in 0 .. %d" % (total - 1))
        mesh = np.searchsorted(self._tri_end, ids, side="right")
        first = np.concatenate([[0], self._tri_end[:-1]])[mesh] if len(ids) else ids
        at = meshes[mesh, 3].astype(np.int64)[:, None] + 3 * (ids - first)[:, None] + np.arange(3)
        v = pos[meshes[mesh, 1].astype(np.int64)[:, None] + idx[at].astype(np.int64)]
        return self.triangle_queries(v[:, 0], v[:, 1], v[:, 2], ids)

    def _cell_boxes(self, origin, cell, dims):
        """(dims, the (nx * ny * nz, 8) float32 CapBoxDesc rows of the grid's cells on this context's device): per axis cell i spans
        lo = fl(origin + fl(i * cell)) to hi = fl(origin + fl((i + 1) * cell)) in float32, so neighbours share their faces exactly"""
        import torch
        dev = torch.device("cuda", self.device)
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise CapError("dims must be three positive cell counts, got %r" % (dims,))
        origin = [float(o) for o in origin]
        if len(origin) != 3:
            raise CapError("origin must be three coordinates, got %r" % (origin,))
        step = torch.tensor(float(cell), dtype=torch.float32, device=dev)
        boxes = torch.zeros(dims + (8,), dtype=torch.float32, device=dev)
        for axis, d in enumerate(dims):
            o = torch.tensor(origin[axis], dtype=torch.float32, device=dev)
            edges = o + torch.arange(d + 1, dtype=torch.float32, device=dev) * step  # (one rounded product, one rounded sum)
            shape = [1, 1, 1]
            shape[axis] = d
            boxes[..., axis] = edges[:-1].reshape(shape)
            boxes[..., 4 + axis] = edges[1:].reshape(shape)
        return dims, boxes.reshape(-1, 8)

    def voxel_occupancy(self, origin, cell, dims, mask=None):
        """Surface voxelisation: the number of triangles that meet each cell of the grid of dims = (nx, ny, nz) cubes of edge `cell`
        from `origin`, as a (nx, ny, nz) int32 tensor on this context's device (cap_overlap_boxes, counts only).  Per axis cell i spans
        lo = fl(origin + fl(i * cell)) to hi = fl(origin + fl((i + 1) * cell)) in float32, so neighbours share their faces exactly and
        a triangle lying in a shared face counts in both cells."""
        dims, boxes = self._cell_boxes(origin, cell, dims)
        _, cnt = self.overlap_boxes(boxes, 0, counts=True, mask=mask)
        return cnt.reshape(dims)

    def voxel_occupancy_instances(self, origin, cell, dims, mask=None):
        """voxel_occupancy over the instance table: the number of (instance, triangle) pairs whose world-space triangle meets each cell
        of the same grid, in world space (cap_overlap_instances, counts only).  Needs set_instances()."""
        dims, boxes = self._cell_boxes(origin, cell, dims)
        _, _, cnt = self.overlap_instances(boxes, 0, counts=True, mask=mask)
        return cnt.reshape(dims)

    # ---- instanced ray queries (cap_instances_set, cap_trace_instances*) ----
    def set_objects(self, ranges):
        """Installs the object table (cap_objects_set): ranges is (K, 2) (first_mesh, mesh_count) rows, disjoint mesh ranges of the
        uploaded scene, each built into a tree of its own; None or an empty list removes the table.  Drops the instance table: call
        set_instances(..., objects=...) afterwards.  Returns the CapObjectsInfo (count, triangles, nodes, max_depth, ms)."""
        info = ObjectsInfo()
        r = np.zeros((0, 2), np.uint32) if ranges is None else np.ascontiguousarray(ranges, np.uint32).reshape(-1, 2)
        _check(lib().cap_objects_set(self.ctx, _p(r) if len(r) else None, len(r), C.byref(info)), "cap_objects_set")
        self._instances_n = 0
        return info

    def objects_info(self):
        """One OBJECT_INFO_DTYPE record per object of the installed table (cap_objects_info): triangle range, node count, depth, exact
        bounds and the builder that made its tree; empty without a table."""
        n = C.c_uint32(0)
        _check(lib().cap_objects_info(self.ctx, None, 0, C.byref(n)), "cap_objects_info")
        out = np.zeros(n.value, OBJECT_INFO_DTYPE)
        if n.value:
            _check(lib().cap_objects_info(self.ctx, _p(out), n.value, None), "cap_objects_info")
        return out

    def set_instances(self, transforms, masks=None, sync=True, objects=None):
        """Installs N instances of the uploaded scene (cap_instances_set) and builds the top-level tree; None removes the table.
        objects: N object indices into the table set_objects installed (cap_instances_set_ex) -- a numpy array with numpy transforms, a
        tensor on the device with device transforms; None shows object 0 (without an object table: the whole scene).
        transforms: (N, 3, 4) or (N, 12) float32 object-to-world matrices, row-major -- a numpy array (host path), or a torch tensor on
        this context's device: then the 64-byte descriptors are assembled on the device and the call takes CAP_INSTANCES_DEVICE, nothing
        goes through the host.  masks: N values 0..0xFF, default 0xFF.  sync as trace_rays (the device path with sync=False only
        enqueues and returns None).  Returns the CapInstancesInfo (count, inert, tlas_nodes, tlas_depth, ms)."""
        info = InstancesInfo()
        if transforms is None:
            _check(lib().cap_instances_set(self.ctx, None, 0, 0, C.byref(info)), "cap_instances_set")
            self._instances_n = 0
            return info
        if isinstance(transforms, np.ndarray) or not hasattr(transforms, "device"):
            t = np.ascontiguousarray(transforms, np.float32)
            if t.ndim < 2 or t.size != t.shape[0] * 12:
                raise CapError("transforms must be (N, 3, 4) or (N, 12), got %s" % (t.shape,))
            d = np.zeros(t.shape[0], INSTANCE_DESC_DTYPE)
            d["transform"] = t.reshape(-1, 12)
            d["mask"] = 0xFF if masks is None else np.asarray(masks).astype(np.uint32).reshape(-1)
            if objects is None:
                _check(lib().cap_instances_set(self.ctx, _p(d), d.shape[0], 0, C.byref(info)), "cap_instances_set")
            else:
                o = np.ascontiguousarray(np.asarray(objects).astype(np.uint32).reshape(-1))
                if o.size != d.shape[0]:
                    raise CapError("objects must hold one index per instance (%d), got %d" % (d.shape[0], o.size))
                _check(lib().cap_instances_set_ex(self.ctx, _p(d), _p(o), d.shape[0], 0, C.byref(info)), "cap_instances_set_ex")
            self._instances_n = d.shape[0]
            return info
        import torch
        dev = torch.device("cuda", self.device)
        if transforms.dtype != torch.float32 or transforms.device != dev or transforms.numel() != transforms.shape[0] * 12:
            raise CapError("transforms must be an (N, 3, 4) or (N, 12) float32 tensor on %s" % (dev,))
        n = transforms.shape[0]
        d = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        d[:, :12] = transforms.reshape(n, 12)
        m = torch.full((n,), 0xFF, dtype=torch.int32, device=dev) if masks is None else torch.as_tensor(masks, device=dev).to(torch.int32).reshape(n)
        d[:, 12] = m.view(torch.float32)
        o = None
        if objects is not None:
            o = torch.as_tensor(objects, device=dev).to(torch.int32).reshape(n).contiguous()
        if sync:
            torch.cuda.current_stream(dev).synchronize()  # the descriptors were written on torch's stream
        if o is None:
            _check(lib().cap_instances_set(self.ctx, C.c_void_p(d.data_ptr()), n, INSTANCES_DEVICE, C.byref(info) if sync else None), "cap_instances_set")
        else:
            _check(lib().cap_instances_set_ex(self.ctx, C.c_void_p(d.data_ptr()), C.c_void_p(o.data_ptr()), n, INSTANCES_DEVICE,
                                              C.byref(info) if sync else None), "cap_instances_set_ex")
        self._instances_n = n
        if not sync:
            self._instances_keepalive = (d, o)  # read on the context's stream after the call returns
            return None
        return info

    def instances_readback(self):
        """(W, boxes) of the table set_instances installed (cap_instances_readback): W (N, 3, 4) float32 world-to-object as stored --
        all zero for an inert instance -- and the padded world boxes (N, 2, 3) float32 (lo, hi)."""
        count = getattr(self, "_instances_n", 0)
        w = np.zeros((count, 3, 4), np.float32)
        b = np.zeros((count, 2, 3), np.float32)
        _check(lib().cap_instances_readback(self.ctx, _p(w), _p(b)), "cap_instances_readback")
        return w, b

    def trace_instances(self, rays, out=None, sync=True, cull=None, mask=None, first_hit=False):
        """Closest hit of each ray over the instance table (cap_trace_instances): (hits (N, 4) float32, instance (N,) int32, -1 on a
        miss).  Records as trace_rays, with object-space (u, v) and the scene's triangle id.  Arguments as trace_rays."""
        import torch
        return self._single("cap_trace_instances", rays, 8, "rays", out, 4, torch.float32, sync, (self.trace_options(cull, mask, first_hit),), (torch.int32,))

    def trace_instances_occlusion(self, rays, out=None, sync=True, cull=None, mask=None):
        """1 where some triangle of some instance occludes the ray's open interval, else 0: (N,) int32 (cap_trace_instances_occlusion)."""
        import torch
        return self._single("cap_trace_instances_occlusion", rays, 8, "rays", out, 0, torch.int32, sync, (self.trace_options(cull, mask),))

    def trace_rays_multi(self, rays, k, counts=False, resume=None, sync=True, cull=None, mask=None):
        """The first k hits of each ray in (t, triangle) order (cap_trace_rays_multi): (N, k, 4) float32 records as trace_rays writes
        them, miss records (tmax, 0, 0, MISS) after a ray's last hit.  counts=True also returns the number of ALL hits per ray, (N,)
        int32 (k = 0: counts only, hits is (N, 0, 4)).  resume=<previous page> (the (N, k, 4) result of a call with the same rays)
        continues after it with CAP_MULTI_CONTINUE, writes the next page over it and returns it.  rays and sync as trace_rays; numpy
        rays (or a numpy resume page) give numpy results.  cull= and mask= as trace_rays: hits, counts and pages are those of the
        filtered hit set (cap_trace_rays_multi_ex)."""
        name, tail = self._plain_or_ex("cap_trace_rays_multi", self.trace_options(cull, mask), ())
        return self._multi(name, rays, 8, "rays", 4, False, k, counts, resume, sync, tail)

    def trace_instances_multi(self, rays, k, counts=False, resume=None, sync=True, cull=None, mask=None):
        """The first k (instance, triangle) pairs of each ray over the instance table, in (t, instance, triangle) order
        (cap_trace_instances_multi): (hits (N, k, 4) float32 records as trace_instances writes them, instances (N, k) int32, -1 in the
        miss slots after a ray's last pair[, counts (N,) int32 = the number of ALL pairs per ray with counts=True]).  k = 0: counts
        only, hits is (N, 0, 4) and instances (N, 0).  resume=(hits, instances) of the previous call with the same rays continues
        after it with CAP_MULTI_CONTINUE and writes the next pages over both.  rays, sync, cull= and mask= as trace_rays_multi; numpy
        rays (or numpy resume pages) give numpy results."""
        return self._multi("cap_trace_instances_multi", rays, 8, "rays", 4, True, k, counts, resume, sync, (self.trace_options(cull, mask),))

    def triangle_to_instance_primitive(self, ids):
        """Global triangle ids (hit_triangles) -> (instance, primitive) = (mesh index, triangle index within the mesh), the pair
        CAP_BUF_GBUFFER_GEO stores; a miss (or any id past the scene) maps to (MISS, MISS).  numpy or torch, int64 out."""
        ends = self._tri_end
        if isinstance(ids, np.ndarray) or not hasattr(ids, "device"):
            g = np.asarray(ids).astype(np.int64)
            m = np.searchsorted(ends, g, side="right")
            valid = (g >= 0) & (m < len(ends))
            start = np.concatenate(([0], ends))[np.minimum(m, len(ends))]
            return np.where(valid, m, MISS).astype(np.int64), np.where(valid, g - start, MISS).astype(np.int64)
        import torch
        g = ids.to(torch.int64)
        e = torch.as_tensor(ends, device=g.device)
        m = torch.searchsorted(e, g, right=True)
        valid = (g >= 0) & (m < len(ends))
        start = torch.cat([torch.zeros(1, dtype=torch.int64, device=g.device), e])[torch.clamp(m, max=len(ends))]
        miss = torch.full_like(g, MISS)
        return torch.where(valid, m, miss), torch.where(valid, g - start, miss)

    # ---- reconstruction chain ----
    def post_frame(self, settings, frame_count, prev_camera):
        """Gather -> Accumulate -> Denoise -> Combine -> TAA on the last CAP_RENDER_AOV frame (raytracing_system.cpp:294-317)."""
        _check(lib().cap_post_frame(self.ctx, C.byref(settings), frame_count, C.byref(prev_camera)), "cap_post_frame")

    def post_reset(self):
        _check(lib().cap_post_reset(self.ctx), "cap_post_reset")

    def post_readback(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        _check(lib().cap_post_readback(self.ctx, _p(out)), "cap_post_readback")
        return out

    # ---- multi-GPU tile exchange ----
    def tile_buffer_floats(self):
        n = C.c_size_t()
        _check(lib().cap_tile_buffer_floats(self.ctx, C.byref(n)), "cap_tile_buffer_floats")
        return int(n.value)

    def aov_tile_buffer_floats(self):
        n = C.c_size_t()
        _check(lib().cap_aov_tile_buffer_floats(self.ctx, C.byref(n)), "cap_aov_tile_buffer_floats")
        return n.value

    def resolve_aov_tiles(self, device_ptr):
        _check(lib().cap_resolve_aov_tiles(self.ctx, C.c_void_p(device_ptr)), "cap_resolve_aov_tiles")

    def post_frame_gathered(self, settings, frame_count, prev_camera, device_gathered, shard_count):
        _check(lib().cap_post_frame_gathered(self.ctx, C.byref(settings), frame_count, C.byref(prev_camera), C.c_void_p(device_gathered),
                                             shard_count), "cap_post_frame_gathered")

    def feedback_buffer_floats(self):
        n = C.c_size_t()
        _check(lib().cap_feedback_buffer_floats(self.ctx, C.byref(n)), "cap_feedback_buffer_floats")
        return n.value

    def feedback_export(self, device_ptr):
        _check(lib().cap_feedback_export(self.ctx, C.c_void_p(device_ptr)), "cap_feedback_export")

    def feedback_import(self, device_ptr, frame_count):
        _check(lib().cap_feedback_import(self.ctx, C.c_void_p(device_ptr), frame_count), "cap_feedback_import")

    def resolve_tiles(self, device_ptr):
        _check(lib().cap_resolve_tiles(self.ctx, C.c_void_p(device_ptr)), "cap_resolve_tiles")

    def assemble_tiles(self, device_src, shard_count, device_image):
        _check(lib().cap_assemble_tiles(self.ctx, C.c_void_p(device_src), shard_count, C.c_void_p(device_image)), "cap_assemble_tiles")

    # ---- the exchange below Python: RCCL gather of tile radiance + assembly on rank 0 (cap_comm_*) ----
    def comm_init_rank(self, unique_id, rank, nranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().cap_comm_init_rank(self.ctx, C.cast(buf, C.c_void_p), rank, nranks), "cap_comm_init_rank")

    def comm_gather_frame(self):
        _check(lib().cap_comm_gather_frame(self.ctx), "cap_comm_gather_frame")

    def comm_image_ptr(self):
        p = C.c_void_p()
        _check(lib().cap_comm_image(self.ctx, C.byref(p)), "cap_comm_image")
        return p.value

    def comm_readback(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(lib().cap_comm_readback(self.ctx, _p(out)), "cap_comm_readback")
        return out

    def comm_info(self):
        r, n, u = _u32(), _u32(), _u32()
        _check(lib().cap_comm_info(self.ctx, C.byref(r), C.byref(n), C.byref(u)), "cap_comm_info")
        return int(r.value), int(n.value), bool(u.value)

    def comm_destroy(self):
        _check(lib().cap_comm_destroy(self.ctx), "cap_comm_destroy")

    def comm_abort(self):
        _check(lib().cap_comm_abort(self.ctx), "cap_comm_abort")
