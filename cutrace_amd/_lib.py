"""ctypes view of the C-ABI (include/cutrace_amd.h, include/cutrace_host.h).

Python is plumbing here (tests, bench.py); the product is the C-ABI library and the
C++ host code.  There is NO Python/CPU fallback for rendering: if libcutrace_amd.so
is missing or no HIP device is present, rendering raises.
"""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tup(self):
        return (self.x, self.y, self.z)


class Triangle(C.Structure):
    _fields_ = [("p1", Vec3), ("p2", Vec3), ("p3", Vec3)]


class Object(C.Structure):
    _fields_ = [("type", C.c_uint32), ("reserved", C.c_uint32), ("mat_idx", C.c_uint64),
                ("v0", Vec3), ("v1", Vec3), ("v2", Vec3), ("f0", C.c_float),
                ("tri_begin", C.c_uint64), ("tri_count", C.c_uint64)]


class Light(C.Structure):
    _fields_ = [("type", C.c_uint32), ("v", Vec3), ("color", Vec3)]


class Material(C.Structure):
    _fields_ = [("type", C.c_uint32), ("color", Vec3), ("specular", C.c_float), ("reflexivity", C.c_float),
                ("phong_exp", C.c_float), ("transparency", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("pos", Vec3), ("up", Vec3), ("forward", Vec3), ("right", Vec3),
                ("near_plane", C.c_float), ("far_plane", C.c_float), ("ambient", C.c_float),
                ("reserved", C.c_uint32), ("w", C.c_uint64), ("h", C.c_uint64)]


class SceneDesc(C.Structure):
    _fields_ = [("objects", C.POINTER(Object)), ("n_objects", C.c_uint64),
                ("triangles", C.POINTER(Triangle)), ("n_triangles", C.c_uint64),
                ("lights", C.POINTER(Light)), ("n_lights", C.c_uint64),
                ("materials", C.POINTER(Material)), ("n_materials", C.c_uint64),
                ("cam", Camera)]


class Rows(C.Structure):
    _fields_ = [("row_begin", C.c_uint64), ("row_end", C.c_uint64), ("block_rows", C.c_uint64),
                ("part", C.c_uint32), ("n_parts", C.c_uint32)]


class ReintPart(C.Structure):
    _fields_ = [("d_depth", C.c_void_p), ("d_color3", C.c_void_p), ("d_normal3", C.c_void_p)]


class RenderStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("ray_count", C.c_uint64),
                ("rows", C.c_uint64), ("max_depth", C.c_float), ("reserved", C.c_uint32)]


class RebuildInfo(C.Structure):
    """ctr_rebuild_info (include/cutrace_rebuild.h)"""
    _fields_ = [("builder", C.c_uint32), ("fell_back", C.c_uint32), ("node_count", C.c_uint32), ("levels", C.c_uint32),
                ("moved", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class ReplaceInfo(C.Structure):
    """ctr_replace_info (include/cutrace_replace.h)"""
    _fields_ = [("builder", C.c_uint32), ("fell_back", C.c_uint32), ("node_count", C.c_uint32), ("levels", C.c_uint32),
                ("nodes_moved", C.c_uint32), ("tris_moved", C.c_uint32), ("tri_cap", C.c_uint32), ("reserved", C.c_uint32)]


class AddInfo(C.Structure):
    """ctr_add_info (include/cutrace_topology.h)"""
    _fields_ = [("index", C.c_uint32), ("builder", C.c_uint32), ("fell_back", C.c_uint32), ("node_count", C.c_uint32), ("levels", C.c_uint32),
                ("tris_reused", C.c_uint32), ("nodes_reused", C.c_uint32), ("tri_cap", C.c_uint32)]


class SceneRoom(C.Structure):
    """struct ctr_scene_room (include/cutrace_topology.h)"""
    _fields_ = [("tris_live", C.c_uint64), ("tris_total", C.c_uint64), ("nodes4_live", C.c_uint64), ("nodes4_total", C.c_uint64)]


class RayQuery(C.Structure):
    """ctr_ray_query (include/cutrace_rays.h)"""
    _fields_ = [("n_rays", C.c_uint64), ("flags", C.c_uint32), ("min_t", C.c_float), ("max_t", C.c_float),
                ("reserved", C.c_uint32), ("d_origin", C.c_void_p), ("d_dir", C.c_void_p), ("d_min_t", C.c_void_p),
                ("d_max_t", C.c_void_p), ("d_t", C.c_void_p), ("d_object", C.c_void_p), ("d_prim", C.c_void_p),
                ("d_point", C.c_void_p), ("d_normal", C.c_void_p), ("d_uv", C.c_void_p), ("d_shadow", C.c_void_p)]


class ShadeQuery(C.Structure):
    """ctr_shade_query (include/cutrace_rays.h)"""
    _fields_ = [("n_rays", C.c_uint64), ("flags", C.c_uint32), ("bounces", C.c_int32), ("min_t", C.c_float),
                ("ambient", C.c_float), ("d_origin", C.c_void_p), ("d_dir", C.c_void_p), ("d_color", C.c_void_p),
                ("d_t", C.c_void_p), ("d_object", C.c_void_p), ("d_normal", C.c_void_p)]


class PointQuery(C.Structure):
    """ctr_point_query (include/cutrace_rays.h)"""
    _fields_ = [("n_points", C.c_uint64), ("flags", C.c_uint32), ("material", C.c_int32), ("ambient", C.c_float),
                ("reserved", C.c_uint32), ("d_point", C.c_void_p), ("d_normal", C.c_void_p), ("d_view", C.c_void_p),
                ("d_material", C.c_void_p), ("d_object", C.c_void_p), ("d_color", C.c_void_p), ("d_light_shadow", C.c_void_p)]


class HitQuery(C.Structure):
    """ctr_hit_query (include/cutrace_hits.h)"""
    _fields_ = [("n_rays", C.c_uint64), ("flags", C.c_uint32), ("max_hits", C.c_uint32), ("min_t", C.c_float), ("max_t", C.c_float),
                ("step", C.c_double), ("d_origin", C.c_void_p), ("d_dir", C.c_void_p), ("d_min_t", C.c_void_p), ("d_max_t", C.c_void_p),
                ("d_count", C.c_void_p), ("d_t", C.c_void_p), ("d_object", C.c_void_p), ("d_prim", C.c_void_p), ("d_point", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_uv", C.c_void_p)]


class NearestQuery(C.Structure):
    """ctr_nearest_query (include/cutrace_nearest.h)"""
    _fields_ = [("n_points", C.c_uint64), ("flags", C.c_uint32), ("object", C.c_int32), ("max_dist", C.c_float), ("reserved", C.c_uint32),
                ("d_point", C.c_void_p), ("d_max_dist", C.c_void_p), ("d_distance", C.c_void_p), ("d_object", C.c_void_p),
                ("d_prim", C.c_void_p), ("d_nearest", C.c_void_p), ("d_normal", C.c_void_p)]


class CrossingQuery(C.Structure):
    """ctr_crossing_query (include/cutrace_inside.h)"""
    _fields_ = [("n_rays", C.c_uint64), ("flags", C.c_uint32), ("object", C.c_int32), ("min_t", C.c_float), ("max_t", C.c_float),
                ("d_origin", C.c_void_p), ("d_dir", C.c_void_p), ("d_min_t", C.c_void_p), ("d_max_t", C.c_void_p),
                ("d_count", C.c_void_p), ("d_signed", C.c_void_p)]


class InsideQuery(C.Structure):
    """ctr_inside_query (include/cutrace_inside.h)"""
    _fields_ = [("n_points", C.c_uint64), ("flags", C.c_uint32), ("object", C.c_int32), ("n_dirs", C.c_uint32), ("reserved", C.c_uint32),
                ("dirs", C.POINTER(C.c_float)), ("d_point", C.c_void_p), ("d_inside", C.c_void_p), ("d_votes", C.c_void_p),
                ("d_distance", C.c_void_p)]


class Lens(C.Structure):
    """ctr_lens (include/cutrace_lens.h)"""
    _fields_ = [("n_rays", C.c_uint64), ("samples", C.c_uint32), ("ambient", C.c_float), ("d_origin", C.c_void_p),
                ("d_dir", C.c_void_p)]


class ImagePlanes(C.Structure):
    """ctr_image_planes (include/cutrace_images.h)"""
    _fields_ = [("n_pixels", C.c_uint64), ("d_depth", C.c_void_p), ("d_color3", C.c_void_p), ("d_normal3", C.c_void_p),
                ("d_depth8", C.c_void_p), ("d_color8", C.c_void_p), ("d_normal8", C.c_void_p), ("d_counters", C.c_void_p),
                ("max_depth", C.c_float), ("reserved", C.c_uint32)]


_int, _u32, _u64, _f32, _ptr, _str, _P = C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p, C.c_char_p, C.POINTER
_f32p = _P(C.c_float)

# One table per library: header -> symbol -> (argtypes, restype), or None for a symbol called without a prototype.
# argtypes None: none declared; restype None: void.  A new entry point is added here and nowhere else.
HOST_PROTOS = {
    "cutrace_host.h": {
        "ctr_host_scene_load": ([_str, _P(_ptr)], _int),
        "ctr_host_scene_parse": ([_str, _P(_ptr)], _int),
        "ctr_host_scene_free": ([_ptr], _int),
        "ctr_host_scene_desc": ([_ptr], _P(SceneDesc)),
        "ctr_host_scene_set_size": ([_ptr, _u64, _u64], _int),
        "ctr_host_scene_set_material": ([_ptr, _u64, _P(Material)], _int),
        "ctr_stl_read": ([_str, _P(Triangle), _u64], C.c_int64),
        "ctr_stl_write": ([_str, _P(Triangle), _u64], _int),
        "ctr_dump_scene": ([_P(SceneDesc)], _int),
        "ctr_dump_schema": None,
        "ctr_quantise_depth": ([_ptr, _u64, _f32, _ptr], _int),
        "ctr_quantise_normal": ([_ptr, _u64, _ptr], _int),
        "ctr_quantise_color": ([_ptr, _u64, _ptr], _int),
        "ctr_write_jpg": ([_str, _int, _int, _ptr, _int], _int),
        "ctr_write_depth_map": ([_str, _ptr, _u64, _u64, _f32], _int),
        "ctr_write_normal_map": ([_str, _ptr, _u64, _u64], _int),
        "ctr_write_colorized": ([_str, _ptr, _u64, _u64], _int),
        "ctr_camera_look_at": ([_P(Camera), Vec3, Vec3, Vec3], _int),
        "ctr_mesh_bounds": ([_P(Triangle), _u64, _P(Vec3), _P(Vec3)], _int),
        "ctr_rows_count": ([_P(Rows), _u64], _u64),
    },
}
HIP_PROTOS = {
    "cutrace_amd.h": {
        "ctr_abi_version": None,
        "ctr_last_error": (None, _str),
        "ctr_device_count": None,
        "ctr_scene_create": ([_P(SceneDesc), _int, _P(_ptr)], _int),
        "ctr_scene_destroy": ([_ptr], _int),
        "ctr_scene_size": ([_ptr, _P(_u64), _P(_u64)], _int),
        "ctr_scene_set_size": ([_ptr, _u64, _u64], _int),
        "ctr_render": ([_ptr, _f32, _int, _P(Rows), _ptr, _ptr, _ptr, _P(RenderStats)], _int),
        "ctr_render_device": ([_ptr, _f32, _int, _P(Rows), _ptr, _ptr, _ptr, _ptr, _ptr], _int),
        "ctr_set_variant": ([_ptr, _u32], _int),
        "ctr_scene_set_cameras": ([_ptr, _P(Camera), _u32], _int),
        "ctr_render_device_batch": ([_ptr, _f32, _int, _P(Rows), _u32, _u32, _u64, _u32, _ptr, _ptr, _ptr, _ptr, _ptr], _int),
        "ctr_algorithmic_bytes": ([_ptr, _f32, _int, _P(Rows), _P(_u64), _P(_u64)], _int),
        "ctr_frame_alloc": ([_u64, _P(_f32p), _P(_f32p), _P(_f32p)], _int),
        "ctr_frame_free": ([_f32p], None),
        "ctr_tile_costs": ([_ptr, _ptr, _u64, _P(_u64)], _int),
        "ctr_last_counters": ([_ptr, _ptr], _int),
        "ctr_selftest_exact_math": ([_P(_u64)], _int),
        "ctr_debug_poison_next_order": ([_ptr], _int),
        "ctr_render_uv": ([_ptr, _f32, _int, _P(Rows), _ptr, _ptr, _ptr, _ptr, _P(RenderStats)], _int),
        "ctr_debug_lane_stats": ([_ptr, _int], _int),
        "ctr_debug_last_kernel": ([_ptr, _P(_u32)], _int),
        "ctr_debug_last_shape": ([_ptr, _P(_u32)], _int),
        "ctr_debug_last_opaque": ([_ptr, _P(_u32)], _int),
        "ctr_debug_last_phased": ([_ptr, _P(_u32)], _int),
        "ctr_debug_room_facts": ([_ptr, _ptr, _P(_u32)], _int),
        "ctr_debug_dark_skip": ([_ptr, _P(_u32)], _int),
        "ctr_multi_create": ([_P(SceneDesc), _P(_int), _int, _P(_ptr)], _int),
        "ctr_multi_destroy": ([_ptr], None),
        "ctr_multi_devices": ([_ptr], _int),
        "ctr_multi_transport": ([_ptr], _str),
        "ctr_multi_size": ([_ptr, _P(_u64), _P(_u64)], _int),
        "ctr_multi_set_size": ([_ptr, _u64, _u64], _int),
        "ctr_multi_set_variant": ([_ptr, _u32], _int),
        "ctr_render_multi": ([_ptr, _f32, _int, _u64, _ptr, _ptr, _ptr, _P(RenderStats)], _int),
        "ctr_multi_kernel_ms": ([_ptr, _P(C.c_double), _int], _int),
        "ctr_reinterleave_device": ([_P(ReintPart), _u32, _u64, _u64, _u64, _ptr, _ptr, _ptr, _ptr], _int),
        "ctr_multi_submit": ([_ptr, _f32, _int, _u64, _ptr, _ptr, _ptr], _int),
        "ctr_multi_wait": ([_ptr, _P(RenderStats)], _int),
    },
    "cutrace_rays.h": {
        "ctr_cast_rays": ([_ptr, _P(RayQuery), _ptr], _int),
        "ctr_shade_rays": ([_ptr, _P(ShadeQuery), _ptr], _int),
        "ctr_shade_points": ([_ptr, _P(PointQuery), _ptr], _int),
    },
    "cutrace_aa.h": {
        "ctr_render_aa": ([_ptr, _f32, _int, _u32, _P(Rows), _ptr, _ptr, _ptr, _P(RenderStats)], _int),
        "ctr_render_device_aa": ([_ptr, _f32, _int, _u32, _P(Rows), _ptr, _ptr, _ptr, _ptr, _ptr], _int),
    },
    "cutrace_lens.h": {
        "ctr_render_device_lens": ([_ptr, _f32, _int, _P(Lens), _P(Rows), _ptr, _ptr, _ptr, _ptr, _ptr], _int),
    },
    "cutrace_images.h": {
        "ctr_quantise_device": ([_int, _P(ImagePlanes), _ptr], _int),
        "ctr_render_images": ([_ptr, _f32, _int, _u32, _P(Rows), _ptr, _ptr, _ptr, _P(RenderStats)], _int),
    },
}
# Headers of libcutrace_amd.so that came after tests/test_bindings_cpu.py, which holds HIP_PROTOS to the six symbol lists it names:
# the same kind of table, declared by hip_lib() all the same (tests/test_mesh_update_cpu.py checks this one as that test checks those).
HIP_LATER_PROTOS = {
    "cutrace_update.h": {
        "ctr_scene_update_mesh": ([_ptr, _u32, _ptr, _u64, _ptr], _int),
        "ctr_scene_mesh_box": ([_ptr, _u32, _P(Vec3), _P(Vec3)], _int),
    },
    "cutrace_edit.h": {
        "ctr_scene_set_lights": ([_ptr, _P(Light), _u64], _int),
        "ctr_scene_set_materials": ([_ptr, _P(Material), _u64], _int),
        "ctr_scene_light_count": ([_ptr, _P(_u64)], _int),
        "ctr_scene_material_count": ([_ptr, _P(_u64)], _int),
        "ctr_debug_guard_state": ([_ptr, _u32, _P(_u32), _u64, _P(_u64), _P(_int)], _int),
    },
    "cutrace_objects.h": {
        "ctr_scene_set_objects": ([_ptr, _P(Object), _u64], _int),
        "ctr_scene_object_count": ([_ptr, _P(_u64)], _int),
        "ctr_scene_get_object": ([_ptr, _u64, _P(Object)], _int),
    },
    "cutrace_rebuild.h": {
        "ctr_scene_rebuild_mesh": ([_ptr, _u32, _ptr, _u64, _u32, _P(RebuildInfo), _ptr], _int),
    },
    "cutrace_replace.h": {
        "ctr_scene_replace_mesh": ([_ptr, _u32, _ptr, _u64, _u32, _P(ReplaceInfo), _ptr], _int),
    },
    "cutrace_topology.h": {
        "ctr_scene_add_object": ([_ptr, _P(Object), _P(_u64)], _int),
        "ctr_scene_add_mesh": ([_ptr, _u64, _ptr, _u64, _u32, _P(AddInfo), _ptr], _int),
        "ctr_scene_remove_object": ([_ptr, _u64], _int),
        "ctr_scene_room": ([_ptr, _P(SceneRoom)], _int),
    },
    "cutrace_hits.h": {
        "ctr_list_hits": ([_ptr, _P(HitQuery), _ptr], _int),
    },
    "cutrace_nearest.h": {
        "ctr_nearest_points": ([_ptr, _P(NearestQuery), _ptr], _int),
    },
    "cutrace_inside.h": {
        "ctr_count_crossings": ([_ptr, _P(CrossingQuery), _ptr], _int),
        "ctr_inside_points": ([_ptr, _P(InsideQuery), _ptr], _int),
        "ctr_inside_default_dirs": ([_f32p], None),
    },
}

# the symbols each header declares (the tests compare them with the headers)
HOST_SYMBOLS = list(HOST_PROTOS["cutrace_host.h"])
HIP_SYMBOLS = list(HIP_PROTOS["cutrace_amd.h"])
RAY_SYMBOLS = list(HIP_PROTOS["cutrace_rays.h"])
AA_SYMBOLS = list(HIP_PROTOS["cutrace_aa.h"])
LENS_SYMBOLS = sorted(HIP_PROTOS["cutrace_lens.h"])
IMAGES_SYMBOLS = list(HIP_PROTOS["cutrace_images.h"])
UPDATE_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_update.h"])
EDIT_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_edit.h"])
OBJECT_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_objects.h"])
REBUILD_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_rebuild.h"])
REBUILD_HOST = 1   # CTR_REBUILD_HOST
REPLACE_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_replace.h"])
REPLACE_HOST = 1   # CTR_REPLACE_HOST
TOPOLOGY_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_topology.h"])
ADD_HOST = 1       # CTR_ADD_HOST
HITS_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_hits.h"])
NEAREST_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_nearest.h"])
INSIDE_SYMBOLS = list(HIP_LATER_PROTOS["cutrace_inside.h"])

_host = None
_hip = None


def _declare(L, protos):
    """Give every symbol of the table that L exports its prototype; an older build (loaded through CUTRACE_AMD_LIB for A/B
    timing) may lack the later entry points."""
    for symbols in protos.values():
        for name, proto in symbols.items():
            if proto is not None and hasattr(L, name):
                fn = getattr(L, name)
                fn.argtypes, fn.restype = proto
    return L


def host_lib():
    global _host
    if _host is None:
        path = os.environ.get("CUTRACE_HOST_LIB") or os.path.join(PKG, "libcutrace_host.so")  # override: sanitizer builds (scripts/cpu_sanitize.sh)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -m cutrace_amd.build` (or __graft_entry__.build())")
        _host = _declare(C.CDLL(path), HOST_PROTOS)
    return _host


def hip_lib():
    """The HIP C-ABI library.  Fails loudly when it is missing: there is no fallback."""
    global _hip
    if _hip is None:
        path = os.environ.get("CUTRACE_AMD_LIB") or os.path.join(PKG, "libcutrace_amd.so")  # override: tuning builds
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: the HIP extension is not built; refusing to fall back to CPU")
        # the CLI links both libs; load host first so shared symbols resolve identically
        host_lib()
        _hip = _declare(_declare(C.CDLL(path, mode=C.RTLD_GLOBAL), HIP_PROTOS), HIP_LATER_PROTOS)
    return _hip
