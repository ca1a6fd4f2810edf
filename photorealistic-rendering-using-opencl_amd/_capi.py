"""ctypes view of include/prt.h, include/prt_types.h and csrc/host/host_capi.h.

The product is the C-ABI shared library `libprt.so` (HIP kernels + host model).  This module
only declares the structs and prototypes so Python plumbing (tests, bench.py, torch.distributed
launch) can call it; nothing here computes pixels and there is no Python or CPU fallback.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRT_LIB", os.path.join(HERE, "libprt.so"))   # PRT_LIB: A/B builds of the same product

PRT_MAX_LIGHTS = 16
PRT_ABI_VERSION = 3


class Material(C.Structure):
    _fields_ = [("color", C.c_float * 4), ("eta", C.c_float * 4), ("k", C.c_float * 4),
                ("roughness", C.c_float), ("t", C.c_uint16), ("lobes", C.c_uint8), ("dist", C.c_uint8),
                ("_pad", C.c_uint8 * 8)]


class Mesh(C.Structure):
    _fields_ = [("mat", Material), ("pos", C.c_float * 4), ("_pad0", C.c_uint8 * 48),
                ("joker", C.c_float * 16), ("t", C.c_uint8), ("_pad1", C.c_uint8 * 63)]


class BvhNode(C.Structure):
    _fields_ = [("bounds", C.c_float * 6), ("first_child_or_primitive", C.c_uint32),
                ("primitive_count", C.c_uint32), ("is_leaf", C.c_uint8), ("_pad", C.c_uint8 * 3)]


class Camera(C.Structure):
    _fields_ = [("position", C.c_float * 4), ("view", C.c_float * 4), ("up", C.c_float * 4),
                ("resolution", C.c_float * 2), ("fov", C.c_float * 2), ("apertureRadius", C.c_float),
                ("focalDistance", C.c_float), ("_pad", C.c_uint8 * 8)]


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32),
                ("max_bounces", C.c_int32), ("max_diff_bounces", C.c_int32), ("max_spec_bounces", C.c_int32),
                ("max_trans_bounces", C.c_int32), ("max_scattering_events", C.c_int32),
                ("marching_steps", C.c_int32), ("shadow_marching_steps", C.c_int32),
                ("active_mats", C.c_uint32), ("geom_flags", C.c_uint32), ("light_count", C.c_uint32),
                ("light_indices", C.c_uint32 * PRT_MAX_LIGHTS),
                ("has_global_medium", C.c_int32), ("fog_density", C.c_float), ("fog_sigma_a", C.c_float),
                ("fog_sigma_s", C.c_float), ("fog_sigma_t", C.c_float), ("fog_abs_only", C.c_int32),
                ("alpha_testing", C.c_int32), ("phase_function", C.c_int32), ("phase_g", C.c_float),
                ("view_option", C.c_uint32), ("pick_random_light", C.c_uint32), ("env_importance_sampling", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [("meshes", C.c_void_p), ("object_count", C.c_uint32 * 8), ("obj_material", C.c_void_p),
                ("vertices", C.c_void_p), ("normals", C.c_void_p), ("primitive_indices", C.c_void_p),
                ("triangle_count", C.c_uint32), ("bvh_nodes", C.c_void_p), ("bvh_node_count", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("launches", C.c_uint32), ("frames", C.c_uint32),
                ("samples", C.c_uint64), ("segments", C.c_uint64), ("finished_pixels", C.c_uint64),
                ("kernel_sum_ms", C.c_double), ("concurrent", C.c_uint32), ("_pad", C.c_uint32)]


class Adaptive(C.Structure):
    _fields_ = [("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("rel_err", C.c_float), ("abs_floor", C.c_float)]


class AdaptiveReport(C.Structure):
    _fields_ = [("tile_launches", C.c_uint32), ("list_launches", C.c_uint32), ("list_builds", C.c_uint32), ("_pad", C.c_uint32),
                ("list_lanes", C.c_uint64), ("list_live_lanes", C.c_uint64)]


class DenoiseParams(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("var_source", C.c_uint32), ("sigma_l", C.c_float), ("sigma_n", C.c_float),
                ("sigma_z", C.c_float), ("sigma_a", C.c_float)]


# prt_denoise_params::var_source and the defaults of a NULL params pointer (include/prt.h)
PRT_DENOISE_VAR_AUTO, PRT_DENOISE_VAR_STATS, PRT_DENOISE_VAR_SPATIAL = 0, 1, 2
DENOISE_DEFAULTS = dict(passes=5, sigma_l=3.0, sigma_n=128.0, sigma_z=1.0, sigma_a=0.1)
DENOISE_RECORD_FLOATS = 16      # PRT_DENOISE_RECORD_FLOATS: one record of prt_export_denoise_inputs / prt_denoise_records
MOTION_FLOATS = 4               # one pixel of the motion plane {D.x, D.y, D.z, m} (prt_read_motion / prt_export_motion)


class TemporalParams(C.Structure):
    _fields_ = [("alpha_color", C.c_float), ("alpha_moments", C.c_float), ("tau_z", C.c_float), ("cos_n", C.c_float),
                ("history_cap", C.c_uint32), ("feedback", C.c_uint32)]


# prt_temporal_params::feedback and the defaults of a NULL params pointer (include/prt.h)
PRT_TEMPORAL_FEEDBACK_INTEGRATED, PRT_TEMPORAL_FEEDBACK_ATROUS = 0, 1
TEMPORAL_DEFAULTS = dict(alpha_color=0.2, alpha_moments=0.2, tau_z=0.05, cos_n=0.9, history_cap=32, feedback="atrous")


# prt_set_temporal_response: prt_temporal_response and its suggested values (PRT_RESPONSE_DEFAULT_* of include/prt.h)
class TemporalResponse(C.Structure):
    _fields_ = [("fast_cap", C.c_uint32), ("radius", C.c_uint32), ("k", C.c_float), ("_pad", C.c_uint32)]


RESPONSE_DEFAULTS = dict(fast_cap=4, radius=2, k=2.0)

# prt_set_pixel_filter kinds by name, and the default radius of each (include/prt.h)
PIXEL_FILTERS = {"none": 0, "box": 1, "tent": 2, "gaussian": 3, "blackman-harris": 4}
PIXEL_FILTER_DEFAULT_RADIUS = {"none": 0.0, "box": 0.5, "tent": 1.0, "gaussian": 1.5, "blackman-harris": 2.0}


assert C.sizeof(Material) == 64 and C.sizeof(Mesh) == 256 and C.sizeof(BvhNode) == 36 and C.sizeof(Camera) == 80

# numpy view of the 112-byte RTD (prt_path_state)
PATH_STATE_DTYPE = [("origin", "<f4", 4), ("dir", "<f4", 4), ("time", "<f4"), ("dist", "<f4"), ("_p0", "u1", 8),
                    ("mask", "<f4", 4), ("acc", "<f4", 4), ("total", "<u4"),
                    ("diff", "<u2"), ("spec", "<u2"), ("trans", "<u2"), ("scatters", "<u2"),
                    ("was_specular", "u1"), ("_p1", "u1", 3), ("reset", "u1"), ("_p2", "u1", 3),
                    ("samples", "<u4"), ("_p3", "u1", 8)]

# numpy view of the 36-byte prt_bvh_node (BvhNode above)
BVH_NODE_DTYPE = [("bounds", "<f4", 6), ("first", "<u4"), ("count", "<u4"), ("leaf", "u1"), ("_p", "u1", 3)]

# numpy views of prt_ray (32 bytes; as float32 [n, 8]: origin, tmax, dir, pad) and prt_hit (48 bytes) of the ray queries (include/prt.h)
RAY_FLOATS, HIT_FLOATS = 8, 12
HIT_DTYPE = [("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"), ("normal", "<f4", 3), ("id", "<i4"), ("pos", "<f4", 3), ("flags", "<u4")]
HIT_MISS, HIT_TRIANGLE = -2, -1

# prt_set_smooth_normals: the weightings by name and the loader's crease (PRT_NORMALS_*, PRT_LOADER_CREASE_COS of include/prt.h)
NORMALS_WEIGHTINGS = {"unit": 0, "area": 1}
LOADER_CREASE_COS = -0.99619470

# prt_set_skin / prt_pose: prt_skin and the modes (PRT_POSE_* of include/prt.h)
class Skin(C.Structure):
    _fields_ = [("rest_vertices", C.c_void_p), ("rest_normals", C.c_void_p), ("bone_index", C.c_void_p), ("bone_weight", C.c_void_p),
                ("n_bones", C.c_uint32), ("_pad", C.c_uint32)]


POSE_REFIT, POSE_REBUILD = 0, 1


# prt_set_morph_targets: prt_morph_target and prt_morph_set of include/prt.h
class MorphTarget(C.Structure):
    _fields_ = [("corner", C.c_void_p), ("d_position", C.c_void_p), ("d_normal", C.c_void_p), ("n_entries", C.c_uint32), ("_pad", C.c_uint32)]


class MorphSet(C.Structure):
    _fields_ = [("base_vertices", C.c_void_p), ("base_normals", C.c_void_p), ("targets", C.POINTER(MorphTarget)), ("n_targets", C.c_uint32),
                ("_pad", C.c_uint32)]


# prt_set_morph_targets_layout / prt_get_morph_report: PRT_MORPH_LAYOUT_* and prt_morph_report
MORPH_LAYOUT_CORNERS, MORPH_LAYOUT_PLANES = 0, 1
MORPH_LAYOUTS = {"corners": MORPH_LAYOUT_CORNERS, "planes": MORPH_LAYOUT_PLANES}


class MorphReport(C.Structure):
    _fields_ = [("layout", C.c_uint32), ("n_targets", C.c_uint32), ("entries", C.c_uint64), ("planes", C.c_uint64), ("table_bytes", C.c_uint64)]


# prt_set_rebuild_policy / prt_get_rebuild_report: prt_rebuild_policy and prt_rebuild_report of include/prt.h
class RebuildPolicy(C.Structure):
    _fields_ = [("limit", C.c_float), ("max_leaf", C.c_uint32)]


class RebuildReport(C.Structure):
    _fields_ = [("cost", C.c_double), ("baseline", C.c_double), ("rebuilt", C.c_uint32), ("rebuilds", C.c_uint32)]


# (name, restype, argtypes) of every symbol include/prt.h declares
PRT_API = [
    ("prt_create", C.c_int, [C.c_int, C.POINTER(Config), C.POINTER(C.c_void_p)]),
    ("prt_destroy", None, [C.c_void_p]),
    ("prt_upload_scene", C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    ("prt_update_vertices", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_update_vertices_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_update_primitives", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("prt_update_primitives_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("prt_cast_rays", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("prt_cast_rays_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("prt_occluded", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("prt_occluded_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("prt_cast_pixels", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("prt_read_bvh_bounds", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_rebuild_bvh", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("prt_rebuild_bvh_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("prt_read_bvh", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_bvh_cost", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("prt_set_rebuild_policy", C.c_int, [C.c_void_p, C.POINTER(RebuildPolicy)]),
    ("prt_get_rebuild_report", C.c_int, [C.c_void_p, C.POINTER(RebuildReport)]),
    ("prt_weld_corners", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("prt_set_smooth_normals", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float]),
    ("prt_read_normals", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_set_skin", C.c_int, [C.c_void_p, C.POINTER(Skin)]),
    ("prt_pose", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("prt_pose_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("prt_read_posed", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_set_morph_targets", C.c_int, [C.c_void_p, C.POINTER(MorphSet)]),
    ("prt_morph", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("prt_morph_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("prt_pose_morphed", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("prt_pose_morphed_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("prt_read_morphed", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_set_morph_targets_layout", C.c_int, [C.c_void_p, C.POINTER(MorphSet), C.c_uint32]),
    ("prt_get_morph_report", C.c_int, [C.c_void_p, C.POINTER(MorphReport)]),
    ("prt_set_camera", C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    ("prt_upload_envmap", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("prt_resize", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("prt_set_tile", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("prt_set_row_blocks", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("prt_reset", C.c_int, [C.c_void_p]),
    ("prt_render_frames", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("prt_render_spp", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("prt_render_adaptive", C.c_int, [C.c_void_p, C.POINTER(Adaptive), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("prt_read_adaptive_stats", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_get_adaptive_report", C.c_int, [C.c_void_p, C.POINTER(AdaptiveReport)]),
    ("prt_render_guides", C.c_int, [C.c_void_p, C.c_uint32]),
    ("prt_read_guides", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_set_motion", C.c_int, [C.c_void_p, C.c_int]),
    ("prt_read_motion", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_export_motion", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_denoise", C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p]),
    ("prt_denoise_temporal", C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p]),
    ("prt_read_history", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_reset_history", C.c_int, [C.c_void_p]),
    ("prt_set_temporal_response", C.c_int, [C.c_void_p, C.POINTER(TemporalResponse)]),
    ("prt_read_response", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_export_denoise_inputs", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_denoise_records", C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_denoise_records_temporal", C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(Camera), C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_denoise_records_temporal_motion", C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(Camera), C.c_int,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("prt_reset_records_history", C.c_int, [C.c_void_p]),
    ("prt_read_records_history", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("prt_read_records_response", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("prt_set_pixel_filter", C.c_int, [C.c_void_p, C.c_uint32, C.c_float]),
    ("prt_pixel_filter_offsets", C.c_int, [C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("prt_env_cdf", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("prt_set_walk_min_lanes", C.c_int, [C.c_void_p, C.c_uint32]),
    ("prt_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ("prt_kernel_variant", C.c_char_p, [C.c_void_p]),
    ("prt_build_id", C.c_char_p, []),
    ("prt_synchronize", C.c_int, [C.c_void_p]),
    ("prt_read_framebuffer", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_tonemap_rgba8", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_copy_framebuffer_to_device", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_read_state", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_write_state", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("prt_get_stats", C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    ("prt_query_counts", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(Stats)]),
    ("prt_selftest_math", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("prt_selftest_fn", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("prt_last_error", C.c_char_p, [C.c_void_p]),
    ("prt_last_global_error", C.c_char_p, []),
]

PRTH_API = [
    ("prth_scene_load", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    ("prth_scene_load_text", C.c_void_p, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    ("prth_scene_free", None, [C.c_void_p]),
    ("prth_scene_get_desc", C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    ("prth_scene_get_config", C.c_int, [C.c_void_p, C.c_int, C.POINTER(Config)]),
    ("prth_scene_bvh_depth", C.c_int, [C.c_void_p]),
    ("prth_scene_obj_path", C.c_char_p, [C.c_void_p]),
    ("prth_default_camera", C.c_int, [C.c_int, C.c_int, C.c_float, C.POINTER(Camera)]),
    ("prth_orbit_camera", C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.POINTER(Camera)]),
    ("prth_seed_pairs", C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p]),
    ("prth_convert_model", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    ("prth_model_meshes", C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]),
    ("prth_make_sky", C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    ("prth_hdr_load", C.c_void_p, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_float)), C.c_char_p, C.c_int]),
    ("prth_hdr_free", None, [C.c_void_p]),
    ("prth_hdr_write", C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
]

_lib = None


def load_library(path=None):
    """dlopen libprt.so and bind every prototype.  Raises if the library or a symbol is missing:
    there is no fallback path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError("libprt.so not built: run `python __graft_entry__.py build` (%s)" % p)
    # PyTorch-ROCm ships its own copy of the HIP runtime.  Two copies in one process do not share the device: the one
    # that initialises second reports "no ROCm-capable device".  Loading torch FIRST makes libprt.so's libamdhip64
    # dependency resolve to the copy that is already there, so every Python process that might use both (bench.py,
    # build() followed by smoke(), tests that hand torch tensors to libprt) gets one runtime.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(p)
    for name, res, args in PRT_API + PRTH_API:
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib
