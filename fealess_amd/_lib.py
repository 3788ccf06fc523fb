"""ctypes binding of libfealess_hip.so (the C ABI declared in include/fealess_hip.h).

The library is the product: hand-written HIP kernels for gfx950.  There is no CPU fallback --
if the shared object is missing this module raises, and without a HIP device
``fl_context_create`` returns FL_ERR_NO_DEVICE.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FEALESS_HIP_LIB: development knob -- another build of the same library (A/B timing of two builds on one GPU box)
LIB_PATH = os.environ.get("FEALESS_HIP_LIB") or os.path.join(_HERE, "csrc", "libfealess_hip.so")

FL_OK = 0
FL_ERR_INVALID, FL_ERR_HIP, FL_ERR_ASSERT, FL_ERR_OVERFLOW, FL_ERR_NO_DEVICE, FL_ERR_STATE, FL_ERR_NO_TEMPLATE = -1, -2, -3, -4, -5, -6, -7
FL_MEM_HOST, FL_MEM_DEVICE = 0, 1
FL_ICP_PARITY, FL_ICP_FAST, FL_ICP_POINT_TO_PLANE = 0, 1, 2


class Feature(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("label", C.c_int32)]


class Template(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("offset_x", C.c_int32), ("offset_y", C.c_int32),
                ("pyramid_level", C.c_int32), ("feat_begin", C.c_int32), ("feat_count", C.c_int32)]


class Match(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("similarity", C.c_float), ("class_idx", C.c_int32),
                ("template_id", C.c_int32)]


class Intrinsics(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("T", C.c_float * 3), ("dist_mean", C.c_float), ("px_ratio", C.c_float),
                ("iters", C.c_int32), ("n_corr_last", C.c_int32)]


class DetectionResult(C.Structure):
    _fields_ = [("R_final", C.c_float * 9), ("T_final", C.c_float * 3), ("icp", IcpResult), ("n_points", C.c_int32),
                ("status", C.c_int32)]


class RecognitionResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("found", C.c_int32), ("n_matches", C.c_int32), ("best", Match),
                ("pose", C.c_float * 16), ("det", DetectionResult)]


class RecognitionParams(C.Structure):
    _fields_ = [("matching_threshold", C.c_float), ("icp_it_thr", C.c_int32), ("dist_mean_thr", C.c_float),
                ("dist_diff_thr", C.c_float), ("icp_mode", C.c_int32)]


class InstanceParams(C.Structure):
    _fields_ = [("max_instances", C.c_int32), ("min_dist_px", C.c_int32), ("hyp_per_instance", C.c_int32)]


class InstanceResult(C.Structure):
    _fields_ = [("reco", RecognitionResult), ("rank", C.c_int32), ("n_members", C.c_int32), ("n_refined", C.c_int32),
                ("reserved", C.c_int32)]


class RenderParams(C.Structure):
    _fields_ = [("light", C.c_float * 3), ("ambient", C.c_float)]


class TrackParams(C.Structure):
    _fields_ = [("margin_px", C.c_int32), ("passes", C.c_int32), ("icp_it_thr", C.c_int32), ("dist_mean_thr", C.c_float),
                ("dist_diff_thr", C.c_float), ("icp_mode", C.c_int32), ("max_dist_mean", C.c_float), ("min_px_ratio", C.c_float)]


class TrackResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("tracked", C.c_int32), ("rect_model", C.c_int32 * 4), ("rect_ref", C.c_int32 * 4),
                ("pose", C.c_float * 16), ("det", DetectionResult)]


class VerifyParams(C.Structure):
    _fields_ = [("tau_mm", C.c_int32), ("min_model_px", C.c_int32), ("min_inlier_ratio", C.c_float), ("max_behind_ratio", C.c_float)]


class VerifyResult(C.Structure):       # 64 bytes
    _fields_ = [("status", C.c_int32), ("accepted", C.c_int32), ("best", C.c_int32), ("rect", C.c_int32 * 4), ("n_model", C.c_int32),
                ("n_missing", C.c_int32), ("n_inlier", C.c_int32), ("n_front", C.c_int32), ("n_behind", C.c_int32),
                ("sum_abs_inlier", C.c_int64), ("inlier_ratio", C.c_float), ("behind_ratio", C.c_float)]


class TrackVerifyParams(C.Structure):
    _fields_ = [("verify", VerifyParams), ("keep_input", C.c_int32), ("reserved", C.c_int32)]


class VerifiedTrackResult(C.Structure):       # 368 bytes
    _fields_ = [("track", TrackResult), ("verify", VerifyResult), ("verify_in", VerifyResult), ("icp_tracked", C.c_int32),
                ("kept_input", C.c_int32), ("best", C.c_int32), ("reserved", C.c_int32)]


class InstanceVerifyParams(C.Structure):
    _fields_ = [("verify", VerifyParams), ("class_idx", C.c_int32), ("reserved", C.c_int32)]


class VerifiedInstanceResult(C.Structure):
    _fields_ = [("inst", InstanceResult), ("verify", VerifyResult), ("nms_rank", C.c_int32), ("verified", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class SceneParams(C.Structure):        # fl_scene_params
    _fields_ = [("verify", VerifyParams), ("max_shared_ratio", C.c_float), ("min_shared_px", C.c_int32)]


class SceneResult(C.Structure):        # fl_scene_result, 80 bytes
    _fields_ = [("verify", VerifyResult), ("kept", C.c_int32), ("order", C.c_int32), ("rival", C.c_int32), ("n_shared", C.c_int32)]


class Mesh(C.Structure):               # fl_mesh
    _fields_ = [("vertices", C.c_void_p), ("triangles", C.c_void_p), ("n_vertices", C.c_int32), ("n_triangles", C.c_int32)]


class Extrinsics(C.Structure):         # fl_extrinsics: X_colour = R * X_depth + t, mm
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3)]


class RegisterParams(C.Structure):     # fl_register_params
    _fields_ = [("fill_cracks", C.c_int32)]


class StageTimes(C.Structure):
    _fields_ = [("frontend_ms", C.c_float), ("linmem_ms", C.c_float), ("scan_ms", C.c_float), ("refine_ms", C.c_float),
                ("sort_ms", C.c_float), ("backproject_ms", C.c_float), ("icp_ms", C.c_float), ("total_ms", C.c_float),
                ("icp_iters_total", C.c_int32), ("icp_launches", C.c_int32), ("scan_algorithmic_bytes", C.c_double),
                ("lazy_frontend_ms", C.c_float), ("group_ms", C.c_float)]


class DevSelectJob(C.Structure):       # fl_internal.h fl_dev_select_job
    _fields_ = [("w", C.c_int32), ("total_px", C.c_int32), ("num_features", C.c_int32), ("depth_mode", C.c_int32),
                ("area", C.c_int32), ("n_cand", C.c_int32), ("raster", C.c_void_p), ("score", C.c_void_p), ("labels", C.c_void_p),
                ("n_out", C.c_void_p), ("features", C.c_void_p), ("sorted_keys", C.c_void_p)]


class DevExtractView(C.Structure):     # fl_internal.h fl_dev_extract_view
    _fields_ = [("quantized", C.c_void_p), ("magnitude", C.c_void_p), ("mask", C.c_void_p), ("local_mask", C.c_void_p),
                ("counters", C.c_void_p), ("cand_raster", C.c_void_p), ("cand_score", C.c_void_p), ("sorted_keys", C.c_void_p),
                ("features", C.c_void_p)]


FL_RENDER_AMBIENT = 0.2    # include/fealess_hip.h: fl_render_views' ambient when no fl_render_params is given
FL_TRACK_MAX_PASSES = 4    # include/fealess_hip.h: fl_track_params.passes
FL_TRACK_MAX_MESHES = 256  # include/fealess_hip.h: fl_tracker_create_meshes
FL_RENDER_MAX_DIM = 8192   # include/fealess_hip.h: the largest image width and height of fl_render_views and fl_register_depth_batch
FL_REGISTER_MAX_SPLAT = 8  # include/fealess_hip.h: pixels a footprint of fl_register_depth_batch spans along an axis at most
FL_REGISTER_CHUNK_FRAMES = 64   # include/fealess_hip.h: frames of one launch of fl_register_depth_batch
FL_TOPK_OVERFLOW = -2      # fl_export_topk_batch: template id of record 0 of a frame whose candidate buffers overflowed

_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_D = C.c_double

# name -> (restype, argtypes); every symbol include/fealess_hip.h declares
SIGNATURES = {
    "fl_abi_version": (_I, []),
    "fl_context_create": (_I, [_I, C.POINTER(_P)]),
    "fl_context_destroy": (None, [_P]),
    "fl_last_error": (C.c_char_p, [_P]),
    "fl_context_set_stream": (_I, [_P, _P]),
    "fl_context_synchronize": (_I, [_P]),
    "fl_context_get_stream": (_P, [_P]),
    "fl_context_get_device": (_I, [_P]),
    "fl_detector_get_context": (_P, [_P]),
    "fl_context_set_option": (_I, [_P, C.c_char_p, C.c_long]),
    "fl_context_get_option": (_I, [_P, C.c_char_p, C.POINTER(C.c_long)]),
    "fl_detector_create": (_I, [_P, _I, _I, C.POINTER(_I), C.POINTER(_P)]),
    "fl_detector_destroy": (None, [_P]),
    "fl_detector_add_class": (_I, [_P, C.c_char_p, _I, _P, _P, _I, _P]),
    "fl_detector_set_model_depths": (_I, [_P, _I, _I, _I, _P, _I, _I, _I]),
    "fl_detector_finalize": (_I, [_P, _I, _I, _I, _I]),
    "fl_detector_grow_candidates": (_I, [_P, _I, C.POINTER(_I)]),
    "fl_detector_set_class_filter": (_I, [_P, C.POINTER(C.c_char_p), _I]),
    "fl_detector_num_templates": (_I, [_P]),
    "fl_detector_num_classes": (_I, [_P]),
    "fl_quantized_orientations": (_I, [_P, _P, _I, _I, _F, _P, _I]),
    "fl_quantized_normals": (_I, [_P, _P, _I, _I, _I, _I, _P, _I]),
    "fl_pyrdown_bgr": (_I, [_P, _P, _I, _I, _P, _I]),
    "fl_extract_template_pyramid": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, C.POINTER(_I)]),
    "fl_extract_template_batch": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "fl_render_views": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _P, C.POINTER(Intrinsics), C.POINTER(RenderParams), _I, _P, _P, _P, _P]),
    "fl_view_sphere": (_I, [_I, _I, _P, _I, _I, _F, _P, _I, C.POINTER(_I)]),
    "fl_resize_linear_bgr8": (_I, [_P, _P, _I, _I, _P, _I, _I, _I]),
    "fl_resize_linear_u16": (_I, [_P, _P, _I, _I, _P, _I, _I, _I]),
    "fl_register_depth_batch": (_I, [_P, _I, C.POINTER(_P), _I, C.POINTER(Intrinsics), C.POINTER(Intrinsics), C.POINTER(Extrinsics),
                                     C.POINTER(RegisterParams), C.POINTER(_P)]),
    "fl_register_check": (_I, [C.POINTER(Intrinsics), C.POINTER(Intrinsics), C.POINTER(Extrinsics), C.POINTER(RegisterParams)]),
    "fl_lm_label_stride": (C.c_size_t, [_I, _I, _I]),
    "fl_build_linear_memories": (_I, [_P, _P, _I, _I, _I, _P, _I]),
    "fl_depth_to_3d": (_I, [_P, _P, _I, _I, _D, _D, _D, _D, _P, _I]),
    "fl_icp": (_I, [_P, _P, _I, _P, _I, _I, _F, _F, _I, _I, C.POINTER(IcpResult)]),
    "fl_icp_point_to_plane": (_I, [_P, _P, _P, _I, _P, _I, _I, _F, _F, _I, C.POINTER(IcpResult)]),
    "fl_detection": (_I, [_P, _P, _P, _I, _I, C.POINTER(Intrinsics), C.POINTER(_I), C.POINTER(_I), _I, _F, _F,
                          C.POINTER(_F), C.POINTER(_F), _I, _I, C.POINTER(DetectionResult)]),
    "fl_match_quantized": (_I, [_P, C.POINTER(_P), _I, _F, _P, _I, C.POINTER(_I)]),
    "fl_match_frame": (_I, [_P, _P, _P, _I, _F, _P, _I, C.POINTER(_I)]),
    "fl_match_frame_masked": (_I, [_P, _P, _P, C.POINTER(_P), _I, _F, _P, _I, C.POINTER(_I)]),
    "fl_match_batch_submit": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, _F]),
    "fl_match_batch_collect": (_I, [_P, _I, _P, _I, C.POINTER(_I)]),
    "fl_similarity_maps": (_I, [_P, _I, _I, _P]),
    "fl_last_quantized": (_I, [_P, _P]),
    "fl_recognize_batch": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics),
                                C.POINTER(RecognitionParams), _P]),
    "fl_recognize_batch_zoom": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, _I, _I, C.POINTER(Intrinsics),
                                     C.POINTER(RecognitionParams), _P]),
    "fl_recognize_submit": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics),
                                 C.POINTER(RecognitionParams)]),
    "fl_recognize_collect": (_I, [_P, _I, _P]),
    "fl_recognize_collect_previous": (_I, [_P, _I, _P]),
    "fl_recognize_topk": (_I, [_P, _P, _P, _I, C.POINTER(Intrinsics), C.POINTER(RecognitionParams), _I, _P, C.POINTER(_I)]),
    "fl_recognize_batch_topk": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics), C.POINTER(RecognitionParams), _I, _P,
                                     C.POINTER(_I)]),
    "fl_group_matches": (_I, [_P, _P, _I, _I, C.POINTER(InstanceParams), _P, _P, _P]),
    "fl_recognize_batch_instances": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics), C.POINTER(RecognitionParams),
                                          C.POINTER(InstanceParams), _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "fl_recognize_batch_instances_verified": (_I, [_P, _P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics), C.POINTER(RecognitionParams),
                                                   C.POINTER(InstanceParams), C.POINTER(InstanceVerifyParams), _P, C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32), _P]),
    "fl_tracker_create": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "fl_tracker_destroy": (None, [_P]),
    "fl_track_batch": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, C.POINTER(Intrinsics), C.POINTER(TrackParams), _P]),
    "fl_verify_batch": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, _I, _P, C.POINTER(Intrinsics), C.POINTER(VerifyParams), _P]),
    "fl_track_batch_verified": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, _I, _P, C.POINTER(Intrinsics), C.POINTER(TrackParams),
                                     C.POINTER(TrackVerifyParams), _P]),
    "fl_tracker_create_meshes": (_I, [_P, C.POINTER(Mesh), _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "fl_tracker_num_meshes": (_I, [_P]),
    "fl_track_batch_meshes": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, _P, C.POINTER(Intrinsics), C.POINTER(TrackParams), _P]),
    "fl_verify_batch_meshes": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, _P, _I, _P, C.POINTER(Intrinsics), C.POINTER(VerifyParams), _P]),
    "fl_track_batch_verified_meshes": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, _P, _I, _P, C.POINTER(Intrinsics), C.POINTER(TrackParams),
                                            C.POINTER(TrackVerifyParams), _P]),
    "fl_recognize_batch_instances_verified_meshes": (_I, [_P, _P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics),
                                                          C.POINTER(RecognitionParams), C.POINTER(InstanceParams), C.POINTER(InstanceVerifyParams),
                                                          _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "fl_verify_scene_batch": (_I, [_P, _I, C.POINTER(_P), _I, _I, _P, _P, _P, _I, _P, C.POINTER(Intrinsics), C.POINTER(SceneParams), _P]),
    "fl_scene_pick": (_I, [_P, _I, _I, _P, _P, C.POINTER(SceneParams), _P]),
    "fl_nms": (_I, [_P, _I, _F, C.POINTER(_I), C.POINTER(_I)]),
    "fl_export_topk": (_I, [_P, _I, _I, _I, _P]),
    "fl_merge_topk": (_I, [_P, _I, _P, _I]),
    "fl_export_topk_batch": (_I, [_P, _I, _I, _I, _P]),
    "fl_merge_topk_batch": (_I, [_P, _I, _I, _I, _P, _I, C.POINTER(_I)]),
    "fl_refine_matches": (_I, [_P, _I, C.POINTER(C.c_int32), _P, C.POINTER(Intrinsics), C.POINTER(RecognitionParams), _P]),
    "fl_select_best_batch": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "fl_refine_selected": (_I, [_P, _I, C.POINTER(Intrinsics), C.POINTER(RecognitionParams), _P, C.c_size_t, _P]),
    "fl_last_stage_times": (_I, [_P, C.POINTER(StageTimes)]),
    "fl_frame_counters": (_I, [_P, _I, C.POINTER(C.c_int32)]),
}

# development / test aids the library exports without declaring them in the header (fl_internal.h)
DEV_SIGNATURES = {
    "fl_dev_detector_create_host": (_I, [_I, _I, C.POINTER(_I), C.POINTER(_P)]),
    "fl_dev_group_jobs": (_I, [_P, _P, _I, C.POINTER(InstanceParams), _P, _P, _P, _P, _P]),
    "fl_dev_extract_select": (_I, [_P, _I, _P]),
    "fl_dev_extract_quantized": (_I, [_P, _I, _P, _I, _I, _I, _F, _I, _I]),
    "fl_dev_quantized_orientations_mag": (_I, [_P, _P, _I, _I, _I, _F, _P, _P]),
    "fl_dev_front_images": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, C.c_size_t]),
    "fl_dev_ranged_math": (_I, [_P, _I, C.c_uint32, C.c_uint32, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint32)]),
    "fl_dev_tracker_create_host": (_I, [_I, _I, _I, _I, _I, C.POINTER(_P)]),
    "fl_dev_tracker_create_host_meshes": (_I, [C.POINTER(Mesh), _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "fl_dev_tracker_stage_ms": (_I, [_P, C.POINTER(C.c_float)]),
    "fl_dev_tracker_verify_ms": (_I, [_P, C.POINTER(C.c_float)]),
    "fl_dev_tracker_track_verified_ms": (_I, [_P, C.POINTER(C.c_float)]),
    "fl_dev_tracker_scene_shared": (_I, [_P, _P, _I, C.POINTER(_I)]),
    "fl_dev_tracker_scene_ms": (_I, [_P, C.POINTER(C.c_float)]),
    "fl_dev_instances_verify_ms":(_I, [_P, C.POINTER(C.c_float)]),
    "fl_dev_pick_verified": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "fl_dev_cq_window_addr": (None, [C.c_uint, _I, _I, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(_I)]),
    "fl_dev_cq_window_taps": (None, [_P, C.c_uint, _I, _I, _I, _I, _P]),
    "fl_dev_scan_items": (_I, [_P, _I, _I, _I, C.c_uint, _P, _I, _P, _I, _P]),
    "fl_dev_refine_pitch": (_I, [_I, _I]),
    "fl_dev_refine_plan": (_I, [_P, _I, _I, C.c_long, _I, _P]),
    "fl_dev_refine_kernel": (_I, [_P, _I]),
    "fl_dev_refine_window_max": (C.c_long, [_P, _I]),
    "fl_dev_build_lm_band": (_I, [_I, _I, _I, _I, _I]),
}


def dev(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = DEV_SIGNATURES[name]
    return fn


class MgResult(C.Structure):         # include/fealess_mg.h fl_mg_result
    _fields_ = [("status", C.c_int32), ("found", C.c_int32), ("best", Match), ("pose", C.c_float * 16)]


FL_MG_ID_BYTES = 128
MG_LIB_PATH = os.path.join(_HERE, "mg", "libfealess_mg.so")
# every symbol include/fealess_mg.h declares (libfealess_mg.so: the C++ multi-GPU host on RCCL)
MG_SIGNATURES = {
    "fl_mg_unique_id": (_I, [_P, C.c_size_t]),
    "fl_mg_create": (_I, [_P, _P, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "fl_mg_destroy": (None, [_P]),
    "fl_mg_last_error": (C.c_char_p, [_P]),
    "fl_mg_recognize_batch": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P), _I, C.POINTER(Intrinsics), C.POINTER(RecognitionParams), _P]),
    "fl_mg_last_stats": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
}

_lib = None
_mg_lib = None


def load_mg():
    """Load libfealess_mg.so (links librccl and libfealess_hip.so); raises if it has not been built."""
    global _mg_lib
    if _mg_lib is None:
        load()
        if not os.path.exists(MG_LIB_PATH):
            raise RuntimeError(f"{MG_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(MG_LIB_PATH)
        for name, (res, args) in MG_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _mg_lib = lib
    return _mg_lib



def load():
    """Load libfealess_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). fealess_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
