"""ctypes binding of include/lcd.h (rtabmap_amd/liblcd_hip.so).

This is plumbing: the product is the shared library.  There is no Python/CPU fallback -- if the library is missing it
is built with hipcc, and if that is impossible the import fails loudly.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import build as _build

LCD_OK = 0
LCD_F32, LCD_U8 = 0, 1
LCD_Q_INCREMENTAL, LCD_Q_NEW_WORDS_COMPARED = 1, 2
LCD_GLOBAL_MAX_CHANNELS, LCD_GLOBAL_MAX_DIM = 4, 16384      # global descriptors per signature, floats per descriptor (include/lcd.h)
LCD_MATCH_DICTIONARY, LCD_MATCH_CROSS_CHECK = 0, 1          # lcd_match_args.mode (include/lcd.h)
LCD_GUIDED_PROJECTED_TO_FRAME, LCD_GUIDED_FRAME_TO_PROJECTED = 0, 1   # lcd_guided_args.direction (include/lcd.h)
LCD_GUIDED_RATIO, LCD_GUIDED_NEAREST = 0, 1                          # lcd_guided_args.nn_type
LCD_SELECT_KEEP_ORDER, LCD_SELECT_BY_RESPONSE = 0, 1                 # lcd_select_args.order
LCD_SELECT_SSC = 1                                                   # lcd_select_args.flags: Kp/SSC, the square covering
LCD_DEPTH_U16_MM, LCD_DEPTH_F32_M = 0, 1                             # lcd_depth_image.type
LCD_KP3D_KEEP_ALL, LCD_KP3D_FILTER_3D, LCD_KP3D_FILTER_PIXEL = 0, 1, 2  # lcd_keypoints_3d_args.filter
LCD_NEW_WORD_IDS_AUTO = -1      # lcd_frame_args.first_new_word_id: the device numbers the frame's new words (include/lcd.h)
STATUS = {0: "LCD_OK", 1: "LCD_ERR_INVALID", 2: "LCD_ERR_HIP", 3: "LCD_ERR_NOMEM", 4: "LCD_ERR_STATE", 5: "LCD_ERR_UNSUPPORTED"}

# every symbol include/lcd.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "lcd_abi_version", "lcd_create", "lcd_destroy", "lcd_last_error", "lcd_synchronize", "lcd_pipeline_depth",
    "lcd_vocab_clear", "lcd_vocab_append", "lcd_vocab_remove", "lcd_vocab_remove_unused", "lcd_vocab_remove_unused_async", "lcd_vocab_rebuild", "lcd_vocab_count", "lcd_vocab_read",
    "lcd_knn2", "lcd_selfdist", "lcd_quantize", "lcd_find_nn",
    "lcd_sig_add", "lcd_sig_remove", "lcd_sig_add_bulk", "lcd_sig_count", "lcd_word_nrefs",
    "lcd_likelihood", "lcd_similarity", "lcd_similarity_dev", "lcd_sig_set_globals", "lcd_sig_set_globals_dev", "lcd_sig_set_global_bulk", "lcd_sig_clear_globals", "lcd_compare_to", "lcd_compare_to_dev", "lcd_match_pairs", "lcd_match_pairs_dev", "lcd_match_guided", "lcd_match_guided_dev", "lcd_select_features", "lcd_select_features_dev", "lcd_expand_word_ids", "lcd_expand_word_ids_dev", "lcd_keypoints_3d", "lcd_keypoints_3d_dev", "lcd_keypoints_3d_stereo", "lcd_keypoints_3d_stereo_dev", "lcd_track_flow", "lcd_track_flow_dev", "lcd_estimate_motion_3d", "lcd_estimate_motion_3d_dev", "lcd_estimate_motion_pnp", "lcd_estimate_motion_pnp_dev", "lcd_verify_epipolar", "lcd_verify_epipolar_dev", "lcd_estimate_motion_mono", "lcd_estimate_motion_mono_dev", "lcd_refine_motion_ba", "lcd_refine_motion_ba_dev", "lcd_register_icp", "lcd_register_icp_dev", "lcd_register_icp_plane", "lcd_register_icp_plane_dev", "lcd_filter_scans", "lcd_filter_scans_dev", "lcd_adjust_likelihood", "lcd_adjust_likelihood_dev", "lcd_frame_dev", "lcd_frame_host", "lcd_slot_count", "lcd_knn2_dev", "lcd_shard_knn2_dev", "lcd_shard_frame_dev", "lcd_finalize_dev", "lcd_slots_dev", "lcd_stream", "lcd_get_stats", "lcd_profile_begin", "lcd_profile_read", "lcd_profile_read_likelihood", "lcd_profile_score_work", "lcd_set_option", "lcd_record_event", "lcd_trace_push", "lcd_trace_pop",
    "lcd_bayes_configure", "lcd_bayes_reset", "lcd_bayes_set_neighbors", "lcd_bayes_update_dev", "lcd_bayes_update", "lcd_bayes_posterior",
]


LCD_KNN_DEFAULT, LCD_KNN_EXACT_VALU, LCD_KNN_F32_MFMA, LCD_KNN_BF16X3, LCD_KNN_F16, LCD_KNN_HAMMING_MFMA = 0, 1, 2, 3, 4, 5
KNN_MODES = {None: 0, "default": 0, "valu": 1, "exact": 1, "mfma32": 2, "f32": 2, "bf16": 3, "bf16x3": 3, "f16": 4, "fp16": 4,
             "hamming_mfma": 5}     # u8 handles: Hamming 2-NN on the i8 matrix cores; on an f32 handle the default


class LcdConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("dtype", C.c_int32), ("dim", C.c_int32),
                ("vocab_capacity", C.c_int64), ("sig_capacity", C.c_int64), ("max_queries", C.c_int32),
                ("knn_mode", C.c_int32), ("stream", C.c_void_p), ("pipeline", C.c_int32), ("reserved1", C.c_int32)]


class LcdHypothesis(C.Structure):
    _fields_ = [("sig_id", C.c_int32), ("slot", C.c_int32), ("likelihood", C.c_float), ("adjusted", C.c_float),
                ("virtual_place", C.c_float), ("mean", C.c_float), ("stddev", C.c_float), ("n_positive", C.c_int32)]


class LcdFrameArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("q", C.c_int32), ("d_descriptors", C.c_void_p), ("flags", C.c_int32),
                ("nndr_ratio", C.c_float), ("sig_id", C.c_int32), ("first_new_word_id", C.c_int32), ("N", C.c_float),
                ("exclude_recent", C.c_int32), ("d_word_ids", C.c_void_p), ("d_likelihood", C.c_void_p),
                ("likelihood_capacity", C.c_int64), ("d_hypothesis", C.c_void_p), ("d_adjusted", C.c_void_p),
                ("virtual_place_ratio", C.c_float), ("append_new_words", C.c_int32), ("d_first_new_word_id", C.c_void_p),
                ("d_posterior", C.c_void_p), ("d_bayes", C.c_void_p)]


class LcdFrameHostArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("q", C.c_int32), ("descriptors", C.c_void_p), ("flags", C.c_int32), ("nndr_ratio", C.c_float),
                ("sig_id", C.c_int32), ("first_new_word_id", C.c_int32), ("N", C.c_float), ("append_new_words", C.c_int32),
                ("word_ids", C.c_void_p), ("likelihood", C.c_void_p), ("likelihood_capacity", C.c_int64), ("n_slots", C.c_void_p)]


class LcdBayesResult(C.Structure):
    _fields_ = [("sig_id", C.c_int32), ("slot", C.c_int32), ("posterior", C.c_float), ("value", C.c_float),
                ("virtual_place", C.c_float), ("n_considered", C.c_int32), ("sum", C.c_float), ("reserved", C.c_int32)]


class LcdStats(C.Structure):
    _fields_ = [("vocab_rows", C.c_int64), ("vocab_live", C.c_int64), ("signatures", C.c_int64), ("postings", C.c_int64),
                ("knn_launches", C.c_int64), ("likelihood_launches", C.c_int64), ("rebuilds", C.c_int64),
                ("buckets_sealed", C.c_int64), ("word_slots", C.c_int64), ("dense_words", C.c_int64),
                ("frame_calls", C.c_int64), ("frame_host_ns", C.c_int64),
                ("bytes_device", C.c_int64), ("knn_last_fallback_queries", C.c_int64), ("knn_max_err_ratio", C.c_double),
                ("clean_divergent_refs", C.c_int64)]


class LcdGlobalDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("dim", C.c_int32), ("data", C.c_void_p)]


class LcdMatchArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("mode", C.c_int32), ("n_pairs", C.c_int32), ("flags", C.c_int32), ("nndr_ratio", C.c_float),
                ("reserved", C.c_int32), ("from_rows", C.c_void_p), ("to_rows", C.c_void_p), ("from_offsets", C.c_void_p),
                ("to_offsets", C.c_void_p), ("from_word_ids", C.c_void_p), ("out_from_word_ids", C.c_void_p),
                ("out_to_word_ids", C.c_void_p), ("out_to_match", C.c_void_p), ("out_to_dist", C.c_void_p)]


MATCH_MODES = {"dictionary": LCD_MATCH_DICTIONARY, "cross_check": LCD_MATCH_CROSS_CHECK}


class LcdGuidedArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("direction", C.c_int32), ("nn_type", C.c_int32), ("n_pairs", C.c_int32), ("radius", C.c_float),
                ("nndr_ratio", C.c_float), ("from_rows", C.c_void_p), ("to_rows", C.c_void_p), ("corners", C.c_void_p),
                ("corner_from_row", C.c_void_p), ("to_points", C.c_void_p), ("from_offsets", C.c_void_p), ("to_offsets", C.c_void_p),
                ("corner_offsets", C.c_void_p), ("out_count", C.c_void_p), ("out_match", C.c_void_p), ("out_dist", C.c_void_p),
                ("out_to_owner", C.c_void_p)]


GUIDED_DIRECTIONS = {"projected_to_frame": LCD_GUIDED_PROJECTED_TO_FRAME, "frame_to_projected": LCD_GUIDED_FRAME_TO_PROJECTED}
GUIDED_NN_TYPES = {"ratio": LCD_GUIDED_RATIO, "nearest": LCD_GUIDED_NEAREST}


class LcdSelectArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_frames", C.c_int32), ("order", C.c_int32), ("max_features", C.c_int32), ("grid_rows", C.c_int32),
                ("grid_cols", C.c_int32), ("aux_bytes", C.c_int32), ("flags", C.c_int32), ("offsets", C.c_void_p), ("image_size", C.c_void_p),
                ("response", C.c_void_p), ("points", C.c_void_p), ("rows", C.c_void_p), ("aux", C.c_void_p), ("out_count", C.c_void_p),
                ("out_index", C.c_void_p), ("out_rows", C.c_void_p), ("out_aux", C.c_void_p), ("n_in", C.c_void_p)]


class LcdExpandArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_frames", C.c_int32), ("offsets", C.c_void_p), ("count", C.c_void_p), ("index", C.c_void_p),
                ("word_ids", C.c_void_p), ("first_new_word_id", C.c_void_p), ("out_word_ids", C.c_void_p), ("n_features", C.c_void_p)]


class LcdCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("image_width", C.c_int32), ("image_height", C.c_int32),
                ("has_local_transform", C.c_int32), ("reserved", C.c_int32), ("local_transform", C.c_float * 12)]


class LcdDepthImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pitch_bytes", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("type", C.c_int32),
                ("n_cameras", C.c_int32), ("cameras", C.POINTER(LcdCamera))]


class LcdKeypoints3dArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_frames", C.c_int32), ("filter", C.c_int32), ("aux_bytes", C.c_int32), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("offsets", C.c_void_p), ("images", C.POINTER(LcdDepthImage)), ("points", C.c_void_p),
                ("response", C.c_void_p), ("rows", C.c_void_p), ("aux", C.c_void_p), ("out_count", C.c_void_p), ("out_index", C.c_void_p),
                ("out_xyz", C.c_void_p), ("out_points", C.c_void_p), ("out_response", C.c_void_p), ("out_rows", C.c_void_p), ("out_aux", C.c_void_p)]


class LcdStereoCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("right_cx", C.c_double), ("baseline", C.c_double),
                ("has_local_transform", C.c_int32), ("reserved", C.c_int32), ("local_transform", C.c_float * 12)]


class LcdStereoImage(C.Structure):
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("left_pitch_bytes", C.c_int64), ("right_pitch_bytes", C.c_int64), ("width", C.c_int32),
                ("height", C.c_int32), ("camera", C.POINTER(LcdStereoCamera))]


class LcdStereoParams(C.Structure):
    _fields_ = [("win_width", C.c_int32), ("win_height", C.c_int32), ("max_level", C.c_int32), ("iterations", C.c_int32), ("eps", C.c_double),
                ("use_min_eigenvals", C.c_int32), ("reserved", C.c_int32), ("min_eig_threshold", C.c_double), ("error_threshold", C.c_double),
                ("min_disparity", C.c_float), ("max_disparity", C.c_float)]


class LcdKeypoints3dStereoArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_frames", C.c_int32), ("filter", C.c_int32), ("aux_bytes", C.c_int32), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("offsets", C.c_void_p), ("images", C.POINTER(LcdStereoImage)), ("params", C.POINTER(LcdStereoParams)),
                ("points", C.c_void_p), ("response", C.c_void_p), ("rows", C.c_void_p), ("aux", C.c_void_p), ("out_count", C.c_void_p),
                ("out_index", C.c_void_p), ("out_xyz", C.c_void_p), ("out_points", C.c_void_p), ("out_response", C.c_void_p), ("out_rows", C.c_void_p),
                ("out_aux", C.c_void_p), ("out_right", C.c_void_p), ("out_status", C.c_void_p)]


# lcd_stereo_params: the reference's defaults (Stereo/WinWidth .. Stereo/MaxDisparity)
STEREO_DEFAULTS = dict(win_width=15, win_height=3, max_level=5, iterations=30, eps=0.01, use_min_eigenvals=1, min_eig_threshold=1e-4,
                       error_threshold=50.0, min_disparity=0.5, max_disparity=128.0)


def stereo_params(params=None):
    """a dict over STEREO_DEFAULTS -> LcdStereoParams"""
    v = dict(STEREO_DEFAULTS, **(params or {}))
    return LcdStereoParams(int(v["win_width"]), int(v["win_height"]), int(v["max_level"]), int(v["iterations"]), float(v["eps"]),
                           int(v["use_min_eigenvals"]), 0, float(v["min_eig_threshold"]), float(v["error_threshold"]), float(v["min_disparity"]),
                           float(v["max_disparity"]))


class LcdFlowPair(C.Structure):
    _fields_ = [("from_", C.c_void_p), ("to", C.c_void_p), ("from_pitch_bytes", C.c_int64), ("to_pitch_bytes", C.c_int64), ("width", C.c_int32),
                ("height", C.c_int32), ("max_level", C.c_int32), ("use_initial", C.c_int32)]


class LcdFlowParams(C.Structure):
    _fields_ = [("win_width", C.c_int32), ("win_height", C.c_int32), ("iterations", C.c_int32), ("use_min_eigenvals", C.c_int32), ("eps", C.c_double),
                ("min_eig_threshold", C.c_double), ("error_threshold", C.c_float), ("reserved", C.c_int32)]


class LcdTrackFlowArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("aux_bytes", C.c_int32), ("reserved", C.c_int32), ("offsets", C.c_void_p),
                ("pairs", C.POINTER(LcdFlowPair)), ("params", C.POINTER(LcdFlowParams)), ("points", C.c_void_p), ("initial", C.c_void_p),
                ("aux", C.c_void_p), ("out_count", C.c_void_p), ("out_index", C.c_void_p), ("out_from", C.c_void_p), ("out_to", C.c_void_p),
                ("out_aux", C.c_void_p), ("out_track", C.c_void_p), ("out_status", C.c_void_p), ("out_err", C.c_void_p)]


# lcd_flow_params: the reference's defaults (Vis/CorFlowWinSize .. Vis/CorFlowErrorThreshold)
FLOW_DEFAULTS = dict(win_width=16, win_height=16, iterations=30, eps=0.01, use_min_eigenvals=1, min_eig_threshold=1e-4, error_threshold=20.0)


def flow_params(params=None):
    """a dict over FLOW_DEFAULTS -> LcdFlowParams"""
    v = dict(FLOW_DEFAULTS, **(params or {}))
    return LcdFlowParams(int(v["win_width"]), int(v["win_height"]), int(v["iterations"]), int(v["use_min_eigenvals"]), float(v["eps"]),
                         float(v["min_eig_threshold"]), float(v["error_threshold"]), 0)


class LcdMotion3dArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("min_inliers", C.c_int32), ("iterations", C.c_int32),
                ("refine_iterations", C.c_int32), ("seed", C.c_uint32), ("inlier_distance", C.c_double), ("from_word_ids", C.c_void_p),
                ("from_xyz", C.c_void_p), ("to_word_ids", C.c_void_p), ("to_xyz", C.c_void_p), ("from_offsets", C.c_void_p),
                ("to_offsets", C.c_void_p), ("out_transform", C.c_void_p), ("out_status", C.c_void_p), ("out_n_matches", C.c_void_p),
                ("out_n_inliers", C.c_void_p), ("out_variance", C.c_void_p), ("out_matches", C.c_void_p), ("out_inliers", C.c_void_p)]


class LcdIcpArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("max_iterations", C.c_int32), ("force_3dof", C.c_int32),
                ("max_laser_scans", C.c_int32), ("search", C.c_int32), ("max_correspondence_distance", C.c_double), ("epsilon", C.c_float),
                ("correspondence_ratio", C.c_float), ("from_xyz", C.c_void_p), ("to_xyz", C.c_void_p), ("from_offsets", C.c_void_p),
                ("to_offsets", C.c_void_p), ("guesses", C.c_void_p), ("out_transform", C.c_void_p), ("out_icp_transform", C.c_void_p),
                ("out_correction", C.c_void_p), ("out_status", C.c_void_p), ("out_stop", C.c_void_p), ("out_iterations", C.c_void_p),
                ("out_n_correspondences", C.c_void_p), ("out_ratio", C.c_void_p), ("out_variance", C.c_void_p), ("out_match", C.c_void_p)]


class LcdIcpPlaneArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("max_iterations", C.c_int32), ("force_3dof", C.c_int32),
                ("max_laser_scans", C.c_int32), ("search", C.c_int32), ("max_correspondence_distance", C.c_double), ("epsilon", C.c_float),
                ("correspondence_ratio", C.c_float), ("min_complexity", C.c_float), ("low_complexity_strategy", C.c_int32),
                ("normal_gate", C.c_int32), ("reserved", C.c_int32), ("min_normal_cos", C.c_double), ("from_xyz", C.c_void_p), ("to_xyz", C.c_void_p),
                ("from_normals", C.c_void_p), ("to_normals", C.c_void_p), ("from_offsets", C.c_void_p), ("to_offsets", C.c_void_p),
                ("guesses", C.c_void_p), ("out_transform", C.c_void_p), ("out_icp_transform", C.c_void_p), ("out_correction", C.c_void_p),
                ("out_status", C.c_void_p), ("out_stop", C.c_void_p), ("out_iterations", C.c_void_p), ("out_n_correspondences", C.c_void_p),
                ("out_ratio", C.c_void_p), ("out_variance", C.c_void_p), ("out_match", C.c_void_p), ("out_branch", C.c_void_p),
                ("out_complexity", C.c_void_p), ("out_complexity_values", C.c_void_p), ("out_complexity_vectors", C.c_void_p),
                ("out_second_eigenvalue", C.c_void_p)]


class LcdScanFilterArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_scans", C.c_int32), ("downsampling_step", C.c_int32), ("is_2d", C.c_int32), ("normal_k", C.c_int32),
                ("reserved", C.c_int32), ("range_min", C.c_float), ("range_max", C.c_float), ("voxel_size", C.c_float), ("normal_radius", C.c_float),
                ("ground_normals_up", C.c_float), ("viewpoint", C.c_float * 3), ("xyz", C.c_void_p), ("offsets", C.c_void_p), ("out_offsets", C.c_void_p),
                ("out_xyz", C.c_void_p), ("out_normals", C.c_void_p), ("out_count", C.c_void_p), ("out_stage_counts", C.c_void_p), ("out_status", C.c_void_p)]


LCD_SCAN_OK, LCD_SCAN_EMPTY, LCD_SCAN_GRID_TOO_LARGE, LCD_SCAN_TOO_MANY_ROWS, LCD_SCAN_NO_ROOM = 0, 1, 2, 3, 4  # lcd_scan_status
LCD_SCAN_MAX_K = 32
LCD_ICP_OK, LCD_ICP_EMPTY, LCD_ICP_NOT_CONVERGED, LCD_ICP_BELOW_RATIO, LCD_ICP_LOW_COMPLEXITY = 0, 1, 2, 3, 4  # lcd_icp_status
LCD_ICP_STOP_NONE, LCD_ICP_STOP_ITERATIONS, LCD_ICP_STOP_TRANSFORM, LCD_ICP_STOP_MSE, LCD_ICP_STOP_FEW_CORRESPONDENCES, LCD_ICP_STOP_SINGULAR = 0, 1, 2, 3, 4, 5  # lcd_icp_stop
LCD_ICP_SEARCH_AUTO, LCD_ICP_SEARCH_BRUTE, LCD_ICP_SEARCH_GRID = 0, 1, 2  # lcd_icp_search


LCD_M3D_OK, LCD_M3D_FEW_CORRESPONDENCES, LCD_M3D_NO_MODEL, LCD_M3D_FEW_INLIERS, LCD_M3D_BELOW_MIN_INLIERS = 0, 1, 2, 3, 4  # lcd_motion_3d_status


class LcdMotionPnpArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("min_inliers", C.c_int32), ("iterations", C.c_int32),
                ("refine_iterations", C.c_int32), ("variance_median_ratio", C.c_int32), ("seed", C.c_uint32), ("max_variance", C.c_float),
                ("reproj_error", C.c_double), ("from_word_ids", C.c_void_p), ("from_xyz", C.c_void_p), ("to_word_ids", C.c_void_p),
                ("to_points", C.c_void_p), ("to_xyz", C.c_void_p), ("from_offsets", C.c_void_p), ("to_offsets", C.c_void_p),
                ("cameras", C.c_void_p), ("guesses", C.c_void_p), ("out_transform", C.c_void_p), ("out_status", C.c_void_p),
                ("out_n_matches", C.c_void_p), ("out_n_inliers", C.c_void_p), ("out_variance_lin", C.c_void_p), ("out_angle_cos", C.c_void_p),
                ("out_variance_kind", C.c_void_p), ("out_matches", C.c_void_p), ("out_inliers", C.c_void_p)]


LCD_PNP_OK, LCD_PNP_FEW_CORRESPONDENCES, LCD_PNP_NO_MODEL, LCD_PNP_BELOW_MIN_INLIERS, LCD_PNP_VARIANCE_REJECTED = 0, 1, 2, 3, 4  # lcd_motion_pnp_status


class LcdEpipolarArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("match_count_min", C.c_int32), ("iterations", C.c_int32), ("seed", C.c_uint32),
                ("ransac_threshold", C.c_double), ("from_word_ids", C.c_void_p), ("from_points", C.c_void_p), ("to_word_ids", C.c_void_p),
                ("to_points", C.c_void_p), ("from_offsets", C.c_void_p), ("to_offsets", C.c_void_p), ("out_fundamental", C.c_void_p),
                ("out_status", C.c_void_p), ("out_n_pairs", C.c_void_p), ("out_n_inliers", C.c_void_p), ("out_matches", C.c_void_p),
                ("out_inliers", C.c_void_p)]


LCD_EPI_OK, LCD_EPI_FEW_PAIRS, LCD_EPI_NO_MODEL, LCD_EPI_FEW_INLIERS = 0, 1, 2, 3  # lcd_epipolar_status


class LcdMotionMonoArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("min_inliers", C.c_int32), ("iterations", C.c_int32), ("seed", C.c_uint32),
                ("variance_median_ratio", C.c_int32), ("reproj_threshold", C.c_double), ("distance_threshold", C.c_double),
                ("max_variance", C.c_float), ("reserved", C.c_int32), ("from_word_ids", C.c_void_p), ("from_points", C.c_void_p),
                ("from_points3", C.c_void_p), ("to_word_ids", C.c_void_p), ("to_points", C.c_void_p), ("from_offsets", C.c_void_p),
                ("to_offsets", C.c_void_p), ("cameras", C.c_void_p), ("guesses", C.c_void_p), ("out_transform", C.c_void_p),
                ("out_status", C.c_void_p), ("out_n_matches", C.c_void_p), ("out_n_inliers", C.c_void_p), ("out_variance", C.c_void_p),
                ("out_matches", C.c_void_p), ("out_inliers", C.c_void_p), ("out_points3", C.c_void_p)]


LCD_MONO_OK, LCD_MONO_FEW_FEATURES, LCD_MONO_FEW_PAIRS, LCD_MONO_NO_MODEL, LCD_MONO_FEW_INLIERS, LCD_MONO_HIGH_VARIANCE = 0, 1, 2, 3, 4, 5  # lcd_motion_mono_status
LCD_MONO_BISECT = 56


class LcdMotionBaArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_pairs", C.c_int32), ("min_inliers", C.c_int32), ("iterations", C.c_int32),
                ("pixel_variance", C.c_double), ("robust_delta", C.c_double), ("default_baseline", C.c_double),
                ("max_inliers_mean_distance", C.c_float), ("min_inliers_distribution", C.c_float), ("from_word_ids", C.c_void_p),
                ("from_xyz", C.c_void_p), ("from_points", C.c_void_p), ("to_word_ids", C.c_void_p), ("to_points", C.c_void_p), ("to_xyz", C.c_void_p),
                ("inliers", C.c_void_p), ("n_inliers", C.c_void_p), ("transforms", C.c_void_p), ("prior_variance", C.c_void_p),
                ("from_offsets", C.c_void_p), ("to_offsets", C.c_void_p), ("cameras_from", C.c_void_p), ("cameras_to", C.c_void_p),
                ("baselines", C.c_void_p), ("out_transform", C.c_void_p), ("out_status", C.c_void_p), ("out_inliers", C.c_void_p),
                ("out_n_inliers", C.c_void_p), ("out_n_outliers", C.c_void_p), ("out_chi2_before", C.c_void_p), ("out_chi2_after", C.c_void_p),
                ("out_lm_accepted", C.c_void_p), ("out_inliers_mean_distance", C.c_void_p), ("out_inliers_distribution", C.c_void_p)]


LCD_BA_OK, LCD_BA_NO_INPUT, LCD_BA_BAD_INLIER, LCD_BA_DIVERGED, LCD_BA_BELOW_MIN_INLIERS, LCD_BA_MEAN_DISTANCE_REJECTED, LCD_BA_DISTRIBUTION_REJECTED = \
    0, 1, 2, 3, 4, 5, 6  # lcd_motion_ba_status


KP3D_FILTERS = {"keep_all": LCD_KP3D_KEEP_ALL, "filter_3d": LCD_KP3D_FILTER_3D, "filter_pixel": LCD_KP3D_FILTER_PIXEL}


SELECT_ORDERS = {"keep_order": LCD_SELECT_KEEP_ORDER, "by_response": LCD_SELECT_BY_RESPONSE}


class LcdError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("%s: %s" % (STATUS.get(status, status), msg))
        self.status = status


_lib = None


def library_path():
    return _build.OUT


def load():
    """Load (building if needed) liblcd_hip.so.  Raises if it cannot be produced: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("LCD_LIB_PATH") or _build.build()      # LCD_LIB_PATH: timing experiments with variant builds
    # PyTorch-ROCm ships its own libamdhip64: a process that loads the system runtime first (through this library) and torch
    # later ends up with two HIP runtimes, and the second one finds no GPU.  When torch is installed, let it load first.
    if "torch" not in sys.modules and not os.environ.get("LCD_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(path)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.lcd_abi_version.restype = C.c_int
    L.lcd_create.argtypes = [C.POINTER(LcdConfig), C.POINTER(vp)]
    L.lcd_destroy.argtypes = [vp]
    L.lcd_destroy.restype = None
    L.lcd_last_error.argtypes = [vp]
    L.lcd_last_error.restype = C.c_char_p
    L.lcd_synchronize.argtypes = [vp]
    L.lcd_pipeline_depth.argtypes = [vp]
    L.lcd_pipeline_depth.restype = C.c_int
    L.lcd_vocab_clear.argtypes = [vp]
    L.lcd_vocab_append.argtypes = [vp, vp, C.c_int, vp]
    L.lcd_vocab_remove.argtypes = [vp, vp, C.c_int]
    L.lcd_vocab_remove_unused.argtypes = [vp, vp, C.c_int, vp]
    L.lcd_vocab_remove_unused_async.argtypes = [vp]
    L.lcd_vocab_rebuild.argtypes = [vp]
    L.lcd_vocab_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.lcd_vocab_read.argtypes = [vp, i64, C.c_int, vp, vp]
    L.lcd_knn2.argtypes = [vp, vp, C.c_int, vp, vp]
    L.lcd_selfdist.argtypes = [vp, vp, C.c_int, vp]
    L.lcd_quantize.argtypes = [vp, vp, C.c_int, C.c_int, f32, vp, C.POINTER(i32)]
    L.lcd_find_nn.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, f32, vp]
    L.lcd_sig_add.argtypes = [vp, i32, vp, C.c_int, i32]
    L.lcd_sig_remove.argtypes = [vp, i32]
    L.lcd_sig_add_bulk.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.lcd_sig_count.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.lcd_word_nrefs.argtypes = [vp, i32, C.POINTER(i32)]
    L.lcd_likelihood.argtypes = [vp, vp, C.c_int, vp, C.c_int, f32, vp]
    L.lcd_similarity.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp]
    L.lcd_similarity_dev.argtypes = [vp, vp, C.c_int, vp, i64]
    L.lcd_sig_set_globals.argtypes = [vp, i32, vp, C.c_int]
    L.lcd_sig_set_globals_dev.argtypes = [vp, i32, vp, C.c_int]
    L.lcd_sig_set_global_bulk.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int]
    L.lcd_sig_clear_globals.argtypes = [vp, i32]
    L.lcd_compare_to.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]
    L.lcd_compare_to_dev.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, i64]
    L.lcd_match_pairs.argtypes = [vp, C.POINTER(LcdMatchArgs)]
    L.lcd_match_pairs_dev.argtypes = [vp, C.POINTER(LcdMatchArgs)]
    L.lcd_match_guided.argtypes = [vp, C.POINTER(LcdGuidedArgs)]
    L.lcd_match_guided_dev.argtypes = [vp, C.POINTER(LcdGuidedArgs)]
    L.lcd_select_features.argtypes = [vp, C.POINTER(LcdSelectArgs)]
    L.lcd_select_features_dev.argtypes = [vp, C.POINTER(LcdSelectArgs)]
    L.lcd_expand_word_ids.argtypes = [vp, C.POINTER(LcdExpandArgs)]
    L.lcd_expand_word_ids_dev.argtypes = [vp, C.POINTER(LcdExpandArgs)]
    L.lcd_keypoints_3d.argtypes = [vp, C.POINTER(LcdKeypoints3dArgs)]
    L.lcd_keypoints_3d_dev.argtypes = [vp, C.POINTER(LcdKeypoints3dArgs)]
    L.lcd_keypoints_3d_stereo.argtypes = [vp, C.POINTER(LcdKeypoints3dStereoArgs)]
    L.lcd_keypoints_3d_stereo_dev.argtypes = [vp, C.POINTER(LcdKeypoints3dStereoArgs)]
    L.lcd_track_flow.argtypes = [vp, C.POINTER(LcdTrackFlowArgs)]
    L.lcd_track_flow_dev.argtypes = [vp, C.POINTER(LcdTrackFlowArgs)]
    L.lcd_estimate_motion_3d.argtypes = [vp, C.POINTER(LcdMotion3dArgs)]
    L.lcd_estimate_motion_3d_dev.argtypes = [vp, C.POINTER(LcdMotion3dArgs)]
    L.lcd_estimate_motion_pnp.argtypes = [vp, C.POINTER(LcdMotionPnpArgs)]
    L.lcd_estimate_motion_pnp_dev.argtypes = [vp, C.POINTER(LcdMotionPnpArgs)]
    L.lcd_verify_epipolar.argtypes = [vp, C.POINTER(LcdEpipolarArgs)]
    L.lcd_verify_epipolar_dev.argtypes = [vp, C.POINTER(LcdEpipolarArgs)]
    L.lcd_estimate_motion_mono.argtypes = [vp, C.POINTER(LcdMotionMonoArgs)]
    L.lcd_estimate_motion_mono_dev.argtypes = [vp, C.POINTER(LcdMotionMonoArgs)]
    L.lcd_refine_motion_ba.argtypes = [vp, C.POINTER(LcdMotionBaArgs)]
    L.lcd_refine_motion_ba_dev.argtypes = [vp, C.POINTER(LcdMotionBaArgs)]
    L.lcd_register_icp.argtypes = [vp, C.POINTER(LcdIcpArgs)]
    L.lcd_register_icp_dev.argtypes = [vp, C.POINTER(LcdIcpArgs)]
    L.lcd_register_icp_plane.argtypes = [vp, C.POINTER(LcdIcpPlaneArgs)]
    L.lcd_register_icp_plane_dev.argtypes = [vp, C.POINTER(LcdIcpPlaneArgs)]
    L.lcd_filter_scans.argtypes = [vp, C.POINTER(LcdScanFilterArgs)]
    L.lcd_filter_scans_dev.argtypes = [vp, C.POINTER(LcdScanFilterArgs)]
    L.lcd_adjust_likelihood.argtypes = [vp, vp, C.c_int, f32]
    L.lcd_adjust_likelihood_dev.argtypes = [vp, vp, C.c_int, f32]
    L.lcd_frame_dev.argtypes = [vp, C.POINTER(LcdFrameArgs)]
    L.lcd_frame_host.argtypes = [vp, C.POINTER(LcdFrameHostArgs)]
    L.lcd_slot_count.argtypes = [vp, C.POINTER(C.c_int64)]
    L.lcd_knn2_dev.argtypes = [vp, vp, C.c_int, vp, vp]
    L.lcd_shard_knn2_dev.argtypes = [vp, vp, C.c_int, vp]
    L.lcd_shard_frame_dev.argtypes = [vp, vp, C.c_int, C.c_int, f32, i32, i32, f32, C.c_int, C.c_int, vp, i64, vp, vp, i64]
    L.lcd_finalize_dev.argtypes = [vp, vp, i64, vp]
    L.lcd_slots_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.lcd_stream.argtypes = [vp]
    L.lcd_stream.restype = vp
    L.lcd_profile_begin.argtypes = [vp, C.c_int]
    L.lcd_profile_read.argtypes = [vp, C.POINTER(f32), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    L.lcd_profile_read_likelihood.argtypes = [vp, C.POINTER(f32), C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    L.lcd_get_stats.argtypes = [vp, C.POINTER(LcdStats)]
    L.lcd_profile_score_work.argtypes = [vp, C.POINTER(i64)]
    L.lcd_set_option.argtypes = [vp, C.c_char_p, i64]
    L.lcd_record_event.argtypes = [vp, vp]
    L.lcd_bayes_configure.argtypes = [vp, vp, C.c_int, f32]
    L.lcd_bayes_reset.argtypes = [vp]
    L.lcd_bayes_set_neighbors.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.lcd_bayes_update_dev.argtypes = [vp, vp, C.c_int, vp, vp]
    L.lcd_bayes_update.argtypes = [vp, vp, vp, C.c_int, vp]
    L.lcd_bayes_posterior.argtypes = [vp, vp, C.c_int, vp]
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Engine:
    """One lcd_engine handle.  numpy in / numpy out through the C-ABI; *_dev methods take raw device pointers."""

    def __init__(self, dtype, dim, device=0, vocab_capacity=0, sig_capacity=0, stream=None, knn_mode=None, pipeline=False):
        self.L = load()
        self.dtype = LCD_F32 if dtype in (LCD_F32, np.float32, "f32") else LCD_U8
        self.np_dtype = np.float32 if self.dtype == LCD_F32 else np.uint8
        self.dim = int(dim)
        if knn_mode is None:                              # test runs of the whole suite on another filter (this glue only: the library reads no environment)
            knn_mode = os.environ.get("LCD_PY_KNN_MODE") or None
        mode = KNN_MODES[knn_mode] if (knn_mode is None or isinstance(knn_mode, str)) else int(knn_mode)
        cfg = LcdConfig(C.sizeof(LcdConfig), device, self.dtype, self.dim, vocab_capacity, sig_capacity, 0, mode, stream,
                        1 if pipeline else 0, 0)
        h = C.c_void_p()
        rc = self.L.lcd_create(C.byref(cfg), C.byref(h))
        if rc != LCD_OK:
            raise LcdError(rc, "lcd_create failed (no gfx950 device / HIP runtime?)")
        self.h = h
        # experiments: LCD_PY_OPTS="key=value,..." sets engine options on every handle this glue creates (the library reads no environment)
        for kv in filter(None, os.environ.get("LCD_PY_OPTS", "").split(",")):
            self._ck(self.L.lcd_set_option(self.h, kv.split("=")[0].encode(), int(kv.split("=")[1])))

    def close(self):
        if getattr(self, "h", None):
            self.L.lcd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != LCD_OK:
            raise LcdError(rc, self.L.lcd_last_error(self.h).decode())

    def _rows(self, a):
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError("expected [n, %d] %s" % (self.dim, self.np_dtype.__name__))
        return a

    def synchronize(self):
        self._ck(self.L.lcd_synchronize(self.h))

    def pipeline_depth(self):
        """later frame_dev calls that still enqueue work of a frame (0: plain handle): keep pipeline_depth() + 1 buffer sets"""
        return int(self.L.lcd_pipeline_depth(self.h))

    # ---- vocabulary
    def vocab_clear(self):
        self._ck(self.L.lcd_vocab_clear(self.h))

    def vocab_append(self, rows, word_ids):
        rows = self._rows(rows)
        ids = np.ascontiguousarray(word_ids, dtype=np.int32)
        assert ids.shape[0] == rows.shape[0]
        self._ck(self.L.lcd_vocab_append(self.h, _p(rows), rows.shape[0], _p(ids)))

    def vocab_remove(self, word_ids):
        ids = np.ascontiguousarray(word_ids, dtype=np.int32)
        self._ck(self.L.lcd_vocab_remove(self.h, _p(ids), ids.shape[0]))

    def vocab_remove_unused(self, capacity=0):
        """Memory::cleanUnusedWords from the device's reference counts -> (number removed, the first `capacity` removed ids)"""
        out = np.zeros(max(capacity, 1), np.int32)
        n = C.c_int32()
        self._ck(self.L.lcd_vocab_remove_unused(self.h, _p(out) if capacity else None, capacity, C.byref(n)))
        return n.value, out[: min(n.value, capacity)]

    def vocab_remove_unused_async(self):
        """cleanUnusedWords enqueued behind the frames in flight: nothing is completed, nothing comes back"""
        self._ck(self.L.lcd_vocab_remove_unused_async(self.h))

    def vocab_rebuild(self):
        self._ck(self.L.lcd_vocab_rebuild(self.h))

    def vocab_count(self):
        r, l = C.c_int64(), C.c_int64()
        self._ck(self.L.lcd_vocab_count(self.h, C.byref(r), C.byref(l)))
        return r.value, l.value

    def vocab_read(self, first, n):
        rows = np.empty((n, self.dim), self.np_dtype)
        ids = np.empty(n, np.int32)
        self._ck(self.L.lcd_vocab_read(self.h, first, n, _p(rows), _p(ids)))
        return rows, ids

    # ---- search
    def knn2(self, queries):
        q = self._rows(queries)
        ids = np.zeros((q.shape[0], 2), np.int32)
        dist = np.zeros((q.shape[0], 2), np.float32)
        self._ck(self.L.lcd_knn2(self.h, _p(q), q.shape[0], _p(ids), _p(dist)))
        return ids, dist

    def selfdist(self, queries):
        q = self._rows(queries)
        out = np.zeros((q.shape[0], q.shape[0]), np.float32)
        self._ck(self.L.lcd_selfdist(self.h, _p(q), q.shape[0], _p(out)))
        return out

    def quantize(self, descriptors, incremental=True, new_words_compared=True, nndr=0.8):
        q = self._rows(descriptors)
        out = np.zeros(q.shape[0], np.int32)
        nn = C.c_int32()
        flags = (LCD_Q_INCREMENTAL if incremental else 0) | (LCD_Q_NEW_WORDS_COMPARED if new_words_compared else 0)
        self._ck(self.L.lcd_quantize(self.h, _p(q), q.shape[0], flags, nndr, _p(out), C.byref(nn)))
        return out, nn.value

    def find_nn(self, queries, extra_rows=None, extra_word_ids=None, incremental=True, nndr=0.8):
        q = self._rows(queries)
        out = np.zeros(q.shape[0], np.int32)
        ne = 0
        er = ei = None
        if extra_rows is not None and len(extra_rows):
            er = self._rows(extra_rows)
            ei = np.ascontiguousarray(extra_word_ids, dtype=np.int32)
            ne = er.shape[0]
        flags = LCD_Q_INCREMENTAL if incremental else 0
        self._ck(self.L.lcd_find_nn(self.h, _p(q), q.shape[0], _p(er), _p(ei), ne, flags, nndr, _p(out)))
        return out

    # ---- inverted index
    def sig_add(self, sig_id, word_ids, ni=None):
        w = np.ascontiguousarray(word_ids, dtype=np.int32)
        self._ck(self.L.lcd_sig_add(self.h, sig_id, _p(w), w.shape[0], w.shape[0] if ni is None else ni))

    def sig_add_bulk(self, sig_ids, offsets, word_ids, ni=None):
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        w = np.ascontiguousarray(word_ids, dtype=np.int32)
        n = None if ni is None else np.ascontiguousarray(ni, dtype=np.int32)
        self._ck(self.L.lcd_sig_add_bulk(self.h, s.shape[0], _p(s), _p(o), _p(w), _p(n)))

    def sig_remove(self, sig_id):
        self._ck(self.L.lcd_sig_remove(self.h, sig_id))

    def sig_count(self):
        a, b = C.c_int64(), C.c_int64()
        self._ck(self.L.lcd_sig_count(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def word_nrefs(self, word_id):
        v = C.c_int32()
        self._ck(self.L.lcd_word_nrefs(self.h, word_id, C.byref(v)))
        return v.value

    def likelihood(self, query_word_ids, sig_ids, N):
        w = np.ascontiguousarray(query_word_ids, dtype=np.int32)
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        out = np.zeros(s.shape[0], np.float32)
        self._ck(self.L.lcd_likelihood(self.h, _p(w), w.shape[0], _p(s), s.shape[0], float(N), _p(out)))
        return out

    def similarity(self, query_word_ids, sig_ids, with_counts=False):
        """lcd_similarity: Signature::compareTo's words branch of the query against sig_ids; with_counts: also (pairs, valid words)."""
        w = np.ascontiguousarray(query_word_ids, dtype=np.int32)
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        out = np.zeros(s.shape[0], np.float32)
        pairs = np.zeros(s.shape[0], np.int32) if with_counts else None
        valid = np.zeros(s.shape[0], np.int32) if with_counts else None
        self._ck(self.L.lcd_similarity(self.h, _p(w), w.shape[0], _p(s), s.shape[0], _p(out), _p(pairs), _p(valid)))
        return (out, pairs, valid) if with_counts else out

    def similarity_dev(self, d_query_word_ids, d_out):
        """lcd_similarity_dev on torch tensors of the engine's device: int32 word ids in, float32 similarity over the signature slots out
        (d_out holds at least slot_count entries); enqueued on the engine stream, not synchronised."""
        import torch
        if d_query_word_ids.dtype != torch.int32 or d_out.dtype != torch.float32 or not (d_query_word_ids.is_cuda and d_out.is_cuda) or \
                not (d_query_word_ids.is_contiguous() and d_out.is_contiguous()):
            raise ValueError("similarity_dev: contiguous device tensors expected, int32 word ids and float32 output")
        self._ck(self.L.lcd_similarity_dev(self.h, d_query_word_ids.data_ptr() if d_query_word_ids.numel() else None, int(d_query_word_ids.numel()),
                                           d_out.data_ptr(), int(d_out.numel())))

    # ---- two-frame descriptor matching (stateless: nothing of the handle is read or written)
    def _match_args(self, mode, n_pairs, from_offsets, to_offsets, new_words_compared, nndr):
        mode = MATCH_MODES[mode] if isinstance(mode, str) else int(mode)
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64)
        if fo.shape != (n_pairs + 1,) or to.shape != (n_pairs + 1,):
            raise ValueError("match_pairs: offsets are [n_pairs + 1]")
        flags = LCD_Q_INCREMENTAL | (LCD_Q_NEW_WORDS_COMPARED if new_words_compared else 0)
        a = LcdMatchArgs(C.sizeof(LcdMatchArgs), mode, n_pairs, flags if mode == LCD_MATCH_DICTIONARY else 0, nndr, 0)
        a.from_offsets, a.to_offsets = fo.ctypes.data, to.ctypes.data
        return a, mode, fo, to

    def match_pairs(self, from_rows, to_rows, from_offsets, to_offsets, mode="dictionary", new_words_compared=True, nndr=0.8,
                    from_word_ids=None):
        """lcd_match_pairs over host arrays: pair p is from_rows[from_offsets[p]:from_offsets[p+1]] against to_rows[to_offsets[p]:...].
        "dictionary" -> (from_word_ids, to_word_ids); "cross_check" -> (match per to-row: from-row index within the pair or -1, distance)."""
        f, t = self._rows(from_rows), self._rows(to_rows)
        a, mode, fo, to = self._match_args(mode, len(from_offsets) - 1, from_offsets, to_offsets, new_words_compared, nndr)
        if int(fo[-1]) != f.shape[0] or int(to[-1]) != t.shape[0]:
            raise ValueError("match_pairs: the last offset is the number of rows")
        ids = None if from_word_ids is None else np.ascontiguousarray(from_word_ids, dtype=np.int32)
        if ids is not None and ids.shape != (f.shape[0],):
            raise ValueError("match_pairs: one word id per from-row")
        a.from_rows, a.to_rows, a.from_word_ids = _p(f), _p(t), _p(ids)
        nf, nt = f.shape[0], t.shape[0]
        if mode == LCD_MATCH_DICTIONARY:
            o1, o2 = np.zeros(max(nf, 1), np.int32), np.zeros(max(nt, 1), np.int32)
            a.out_from_word_ids, a.out_to_word_ids = _p(o1), _p(o2)
        else:
            o1, o2 = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.float32)
            a.out_to_match, a.out_to_dist = _p(o1), _p(o2)
        self._ck(self.L.lcd_match_pairs(self.h, C.byref(a)))
        return (o1[:nf], o2[:nt]) if mode == LCD_MATCH_DICTIONARY else (o1[:nt], o2[:nt])

    def match_pair(self, from_rows, to_rows, mode="dictionary", **kw):
        """one pair: match_pairs with the offsets [0, n]"""
        return self.match_pairs(from_rows, to_rows, [0, len(from_rows)], [0, len(to_rows)], mode, **kw)

    def match_pairs_dev(self, d_from, d_to, from_offsets, to_offsets, d_out_a, d_out_b, mode="dictionary", new_words_compared=True,
                        nndr=0.8, d_from_word_ids=None):
        """lcd_match_pairs_dev on torch tensors of the engine's device (rows of the handle's dtype, int32 ids; offsets stay on the host):
        "dictionary" writes d_out_a = from word ids, d_out_b = to word ids (int32); "cross_check" d_out_a = match per to-row (int32),
        d_out_b = distance per to-row (float32) or None.  Enqueued on the engine stream, not synchronised."""
        a, mode, fo, to = self._match_args(mode, len(from_offsets) - 1, from_offsets, to_offsets, new_words_compared, nndr)
        ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
        a.from_rows, a.to_rows, a.from_word_ids = ptr(d_from), ptr(d_to), ptr(d_from_word_ids)
        if mode == LCD_MATCH_DICTIONARY:
            a.out_from_word_ids, a.out_to_word_ids = ptr(d_out_a), ptr(d_out_b)
        else:
            a.out_to_match, a.out_to_dist = ptr(d_out_a), ptr(d_out_b)
        self._ck(self.L.lcd_match_pairs_dev(self.h, C.byref(a)))

    # ---- guided two-frame matching (stateless; the projection is the caller's)
    def _guided_args(self, from_offsets, to_offsets, corner_offsets, radius, nndr, nn_type, direction):
        offs = [np.ascontiguousarray(o, dtype=np.int64) for o in (from_offsets, to_offsets, corner_offsets)]
        n_pairs = offs[0].shape[0] - 1
        if n_pairs < 0 or any(o.shape != (n_pairs + 1,) for o in offs):
            raise ValueError("match_guided: offsets are [n_pairs + 1]")
        direction = GUIDED_DIRECTIONS[direction] if isinstance(direction, str) else int(direction)
        nn_type = GUIDED_NN_TYPES[nn_type] if isinstance(nn_type, str) else int(nn_type)
        a = LcdGuidedArgs(C.sizeof(LcdGuidedArgs), direction, nn_type, n_pairs, radius, nndr)
        a.from_offsets, a.to_offsets, a.corner_offsets = (o.ctypes.data for o in offs)
        return a, direction, offs

    def match_guided(self, from_rows, to_rows, corners, corner_from_row, to_points, from_offsets, to_offsets, corner_offsets, radius=40.0,
                     nndr=0.8, nn_type="ratio", direction="projected_to_frame", with_dist=True):
        """lcd_match_guided over host arrays (include/lcd.h has the rule): pair p owns from_rows[from_offsets[p]:from_offsets[p+1]], the
        to-rows and to_points [to_offsets[p]:...] and the corners / corner_from_row [corner_offsets[p]:...].
        -> (count, match, dist [n_queries x 2] or None, to_owner or None); queries are the corners ("projected_to_frame", which also
        gives to_owner per to-row) or the to-rows ("frame_to_projected")."""
        f, t = self._rows(from_rows), self._rows(to_rows)
        c = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 2)
        r = np.ascontiguousarray(corner_from_row, dtype=np.int32).reshape(-1)
        pts = np.ascontiguousarray(to_points, dtype=np.float32).reshape(-1, 2)
        a, direction, (fo, to, co) = self._guided_args(from_offsets, to_offsets, corner_offsets, radius, nndr, nn_type, direction)
        if int(fo[-1]) != f.shape[0] or int(to[-1]) != t.shape[0] or pts.shape[0] != t.shape[0] or int(co[-1]) != c.shape[0] or r.shape[0] != c.shape[0]:
            raise ValueError("match_guided: the last offset is the number of rows / corners, one point per to-row, one from-row per corner")
        p2f = direction == LCD_GUIDED_PROJECTED_TO_FRAME
        nq, nt = (c.shape[0] if p2f else t.shape[0]), t.shape[0]
        count, match = np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.int32)
        dist = np.zeros((max(nq, 1), 2), np.float32) if with_dist else None
        owner = np.zeros(max(nt, 1), np.int32) if p2f else None
        a.from_rows, a.to_rows, a.corners, a.corner_from_row, a.to_points = _p(f), _p(t), _p(c), _p(r), _p(pts)
        a.out_count, a.out_match, a.out_dist, a.out_to_owner = _p(count), _p(match), _p(dist), _p(owner)
        self._ck(self.L.lcd_match_guided(self.h, C.byref(a)))
        return count[:nq], match[:nq], (dist[:nq] if with_dist else None), (owner[:nt] if p2f else None)

    def match_guided_dev(self, d_from, d_to, d_corners, d_corner_from_row, d_to_points, from_offsets, to_offsets, corner_offsets, d_count,
                         d_match, d_dist, d_to_owner, radius=40.0, nndr=0.8, nn_type="ratio", direction="projected_to_frame"):
        """lcd_match_guided_dev on torch tensors of the engine's device (rows of the handle's dtype, float32 points, int32 corner_from_row and
        outputs; the offsets stay on the host); d_dist may be None, d_to_owner is written in "projected_to_frame" only.  Enqueued on the
        engine stream, not synchronised."""
        a, direction, _ = self._guided_args(from_offsets, to_offsets, corner_offsets, radius, nndr, nn_type, direction)
        ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
        a.from_rows, a.to_rows, a.corners, a.corner_from_row, a.to_points = ptr(d_from), ptr(d_to), ptr(d_corners), ptr(d_corner_from_row), ptr(d_to_points)
        a.out_count, a.out_match, a.out_dist, a.out_to_owner = ptr(d_count), ptr(d_match), ptr(d_dist), ptr(d_to_owner)
        self._ck(self.L.lcd_match_guided_dev(self.h, C.byref(a)))

    # ---- keypoint limiting and the -1, -2, ... word ids (stateless; include/lcd.h has the rule)
    def _select_args(self, offsets, max_features, order, grid, image_size, aux_bytes, ssc=False):
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        n_frames = off.shape[0] - 1
        if n_frames < 0:
            raise ValueError("select_features: offsets are [n_frames + 1]")
        order = SELECT_ORDERS[order] if isinstance(order, str) else int(order)
        size = None if image_size is None else np.ascontiguousarray(image_size, dtype=np.int32).reshape(-1, 2)
        if size is not None and size.shape[0] != n_frames:
            raise ValueError("select_features: one (width, height) per frame")
        a = LcdSelectArgs(C.sizeof(LcdSelectArgs), n_frames, order, int(max_features), int(grid[0]), int(grid[1]), int(aux_bytes),
                          LCD_SELECT_SSC if ssc else 0)
        a.offsets, a.image_size = off.ctypes.data, (None if size is None else size.ctypes.data)
        return a, off, size

    def select_features(self, response, offsets, max_features, order="keep_order", grid=(1, 1), image_size=None, points=None, rows=None, aux=None, n_in=None, ssc=False):
        """lcd_select_features over host arrays: frame f owns the features [offsets[f], offsets[f+1]); aux is a [N x aux_bytes] uint8 payload.
        -> (count [n_frames], index [N], rows or None, aux or None); only the first count[f] entries of a frame's region are meaningful.
        ssc: LCD_SELECT_SSC, Kp/SSC's square covering (points and image sizes are needed; count is data-dependent)."""
        r = np.ascontiguousarray(response, dtype=np.float32).reshape(-1)
        p = None if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        d = None if rows is None else self._rows(rows)
        x = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint8).reshape(r.shape[0], -1)
        a, off, _size = self._select_args(offsets, max_features, order, grid, image_size, 0 if x is None else x.shape[1], ssc)
        n = r.shape[0]
        if int(off[-1]) != n or (p is not None and p.shape[0] != n) or (d is not None and d.shape[0] != n):
            raise ValueError("select_features: the last offset is the number of features; one point and one row per feature")
        count, index = np.zeros(max(a.n_frames, 1), np.int32), np.zeros(max(n, 1), np.int32)
        out_rows = None if d is None else np.zeros((max(n, 1), self.dim), self.np_dtype)
        out_aux = None if x is None else np.zeros((max(n, 1), x.shape[1]), np.uint8)
        a.response, a.points, a.rows, a.aux = _p(r), _p(p), _p(d), _p(x)
        a.out_count, a.out_index, a.out_rows, a.out_aux = _p(count), _p(index), _p(out_rows), _p(out_aux)
        k = None if n_in is None else np.ascontiguousarray(n_in, dtype=np.int32).reshape(a.n_frames)
        a.n_in = _p(k)
        self._ck(self.L.lcd_select_features(self.h, C.byref(a)))
        return count[:a.n_frames], index[:n], (None if d is None else out_rows[:n]), (None if x is None else out_aux[:n])

    def select_features_dev(self, d_response, offsets, max_features, d_count, d_index, order="keep_order", grid=(1, 1), image_size=None,
                            d_points=None, d_rows=None, d_aux=None, aux_bytes=0, d_out_rows=None, d_out_aux=None, d_n_in=None, ssc=False):
        """lcd_select_features_dev on torch tensors of the engine's device (float32 responses and points, rows of the handle's dtype, int32
        outputs; offsets and image sizes stay on the host).  Enqueued on the engine stream, not synchronised."""
        a, _off, _size = self._select_args(offsets, max_features, order, grid, image_size, aux_bytes, ssc)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a.response, a.points, a.rows, a.aux = ptr(d_response), ptr(d_points), ptr(d_rows), ptr(d_aux)
        a.out_count, a.out_index, a.out_rows, a.out_aux = ptr(d_count), ptr(d_index), ptr(d_out_rows), ptr(d_out_aux)
        a.n_in = ptr(d_n_in)
        self._ck(self.L.lcd_select_features_dev(self.h, C.byref(a)))

    def expand_word_ids(self, offsets, count, index, word_ids, first_new_word_id=None, n_features=None):
        """lcd_expand_word_ids over host arrays -> one id per feature [N]"""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        c = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        i = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(word_ids, dtype=np.int32).reshape(-1)
        f = None if first_new_word_id is None else np.ascontiguousarray(first_new_word_id, dtype=np.int32).reshape(-1)
        n_frames, n = off.shape[0] - 1, int(off[-1])
        if n_frames < 0 or c.shape[0] != n_frames or i.shape[0] != n or w.shape[0] != n or (f is not None and f.shape[0] != n_frames):
            raise ValueError("expand_word_ids: count and first ids per frame, index and ids per feature")
        out = np.zeros(max(n, 1), np.int32)
        a = LcdExpandArgs(C.sizeof(LcdExpandArgs), n_frames)
        a.offsets, a.count, a.index, a.word_ids, a.first_new_word_id, a.out_word_ids = off.ctypes.data, _p(c), _p(i), _p(w), _p(f), _p(out)
        k = None if n_features is None else np.ascontiguousarray(n_features, dtype=np.int32).reshape(n_frames)
        a.n_features = _p(k)
        self._ck(self.L.lcd_expand_word_ids(self.h, C.byref(a)))
        return out[:n]

    def expand_word_ids_dev(self, offsets, d_count, d_index, d_word_ids, d_out_word_ids, d_first_new_word_id=None, d_n_features=None):
        """lcd_expand_word_ids_dev on int32 torch tensors of the engine's device (the offsets stay on the host); enqueued, not synchronised"""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a = LcdExpandArgs(C.sizeof(LcdExpandArgs), off.shape[0] - 1)
        a.offsets = off.ctypes.data
        a.count, a.index, a.word_ids, a.first_new_word_id, a.out_word_ids = ptr(d_count), ptr(d_index), ptr(d_word_ids), ptr(d_first_new_word_id), ptr(d_out_word_ids)
        a.n_features = ptr(d_n_features)
        self._ck(self.L.lcd_expand_word_ids_dev(self.h, C.byref(a)))

    # ---- depth to 3-D keypoints and the depth filter (stateless; include/lcd.h has the rule)
    @staticmethod
    def _kp3d_images(images, data_ptr):
        """images: one dict per frame -- data (a 2-D uint16 or float32 array / tensor, possibly a view with a row stride), cameras (a list of
        dicts fx, fy, cx, cy and optionally image_width, image_height, transform (12 floats or None)), optionally width (pixels, when the
        array is wider than the image) -> (lcd_depth_image array, what must stay alive)"""
        arr = (LcdDepthImage * max(len(images), 1))()
        keep = []
        for f, im in enumerate(images):
            d = im["data"]
            u16 = "16" in str(d.dtype)
            cams = (LcdCamera * len(im["cameras"]))()
            for c, m in enumerate(im["cameras"]):
                t = m.get("transform")
                cams[c] = LcdCamera(m["fx"], m["fy"], m["cx"], m["cy"], int(m.get("image_width", 0)), int(m.get("image_height", 0)),
                                    0 if t is None else 1, 0, (C.c_float * 12)(*([0.0] * 12 if t is None else [float(v) for v in t])))
            keep.append(cams)
            pitch = im["pitch_bytes"] if "pitch_bytes" in im else int(d.strides[0] if hasattr(d, "strides") else d.stride(0) * d.element_size())
            arr[f] = LcdDepthImage(data_ptr(d), pitch, int(im.get("width", d.shape[1])), int(im.get("height", d.shape[0])),
                                   int(im.get("type", LCD_DEPTH_U16_MM if u16 else LCD_DEPTH_F32_M)), int(im.get("n_cameras", len(im["cameras"]))), cams)
        return arr, keep

    def keypoints_3d(self, points, offsets, images, filter="keep_all", min_depth=0.0, max_depth=0.0, response=None, rows=None, aux=None, xyz=True):
        """lcd_keypoints_3d over host arrays -> dict(count [n_frames], index [N], xyz [N x 3] or None, points, response, rows, aux or None);
        only the first count[f] entries of a frame's region are meaningful (outputs start as zeros)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n, n_frames = p.shape[0], off.shape[0] - 1
        r = None if response is None else np.ascontiguousarray(response, dtype=np.float32).reshape(-1)
        d = None if rows is None else self._rows(rows)
        x = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint8).reshape(n, -1)
        flt = KP3D_FILTERS[filter] if isinstance(filter, str) else int(filter)
        arr, keep = self._kp3d_images(images, lambda a: a.ctypes.data)
        a = LcdKeypoints3dArgs(C.sizeof(LcdKeypoints3dArgs), n_frames, flt, 0 if x is None else x.shape[1], float(min_depth), float(max_depth))
        a.offsets, a.images = off.ctypes.data, arr
        out = dict(count=np.zeros(max(n_frames, 1), np.int32), index=np.zeros(max(n, 1), np.int32),
                   xyz=np.zeros((max(n, 1), 3), np.float32) if xyz else None, points=np.zeros((max(n, 1), 2), np.float32),
                   response=None if r is None else np.zeros(max(n, 1), np.float32),
                   rows=None if d is None else np.zeros((max(n, 1), self.dim), self.np_dtype),
                   aux=None if x is None else np.zeros((max(n, 1), x.shape[1]), np.uint8))
        a.points, a.response, a.rows, a.aux = _p(p), _p(r), _p(d), _p(x)
        a.out_count, a.out_index, a.out_xyz, a.out_points = _p(out["count"]), _p(out["index"]), _p(out["xyz"]), _p(out["points"])
        a.out_response, a.out_rows, a.out_aux = _p(out["response"]), _p(out["rows"]), _p(out["aux"])
        self._ck(self.L.lcd_keypoints_3d(self.h, C.byref(a)))
        out["count"] = out["count"][:n_frames]
        for k in ("index", "xyz", "points", "response", "rows", "aux"):
            out[k] = None if out[k] is None else out[k][:n]
        return out

    def keypoints_3d_dev(self, d_points, offsets, images, d_count, d_index, d_xyz=None, filter="keep_all", min_depth=0.0, max_depth=0.0,
                         d_response=None, d_rows=None, d_aux=None, aux_bytes=0, d_out_points=None, d_out_response=None, d_out_rows=None,
                         d_out_aux=None):
        """lcd_keypoints_3d_dev on torch tensors of the engine's device (the images' data too; offsets, images and cameras stay on the host).
        Enqueued on the engine stream, not synchronised."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        flt = KP3D_FILTERS[filter] if isinstance(filter, str) else int(filter)
        arr, keep = self._kp3d_images(images, lambda t: t.data_ptr())
        a = LcdKeypoints3dArgs(C.sizeof(LcdKeypoints3dArgs), off.shape[0] - 1, flt, int(aux_bytes), float(min_depth), float(max_depth))
        a.offsets, a.images = off.ctypes.data, arr
        a.points, a.response, a.rows, a.aux = ptr(d_points), ptr(d_response), ptr(d_rows), ptr(d_aux)
        a.out_count, a.out_index, a.out_xyz, a.out_points = ptr(d_count), ptr(d_index), ptr(d_xyz), ptr(d_out_points)
        a.out_response, a.out_rows, a.out_aux = ptr(d_out_response), ptr(d_out_rows), ptr(d_out_aux)
        self._ck(self.L.lcd_keypoints_3d_dev(self.h, C.byref(a)))

    # ---- stereo keypoints to 3-D (stateless; include/lcd.h has the rule)
    @staticmethod
    def _stereo_images(images, data_ptr):
        """images: one dict per frame -- left, right (2-D uint8 arrays / tensors, possibly views with a row stride), camera (a dict fx, fy, cx,
        cy, right_cx, baseline and optionally transform (12 floats or None)), optionally width, height, left_pitch_bytes, right_pitch_bytes
        -> (lcd_stereo_image array, what must stay alive)"""
        arr = (LcdStereoImage * max(len(images), 1))()
        keep = []
        pitch_of = lambda d: 0 if d is None else int(d.strides[0] if hasattr(d, "strides") else d.stride(0) * d.element_size())
        for f, im in enumerate(images):
            m = im["camera"]
            cam = None
            if m is not None:
                t = m.get("transform")
                cam = LcdStereoCamera(m["fx"], m["fy"], m["cx"], m["cy"], m.get("right_cx", 0.0), m["baseline"], 0 if t is None else 1, 0,
                                      (C.c_float * 12)(*([0.0] * 12 if t is None else [float(v) for v in t])))
                keep.append(cam)
            l, r = im["left"], im["right"]
            arr[f] = LcdStereoImage(None if l is None else data_ptr(l), None if r is None else data_ptr(r),
                                    int(im["left_pitch_bytes"]) if "left_pitch_bytes" in im else pitch_of(l),
                                    int(im["right_pitch_bytes"]) if "right_pitch_bytes" in im else pitch_of(r),
                                    int(im.get("width", l.shape[1] if l is not None else 0)), int(im.get("height", l.shape[0] if l is not None else 0)),
                                    None if cam is None else C.pointer(cam))
        return arr, keep

    def keypoints_3d_stereo(self, points, offsets, images, params=None, filter="keep_all", min_depth=0.0, max_depth=0.0, response=None, rows=None,
                            aux=None, right=True, status=True):
        """lcd_keypoints_3d_stereo over host arrays -> dict(count [n_frames], index [N], xyz [N x 3], points, response, rows, aux or None,
        right [N x 2] and status [N] by input index or None); only the first count[f] entries of a frame's region of the compacted
        arrays are meaningful (outputs start as zeros)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n, n_frames = p.shape[0], off.shape[0] - 1
        r = None if response is None else np.ascontiguousarray(response, dtype=np.float32).reshape(-1)
        d = None if rows is None else self._rows(rows)
        x = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint8).reshape(n, -1)
        flt = KP3D_FILTERS[filter] if isinstance(filter, str) else int(filter)
        arr, keep = self._stereo_images(images, lambda a: a.ctypes.data)
        sp = params if isinstance(params, LcdStereoParams) else stereo_params(params)
        a = LcdKeypoints3dStereoArgs(C.sizeof(LcdKeypoints3dStereoArgs), n_frames, flt, 0 if x is None else x.shape[1], float(min_depth), float(max_depth))
        a.offsets, a.images, a.params = off.ctypes.data, arr, C.pointer(sp)
        out = dict(count=np.zeros(max(n_frames, 1), np.int32), index=np.zeros(max(n, 1), np.int32), xyz=np.zeros((max(n, 1), 3), np.float32),
                   points=np.zeros((max(n, 1), 2), np.float32), response=None if r is None else np.zeros(max(n, 1), np.float32),
                   rows=None if d is None else np.zeros((max(n, 1), self.dim), self.np_dtype),
                   aux=None if x is None else np.zeros((max(n, 1), x.shape[1]), np.uint8),
                   right=np.zeros((max(n, 1), 2), np.float32) if right else None, status=np.zeros(max(n, 1), np.uint8) if status else None)
        a.points, a.response, a.rows, a.aux = _p(p), _p(r), _p(d), _p(x)
        a.out_count, a.out_index, a.out_xyz, a.out_points = _p(out["count"]), _p(out["index"]), _p(out["xyz"]), _p(out["points"])
        a.out_response, a.out_rows, a.out_aux = _p(out["response"]), _p(out["rows"]), _p(out["aux"])
        a.out_right, a.out_status = _p(out["right"]), _p(out["status"])
        self._ck(self.L.lcd_keypoints_3d_stereo(self.h, C.byref(a)))
        out["count"] = out["count"][:n_frames]
        for k in ("index", "xyz", "points", "response", "rows", "aux", "right", "status"):
            out[k] = None if out[k] is None else out[k][:n]
        return out

    def keypoints_3d_stereo_dev(self, d_points, offsets, images, d_count, d_index, d_xyz, params=None, filter="keep_all", min_depth=0.0, max_depth=0.0,
                                d_response=None, d_rows=None, d_aux=None, aux_bytes=0, d_out_points=None, d_out_response=None, d_out_rows=None,
                                d_out_aux=None, d_out_right=None, d_out_status=None):
        """lcd_keypoints_3d_stereo_dev on torch tensors of the engine's device (the images too; offsets, images, cameras and params stay on
        the host).  Enqueued on the engine stream, not synchronised."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        flt = KP3D_FILTERS[filter] if isinstance(filter, str) else int(filter)
        arr, keep = self._stereo_images(images, lambda t: t.data_ptr())
        sp = params if isinstance(params, LcdStereoParams) else stereo_params(params)
        a = LcdKeypoints3dStereoArgs(C.sizeof(LcdKeypoints3dStereoArgs), off.shape[0] - 1, flt, int(aux_bytes), float(min_depth), float(max_depth))
        a.offsets, a.images, a.params = off.ctypes.data, arr, C.pointer(sp)
        a.points, a.response, a.rows, a.aux = ptr(d_points), ptr(d_response), ptr(d_rows), ptr(d_aux)
        a.out_count, a.out_index, a.out_xyz, a.out_points = ptr(d_count), ptr(d_index), ptr(d_xyz), ptr(d_out_points)
        a.out_response, a.out_rows, a.out_aux = ptr(d_out_response), ptr(d_out_rows), ptr(d_out_aux)
        a.out_right, a.out_status = ptr(d_out_right), ptr(d_out_status)
        self._ck(self.L.lcd_keypoints_3d_stereo_dev(self.h, C.byref(a)))

    # ---- optical-flow correspondences (stateless; include/lcd.h has the rule)
    @staticmethod
    def _flow_pairs(pairs, data_ptr):
        """pairs: one dict per pair -- from, to (2-D uint8 arrays / tensors, possibly views with a row stride), optionally max_level (3),
        use_initial (0), width, height, from_pitch_bytes, to_pitch_bytes -> the lcd_flow_pair array"""
        arr = (LcdFlowPair * max(len(pairs), 1))()
        pitch_of = lambda d: 0 if d is None else int(d.strides[0] if hasattr(d, "strides") else d.stride(0) * d.element_size())
        for k, pr in enumerate(pairs):
            f, t = pr["from"], pr["to"]
            some = f if f is not None else t
            arr[k] = LcdFlowPair(None if f is None else data_ptr(f), None if t is None else data_ptr(t),
                                 int(pr["from_pitch_bytes"]) if "from_pitch_bytes" in pr else pitch_of(f),
                                 int(pr["to_pitch_bytes"]) if "to_pitch_bytes" in pr else pitch_of(t),
                                 int(pr.get("width", some.shape[1] if some is not None else 0)), int(pr.get("height", some.shape[0] if some is not None else 0)),
                                 int(pr.get("max_level", 3)), int(pr.get("use_initial", 0)))
        return arr

    def track_flow(self, points, offsets, pairs, params=None, initial=None, aux=None, track=True, status=True, err=True):
        """lcd_track_flow over host arrays -> dict(count [n_pairs], index [N], from, to [N x 2], aux or None, track [N x 2], status [N] and
        err [N] by input index or None); only the first count[p] entries of a pair's region of the compacted arrays are meaningful
        (outputs start as zeros)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        q = None if initial is None else np.ascontiguousarray(initial, dtype=np.float32).reshape(-1, 2)
        n, n_pairs = p.shape[0], off.shape[0] - 1
        x = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint8).reshape(n, -1)
        arr = self._flow_pairs(pairs, lambda a: a.ctypes.data)
        fp = params if isinstance(params, LcdFlowParams) else flow_params(params)
        a = LcdTrackFlowArgs(C.sizeof(LcdTrackFlowArgs), n_pairs, 0 if x is None else x.shape[1], 0)
        a.offsets, a.pairs, a.params = off.ctypes.data, arr, C.pointer(fp)
        m = max(n, 1)
        out = {"count": np.zeros(max(n_pairs, 1), np.int32), "index": np.zeros(m, np.int32), "from": np.zeros((m, 2), np.float32),
               "to": np.zeros((m, 2), np.float32), "aux": None if x is None else np.zeros((m, x.shape[1]), np.uint8),
               "track": np.zeros((m, 2), np.float32) if track else None, "status": np.zeros(m, np.uint8) if status else None,
               "err": np.zeros(m, np.float32) if err else None}
        a.points, a.initial, a.aux = _p(p), _p(q), _p(x)
        a.out_count, a.out_index, a.out_from, a.out_to, a.out_aux = _p(out["count"]), _p(out["index"]), _p(out["from"]), _p(out["to"]), _p(out["aux"])
        a.out_track, a.out_status, a.out_err = _p(out["track"]), _p(out["status"]), _p(out["err"])
        self._ck(self.L.lcd_track_flow(self.h, C.byref(a)))
        out["count"] = out["count"][:n_pairs]
        for k in ("index", "from", "to", "aux", "track", "status", "err"):
            out[k] = None if out[k] is None else out[k][:n]
        return out

    def track_flow_dev(self, d_points, offsets, pairs, d_count, d_index, d_from, d_to, params=None, d_initial=None, d_aux=None, aux_bytes=0,
                       d_out_aux=None, d_out_track=None, d_out_status=None, d_out_err=None):
        """lcd_track_flow_dev on torch tensors of the engine's device (the images too; offsets, pairs and params stay on the host).
        Enqueued on the engine stream, not synchronised."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        arr = self._flow_pairs(pairs, lambda t: t.data_ptr())
        fp = params if isinstance(params, LcdFlowParams) else flow_params(params)
        a = LcdTrackFlowArgs(C.sizeof(LcdTrackFlowArgs), off.shape[0] - 1, int(aux_bytes), 0)
        a.offsets, a.pairs, a.params = off.ctypes.data, arr, C.pointer(fp)
        a.points, a.initial, a.aux = ptr(d_points), ptr(d_initial), ptr(d_aux)
        a.out_count, a.out_index, a.out_from, a.out_to, a.out_aux = ptr(d_count), ptr(d_index), ptr(d_from), ptr(d_to), ptr(d_out_aux)
        a.out_track, a.out_status, a.out_err = ptr(d_out_track), ptr(d_out_status), ptr(d_out_err)
        self._ck(self.L.lcd_track_flow_dev(self.h, C.byref(a)))

    # ---- 3-D to 3-D motion estimation (stateless; include/lcd.h has the rule)
    def estimate_motion_3d(self, from_ids, from_xyz, from_offsets, to_ids, to_xyz, to_offsets, min_inliers=20, inlier_distance=0.1, iterations=300,
                           refine_iterations=5, seed=0, struct_size=None):
        """lcd_estimate_motion_3d over host arrays, all pairs concatenated -> dict(transform [n_pairs x 12], status, n_matches, n_inliers,
        variance [n_pairs], matches [Nf], inliers [Nf]); outputs start as -1 / NaN so that what the call left alone shows"""
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fi, ti = np.ascontiguousarray(from_ids, dtype=np.int32).reshape(-1), np.ascontiguousarray(to_ids, dtype=np.int32).reshape(-1)
        fx, tx = np.ascontiguousarray(from_xyz, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
        n_pairs, n = fo.shape[0] - 1, fi.shape[0]
        out = dict(transform=np.full((max(n_pairs, 1), 12), np.nan, np.float32), status=np.full(max(n_pairs, 1), -1, np.int32),
                   n_matches=np.full(max(n_pairs, 1), -1, np.int32), n_inliers=np.full(max(n_pairs, 1), -1, np.int32),
                   variance=np.full(max(n_pairs, 1), np.nan, np.float64), matches=np.full(max(n, 1), -1, np.int32), inliers=np.full(max(n, 1), -1, np.int32))
        a = LcdMotion3dArgs(C.sizeof(LcdMotion3dArgs) if struct_size is None else struct_size, n_pairs, int(min_inliers), int(iterations),
                            int(refine_iterations), int(seed) & 0xFFFFFFFF, float(inlier_distance))
        a.from_word_ids, a.from_xyz, a.to_word_ids, a.to_xyz = _p(fi), _p(fx), _p(ti), _p(tx)
        a.from_offsets, a.to_offsets = fo.ctypes.data, to.ctypes.data
        a.out_transform, a.out_status, a.out_n_matches, a.out_n_inliers = _p(out["transform"]), _p(out["status"]), _p(out["n_matches"]), _p(out["n_inliers"])
        a.out_variance, a.out_matches, a.out_inliers = _p(out["variance"]), _p(out["matches"]), _p(out["inliers"])
        self._ck(self.L.lcd_estimate_motion_3d(self.h, C.byref(a)))
        for k in ("transform", "status", "n_matches", "n_inliers", "variance"):
            out[k] = out[k][:max(n_pairs, 0)]
        out["matches"], out["inliers"] = out["matches"][:n], out["inliers"][:n]
        return out

    def estimate_motion_3d_dev(self, d_from_ids, d_from_xyz, from_offsets, d_to_ids, d_to_xyz, to_offsets, d_transform, d_status, d_n_matches,
                               d_n_inliers, d_variance, d_matches, d_inliers, min_inliers=20, inlier_distance=0.1, iterations=300,
                               refine_iterations=5, seed=0):
        """lcd_estimate_motion_3d_dev on torch tensors of the engine's device (the offsets stay on the host).  Enqueued, not synchronised."""
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a = LcdMotion3dArgs(C.sizeof(LcdMotion3dArgs), fo.shape[0] - 1, int(min_inliers), int(iterations), int(refine_iterations),
                            int(seed) & 0xFFFFFFFF, float(inlier_distance))
        a.from_word_ids, a.from_xyz, a.to_word_ids, a.to_xyz = ptr(d_from_ids), ptr(d_from_xyz), ptr(d_to_ids), ptr(d_to_xyz)
        a.from_offsets, a.to_offsets = fo.ctypes.data, to.ctypes.data
        a.out_transform, a.out_status, a.out_n_matches, a.out_n_inliers = ptr(d_transform), ptr(d_status), ptr(d_n_matches), ptr(d_n_inliers)
        a.out_variance, a.out_matches, a.out_inliers = ptr(d_variance), ptr(d_matches), ptr(d_inliers)
        self._ck(self.L.lcd_estimate_motion_3d_dev(self.h, C.byref(a)))

    # ---- 3-D to 2-D motion estimation, PnP (stateless; include/lcd.h has the rule)
    @staticmethod
    def _pnp_cameras(cameras, n_pairs):
        """cameras: one dict(fx, fy, cx, cy[, image_width, image_height, local_transform]) for every pair, or a list of them"""
        if cameras is None:
            return None
        cams = [cameras] * max(n_pairs, 0) if isinstance(cameras, dict) else list(cameras)
        arr = (LcdCamera * max(len(cams), 1))()
        for i, m in enumerate(cams):
            t = m.get("local_transform")
            arr[i] = LcdCamera(m["fx"], m["fy"], m["cx"], m["cy"], int(m.get("image_width", 0)), int(m.get("image_height", 0)),
                               0 if t is None else 1, 0, (C.c_float * 12)(*([0.0] * 12 if t is None else [float(v) for v in np.asarray(t).reshape(-1)])))
        return arr

    def _pnp_args(self, n_pairs, fo, to, cams, guesses, min_inliers, iterations, refine_iterations, variance_median_ratio, seed, max_variance,
                  reproj_error, struct_size=None):
        a = LcdMotionPnpArgs(C.sizeof(LcdMotionPnpArgs) if struct_size is None else struct_size, n_pairs, int(min_inliers), int(iterations),
                             int(refine_iterations), int(variance_median_ratio), int(seed) & 0xFFFFFFFF, float(max_variance), float(reproj_error))
        a.from_offsets, a.to_offsets = None if fo is None else fo.ctypes.data, None if to is None else to.ctypes.data
        a.cameras = None if cams is None else C.cast(cams, C.c_void_p)
        a.guesses = None if guesses is None else guesses.ctypes.data
        return a

    def estimate_motion_pnp(self, from_ids, from_xyz, from_offsets, to_ids, to_points, to_offsets, cameras, to_xyz=None, guesses=None, min_inliers=20,
                            iterations=100, reproj_error=2.0, refine_iterations=1, variance_median_ratio=4, max_variance=0.0, seed=0, struct_size=None):
        """lcd_estimate_motion_pnp over host arrays, all pairs concatenated -> dict(transform [n_pairs x 12], status, n_matches, n_inliers,
        variance_lin, angle_cos, variance_kind [n_pairs], matches [Nt], inliers [Nt]); outputs start as -1 / NaN so that what the call left
        alone shows"""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fi, ti = np.ascontiguousarray(from_ids, dtype=np.int32).reshape(-1), np.ascontiguousarray(to_ids, dtype=np.int32).reshape(-1)
        fx, tp = np.ascontiguousarray(from_xyz, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(to_points, dtype=np.float32).reshape(-1, 2)
        tx = None if to_xyz is None else np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        n_pairs, n = (to if to is not None else fo).shape[0] - 1, ti.shape[0]
        np1 = max(n_pairs, 1)
        out = dict(transform=np.full((np1, 12), np.nan, np.float32), status=np.full(np1, -1, np.int32), n_matches=np.full(np1, -1, np.int32),
                   n_inliers=np.full(np1, -1, np.int32), variance_lin=np.full(np1, np.nan, np.float64), angle_cos=np.full(np1, np.nan, np.float64),
                   variance_kind=np.full(np1, -1, np.int32), matches=np.full(max(n, 1), -1, np.int32), inliers=np.full(max(n, 1), -1, np.int32))
        cams = self._pnp_cameras(cameras, n_pairs)
        a = self._pnp_args(n_pairs, fo, to, cams, gs, min_inliers, iterations, refine_iterations, variance_median_ratio, seed, max_variance,
                           reproj_error, struct_size)
        a.from_word_ids, a.from_xyz, a.to_word_ids, a.to_points, a.to_xyz = _p(fi), _p(fx), _p(ti), _p(tp), None if tx is None else _p(tx)
        a.out_transform, a.out_status, a.out_n_matches, a.out_n_inliers = _p(out["transform"]), _p(out["status"]), _p(out["n_matches"]), _p(out["n_inliers"])
        a.out_variance_lin, a.out_angle_cos, a.out_variance_kind = _p(out["variance_lin"]), _p(out["angle_cos"]), _p(out["variance_kind"])
        a.out_matches, a.out_inliers = _p(out["matches"]), _p(out["inliers"])
        self._ck(self.L.lcd_estimate_motion_pnp(self.h, C.byref(a)))
        for k in ("transform", "status", "n_matches", "n_inliers", "variance_lin", "angle_cos", "variance_kind"):
            out[k] = out[k][:max(n_pairs, 0)]
        out["matches"], out["inliers"] = out["matches"][:n], out["inliers"][:n]
        return out

    def estimate_motion_pnp_dev(self, d_from_ids, d_from_xyz, from_offsets, d_to_ids, d_to_points, to_offsets, cameras, d_transform, d_status,
                                d_n_matches, d_n_inliers, d_variance_lin, d_angle_cos, d_variance_kind, d_matches, d_inliers, d_to_xyz=None,
                                guesses=None, min_inliers=20, iterations=100, reproj_error=2.0, refine_iterations=1, variance_median_ratio=4,
                                max_variance=0.0, seed=0):
        """lcd_estimate_motion_pnp_dev on torch tensors of the engine's device (offsets, cameras and guesses stay on the host).  Enqueued, not
        synchronised."""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        n_pairs = (to if to is not None else fo).shape[0] - 1
        cams = self._pnp_cameras(cameras, n_pairs)
        a = self._pnp_args(n_pairs, fo, to, cams, gs, min_inliers, iterations, refine_iterations, variance_median_ratio, seed, max_variance, reproj_error)
        a.from_word_ids, a.from_xyz, a.to_word_ids, a.to_points, a.to_xyz = ptr(d_from_ids), ptr(d_from_xyz), ptr(d_to_ids), ptr(d_to_points), ptr(d_to_xyz)
        a.out_transform, a.out_status, a.out_n_matches, a.out_n_inliers = ptr(d_transform), ptr(d_status), ptr(d_n_matches), ptr(d_n_inliers)
        a.out_variance_lin, a.out_angle_cos, a.out_variance_kind = ptr(d_variance_lin), ptr(d_angle_cos), ptr(d_variance_kind)
        a.out_matches, a.out_inliers = ptr(d_matches), ptr(d_inliers)
        self._ck(self.L.lcd_estimate_motion_pnp_dev(self.h, C.byref(a)))

    # ---- epipolar hypothesis check (stateless; include/lcd.h has the rule)
    OUTPUTS_EPIPOLAR = ("fundamental", "status", "n_pairs", "n_inliers", "matches", "inliers")

    def verify_epipolar(self, from_ids, from_points, from_offsets, to_ids, to_points, to_offsets, match_count_min=8, iterations=1000,
                        ransac_threshold=3.0, seed=0, struct_size=None, leave_out=()):
        """lcd_verify_epipolar over host arrays, all pairs concatenated -> dict(fundamental [n_pairs x 9], status, n_pairs, n_inliers [n_pairs],
        matches [Nt], inliers [Nt]); outputs start as -1 / NaN so that what the call left alone shows; leave_out: names of outputs passed as NULL"""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fi, ti = np.ascontiguousarray(from_ids, dtype=np.int32).reshape(-1), np.ascontiguousarray(to_ids, dtype=np.int32).reshape(-1)
        fp, tp = np.ascontiguousarray(from_points, dtype=np.float32).reshape(-1, 2), np.ascontiguousarray(to_points, dtype=np.float32).reshape(-1, 2)
        n_pairs, n = (to if to is not None else fo).shape[0] - 1, ti.shape[0]
        np1 = max(n_pairs, 1)
        out = dict(fundamental=np.full((np1, 9), np.nan, np.float32), status=np.full(np1, -1, np.int32), n_pairs=np.full(np1, -1, np.int32),
                   n_inliers=np.full(np1, -1, np.int32), matches=np.full(max(n, 1), -1, np.int32), inliers=np.full(max(n, 1), -1, np.int32))
        a = LcdEpipolarArgs(C.sizeof(LcdEpipolarArgs) if struct_size is None else struct_size, n_pairs, int(match_count_min), int(iterations),
                            int(seed) & 0xFFFFFFFF, float(ransac_threshold))
        a.from_offsets, a.to_offsets = None if fo is None else fo.ctypes.data, None if to is None else to.ctypes.data
        a.from_word_ids, a.from_points, a.to_word_ids, a.to_points = _p(fi), _p(fp), _p(ti), _p(tp)
        for k in self.OUTPUTS_EPIPOLAR:
            setattr(a, "out_" + k, None if k in leave_out else _p(out[k]))
        self._ck(self.L.lcd_verify_epipolar(self.h, C.byref(a)))
        for k in ("fundamental", "status", "n_pairs", "n_inliers"):
            out[k] = out[k][:max(n_pairs, 0)]
        out["matches"], out["inliers"] = out["matches"][:n], out["inliers"][:n]
        return out

    def verify_epipolar_dev(self, d_from_ids, d_from_points, from_offsets, d_to_ids, d_to_points, to_offsets, d_fundamental, d_status, d_n_pairs,
                            d_n_inliers, d_matches, d_inliers, match_count_min=8, iterations=1000, ransac_threshold=3.0, seed=0):
        """lcd_verify_epipolar_dev on torch tensors of the engine's device (the offsets stay on the host; d_fundamental, d_matches and d_inliers
        may be None).  Enqueued, not synchronised."""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        n_pairs = (to if to is not None else fo).shape[0] - 1
        a = LcdEpipolarArgs(C.sizeof(LcdEpipolarArgs), n_pairs, int(match_count_min), int(iterations), int(seed) & 0xFFFFFFFF, float(ransac_threshold))
        a.from_offsets, a.to_offsets = None if fo is None else fo.ctypes.data, None if to is None else to.ctypes.data
        a.from_word_ids, a.from_points, a.to_word_ids, a.to_points = ptr(d_from_ids), ptr(d_from_points), ptr(d_to_ids), ptr(d_to_points)
        a.out_fundamental, a.out_status, a.out_n_pairs, a.out_n_inliers = ptr(d_fundamental), ptr(d_status), ptr(d_n_pairs), ptr(d_n_inliers)
        a.out_matches, a.out_inliers = ptr(d_matches), ptr(d_inliers)
        self._ck(self.L.lcd_verify_epipolar_dev(self.h, C.byref(a)))

    # ---- monocular motion estimation, Vis/EstimationType = 2 (stateless; include/lcd.h has the rule)
    OUTPUTS_MONO = ("transform", "status", "n_matches", "n_inliers", "variance", "matches", "inliers", "points3")

    def _mono_args(self, n_pairs, fo, to, cams, guesses, min_inliers, iterations, seed, variance_median_ratio, reproj_threshold, distance_threshold,
                   max_variance, struct_size=None):
        a = LcdMotionMonoArgs(C.sizeof(LcdMotionMonoArgs) if struct_size is None else struct_size, n_pairs, int(min_inliers), int(iterations),
                              int(seed) & 0xFFFFFFFF, int(variance_median_ratio), float(reproj_threshold), float(distance_threshold),
                              float(max_variance), 0)
        a.from_offsets, a.to_offsets = None if fo is None else fo.ctypes.data, None if to is None else to.ctypes.data
        a.cameras = None if cams is None else C.cast(cams, C.c_void_p)
        a.guesses = None if guesses is None else guesses.ctypes.data
        return a

    def estimate_motion_mono(self, from_ids, from_points, from_offsets, to_ids, to_points, to_offsets, cameras, from_points3=None, guesses=None,
                             min_inliers=20, iterations=1000, reproj_threshold=2.0, variance_median_ratio=4, max_variance=0.1,
                             distance_threshold=50.0, seed=0, struct_size=None, leave_out=()):
        """lcd_estimate_motion_mono over host arrays, all pairs concatenated -> dict(transform [n_pairs x 12], status, n_matches, n_inliers,
        variance [n_pairs], matches [Nt], inliers [Nt], points3 [Nt x 3]); outputs start as -1 / NaN so that what the call left alone shows;
        leave_out: names of outputs passed as NULL"""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fi, ti = np.ascontiguousarray(from_ids, dtype=np.int32).reshape(-1), np.ascontiguousarray(to_ids, dtype=np.int32).reshape(-1)
        fp, tp = np.ascontiguousarray(from_points, dtype=np.float32).reshape(-1, 2), np.ascontiguousarray(to_points, dtype=np.float32).reshape(-1, 2)
        f3 = None if from_points3 is None else np.ascontiguousarray(from_points3, dtype=np.float32).reshape(-1, 3)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        n_pairs, n = (to if to is not None else fo).shape[0] - 1, ti.shape[0]
        np1 = max(n_pairs, 1)
        out = dict(transform=np.full((np1, 12), np.nan, np.float32), status=np.full(np1, -1, np.int32), n_matches=np.full(np1, -1, np.int32),
                   n_inliers=np.full(np1, -1, np.int32), variance=np.full(np1, np.nan, np.float64), matches=np.full(max(n, 1), -1, np.int32),
                   inliers=np.full(max(n, 1), -1, np.int32), points3=np.full((max(n, 1), 3), np.nan, np.float32))
        cams = self._pnp_cameras(cameras, n_pairs)
        a = self._mono_args(n_pairs, fo, to, cams, gs, min_inliers, iterations, seed, variance_median_ratio, reproj_threshold, distance_threshold,
                            max_variance, struct_size)
        a.from_word_ids, a.from_points, a.to_word_ids, a.to_points = _p(fi), _p(fp), _p(ti), _p(tp)
        a.from_points3 = None if f3 is None else (f3.ctypes.data if f3.size == 0 else _p(f3))
        for k in self.OUTPUTS_MONO:
            setattr(a, "out_" + k, None if k in leave_out else _p(out[k]))
        self._ck(self.L.lcd_estimate_motion_mono(self.h, C.byref(a)))
        for k in ("transform", "status", "n_matches", "n_inliers", "variance"):
            out[k] = out[k][:max(n_pairs, 0)]
        out["matches"], out["inliers"], out["points3"] = out["matches"][:n], out["inliers"][:n], out["points3"][:n]
        return out

    def estimate_motion_mono_dev(self, d_from_ids, d_from_points, from_offsets, d_to_ids, d_to_points, to_offsets, cameras, d_transform, d_status,
                                 d_n_matches, d_n_inliers, d_variance, d_matches=None, d_inliers=None, d_points3=None, d_from_points3=None,
                                 guesses=None, min_inliers=20, iterations=1000, reproj_threshold=2.0, variance_median_ratio=4, max_variance=0.1,
                                 distance_threshold=50.0, seed=0):
        """lcd_estimate_motion_mono_dev on torch tensors of the engine's device (offsets, cameras and guesses stay on the host; d_matches,
        d_inliers, d_points3 and d_from_points3 may be None).  Enqueued, not synchronised."""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        n_pairs = (to if to is not None else fo).shape[0] - 1
        cams = self._pnp_cameras(cameras, n_pairs)
        a = self._mono_args(n_pairs, fo, to, cams, gs, min_inliers, iterations, seed, variance_median_ratio, reproj_threshold, distance_threshold,
                            max_variance)
        a.from_word_ids, a.from_points, a.to_word_ids, a.to_points = ptr(d_from_ids), ptr(d_from_points), ptr(d_to_ids), ptr(d_to_points)
        a.from_points3 = None if d_from_points3 is None else d_from_points3.data_ptr()
        a.out_transform, a.out_status, a.out_n_matches, a.out_n_inliers = ptr(d_transform), ptr(d_status), ptr(d_n_matches), ptr(d_n_inliers)
        a.out_variance, a.out_matches, a.out_inliers, a.out_points3 = ptr(d_variance), ptr(d_matches), ptr(d_inliers), ptr(d_points3)
        self._ck(self.L.lcd_estimate_motion_mono_dev(self.h, C.byref(a)))

    # ---- two-view bundle adjustment behind the motion estimate (stateless; include/lcd.h has the rule)
    def _ba_args(self, n_pairs, fo, to, cams_from, cams_to, prior_variance, baselines, min_inliers, iterations, pixel_variance, robust_delta,
                 default_baseline, max_inliers_mean_distance, min_inliers_distribution, struct_size=None):
        """the host-side fields; the second value keeps their arrays alive for the call"""
        a = LcdMotionBaArgs(C.sizeof(LcdMotionBaArgs) if struct_size is None else struct_size, n_pairs, int(min_inliers), int(iterations),
                            float(pixel_variance), float(robust_delta), float(default_baseline), float(max_inliers_mean_distance),
                            float(min_inliers_distribution))
        pv = None if prior_variance is None else np.ascontiguousarray(prior_variance, dtype=np.float64).reshape(-1, 2)
        bl = None if baselines is None else np.ascontiguousarray(baselines, dtype=np.float64).reshape(-1, 2)
        a.from_offsets, a.to_offsets = None if fo is None else fo.ctypes.data, None if to is None else to.ctypes.data
        a.cameras_from = None if cams_from is None else C.cast(cams_from, C.c_void_p)
        a.cameras_to = None if cams_to is None else C.cast(cams_to, C.c_void_p)
        a.prior_variance, a.baselines = None if pv is None else pv.ctypes.data, None if bl is None else bl.ctypes.data
        return a, (pv, bl)

    def refine_motion_ba(self, from_ids, from_xyz, from_offsets, to_ids, to_points, to_offsets, inliers, n_inliers, transforms, cameras_from, cameras_to,
                         from_points=None, to_xyz=None, prior_variance=None, baselines=None, min_inliers=20, iterations=20, pixel_variance=1.0,
                         robust_delta=8.0, default_baseline=0.075, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0, struct_size=None):
        """lcd_refine_motion_ba over host arrays, all pairs concatenated -> dict(transform [n_pairs x 12], status, n_inliers, n_outliers,
        chi2_before, chi2_after, lm_accepted, inliers_mean_distance, inliers_distribution [n_pairs], inliers [Nt]); outputs start as -1 / NaN
        so that what the call left alone shows"""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fi, ti = np.ascontiguousarray(from_ids, dtype=np.int32).reshape(-1), np.ascontiguousarray(to_ids, dtype=np.int32).reshape(-1)
        fx, tp = np.ascontiguousarray(from_xyz, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(to_points, dtype=np.float32).reshape(-1, 2)
        fp = None if from_points is None else np.ascontiguousarray(from_points, dtype=np.float32).reshape(-1, 2)
        tx = None if to_xyz is None else np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
        il = None if inliers is None else np.ascontiguousarray(inliers, dtype=np.int32).reshape(-1)
        ni = None if n_inliers is None else np.ascontiguousarray(n_inliers, dtype=np.int32).reshape(-1)
        tr = None if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        n_pairs, n = (to if to is not None else fo).shape[0] - 1, ti.shape[0]
        np1 = max(n_pairs, 1)
        out = dict(transform=np.full((np1, 12), np.nan, np.float32), status=np.full(np1, -1, np.int32), n_inliers=np.full(np1, -1, np.int32),
                   n_outliers=np.full(np1, -1, np.int32), chi2_before=np.full(np1, np.nan, np.float64), chi2_after=np.full(np1, np.nan, np.float64),
                   lm_accepted=np.full(np1, -1, np.int32), inliers_mean_distance=np.full(np1, np.nan, np.float32),
                   inliers_distribution=np.full(np1, np.nan, np.float32), inliers=np.full(max(n, 1), -1, np.int32))
        a, keep = self._ba_args(n_pairs, fo, to, self._pnp_cameras(cameras_from, n_pairs), self._pnp_cameras(cameras_to, n_pairs), prior_variance, baselines,
                                min_inliers, iterations, pixel_variance, robust_delta, default_baseline, max_inliers_mean_distance, min_inliers_distribution,
                                struct_size)
        opt = lambda v: None if v is None else _p(v)
        a.from_word_ids, a.from_xyz, a.from_points, a.to_word_ids, a.to_points, a.to_xyz = _p(fi), _p(fx), opt(fp), _p(ti), _p(tp), opt(tx)
        a.inliers, a.n_inliers, a.transforms = opt(il), opt(ni), opt(tr)
        a.out_transform, a.out_status, a.out_inliers, a.out_n_inliers = _p(out["transform"]), _p(out["status"]), _p(out["inliers"]), _p(out["n_inliers"])
        a.out_n_outliers, a.out_chi2_before, a.out_chi2_after = _p(out["n_outliers"]), _p(out["chi2_before"]), _p(out["chi2_after"])
        a.out_lm_accepted, a.out_inliers_mean_distance, a.out_inliers_distribution = \
            _p(out["lm_accepted"]), _p(out["inliers_mean_distance"]), _p(out["inliers_distribution"])
        self._ck(self.L.lcd_refine_motion_ba(self.h, C.byref(a)))
        for k in out:
            out[k] = out[k][:n] if k == "inliers" else out[k][:max(n_pairs, 0)]
        return out

    def refine_motion_ba_dev(self, d_from_ids, d_from_xyz, from_offsets, d_to_ids, d_to_points, to_offsets, d_inliers, d_n_inliers, d_transforms,
                             cameras_from, cameras_to, d_out_transform, d_out_status, d_out_inliers, d_out_n_inliers, d_out_n_outliers,
                             d_out_chi2_before, d_out_chi2_after, d_out_lm_accepted, d_out_mean_distance, d_out_distribution, d_from_points=None,
                             d_to_xyz=None, prior_variance=None, baselines=None, min_inliers=20, iterations=20, pixel_variance=1.0, robust_delta=8.0,
                             default_baseline=0.075, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0):
        """lcd_refine_motion_ba_dev on torch tensors of the engine's device: d_inliers, d_n_inliers and d_transforms are what
        estimate_motion_pnp_dev wrote (offsets, cameras, prior_variance and baselines stay on the host).  Enqueued, not synchronised."""
        fo = None if from_offsets is None else np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = None if to_offsets is None else np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        n_pairs = (to if to is not None else fo).shape[0] - 1
        a, keep = self._ba_args(n_pairs, fo, to, self._pnp_cameras(cameras_from, n_pairs), self._pnp_cameras(cameras_to, n_pairs), prior_variance, baselines,
                                min_inliers, iterations, pixel_variance, robust_delta, default_baseline, max_inliers_mean_distance, min_inliers_distribution)
        a.from_word_ids, a.from_xyz, a.from_points = ptr(d_from_ids), ptr(d_from_xyz), ptr(d_from_points)
        a.to_word_ids, a.to_points, a.to_xyz = ptr(d_to_ids), ptr(d_to_points), ptr(d_to_xyz)
        a.inliers, a.n_inliers, a.transforms = ptr(d_inliers), ptr(d_n_inliers), ptr(d_transforms)
        a.out_transform, a.out_status, a.out_inliers, a.out_n_inliers = ptr(d_out_transform), ptr(d_out_status), ptr(d_out_inliers), ptr(d_out_n_inliers)
        a.out_n_outliers, a.out_chi2_before, a.out_chi2_after = ptr(d_out_n_outliers), ptr(d_out_chi2_before), ptr(d_out_chi2_after)
        a.out_lm_accepted, a.out_inliers_mean_distance, a.out_inliers_distribution = ptr(d_out_lm_accepted), ptr(d_out_mean_distance), ptr(d_out_distribution)
        self._ck(self.L.lcd_refine_motion_ba_dev(self.h, C.byref(a)))

    # ---- scan registration, point-to-point ICP (stateless; include/lcd.h has the rule)
    @staticmethod
    def _icp_args(n_pairs, max_iterations, force_3dof, max_laser_scans, search, max_correspondence_distance, epsilon, correspondence_ratio, struct_size):
        return LcdIcpArgs(C.sizeof(LcdIcpArgs) if struct_size is None else struct_size, n_pairs, int(max_iterations), int(bool(force_3dof)),
                          int(max_laser_scans), int(search), float(max_correspondence_distance), float(epsilon), float(correspondence_ratio))

    def register_icp(self, from_xyz, from_offsets, to_xyz, to_offsets, guesses, max_iterations=30, force_3dof=False, max_laser_scans=0,
                     search=LCD_ICP_SEARCH_AUTO, max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1, struct_size=None):
        """lcd_register_icp over host arrays, all pairs concatenated -> dict(transform, icp_transform, correction [n_pairs x 12], status, stop,
        iterations, n_correspondences, ratio, variance [n_pairs], match [Nf]); outputs start as -7 / NaN so that what the call left alone shows"""
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fx, tx = np.ascontiguousarray(from_xyz, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        n_pairs, n = fo.shape[0] - 1, fx.shape[0]
        m = max(n_pairs, 1)
        out = dict(transform=np.full((m, 12), np.nan, np.float32), icp_transform=np.full((m, 12), np.nan, np.float32),
                   correction=np.full((m, 12), np.nan, np.float32), status=np.full(m, -7, np.int32), stop=np.full(m, -7, np.int32),
                   iterations=np.full(m, -7, np.int32), n_correspondences=np.full(m, -7, np.int32), ratio=np.full(m, np.nan, np.float32),
                   variance=np.full(m, np.nan, np.float64), match=np.full(max(n, 1), -7, np.int32))
        a = self._icp_args(n_pairs, max_iterations, force_3dof, max_laser_scans, search, max_correspondence_distance, epsilon, correspondence_ratio, struct_size)
        a.from_xyz, a.to_xyz, a.from_offsets, a.to_offsets, a.guesses = _p(fx), _p(tx), fo.ctypes.data, to.ctypes.data, None if gs is None else _p(gs)
        a.out_transform, a.out_icp_transform, a.out_correction = _p(out["transform"]), _p(out["icp_transform"]), _p(out["correction"])
        a.out_status, a.out_stop, a.out_iterations, a.out_n_correspondences = _p(out["status"]), _p(out["stop"]), _p(out["iterations"]), _p(out["n_correspondences"])
        a.out_ratio, a.out_variance, a.out_match = _p(out["ratio"]), _p(out["variance"]), _p(out["match"])
        self._ck(self.L.lcd_register_icp(self.h, C.byref(a)))
        for k in out:
            out[k] = out[k][:n] if k == "match" else out[k][:max(n_pairs, 0)]
        return out

    def register_icp_dev(self, d_from_xyz, from_offsets, d_to_xyz, to_offsets, guesses, d_transform, d_icp_transform, d_correction, d_status, d_stop,
                         d_iterations, d_n_correspondences, d_ratio, d_variance, d_match, max_iterations=30, force_3dof=False, max_laser_scans=0,
                         search=LCD_ICP_SEARCH_AUTO, max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1):
        """lcd_register_icp_dev on torch tensors of the engine's device (offsets and guesses stay on the host).  Enqueued, not synchronised."""
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a = self._icp_args(fo.shape[0] - 1, max_iterations, force_3dof, max_laser_scans, search, max_correspondence_distance, epsilon, correspondence_ratio, None)
        a.from_xyz, a.to_xyz, a.from_offsets, a.to_offsets, a.guesses = ptr(d_from_xyz), ptr(d_to_xyz), fo.ctypes.data, to.ctypes.data, None if gs is None else _p(gs)
        a.out_transform, a.out_icp_transform, a.out_correction = ptr(d_transform), ptr(d_icp_transform), ptr(d_correction)
        a.out_status, a.out_stop, a.out_iterations, a.out_n_correspondences = ptr(d_status), ptr(d_stop), ptr(d_iterations), ptr(d_n_correspondences)
        a.out_ratio, a.out_variance, a.out_match = ptr(d_ratio), ptr(d_variance), ptr(d_match)
        self._ck(self.L.lcd_register_icp_dev(self.h, C.byref(a)))

    # ---- scan registration, point to plane with the complexity test and its fallback (stateless; include/lcd.h has the rule)
    ICP_PLANE_OUT = (("transform", 12, np.float32), ("icp_transform", 12, np.float32), ("correction", 12, np.float32), ("status", 0, np.int32),
                     ("stop", 0, np.int32), ("iterations", 0, np.int32), ("n_correspondences", 0, np.int32), ("ratio", 0, np.float32),
                     ("variance", 0, np.float64), ("branch", 0, np.int32), ("complexity", 0, np.float32), ("complexity_values", 3, np.float32),
                     ("complexity_vectors", 9, np.float32), ("second_eigenvalue", 0, np.float32))

    @staticmethod
    def _icp_plane_args(n_pairs, max_iterations, force_3dof, max_laser_scans, search, max_correspondence_distance, epsilon, correspondence_ratio,
                        min_complexity, low_complexity_strategy, normal_gate, min_normal_cos, struct_size):
        return LcdIcpPlaneArgs(C.sizeof(LcdIcpPlaneArgs) if struct_size is None else struct_size, n_pairs, int(max_iterations), int(bool(force_3dof)),
                               int(max_laser_scans), int(search), float(max_correspondence_distance), float(epsilon), float(correspondence_ratio),
                               float(min_complexity), int(low_complexity_strategy), int(bool(normal_gate)), 0, float(min_normal_cos))

    def register_icp_plane(self, from_xyz, from_normals, from_offsets, to_xyz, to_normals, to_offsets, guesses, max_iterations=30, force_3dof=False,
                           max_laser_scans=0, search=LCD_ICP_SEARCH_AUTO, max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1,
                           min_complexity=0.02, low_complexity_strategy=1, normal_gate=False, min_normal_cos=0.0, struct_size=None):
        """lcd_register_icp_plane over host arrays, all pairs concatenated -> dict of ICP_PLANE_OUT's names ([n_pairs] or [n_pairs x k]) and match
        [Nf]; outputs start as -7 / NaN so that what the call left alone shows"""
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        fx, tx = np.ascontiguousarray(from_xyz, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
        fn = None if from_normals is None else np.ascontiguousarray(from_normals, dtype=np.float32).reshape(-1, 3)
        tn = None if to_normals is None else np.ascontiguousarray(to_normals, dtype=np.float32).reshape(-1, 3)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        n_pairs, n = fo.shape[0] - 1, fx.shape[0]
        m = max(n_pairs, 1)
        out = {k: np.full((m, w) if w else m, -7 if dt is np.int32 else np.nan, dt) for k, w, dt in self.ICP_PLANE_OUT}
        out["match"] = np.full(max(n, 1), -7, np.int32)
        a = self._icp_plane_args(n_pairs, max_iterations, force_3dof, max_laser_scans, search, max_correspondence_distance, epsilon, correspondence_ratio,
                                 min_complexity, low_complexity_strategy, normal_gate, min_normal_cos, struct_size)
        a.from_xyz, a.to_xyz, a.from_offsets, a.to_offsets, a.guesses = _p(fx), _p(tx), fo.ctypes.data, to.ctypes.data, None if gs is None else _p(gs)
        a.from_normals, a.to_normals = None if fn is None else _p(fn), None if tn is None else _p(tn)
        for k in out:
            setattr(a, "out_" + k, _p(out[k]))
        self._ck(self.L.lcd_register_icp_plane(self.h, C.byref(a)))
        for k in out:
            out[k] = out[k][:n] if k == "match" else out[k][:max(n_pairs, 0)]
        return out

    def register_icp_plane_dev(self, d_from_xyz, d_from_normals, from_offsets, d_to_xyz, d_to_normals, to_offsets, guesses, d_out, max_iterations=30,
                               force_3dof=False, max_laser_scans=0, search=LCD_ICP_SEARCH_AUTO, max_correspondence_distance=0.1, epsilon=0.0,
                               correspondence_ratio=0.1, min_complexity=0.02, low_complexity_strategy=1, normal_gate=False, min_normal_cos=0.0):
        """lcd_register_icp_plane_dev on torch tensors of the engine's device (offsets and guesses stay on the host); d_out maps ICP_PLANE_OUT's
        names and "match" to the output tensors.  Enqueued, not synchronised."""
        fo = np.ascontiguousarray(from_offsets, dtype=np.int64).reshape(-1)
        to = np.ascontiguousarray(to_offsets, dtype=np.int64).reshape(-1)
        gs = None if guesses is None else np.ascontiguousarray(guesses, dtype=np.float32).reshape(-1, 12)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a = self._icp_plane_args(fo.shape[0] - 1, max_iterations, force_3dof, max_laser_scans, search, max_correspondence_distance, epsilon,
                                 correspondence_ratio, min_complexity, low_complexity_strategy, normal_gate, min_normal_cos, None)
        a.from_xyz, a.to_xyz, a.from_offsets, a.to_offsets, a.guesses = ptr(d_from_xyz), ptr(d_to_xyz), fo.ctypes.data, to.ctypes.data, None if gs is None else _p(gs)
        a.from_normals, a.to_normals = ptr(d_from_normals), ptr(d_to_normals)
        for k, _, _ in self.ICP_PLANE_OUT + (("match", 0, np.int32),):
            setattr(a, "out_" + k, ptr(d_out[k]))
        self._ck(self.L.lcd_register_icp_plane_dev(self.h, C.byref(a)))

    # ---- scan filtering in front of the ICP: downsampling, range, voxel grid, normals (stateless; include/lcd.h has the rule)
    @staticmethod
    def _scan_filter_args(n_scans, downsampling_step, is_2d, normal_k, range_min, range_max, voxel_size, normal_radius, ground_normals_up, viewpoint,
                          struct_size):
        vp = (C.c_float * 3)(*[float(v) for v in viewpoint])
        return LcdScanFilterArgs(C.sizeof(LcdScanFilterArgs) if struct_size is None else struct_size, n_scans, int(downsampling_step), int(bool(is_2d)),
                                 int(normal_k), 0, float(range_min), float(range_max), float(voxel_size), float(normal_radius), float(ground_normals_up), vp)

    def filter_scans(self, xyz, offsets, out_offsets, downsampling_step=1, is_2d=False, normal_k=0, range_min=0.0, range_max=0.0, voxel_size=0.0,
                     normal_radius=0.0, ground_normals_up=0.0, viewpoint=(0.0, 0.0, 0.0), struct_size=None, with_normals=None):
        """lcd_filter_scans over host arrays, all scans concatenated -> dict(xyz, normals [M x 3] (None when no normals are asked for), count, status
        [n_scans], stage_counts [n_scans x 3]); outputs start as -7 / 7.0 so that what the call left alone shows.  with_normals: whether
        out_normals is handed over (default: iff normals are asked for)"""
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        oo = None if out_offsets is None else np.ascontiguousarray(out_offsets, dtype=np.int64).reshape(-1)
        x = None if xyz is None else np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        n_scans = (off if off is not None else oo).shape[0] - 1
        m_rows = int(oo[-1]) if oo is not None and oo.shape[0] else 0
        if with_normals is None:
            with_normals = normal_k > 0 or normal_radius > 0
        m = max(n_scans, 1)
        out = dict(xyz=np.full((max(m_rows, 1), 3), 7.0, np.float32), normals=np.full((max(m_rows, 1), 3), 7.0, np.float32) if with_normals else None,
                   count=np.full(m, -7, np.int32), stage_counts=np.full((m, 3), -7, np.int32), status=np.full(m, -7, np.int32))
        a = self._scan_filter_args(n_scans, downsampling_step, is_2d, normal_k, range_min, range_max, voxel_size, normal_radius, ground_normals_up,
                                   viewpoint, struct_size)
        a.xyz = None if x is None or x.shape[0] == 0 else _p(x)
        a.offsets, a.out_offsets = None if off is None else off.ctypes.data, None if oo is None else oo.ctypes.data
        for k, v in out.items():
            setattr(a, "out_" + k, None if v is None else _p(v))
        self._ck(self.L.lcd_filter_scans(self.h, C.byref(a)))
        out["xyz"] = out["xyz"][:m_rows]
        if with_normals:
            out["normals"] = out["normals"][:m_rows]
        for k in ("count", "stage_counts", "status"):
            out[k] = out[k][:max(n_scans, 0)]
        return out

    def filter_scans_dev(self, d_xyz, offsets, out_offsets, d_out, downsampling_step=1, is_2d=False, normal_k=0, range_min=0.0, range_max=0.0,
                         voxel_size=0.0, normal_radius=0.0, ground_normals_up=0.0, viewpoint=(0.0, 0.0, 0.0)):
        """lcd_filter_scans_dev on torch tensors of the engine's device (both offset arrays stay on the host); d_out maps xyz, normals (None
        without normals), count, stage_counts and status to the output tensors.  Enqueued, not synchronised."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        oo = np.ascontiguousarray(out_offsets, dtype=np.int64).reshape(-1)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        a = self._scan_filter_args(off.shape[0] - 1, downsampling_step, is_2d, normal_k, range_min, range_max, voxel_size, normal_radius,
                                   ground_normals_up, viewpoint, None)
        a.xyz, a.offsets, a.out_offsets = ptr(d_xyz), off.ctypes.data, oo.ctypes.data
        for k in ("xyz", "normals", "count", "stage_counts", "status"):
            setattr(a, "out_" + k, ptr(d_out.get(k)))
        self._ck(self.L.lcd_filter_scans_dev(self.h, C.byref(a)))

    # ---- global descriptors: Signature::compareTo's other branch
    @staticmethod
    def _globals_host(descs):
        """[(type, row or None), ...] or plain rows (type 1) -> (lcd_global_desc array, count, the arrays kept alive)"""
        descs = list(descs or [])
        arr = (LcdGlobalDesc * max(len(descs), 1))()
        keep = []
        for i, d in enumerate(descs):
            typ, row = d if isinstance(d, tuple) else (1, d)
            if row is None:
                arr[i] = LcdGlobalDesc(int(typ), 0, None)
                continue
            row = np.ascontiguousarray(row, dtype=np.float32).reshape(-1)
            keep.append(row)
            arr[i] = LcdGlobalDesc(int(typ), row.shape[0], row.ctypes.data if row.shape[0] else None)
        return arr, len(descs), keep

    @staticmethod
    def _globals_dev(descs):
        """the same for torch tensors of the engine's device"""
        import torch
        descs = list(descs or [])
        arr = (LcdGlobalDesc * max(len(descs), 1))()
        for i, d in enumerate(descs):
            typ, row = d if isinstance(d, tuple) else (1, d)
            if row is None:
                arr[i] = LcdGlobalDesc(int(typ), 0, None)
                continue
            if row.dtype != torch.float32 or not row.is_cuda or not row.is_contiguous():
                raise ValueError("global descriptors: contiguous float32 device tensors expected")
            arr[i] = LcdGlobalDesc(int(typ), int(row.numel()), row.data_ptr() if row.numel() else None)
        return arr, len(descs)

    def sig_set_globals(self, sig_id, descs):
        """lcd_sig_set_globals: descs[i] is channel i, a float row (type 1) or (type, row or None); replaces all of the signature's channels"""
        arr, n, keep = self._globals_host(descs)
        self._ck(self.L.lcd_sig_set_globals(self.h, int(sig_id), C.addressof(arr), n))

    def sig_set_globals_dev(self, sig_id, descs):
        """lcd_sig_set_globals_dev: the rows are torch tensors on the engine's device; enqueued on the engine stream, not synchronised"""
        arr, n = self._globals_dev(descs)
        self._ck(self.L.lcd_sig_set_globals_dev(self.h, int(sig_id), C.addressof(arr), n))

    def sig_set_global_bulk(self, channel, sig_ids, rows):
        """lcd_sig_set_global_bulk: rows[k] becomes the type-1 descriptor of sig_ids[k] on one channel"""
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        r = np.ascontiguousarray(rows, dtype=np.float32)
        if r.ndim != 2 or r.shape[0] != s.shape[0]:
            raise ValueError("sig_set_global_bulk: rows must be [len(sig_ids), dim]")
        self._ck(self.L.lcd_sig_set_global_bulk(self.h, int(channel), s.shape[0], _p(s), _p(r), r.shape[1]))

    def sig_clear_globals(self, sig_id):
        self._ck(self.L.lcd_sig_clear_globals(self.h, int(sig_id)))

    def compare_to(self, query_word_ids, query_globals, sig_ids, with_counts=False):
        """lcd_compare_to: Signature::compareTo of the query (word ids, global descriptors as in sig_set_globals) against sig_ids;
        with_counts: also totalDescs, the number of global descriptors that took part, per id"""
        w = np.ascontiguousarray(query_word_ids, dtype=np.int32)
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        arr, n, keep = self._globals_host(query_globals)
        out = np.zeros(s.shape[0], np.float32)
        cnt = np.zeros(s.shape[0], np.int32) if with_counts else None
        self._ck(self.L.lcd_compare_to(self.h, _p(w), w.shape[0], C.addressof(arr), n, _p(s), s.shape[0], _p(out), _p(cnt)))
        return (out, cnt) if with_counts else out

    def compare_to_dev(self, d_query_word_ids, query_globals, d_out):
        """lcd_compare_to_dev on torch tensors of the engine's device: int32 word ids and float32 descriptor rows in, float32 result over the
        signature slots out (d_out holds at least slot_count entries); enqueued on the engine stream, not synchronised."""
        import torch
        if d_query_word_ids.dtype != torch.int32 or d_out.dtype != torch.float32 or not (d_query_word_ids.is_cuda and d_out.is_cuda) or \
                not (d_query_word_ids.is_contiguous() and d_out.is_contiguous()):
            raise ValueError("compare_to_dev: contiguous device tensors expected, int32 word ids and float32 output")
        arr, n = self._globals_dev(query_globals)
        self._ck(self.L.lcd_compare_to_dev(self.h, d_query_word_ids.data_ptr() if d_query_word_ids.numel() else None, int(d_query_word_ids.numel()),
                                           C.addressof(arr), n, d_out.data_ptr(), int(d_out.numel())))

    def adjust_likelihood_dev(self, d_ptr, n, ratio=0.0):
        self._ck(self.L.lcd_adjust_likelihood_dev(self.h, d_ptr, n, ratio))

    def adjust_likelihood(self, L, ratio=0.0):
        a = np.ascontiguousarray(L, dtype=np.float32).copy()
        self._ck(self.L.lcd_adjust_likelihood(self.h, _p(a), a.shape[0], ratio))
        return a

    # ---- device-resident frame path
    def frame_dev(self, d_desc_ptr, q, sig_id, N, d_word_ids_ptr, d_like_ptr, like_capacity, incremental=True,
                  new_words_compared=True, nndr=0.8, first_new_word_id=0, d_hypothesis_ptr=None, d_adjusted_ptr=None,
                  exclude_recent=0, virtual_place_ratio=0.0, d_first_new_word_id_ptr=None, d_posterior_ptr=None, d_bayes_ptr=None, append_new_words=False):
        flags = (LCD_Q_INCREMENTAL if incremental else 0) | (LCD_Q_NEW_WORDS_COMPARED if new_words_compared else 0)
        a = LcdFrameArgs(C.sizeof(LcdFrameArgs), q, d_desc_ptr, flags, nndr, sig_id, first_new_word_id, float(N), exclude_recent,
                         d_word_ids_ptr, d_like_ptr, like_capacity, d_hypothesis_ptr, d_adjusted_ptr, virtual_place_ratio,
                         1 if append_new_words else 0, d_first_new_word_id_ptr, d_posterior_ptr, d_bayes_ptr)
        self._ck(self.L.lcd_frame_dev(self.h, C.byref(a)))

    def frame_host(self, desc, sig_id, N, incremental=True, new_words_compared=True, nndr=0.8, first_new_word_id=0, append_new_words=False,
                   want_likelihood=True):
        """lcd_frame_host: host descriptors in, (word ids, dense likelihood over the signature slots) out, one synchronisation."""
        d = np.ascontiguousarray(desc)
        q = d.shape[0]
        flags = (LCD_Q_INCREMENTAL if incremental else 0) | (LCD_Q_NEW_WORDS_COMPARED if new_words_compared else 0)
        n = C.c_int64(0)
        self._ck(self.L.lcd_slot_count(self.h, C.byref(n)))
        words = np.zeros(q, np.int32)
        like = np.zeros(n.value + 1, np.float32) if want_likelihood else None
        ns = C.c_int64(0)
        a = LcdFrameHostArgs(C.sizeof(LcdFrameHostArgs), q, _p(d), flags, nndr, sig_id, first_new_word_id, float(N), 1 if append_new_words else 0,
                             _p(words), _p(like) if like is not None else None, like.shape[0] if like is not None else 0,
                             C.cast(C.byref(ns), C.c_void_p))
        self._ck(self.L.lcd_frame_host(self.h, C.byref(a)))
        return words, (like[: ns.value] if like is not None else None)

    def frame_args(self, **kw):
        """A reusable argument block for frame_dev_args (callers in a tight loop change a few fields per frame)."""
        a = LcdFrameArgs()
        a.struct_size = C.sizeof(LcdFrameArgs)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def frame_dev_args(self, a):
        rc = self.L.lcd_frame_dev(self.h, C.byref(a))
        if rc != LCD_OK:
            self._ck(rc)

    # ---- Bayes filter (BayesFilter.cpp)
    def bayes_configure(self, prediction_lc, virtual_place_prior=0.9):
        lc = np.ascontiguousarray(prediction_lc, dtype=np.float64)
        self._ck(self.L.lcd_bayes_configure(self.h, _p(lc), lc.shape[0], virtual_place_prior))

    def bayes_reset(self):
        self._ck(self.L.lcd_bayes_reset(self.h))

    def bayes_set_neighbors(self, sig_ids, offsets, nbr_sig_ids, nbr_margins):
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        n = np.ascontiguousarray(nbr_sig_ids, dtype=np.int32)
        m = np.ascontiguousarray(nbr_margins, dtype=np.int32)
        assert o.shape[0] == s.shape[0] + 1 and n.shape[0] == m.shape[0]
        self._ck(self.L.lcd_bayes_set_neighbors(self.h, s.shape[0], _p(s), _p(o), _p(n), _p(m)))

    def bayes_neighbors_prepared(self, sig_ids, offsets, nbr_sig_ids, nbr_margins):
        """The argument pointers of bayes_set_neighbors for caller-owned arrays (int32 / int64 / int32 / int32, C-contiguous), built
        once for a tight loop: the arrays' CONTENTS may change between calls, their shapes may not."""
        assert sig_ids.dtype == np.int32 and offsets.dtype == np.int64 and nbr_sig_ids.dtype == np.int32 and nbr_margins.dtype == np.int32
        assert offsets.shape[0] == sig_ids.shape[0] + 1 and nbr_sig_ids.shape[0] == nbr_margins.shape[0]
        return (sig_ids.shape[0], _p(sig_ids), _p(offsets), _p(nbr_sig_ids), _p(nbr_margins), (sig_ids, offsets, nbr_sig_ids, nbr_margins))

    def bayes_set_neighbors_prepared(self, prep):
        rc = self.L.lcd_bayes_set_neighbors(self.h, prep[0], prep[1], prep[2], prep[3], prep[4])
        if rc != LCD_OK:
            self._ck(rc)

    def bayes_update_dev(self, d_adjusted_ptr, exclude_recent=0, d_posterior_ptr=None, d_result_ptr=None):
        self._ck(self.L.lcd_bayes_update_dev(self.h, d_adjusted_ptr, exclude_recent, d_posterior_ptr, d_result_ptr))

    def bayes_update(self, sig_ids, adjusted):
        """lcd_bayes_update: the likelihood as parallel host arrays in std::map order (-1 first); returns the highest hypothesis."""
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        a = np.ascontiguousarray(adjusted, dtype=np.float32)
        assert s.shape[0] == a.shape[0]
        r = LcdBayesResult()
        self._ck(self.L.lcd_bayes_update(self.h, _p(s), _p(a), s.shape[0], C.byref(r)))
        return r

    def bayes_posterior(self, sig_ids):
        s = np.ascontiguousarray(sig_ids, dtype=np.int32)
        out = np.zeros(s.shape[0], np.float32)
        self._ck(self.L.lcd_bayes_posterior(self.h, _p(s), s.shape[0], _p(out)))
        return out

    def knn2_dev(self, d_queries_ptr, q, d_word_ids_ptr, d_dist_ptr):
        self._ck(self.L.lcd_knn2_dev(self.h, d_queries_ptr, q, d_word_ids_ptr, d_dist_ptr))

    def shard_knn2_dev(self, d_desc_ptr, q, d_cand_ptr):
        self._ck(self.L.lcd_shard_knn2_dev(self.h, d_desc_ptr, q, d_cand_ptr))

    def shard_frame_dev(self, d_desc_ptr, q, sig_id, N, rank, world, d_all_cand_ptr, total_live_rows, d_word_ids_ptr, d_lfix_ptr,
                        lfix_capacity, incremental=True, new_words_compared=True, nndr=0.8, first_new_word_id=0):
        flags = (LCD_Q_INCREMENTAL if incremental else 0) | (LCD_Q_NEW_WORDS_COMPARED if new_words_compared else 0)
        self._ck(self.L.lcd_shard_frame_dev(self.h, d_desc_ptr, q, flags, nndr, sig_id, first_new_word_id, float(N), rank, world,
                                            d_all_cand_ptr, total_live_rows, d_word_ids_ptr, d_lfix_ptr, lfix_capacity))

    def finalize_dev(self, d_lfix_ptr, n, d_like_ptr):
        self._ck(self.L.lcd_finalize_dev(self.h, d_lfix_ptr, n, d_like_ptr))

    def slots_dev(self):
        p, n = C.c_void_p(), C.c_int64()
        self._ck(self.L.lcd_slots_dev(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def stream(self):
        return self.L.lcd_stream(self.h)

    def profile_begin(self, max_samples):
        self._ck(self.L.lcd_profile_begin(self.h, max_samples))

    def profile_read(self):
        ms, n, name = C.c_float(), C.c_int(), C.c_char_p()
        self._ck(self.L.lcd_profile_read(self.h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def profile_read_likelihood(self):
        ms, n, name = C.c_float(), C.c_int(), C.c_char_p()
        self._ck(self.L.lcd_profile_read_likelihood(self.h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def record_event(self, event_handle):
        self._ck(self.L.lcd_record_event(self.h, event_handle))

    def set_option(self, key, value):
        self._ck(self.L.lcd_set_option(self.h, key.encode(), int(value)))

    def profile_score_work(self):
        out = (C.c_int64 * 8)()
        self._ck(self.L.lcd_profile_score_work(self.h, out))
        keys = ["dense_row_bytes", "sparse_postings", "directory_lookups", "directory_hits", "open_log_entries", "postings",
                "unique_words", "dense_words"]
        return {k: int(v) for k, v in zip(keys, out)}

    def stats(self):
        s = LcdStats()
        self._ck(self.L.lcd_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in LcdStats._fields_}
