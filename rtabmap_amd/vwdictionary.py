"""ctypes view of the C++ host mirror (rtabmap_amd/host: VWDictionaryHip / MemoryHip over the C-ABI).

Same method names as the reference classes (snake_case): update / add_new_words / find_nn / add_word_ref /
remove_all_word_ref / compute_likelihood ...  All search and scoring runs on the device through liblcd_hip.so.
"""
import ctypes as C

import numpy as np

from . import build as _build

kNNFlannNaive, kNNFlannKdTree, kNNFlannLSH, kNNBruteForce, kNNBruteForceGPU, kNNBruteForceHIP = 0, 1, 2, 3, 4, 5
_lib = None


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _type_of(a):
    if a.dtype == np.float32:
        return 0
    if a.dtype == np.uint8:
        return 1
    raise TypeError("descriptors must be float32 or uint8")


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(_build.build_host())
        vp, ci, cf = C.c_void_p, C.c_int, C.c_float
        L.hvwd_create.restype = vp
        L.hvwd_create.argtypes = [ci, ci, cf, ci, C.c_char_p, ci]
        L.hvwd_destroy.argtypes = [vp]
        L.hvwd_available.argtypes = [vp]
        L.hvwd_last_error.argtypes = [vp]
        L.hvwd_last_error.restype = C.c_char_p
        L.hvwd_add_new_words.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci]
        L.hvwd_find_nn.argtypes = [vp, vp, ci, ci, ci, vp]
        L.hvwd_update.argtypes = [vp]
        L.hvwd_match_frames.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, C.c_float, vp, vp, vp]
        L.hvwd_cross_check_word_ids.argtypes = [ci, vp, vp, ci, vp, vp]
        L.hvwd_cross_check_word_ids.restype = None
        L.hvwd_match_frames_guided.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, ci, vp, ci, ci, C.c_float, ci, vp, vp, vp, vp, vp]
        L.hvwd_guided_word_ids.argtypes = [ci, vp, vp, ci, vp, ci, vp, vp, vp, vp]
        L.hvwd_add_word.argtypes = [vp, ci, vp, ci, ci]
        L.hvwd_add_word_ref.argtypes = [vp, ci, ci]
        L.hvwd_remove_all_word_ref.argtypes = [vp, ci, ci]
        L.hvwd_get_unused_word_ids.argtypes = [vp, vp, ci]
        L.hvwd_delete_unused_words.argtypes = [vp]
        L.hvwd_clear.argtypes = [vp]
        L.hvwd_rebuild_engine.argtypes = [vp]
        L.hvwd_rebuild_engine.restype = ci
        L.hvwd_stat.argtypes = [vp, ci]
        L.hvwd_stat.restype = C.c_long
        L.hvwd_get_word_refs.argtypes = [vp, ci, vp, vp, ci]
        L.hvwd_index_ids.argtypes = [vp, vp, ci]
        L.hvwd_export_text.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.hmem_create.restype = vp
        L.hmem_create.argtypes = [ci, ci, cf, ci, C.c_char_p, ci]
        L.hmem_create_stm.restype = vp
        L.hmem_create_stm.argtypes = [ci, ci, cf, ci, C.c_char_p, ci, ci]
        L.hmem_create_select.restype = vp
        L.hmem_create_select.argtypes = [ci, ci, cf, ci, ci, ci, ci, ci, ci]
        L.hmem_update_select.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp]
        L.hmem_create_depth.restype = vp
        L.hmem_create_depth.argtypes = [ci, ci, cf, ci, ci, ci, ci, ci, ci, cf, cf]
        L.hmem_update_depth.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp, C.c_longlong, ci, ci, ci, vp, ci, vp, vp, vp, vp]
        cd = C.c_double
        L.hst_correspondences.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong, ci, ci, vp, ci, vp, vp]
        L.hst_generate.argtypes = [vp, vp, ci, vp, vp, vp, cf, cf, vp]
        L.hst_pyramid.argtypes = [vp, C.c_longlong, ci, ci, ci, ci, ci, vp, vp]
        L.hst_derivative.argtypes = [vp, C.c_longlong, ci, ci, vp]
        L.hst_derivative.restype = None
        L.hflow_track.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp]
        L.hmem_set_stereo_params.argtypes = [vp, vp]
        L.hmem_set_stereo_params.restype = None
        L.hmem_update_stereo.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp, C.c_longlong, vp, C.c_longlong, ci, ci, vp, vp, vp, vp, vp, vp]
        L.hk3_generate.argtypes = [vp, ci, vp, C.c_longlong, ci, ci, ci, vp, ci, cf, cf, vp]
        L.hk3_filter_3d.argtypes = [vp, ci, cf, cf, vp]
        L.hk3_filter_pixel.argtypes = [vp, ci, vp, C.c_longlong, ci, ci, ci, cf, cf, vp]
        L.hm3_cpu.argtypes = [vp, vp, ci, vp, vp, ci, ci, C.c_double, ci, ci, C.c_uint, ci, vp, vp, vp, vp, vp]
        L.hm3_estimate.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, C.c_double, ci, ci, C.c_uint, vp, vp, vp, vp, vp]
        L.hmp_cpu.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, C.c_double, ci, ci, cf, C.c_uint, ci, vp, vp, vp, vp, vp]
        L.hmba_cpu.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.hmba_refine.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        L.hmp_estimate.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, C.c_double, ci, ci, cf, C.c_uint, vp, vp, vp, vp, vp]
        L.hicp_cpu.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, C.c_double, cf, cf, ci, ci, vp, vp, vp, vp, vp]
        L.hicp_cells.argtypes = [vp, ci, C.c_double, vp]
        L.hicp_cells.restype = C.c_float
        L.hicp_finish.argtypes = [vp, vp, cf, C.c_double, cf, cf, cf, vp, vp, vp, vp]
        L.hicp_compute.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, ci, C.c_double, cf, cf, cf, cf, vp, vp, vp, vp]
        L.hicpp_cpu.argtypes = [vp, vp, ci, vp, vp, ci, vp, ci, ci, ci, C.c_double, cf, cf, cf, ci, ci, C.c_double, ci, ci, vp, vp, vp, vp, vp, vp]
        L.hicpp_compute.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, ci, vp, ci, ci, ci, C.c_double, cf, cf, cf, cf, ci, cf, ci, vp, vp, vp, vp]
        L.hicpf_compute.argtypes = [vp, vp, ci, ci, ci, vp, ci, ci, ci, vp, vp, ci, ci, C.c_double, cf, cf, cf, cf, ci, cf, ci, vp, vp, vp, vp, vp]
        L.hsf_cpu.argtypes = [vp, C.c_longlong, ci, ci, cf, cf, cf, ci, cf, cf, vp, C.c_longlong, ci, vp, vp, vp]
        L.hmem_select_error.argtypes = [vp]
        L.hmem_select_error.restype = C.c_char_p
        L.hfs_limit_keypoints.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp]
        L.hfs_limit_keypoints_compact.argtypes = [vp, ci, ci, vp]
        L.hfs_limit_keypoints_ssc.argtypes = [vp, vp, ci, ci, ci, ci, vp]
        L.hfs_limit_keypoints_ssc_compact.argtypes = [vp, vp, ci, ci, ci, ci, vp]
        L.hmem_create_select_ssc.restype = vp
        L.hmem_create_select_ssc.argtypes = [ci, ci, cf, ci, ci, ci, ci, ci, ci, ci]
        L.hfs_expand_word_ids.argtypes = [ci, vp, vp, ci, ci, vp]
        L.hmem_time_loop.argtypes = [vp, vp, ci, ci, ci, ci, ci]
        L.hmem_time_loop.restype = C.c_double
        L.hmem_time_loop_modes.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp]
        L.hmem_set_device_frames.argtypes = [vp, ci]
        L.hmem_set_device_frames.restype = None
        L.hmem_set_tfidf_likelihood_used.argtypes = [vp, ci]
        L.hmem_set_tfidf_likelihood_used.restype = None
        L.hmem_compare_to.argtypes = [vp, ci, ci]
        L.hmem_compare_to.restype = C.c_float
        L.hmem_set_global_descriptors.argtypes = [vp, ci, ci, vp, vp, vp]
        L.hmem_num_global_descriptors.argtypes = [vp, ci]
        L.hmem_fast_frame_device_ms.argtypes = [vp]
        L.hmem_fast_frame_device_ms.restype = C.c_double
        L.hmem_add_signatures_bulk.argtypes = [vp, vp, ci, ci, ci]
        L.hmem_compute_likelihood_flat.argtypes = [vp, ci, vp, vp, ci]
        L.hmem_compute_likelihood_of.argtypes = [vp, ci, vp, ci, vp, vp]
        L.hmem_add_link.argtypes = [vp, ci, ci, ci]
        L.hmem_get_neighbors_id.argtypes = [vp, ci, ci, vp, vp, ci]
        L.hmem_ids.argtypes = [vp, ci, vp, ci]
        L.hbayes_create.restype = vp
        L.hbayes_create.argtypes = [C.c_char_p, cf, ci]
        L.hbayes_destroy.argtypes = [vp]
        L.hbayes_reset.argtypes = [vp]
        L.hbayes_set_prediction_lc.argtypes = [vp, C.c_char_p]
        L.hbayes_get_prediction_lc.argtypes = [vp, vp, ci]
        L.hbayes_compute_posterior.argtypes = [vp, vp, vp, vp, ci, vp, vp, ci, vp, vp]
        L.hbayes_last_error.argtypes = [vp]
        L.hbayes_last_error.restype = C.c_char_p
        L.hrtab_create.restype = vp
        L.hrtab_create.argtypes = [cf, cf, ci, ci, C.c_char_p, cf, ci]
        L.hrtab_destroy.argtypes = [vp]
        L.hrtab_memory.restype = vp
        L.hrtab_memory.argtypes = [vp]
        L.hrtab_process.argtypes = [vp, vp, ci, ci, ci, vp, vp]
        L.hrtab_vector.argtypes = [vp, ci, vp, vp, ci]
        L.hrtab_create_epipolar.restype = vp
        L.hrtab_create_epipolar.argtypes = [cf, cf, ci, ci, C.c_char_p, cf, ci, ci, ci, cf]
        L.hrtab_process_keypoints.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp]
        L.hepi_cpu.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, C.c_double, C.c_uint, vp, vp, vp, vp]
        L.hepi_check.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, C.c_double, C.c_double, C.c_uint, vp, vp, vp, vp]
        L.hmono_cpu.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, ci, C.c_uint, C.c_double, ci, cf, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hmono_estimate.argtypes = [vp, vp, vp, vp, ci, vp, vp, ci, ci, C.c_double, ci, cf, C.c_uint, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hepi_accept.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, C.c_double, C.c_double, C.c_uint]
        L.hrtab_epipolar_kept.argtypes = [vp]
        L.hrtab_last_word_ids.argtypes = [vp, vp, ci]
        L.hmem_destroy.argtypes = [vp]
        L.hmem_vwd.restype = vp
        L.hmem_vwd.argtypes = [vp]
        L.hmem_update.argtypes = [vp, vp, ci, ci, ci, ci, vp]
        L.hmem_add_signature.argtypes = [vp, ci, vp, ci]
        L.hmem_forget.argtypes = [vp, ci]
        L.hmem_statistic.argtypes = [vp, C.c_char_p, ci]
        L.hmem_statistic.restype = C.c_float
        L.hmem_set_engine_option.argtypes = [vp, C.c_char_p, C.c_long]
        L.hmem_get_ni.argtypes = [vp, ci]
        L.hmem_num_signatures.argtypes = [vp]
        L.hmem_num_signatures.restype = C.c_long
        L.hmem_compute_likelihood.argtypes = [vp, vp, ci, vp, ci, vp, vp]
        L.hmem_load_data_from_db.argtypes = [vp, C.c_char_p, ci]
        L.hmem_load_error.argtypes = [vp]
        L.hmem_load_error.restype = C.c_char_p
        _lib = L
    return _lib


# ---- FeatureSelect (rtabmap_amd/host/FeatureSelect.h): the selection and expansion rule of include/lcd.h as plain host code, no engine
def limit_keypoints(response, points=None, max_keypoints=0, image_size=(0, 0), grid_rows=1, grid_cols=1, ssc=False):
    """Feature2D::limitKeypoints' inlier mask -> bool array, or None where the host mirror refuses (NaN response, keypoint outside the grid,
    image not larger than the grid).  ssc: Kp/SSC's square covering (a grid above 1 x 1, max_keypoints == 1, a keypoint outside the image and
    image sides outside 1 .. 16384 are refused as well)."""
    r = np.ascontiguousarray(response, dtype=np.float32).reshape(-1)
    p = None if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    if p is not None and p.shape[0] != r.shape[0]:
        raise ValueError("limit_keypoints: one point per response")
    out = np.zeros(max(r.shape[0], 1), np.uint8)
    if ssc:
        if grid_rows * grid_cols != 1:
            return None
        ok = lib().hfs_limit_keypoints_ssc(_p(r), _p(p), r.shape[0], int(max_keypoints), int(image_size[0]), int(image_size[1]), _p(out))
        return out[:r.shape[0]].astype(bool) if ok else None
    ok = lib().hfs_limit_keypoints(_p(r), _p(p), r.shape[0], int(max_keypoints), int(image_size[0]), int(image_size[1]), int(grid_rows), int(grid_cols), _p(out))
    return out[:r.shape[0]].astype(bool) if ok else None


def limit_keypoints_compact(response, max_keypoints=0, points=None, image_size=(0, 0), ssc=False):
    """the compacting form -> the kept indices in output order, or None on a NaN response.  ssc: Kp/SSC's square covering over points and
    image_size, refusing what limit_keypoints(ssc=True) refuses."""
    r = np.ascontiguousarray(response, dtype=np.float32).reshape(-1)
    out = np.zeros(max(r.shape[0], 1), np.int32)
    if ssc:
        p = None if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        if p is not None and p.shape[0] != r.shape[0]:
            raise ValueError("limit_keypoints_compact: one point per response")
        n = lib().hfs_limit_keypoints_ssc_compact(_p(r), _p(p), r.shape[0], int(max_keypoints), int(image_size[0]), int(image_size[1]), _p(out))
        return None if n < 0 else out[:n].copy()
    n = lib().hfs_limit_keypoints_compact(_p(r), r.shape[0], int(max_keypoints), _p(out))
    return None if n < 0 else out[:n].copy()


def expand_word_ids(n, index, word_ids, first_new_word_id=0):
    """Memory.cpp:6029-6059 -> one id per feature, or None on an index outside [0, n)"""
    i = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
    w = np.ascontiguousarray(word_ids, dtype=np.int32).reshape(-1)
    if i.shape != w.shape:
        raise ValueError("expand_word_ids: one id per index")
    out = np.zeros(max(int(n), 1), np.int32)
    ok = lib().hfs_expand_word_ids(int(n), _p(i), _p(w), i.shape[0], int(first_new_word_id), _p(out))
    return out[:int(n)].copy() if ok else None


# ---- Keypoints3D (rtabmap_amd/host/Keypoints3D.h): the depth stage's rule of include/lcd.h as plain host code, no engine
def _cameras_flat(cameras):
    """dicts fx, fy, cx, cy [, image_width, image_height, transform (12 floats or None)] -> [n x 20] float32 as c_shim.cpp reads them"""
    out = np.zeros((len(cameras), 20), np.float32)
    for c, m in enumerate(cameras):
        t = m.get("transform")
        out[c, :8] = [m["fx"], m["fy"], m["cx"], m["cy"], m.get("image_width", 0), m.get("image_height", 0), 0 if t is None else 1, 0]
        if t is not None:
            out[c, 8:] = np.asarray(t, np.float32).reshape(12)
    return out


def _depth_args(depth, width=None):
    d = depth if depth.strides[1] == depth.itemsize else np.ascontiguousarray(depth)
    assert d.dtype in (np.uint16, np.float32) and d.ndim == 2
    return d, (d.ctypes.data_as(C.c_void_p), d.strides[0], int(d.shape[1] if width is None else width), d.shape[0], 0 if d.dtype == np.uint16 else 1)


def generate_keypoints_3d_depth(points, depth, cameras, min_depth=0.0, max_depth=0.0, width=None):
    """util3d::generateKeypoints3DDepth -> [n x 3] float32, or None where the host mirror refuses"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    d, dargs = _depth_args(depth, width)
    cams = _cameras_flat(cameras)
    out = np.zeros((max(p.shape[0], 1), 3), np.float32)
    ok = lib().hk3_generate(_p(p), p.shape[0], *dargs, _p(cams), cams.shape[0], float(min_depth), float(max_depth), _p(out))
    return out[:p.shape[0]].copy() if ok else None


def filter_keypoints_by_depth_3d(xyz, min_depth=0.0, max_depth=0.0):
    """Feature2D::filterKeypointsByDepth, the 3-D overload -> the kept indices, or None where refused"""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(max(x.shape[0], 1), np.int32)
    n = lib().hk3_filter_3d(_p(x), x.shape[0], float(min_depth), float(max_depth), _p(out))
    return None if n < 0 else out[:n].copy()


def filter_keypoints_by_depth_pixel(points, depth, min_depth=0.0, max_depth=0.0, width=None):
    """... the 2-D overload -> the kept indices, or None where refused"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    d, dargs = _depth_args(depth, width)
    out = np.zeros(max(p.shape[0], 1), np.int32)
    n = lib().hk3_filter_pixel(_p(p), p.shape[0], *dargs, float(min_depth), float(max_depth), _p(out))
    return None if n < 0 else out[:n].copy()


# ---- StereoOpticalFlowHip (rtabmap_amd/host/Stereo.h): the stereo stage's rule of include/lcd.h as plain host code, no engine
STEREO_DEFAULTS = dict(win_width=15, win_height=3, max_level=5, iterations=30, eps=0.01, use_min_eigenvals=1, min_eig_threshold=1e-4,
                       error_threshold=50.0, min_disparity=0.5, max_disparity=128.0)


def _stereo_params_flat(params):
    v = dict(STEREO_DEFAULTS, **(params or {}))
    return np.array([v[k] for k in ("win_width", "win_height", "max_level", "iterations", "eps", "use_min_eigenvals", "min_eig_threshold",
                                    "error_threshold", "min_disparity", "max_disparity")], np.float64)


def _stereo_camera_flat(camera):
    t = camera.get("transform")
    c = np.array([camera["fx"], camera["fy"], camera["cx"], camera["cy"], camera.get("right_cx", 0.0), camera["baseline"], 0 if t is None else 1], np.float64)
    return c, (np.zeros(12, np.float32) if t is None else np.ascontiguousarray(t, dtype=np.float32).reshape(12))


def _gray_args(image, width=None):
    g = image if image.strides[1] == 1 else np.ascontiguousarray(image)
    assert g.dtype == np.uint8 and g.ndim == 2
    return g, (g.ctypes.data_as(C.c_void_p), g.strides[0]), int(g.shape[1] if width is None else width), g.shape[0]


def stereo_correspondences(left, right, points, params=None, width=None):
    """StereoOpticalFlow::computeCorrespondences, updateStatus included -> (right corners [n x 2] float32, status [n] uint8), or None where
    the host mirror refuses; left / right may be views with a row stride, width the image's where the arrays are wider"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    l, largs, w, h = _gray_args(left, width)
    r, rargs, rw, rh = _gray_args(right, width)
    if (w, h) != (rw, rh):
        return None
    sp = _stereo_params_flat(params)
    out, st = np.zeros((max(p.shape[0], 1), 2), np.float32), np.zeros(max(p.shape[0], 1), np.uint8)
    ok = lib().hst_correspondences(_p(sp), *largs, *rargs, w, h, _p(p), p.shape[0], _p(out), _p(st))
    return (out[:p.shape[0]].copy(), st[:p.shape[0]].copy()) if ok else None


def generate_keypoints_3d_stereo(points, right, camera, status=None, min_depth=0.0, max_depth=0.0):
    """util3d::generateKeypoints3DStereo -> [n x 3] float32, or None where the host mirror refuses"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(right, dtype=np.float32).reshape(-1, 2)
    s = None if status is None else np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    c, t = _stereo_camera_flat(camera)
    out = np.zeros((max(p.shape[0], 1), 3), np.float32)
    ok = lib().hst_generate(_p(p), _p(q), p.shape[0], _p(c), _p(t), _p(s), float(min_depth), float(max_depth), _p(out))
    return out[:p.shape[0]].copy() if ok else None


def stereo_pyramid(image, win_width=15, win_height=3, max_level=5, width=None):
    """the engine's pyramid of one image -> a list of uint8 arrays, or None where refused"""
    g, gargs, w, h = _gray_args(image, width)
    levels, sizes = np.zeros(2 * w * h + 16, np.uint8), np.zeros(32, np.int32)
    n = lib().hst_pyramid(*gargs, w, h, int(win_width), int(win_height), int(max_level), _p(levels), _p(sizes))
    if not n:
        return None
    out, at = [], 0
    for l in range(n):
        lw, lh = int(sizes[2 * l]), int(sizes[2 * l + 1])
        out.append(levels[at:at + lw * lh].reshape(lh, lw).copy())
        at += lw * lh
    return out


def stereo_derivative(image, width=None):
    """the Scharr derivative of the rule at every pixel -> (dx, dy) int16 arrays"""
    g, gargs, w, h = _gray_args(image, width)
    out = np.zeros((h, w, 2), np.int16)
    lib().hst_derivative(*gargs, w, h, _p(out))
    return out[:, :, 0].copy(), out[:, :, 1].copy()


# ---- flow_track_cpu (rtabmap_amd/host/FlowTrack.h): lcd_track_flow's rule of include/lcd.h as plain host code, no engine
from .capi import FLOW_DEFAULTS  # noqa: E402  (lcd_flow_params' defaults, stated once)


def flow_track_cpu(image_from, image_to, points, params=None, max_level=3, initial=None, width=None, as_device=False):
    """one pair through the host mirror -> dict(track [n x 2] float32, status [n] uint8, err [n] float32, kept: the indices RegistrationVis
    keeps), or None where the mirror refuses; the images may be views with a row stride, width the image's where the arrays are wider"""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    q = None if initial is None else np.ascontiguousarray(initial, dtype=np.float32).reshape(-1, 2)
    f, fargs, w, h = _gray_args(image_from, width)
    t, targs, tw, th = _gray_args(image_to, width)
    if (w, h) != (tw, th):
        return None
    v = dict(FLOW_DEFAULTS, **(params or {}))
    fp = np.array([v[k] for k in ("win_width", "win_height", "iterations", "eps", "use_min_eigenvals", "min_eig_threshold", "error_threshold")], np.float64)
    n = p.shape[0]
    track, status, err, kept = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
    k = lib().hflow_track(_p(fp), *fargs, *targs, w, h, int(max_level), _p(p), _p(q), n, 1 if as_device else 0, _p(track), _p(status), _p(err), _p(kept))
    return None if k < 0 else dict(track=track[:n].copy(), status=status[:n].copy(), err=err[:n].copy(), kept=kept[:k].copy())


def _frame_arrays(ids, xyz):
    i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    if x.shape[0] != i.shape[0]:
        raise ValueError("one 3-D point per word id")
    return i, x


def motion3d_cpu(from_ids, from_xyz, to_ids, to_xyz, min_inliers=20, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=0, sweeps=0):
    """the rule of lcd_estimate_motion_3d on the CPU (host/Motion3D.cpp, no device) -> dict(transform [12], status, variance, matches, inliers),
    or None where the call is refused.  sweeps != 0 is for measuring how the rule's Jacobi sweep count was chosen."""
    fi, fx = _frame_arrays(from_ids, from_xyz)
    ti, tx = _frame_arrays(to_ids, to_xyz)
    n = max(fi.shape[0], 1)
    t, sc, var = np.zeros(12, np.float32), np.zeros(3, np.int32), np.zeros(1, np.float64)
    om, oi = np.zeros(n, np.int32), np.zeros(n, np.int32)
    if fi.shape[0] > 8192 or ti.shape[0] > 8192:
        return None
    ok = lib().hm3_cpu(_p(fi), _p(fx), fi.shape[0], _p(ti), _p(tx), ti.shape[0], int(min_inliers), float(inlier_distance), int(iterations),
                       int(refine_iterations), int(seed) & 0xFFFFFFFF, int(sweeps), _p(t), _p(sc), _p(var), _p(om), _p(oi))
    if not ok:
        return None
    return dict(transform=t, status=int(sc[0]), variance=var[0], matches=om[:sc[1]].copy(), inliers=oi[:sc[2]].copy())


IDENTITY_GUESS = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _scan_arrays(from_xyz, to_xyz, guess):
    fx = np.ascontiguousarray(from_xyz, dtype=np.float32).reshape(-1, 3)
    tx = np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
    gs = np.ascontiguousarray(IDENTITY_GUESS if guess is None else guess, dtype=np.float32).reshape(12)
    return fx, tx, gs


def register_icp_cpu(from_xyz, to_xyz, guess=None, max_iterations=30, force_3dof=False, max_laser_scans=0, search=0, max_correspondence_distance=0.1,
                     epsilon=0.0, correspondence_ratio=0.1, device_entry=False):
    """the rule of lcd_register_icp on the CPU (host/RegistrationIcp.cpp, no device) -> dict(transform, icp_transform, correction [12], status, stop,
    iterations, n_correspondences, ratio, variance, match [n_from]), or None where the call is refused; device_entry: the refusals of
    lcd_register_icp_dev (a row that is not finite takes no part) instead of lcd_register_icp's (it is refused)"""
    fx, tx, gs = _scan_arrays(from_xyz, to_xyz, guess)
    if fx.shape[0] > 8192 or tx.shape[0] > 8192:
        return None
    t, sc, ratio, var = np.zeros(36, np.float32), np.zeros(4, np.int32), np.zeros(1, np.float32), np.zeros(1, np.float64)
    match = np.zeros(max(fx.shape[0], 1), np.int32)
    ok = lib().hicp_cpu(_p(fx), fx.shape[0], _p(tx), tx.shape[0], _p(gs), int(max_iterations), int(bool(force_3dof)), int(max_laser_scans),
                        float(max_correspondence_distance), float(epsilon), float(correspondence_ratio), int(search), int(bool(device_entry)), _p(t), _p(sc),
                        _p(ratio), _p(var), _p(match))
    if not ok:
        return None
    return dict(transform=t[:12].copy(), icp_transform=t[12:24].copy(), correction=t[24:].copy(), status=int(sc[0]), stop=int(sc[1]), iterations=int(sc[2]),
                n_correspondences=int(sc[3]), ratio=ratio[0], variance=var[0], match=match[:fx.shape[0]].copy())


def register_icp_plane_cpu(from_xyz, from_normals, to_xyz, to_normals, guess=None, max_iterations=30, force_3dof=False, max_laser_scans=0, search=0,
                           max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1, min_complexity=0.02, low_complexity_strategy=1,
                           normal_gate=False, min_normal_cos=0.0, device_entry=False):
    """the rule of lcd_register_icp_plane on the CPU (host/RegistrationIcp.cpp, no device) -> register_icp_cpu's dict and branch, complexity,
    complexity_values [3], complexity_vectors [9], second_eigenvalue; None where the call is refused"""
    fx, tx, gs = _scan_arrays(from_xyz, to_xyz, guess)
    fn, tn = np.ascontiguousarray(from_normals, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(to_normals, dtype=np.float32).reshape(-1, 3)
    if fx.shape[0] > 8192 or tx.shape[0] > 8192 or fn.shape != fx.shape or tn.shape != tx.shape:
        return None
    t, sc, ratio, var = np.zeros(36, np.float32), np.zeros(5, np.int32), np.zeros(1, np.float32), np.zeros(1, np.float64)
    match, cx = np.zeros(max(fx.shape[0], 1), np.int32), np.zeros(14, np.float32)
    ok = lib().hicpp_cpu(_p(fx), _p(fn), fx.shape[0], _p(tx), _p(tn), tx.shape[0], _p(gs), int(max_iterations), int(bool(force_3dof)), int(max_laser_scans),
                         float(max_correspondence_distance), float(epsilon), float(correspondence_ratio), float(min_complexity), int(low_complexity_strategy),
                         int(bool(normal_gate)), float(min_normal_cos), int(search), int(bool(device_entry)), _p(t), _p(sc), _p(ratio), _p(var), _p(match), _p(cx))
    if not ok:
        return None
    return dict(transform=t[:12].copy(), icp_transform=t[12:24].copy(), correction=t[24:].copy(), status=int(sc[0]), stop=int(sc[1]), iterations=int(sc[2]),
                n_correspondences=int(sc[3]), ratio=ratio[0], variance=var[0], match=match[:fx.shape[0]].copy(), branch=int(sc[4]), complexity=cx[0],
                complexity_values=cx[1:4].copy(), complexity_vectors=cx[4:13].copy(), second_eigenvalue=cx[13])


def filter_scans_cpu(xyz, capacity=None, downsampling_step=1, is_2d=False, normal_k=0, range_min=0.0, range_max=0.0, voxel_size=0.0, normal_radius=0.0,
                     ground_normals_up=0.0, viewpoint=(0.0, 0.0, 0.0), device_entry=False):
    """the rule of lcd_filter_scans on the CPU (host/ScanFilter.cpp, no device) for one scan and an output region of `capacity` rows (default:
    the scan's) -> dict(xyz, normals [capacity x 3] (None without normals), count, status, stage_counts [3]); the refusal's code (an int) where
    the call is refused"""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    cap = x.shape[0] if capacity is None else int(capacity)
    normals = normal_k > 0 or normal_radius > 0
    ox, on, ints = np.full((max(cap, 1), 3), 7.0, np.float32), np.full((max(cap, 1), 3), 7.0, np.float32), np.zeros(5, np.int32)
    vp = np.asarray(viewpoint, np.float32)
    rc = lib().hsf_cpu(_p(x), x.shape[0], int(downsampling_step), int(bool(is_2d)), float(range_min), float(range_max), float(voxel_size), int(normal_k),
                       float(normal_radius), float(ground_normals_up), _p(vp), cap, int(bool(device_entry)), _p(ox), _p(on), _p(ints))
    if rc != 0:
        return int(rc)
    return dict(xyz=ox[:cap], normals=on[:cap] if normals else None, count=int(ints[1]), status=int(ints[0]), stage_counts=ints[2:5].copy())


def register_icp_cells(x, max_correspondence_distance):
    """the grid form's cell of every coordinate (csrc/icp_rule.h) -> (cells int64 with None-like INT_MIN where out of range, the cell size)"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    out = np.zeros(max(x.shape[0], 1), np.int32)
    h = lib().hicp_cells(_p(x), x.shape[0], float(max_correspondence_distance), _p(out))
    return out[:x.shape[0]].astype(np.int64), np.float32(h)


def _icp_info(ok, t, info, corr, cov):
    return (t if ok else None), dict(icp_translation=info[0], icp_rotation=info[1], icp_inliers_ratio=info[2], icp_correspondences=int(corr[0]),
                                     covariance=cov.reshape(6, 6))


def register_icp_finish(result, max_translation=0.2, max_rotation=0.78, correspondence_ratio=0.1):
    """RegistrationIcpHip::finish (RegistrationIcp.cpp:856-961: the Euler-angle gate, variance / 10, the covariance) over a result of
    register_icp_cpu or of one pair of the engine's -> (transform [12] or None, info dict)"""
    tr = np.concatenate([np.asarray(result[k], np.float32).reshape(12) for k in ("transform", "icp_transform", "correction")])
    sc = np.array([result["status"], result["stop"], result["iterations"], result["n_correspondences"]], np.int32)
    t, info, corr, cov = np.zeros(12, np.float32), np.zeros(3, np.float32), np.zeros(1, np.int32), np.zeros(36, np.float64)
    ok = lib().hicp_finish(_p(tr), _p(sc), float(result["ratio"]), float(result["variance"]), float(max_translation), float(max_rotation),
                           float(correspondence_ratio), _p(t), _p(info), _p(corr), _p(cov))
    return _icp_info(ok, t, info, corr, cov)


def _pnp_arrays(to_ids, to_points, to_xyz, camera, image_size, local_transform, guess):
    ti = np.ascontiguousarray(to_ids, dtype=np.int32).reshape(-1)
    tp = np.ascontiguousarray(to_points, dtype=np.float32).reshape(-1, 2)
    tx = None if to_xyz is None else np.ascontiguousarray(to_xyz, dtype=np.float32).reshape(-1, 3)
    if tp.shape[0] != ti.shape[0] or (tx is not None and tx.shape[0] != ti.shape[0]):
        raise ValueError("one keypoint (and one 3-D point) per word id")
    cam = np.ascontiguousarray(camera, dtype=np.float32).reshape(4)
    img = np.ascontiguousarray(image_size, dtype=np.int32).reshape(2)
    loc = None if local_transform is None else np.ascontiguousarray(local_transform, dtype=np.float32).reshape(12)
    gs = None if guess is None else np.ascontiguousarray(guess, dtype=np.float32).reshape(12)
    return ti, tp, tx, cam, img, loc, gs


def _pn(a):
    return None if a is None else _p(a)


def motion_pnp_cpu(from_ids, from_xyz, to_ids, to_points, to_xyz=None, camera=(525.0, 525.0, 319.5, 239.5), image_size=(0, 0), local_transform=None,
                   guess=None, min_inliers=20, iterations=100, reproj_error=2.0, refine_iterations=1, variance_median_ratio=4, max_variance=0.0,
                   seed=0, steps=0):
    """the rule of lcd_estimate_motion_pnp on the CPU (host/Motion2D.cpp, no device) -> dict(transform [12], status, variance_lin, angle_cos,
    variance_kind, matches, inliers), or None where the call is refused.  steps != 0 is for measuring how the rule's Gauss-Newton step count
    was chosen."""
    fi, fx = _frame_arrays(from_ids, from_xyz)
    ti, tp, tx, cam, img, loc, gs = _pnp_arrays(to_ids, to_points, to_xyz, camera, image_size, local_transform, guess)
    if fi.shape[0] > 8192 or ti.shape[0] > 8192:
        return None
    n = max(ti.shape[0], 1)
    t, sc, var = np.zeros(12, np.float32), np.zeros(4, np.int32), np.zeros(2, np.float64)
    om, oi = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ok = lib().hmp_cpu(_p(fi), _p(fx), fi.shape[0], _p(ti), _p(tp), _pn(tx), ti.shape[0], _p(cam), _p(img), _pn(loc), _pn(gs), int(min_inliers),
                       int(iterations), float(reproj_error), int(refine_iterations), int(variance_median_ratio), float(max_variance),
                       int(seed) & 0xFFFFFFFF, int(steps), _p(t), _p(sc), _p(var), _p(om), _p(oi))
    if not ok:
        return None
    return dict(transform=t, status=int(sc[0]), variance_lin=var[0], angle_cos=var[1], variance_kind=int(sc[3]), matches=om[:sc[1]].copy(),
                inliers=oi[:sc[2]].copy())


def _kp_arrays(ids, points):
    i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    x = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    if x.shape[0] != i.shape[0]:
        raise ValueError("one keypoint per word id")
    return i, x


def epipolar_cpu(from_ids, from_points, to_ids, to_points, match_count_min=8, iterations=1000, ransac_threshold=3.0, seed=0):
    """the rule of lcd_verify_epipolar on the CPU (host/EpipolarGeometryHip.cpp, no device) -> dict(fundamental [9], status, matches,
    inliers), or None where the call is refused"""
    fi, fp = _kp_arrays(from_ids, from_points)
    ti, tp = _kp_arrays(to_ids, to_points)
    n = max(ti.shape[0], 1)
    f, sc = np.zeros(9, np.float32), np.zeros(3, np.int32)
    om, oi = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ok = lib().hepi_cpu(_p(fi), _p(fp), fi.shape[0], _p(ti), _p(tp), ti.shape[0], int(match_count_min), int(iterations), float(ransac_threshold),
                        int(seed) & 0xFFFFFFFF, _p(f), _p(sc), _p(om), _p(oi))
    if not ok:
        return None
    return dict(fundamental=f, status=int(sc[0]), matches=om[:sc[1]].copy(), inliers=oi[:sc[2]].copy())


def _mono_arrays(camera, local_transform, guess, from_points3, n_from):
    cam = np.array([camera[k] for k in ("fx", "fy", "cx", "cy")] if isinstance(camera, dict) else list(camera), np.float32).reshape(4)
    loc = None if local_transform is None else np.ascontiguousarray(local_transform, dtype=np.float32).reshape(12)
    gs = None if guess is None else np.ascontiguousarray(guess, dtype=np.float32).reshape(12)
    f3 = None if from_points3 is None else np.ascontiguousarray(from_points3, dtype=np.float32).reshape(-1, 3)
    if f3 is not None and f3.shape[0] != n_from:
        raise ValueError("one 3-D point per from word id")
    return cam, loc, gs, f3


def _mono_result(ok, t, var, sc, om, oi, p3):
    if not ok:
        return None
    return dict(transform=t, status=int(sc[0]), variance=float(var[0]), matches=om[:sc[1]].copy(), inliers=oi[:sc[2]].copy(), points3=p3[:sc[2]].copy())


def motion_mono_cpu(from_ids, from_points, to_ids, to_points, camera=(525.0, 525.0, 319.5, 239.5), from_points3=None, local_transform=None, guess=None,
                    min_inliers=20, iterations=1000, reproj_threshold=2.0, variance_median_ratio=4, max_variance=0.1, distance_threshold=50.0, seed=0):
    """the rule of lcd_estimate_motion_mono on the CPU (host/MotionMono.cpp, no device) -> dict(transform [12], status, variance, matches,
    inliers, points3 [inliers x 3]), or None where the call is refused"""
    fi, fp = _kp_arrays(from_ids, from_points)
    ti, tp = _kp_arrays(to_ids, to_points)
    cam, loc, gs, f3 = _mono_arrays(camera, local_transform, guess, from_points3, fi.shape[0])
    n = max(ti.shape[0], 1)
    t, var, sc = np.zeros(12, np.float32), np.zeros(1, np.float64), np.zeros(3, np.int32)
    om, oi, p3 = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
    f3p = None if f3 is None else f3.ctypes.data
    ok = lib().hmono_cpu(_p(fi), _p(fp), f3p, fi.shape[0], _p(ti), _p(tp), ti.shape[0], int(min_inliers), int(iterations), int(seed) & 0xFFFFFFFF,
                         float(reproj_threshold), int(variance_median_ratio), float(max_variance), float(distance_threshold), _p(cam), _pn(loc), _pn(gs),
                         _p(t), _p(var), _p(sc), _p(om), _p(oi), _p(p3))
    return _mono_result(ok, t, var, sc, om, oi, p3)


def _ba_camera(camera):
    """a camera dict(fx, fy, cx, cy[, image_width, image_height, local_transform]) as the shim's three arrays"""
    cam = np.array([camera["fx"], camera["fy"], camera["cx"], camera["cy"]], np.float32)
    img = np.array([camera.get("image_width", 0), camera.get("image_height", 0)], np.int32)
    loc = camera.get("local_transform")
    return cam, img, None if loc is None else np.ascontiguousarray(loc, dtype=np.float32).reshape(12)


def _ba_params(pixel_variance, robust_delta, baselines, max_inliers_mean_distance, min_inliers_distribution):
    return np.array([pixel_variance, robust_delta, baselines[0], baselines[1], max_inliers_mean_distance, min_inliers_distribution], np.float64)


DEFAULT_CAMERA = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def motion_ba_cpu(from_ids, from_xyz, to_ids, to_points, inliers, transform, from_points=None, to_xyz=None, prior_variance=None, camera_from=DEFAULT_CAMERA,
                  camera_to=DEFAULT_CAMERA, baselines=(0.075, 0.075), n_inliers=None, min_inliers=20, iterations=20, pixel_variance=1.0, robust_delta=8.0,
                  max_inliers_mean_distance=0.0, min_inliers_distribution=0.0):
    """the rule of lcd_refine_motion_ba on the CPU (host/MotionBA.cpp, no device) -> dict(transform [12], status, n_outliers, lm_accepted,
    chi2_before, chi2_after, inliers_mean_distance, inliers_distribution, inliers), or None where the call is refused.  n_inliers: the
    count that goes with `inliers` when it is not their number (the device's out_n_inliers)."""
    fi, fx = _frame_arrays(from_ids, from_xyz)
    ti, tp, tx, _, _, _, _ = _pnp_arrays(to_ids, to_points, to_xyz, (0, 0, 0, 0), (0, 0), None, None)
    fp = None if from_points is None else np.ascontiguousarray(from_points, dtype=np.float32).reshape(-1, 2)
    if fi.shape[0] > 8192 or ti.shape[0] > 8192:
        return None
    n = max(ti.shape[0], 1)
    il = np.zeros(n, np.int32)
    given = np.ascontiguousarray(inliers, dtype=np.int32).reshape(-1)[:n]
    il[:given.shape[0]] = given
    count = given.shape[0] if n_inliers is None else int(n_inliers)
    tr = np.ascontiguousarray(transform, dtype=np.float32).reshape(12)
    pv = None if prior_variance is None else np.ascontiguousarray(prior_variance, dtype=np.float64).reshape(2)
    cf, imf, lf = _ba_camera(camera_from)
    ct, imt, lt = _ba_camera(camera_to)
    prm = _ba_params(pixel_variance, robust_delta, baselines, max_inliers_mean_distance, min_inliers_distribution)
    t, ints, chi, gates, oi = np.zeros(12, np.float32), np.zeros(4, np.int32), np.zeros(2, np.float64), np.zeros(2, np.float32), np.zeros(n, np.int32)
    ok = lib().hmba_cpu(_p(fi), _p(fx), _pn(fp), fi.shape[0], _p(ti), _p(tp), _pn(tx), ti.shape[0], _p(il), count, _p(tr), _pn(pv), _p(cf), _p(imf), _pn(lf),
                        _p(ct), _p(imt), _pn(lt), _p(prm), int(iterations), int(min_inliers), _p(t), _p(ints), _p(chi), _p(gates), _p(oi))
    if not ok:
        return None
    return dict(transform=t, status=int(ints[0]), n_outliers=int(ints[2]), lm_accepted=int(ints[3]), chi2_before=chi[0], chi2_after=chi[1],
                inliers_mean_distance=gates[0], inliers_distribution=gates[1], inliers=oi[:ints[1]].copy())


class VWDictionaryHip:
    def __init__(self, strategy=kNNBruteForceHIP, incremental=True, nndr=0.8, new_words_compared_together=True,
                 dictionary_path="", device=0, _handle=None, _owner=None):
        self._owner = _owner
        self.h = _handle if _handle is not None else lib().hvwd_create(
            strategy, int(incremental), float(nndr), int(new_words_compared_together), dictionary_path.encode(), device)

    def close(self):
        if self.h and self._owner is None:
            lib().hvwd_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return lib().hvwd_last_error(self.h).decode()

    def add_new_words(self, desc, sig_id):
        desc = np.ascontiguousarray(desc)
        out = np.zeros(max(desc.shape[0], 1), np.int32)
        n = lib().hvwd_add_new_words(self.h, _p(desc), desc.shape[0], desc.shape[1] if desc.ndim == 2 else 0, _type_of(desc),
                                     sig_id, _p(out), out.shape[0])
        return out[:n].tolist()

    def find_nn(self, desc):
        desc = np.ascontiguousarray(desc)
        out = np.zeros(desc.shape[0], np.int32)
        lib().hvwd_find_nn(self.h, _p(desc), desc.shape[0], desc.shape[1], _type_of(desc), _p(out))
        return out.tolist()

    def match_frames(self, desc_from, desc_to, nn_type=1, nndr=0.8, original_from_ids=None):
        """VWDictionaryHip::matchFrames (RegistrationVis.cpp:1383-1504): (fromWordIds, toWordIds) of a frame pair over this dictionary's
        long-lived engine handle; the dictionary itself is untouched.  nn_type = Vis/CorNNType (0-4 temporary dictionary, 5 cross-check)."""
        f, t = np.ascontiguousarray(desc_from), np.ascontiguousarray(desc_to)
        ids = None if original_from_ids is None else np.ascontiguousarray(original_from_ids, dtype=np.int32)
        of, ot = np.zeros(max(f.shape[0], 1), np.int32), np.zeros(max(t.shape[0], 1), np.int32)
        ok = lib().hvwd_match_frames(self.h, _p(f), f.shape[0], _p(t), t.shape[0], f.shape[1], _type_of(f), nn_type, nndr,
                                     None if ids is None else _p(ids), _p(of), _p(ot))
        if not ok:
            raise RuntimeError("matchFrames: " + self.last_error())
        return of[: f.shape[0]].tolist(), ot[: t.shape[0]].tolist()

    def match_frames_guided(self, desc_from, desc_to, corners, corner_from_row, points_to, win_size=40, nn_type=1, nndr=0.8,
                            match_to_projection=False, original_from_ids=None):
        """VWDictionaryHip::matchFramesGuided (RegistrationVis.cpp:1078-1365): (fromWordIds, toWordIds, projectedIds) of a frame pair under a
        guess, over this dictionary's long-lived engine handle; the projection (corners, corner_from_row) is the caller's."""
        f, t = np.ascontiguousarray(desc_from), np.ascontiguousarray(desc_to)
        c = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 2)
        r = np.ascontiguousarray(corner_from_row, dtype=np.int32).reshape(-1)
        p = np.ascontiguousarray(points_to, dtype=np.float32).reshape(-1, 2)
        if r.shape[0] != c.shape[0] or p.shape[0] != t.shape[0]:
            raise ValueError("match_frames_guided: one from-row per corner, one point per to-row")
        ids = None if original_from_ids is None else np.ascontiguousarray(original_from_ids, dtype=np.int32)
        of, ot, op = np.zeros(max(f.shape[0], 1), np.int32), np.zeros(max(t.shape[0], 1), np.int32), np.zeros(max(c.shape[0], 1), np.int32)
        n = C.c_int(0)
        ok = lib().hvwd_match_frames_guided(self.h, _p(f), f.shape[0], _p(t), t.shape[0], f.shape[1], _type_of(f), _p(c), _p(r), c.shape[0], _p(p),
                                            int(win_size), nn_type, nndr, int(bool(match_to_projection)), None if ids is None else _p(ids),
                                            _p(of), _p(ot), _p(op), C.cast(C.byref(n), C.c_void_p))
        if not ok:
            raise RuntimeError("matchFramesGuided: " + self.last_error())
        return of[: f.shape[0]].tolist(), ot[: t.shape[0]].tolist(), op[: n.value].tolist()

    def estimate_motion_3d(self, words3a, words3b, min_inliers=20, inliers_distance=0.1, iterations=300, refine_iterations=5, seed=0):
        """Motion3D::estimateMotion3DTo3D (util3d_motion_estimation.cpp:730-807) over this dictionary's long-lived engine handle; a frame is
        (word ids, [n x 3] points), an id may repeat as in RegistrationVis' multimaps.  -> (transform [12] or None, covariance [6 x 6],
        matches, inliers)"""
        ia, xa = _frame_arrays(*words3a)
        ib, xb = _frame_arrays(*words3b)
        n = max(ia.shape[0], 1)
        t, cov, counts = np.zeros(12, np.float32), np.zeros(36, np.float64), np.zeros(2, np.int32)
        om, oi = np.zeros(n, np.int32), np.zeros(n, np.int32)
        ok = lib().hm3_estimate(self.h, _p(ia), _p(xa), ia.shape[0], _p(ib), _p(xb), ib.shape[0], int(min_inliers), float(inliers_distance),
                                int(iterations), int(refine_iterations), int(seed) & 0xFFFFFFFF, _p(t), _p(cov), _p(counts), _p(om), _p(oi))
        return (t if ok else None), cov.reshape(6, 6), om[:counts[0]].tolist(), oi[:counts[1]].tolist()

    def estimate_motion_pnp(self, words3a, words2b, words3b=None, camera=(525.0, 525.0, 319.5, 239.5), image_size=(0, 0), local_transform=None,
                            guess=None, min_inliers=20, iterations=100, reproj_error=2.0, refine_iterations=1, variance_median_ratio=4,
                            max_variance=0.0, seed=0):
        """Motion2D::estimateMotion3DTo2D (util3d_motion_estimation.cpp:59-289) over this dictionary's long-lived engine handle; words3a is
        (word ids, [n x 3] points), words2b (word ids, [n x 2] keypoints), words3b None or the [n x 3] points of words2b's rows; an id may
        repeat as in RegistrationVis' multimaps.  -> (transform [12] or None, covariance [6 x 6], matches, inliers)"""
        ia, xa = _frame_arrays(*words3a)
        ib, pb, xb, cam, img, loc, gs = _pnp_arrays(words2b[0], words2b[1], words3b, camera, image_size, local_transform, guess)
        n = max(ib.shape[0], 1)
        t, cov, counts = np.zeros(12, np.float32), np.zeros(36, np.float64), np.zeros(2, np.int32)
        om, oi = np.zeros(n, np.int32), np.zeros(n, np.int32)
        ok = lib().hmp_estimate(self.h, _p(ia), _p(xa), ia.shape[0], _p(ib), _p(pb), _pn(xb), ib.shape[0], _p(cam), _p(img), _pn(loc), _pn(gs),
                                int(min_inliers), int(iterations), float(reproj_error), int(refine_iterations), int(variance_median_ratio),
                                float(max_variance), int(seed) & 0xFFFFFFFF, _p(t), _p(cov), _p(counts), _p(om), _p(oi))
        return (t if ok else None), cov.reshape(6, 6), om[:counts[0]].tolist(), oi[:counts[1]].tolist()

    def verify_epipolar(self, kpts_a, kpts_b, match_count_min=8, ransac_param1=3.0, ransac_param2=0.99, seed=0):
        """EpipolarGeometryHip::check / findFFromWords (EpipolarGeometry.cpp:65-102, :298-379) over this dictionary's long-lived engine handle;
        kpts_a and kpts_b are (word ids, [n x 2] keypoints); an id may repeat.  -> (accepted, fundamental [9], pairs' ids, one status byte per
        pair, the engine's status), or None where the engine refuses the call"""
        ia, pa = _kp_arrays(*kpts_a)
        ib, pb = _kp_arrays(*kpts_b)
        n = max(ib.shape[0], 1)
        f, st, pairs, sc = np.zeros(9, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(3, np.int32)
        ok = lib().hepi_check(self.h, _p(ia), _p(pa), ia.shape[0], _p(ib), _p(pb), ib.shape[0], int(match_count_min), float(ransac_param1),
                              float(ransac_param2), int(seed) & 0xFFFFFFFF, _p(f), _p(st), _p(pairs), _p(sc))
        if not ok:
            return None
        return int(sc[0]) == 0, f, pairs[:sc[1]].tolist(), st[:sc[1]].copy(), int(sc[0])

    def estimate_motion_mono(self, kpts_a, kpts_b, words3a=None, camera=(525.0, 525.0, 319.5, 239.5), local_transform=None, guess=None, min_inliers=20,
                             reproj_threshold=2.0, variance_median_ratio=4, max_variance=0.1, seed=0):
        """MotionMonoHip::estimate (util3d_features.cpp:209-413 behind RegistrationVis.cpp:1584-1675, Vis/EstimationType = 2) over this
        dictionary's long-lived engine handle; kpts_a and kpts_b are (word ids, [n x 2] keypoints), words3a None or the [n x 3] points of
        kpts_a's rows (for the scale); an id may repeat.  -> dict(transform [12] (zeros: none), status, variance, matches, inliers, points3), or
        None where the engine refuses the call"""
        ia, pa = _kp_arrays(*kpts_a)
        ib, pb = _kp_arrays(*kpts_b)
        cam, loc, gs, f3 = _mono_arrays(camera, local_transform, guess, words3a, ia.shape[0])
        n = max(ib.shape[0], 1)
        t, var, sc = np.zeros(12, np.float32), np.zeros(1, np.float64), np.zeros(3, np.int32)
        om, oi, p3 = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
        f3p = None if f3 is None or f3.shape[0] == 0 else f3.ctypes.data
        ok = lib().hmono_estimate(self.h, _p(ia), _p(pa), f3p, ia.shape[0], _p(ib), _p(pb), ib.shape[0], int(min_inliers), float(reproj_threshold),
                                  int(variance_median_ratio), float(max_variance), int(seed) & 0xFFFFFFFF, _p(cam), _pn(loc), _pn(gs), _p(t), _p(var),
                                  _p(sc), _p(om), _p(oi), _p(p3))
        return _mono_result(ok, t, var, sc, om, oi, p3)

    def check_epipolar(self, kpts_a, kpts_b, match_count_min=8, ransac_param1=3.0, ransac_param2=0.99, seed=0):
        """EpipolarGeometryHip::check alone: the accept decision (False also where the engine refuses the call)"""
        ia, pa = _kp_arrays(*kpts_a)
        ib, pb = _kp_arrays(*kpts_b)
        return bool(lib().hepi_accept(self.h, _p(ia), _p(pa), ia.shape[0], _p(ib), _p(pb), ib.shape[0], int(match_count_min), float(ransac_param1),
                                      float(ransac_param2), int(seed) & 0xFFFFFFFF))

    def refine_motion_ba(self, words3a, kpts_b, inliers, transform, kpts_a=None, words3b=None, variance_kind=0, variance_lin=1.0, angle_cos=1.0,
                         camera_from=DEFAULT_CAMERA, camera_to=DEFAULT_CAMERA, baselines=(0.075, 0.075), min_inliers=20, iterations=20, pixel_variance=1.0,
                         robust_delta=8.0, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0):
        """MotionBA::refine (RegistrationVis.cpp:1873-2188, Vis/BundleAdjustment = 1) over this dictionary's long-lived engine handle: the
        transform, the inliers and the covariance's inputs as estimate_motion_pnp's call left them; words3a is (word ids, [n x 3] points),
        kpts_b (word ids, [n x 2] keypoints), kpts_a None or the [n x 2] keypoints of words3a's rows, words3b None or the [n x 3] points of
        kpts_b's rows.  -> (transform [12] or None, surviving inliers, info dict(status, inliers_mean_distance, inliers_distribution))"""
        ia, xa = _frame_arrays(*words3a)
        ib, pb, xb, _, _, _, _ = _pnp_arrays(kpts_b[0], kpts_b[1], words3b, (0, 0, 0, 0), (0, 0), None, None)
        pa = None if kpts_a is None else np.ascontiguousarray(kpts_a, dtype=np.float32).reshape(-1, 2)
        il = np.ascontiguousarray(inliers, dtype=np.int32).reshape(-1).copy()
        buf = np.zeros(max(il.shape[0], 1), np.int32)
        buf[:il.shape[0]] = il
        tr = np.ascontiguousarray(transform, dtype=np.float32).reshape(12)
        cf, imf, lf = _ba_camera(camera_from)
        ct, imt, lt = _ba_camera(camera_to)
        prm = _ba_params(pixel_variance, robust_delta, baselines, max_inliers_mean_distance, min_inliers_distribution)
        var = np.array([variance_lin, angle_cos], np.float64)
        t, ints, gates = np.zeros(12, np.float32), np.zeros(2, np.int32), np.zeros(2, np.float32)
        ok = lib().hmba_refine(self.h, _p(ia), _p(xa), _pn(pa), ia.shape[0], _p(ib), _p(pb), _pn(xb), ib.shape[0], _p(buf), il.shape[0], _p(tr),
                               int(variance_kind), _p(var), _p(cf), _p(imf), _pn(lf), _p(ct), _p(imt), _pn(lt), _p(prm), int(iterations), int(min_inliers),
                               _p(t), _p(ints), _p(gates))
        return (t if ok else None), buf[:ints[1]].tolist(), dict(status=int(ints[0]), inliers_mean_distance=float(gates[0]),
                                                                  inliers_distribution=float(gates[1]))

    def register_icp(self, from_scan, to_scan, guess=None, max_laser_scans=0, max_iterations=30, force_3dof=False, max_correspondence_distance=0.1,
                     epsilon=0.0, correspondence_ratio=0.1, max_translation=0.2, max_rotation=0.78):
        """RegistrationIcpHip::computeTransformation (RegistrationIcp.cpp:662-971, point to point, Icp/Strategy = 0) over this dictionary's
        long-lived engine handle; a scan is [n x 3] points in its base frame.  -> (transform [12] or None, info dict as register_icp_finish)"""
        fx, tx, gs = _scan_arrays(from_scan, to_scan, guess)
        t, info, corr, cov = np.zeros(12, np.float32), np.zeros(3, np.float32), np.zeros(1, np.int32), np.zeros(36, np.float64)
        ok = lib().hicp_compute(self.h, _p(fx), fx.shape[0], _p(tx), tx.shape[0], _p(gs), int(max_iterations), int(bool(force_3dof)), int(max_laser_scans),
                                float(max_correspondence_distance), float(epsilon), float(correspondence_ratio), float(max_translation), float(max_rotation),
                                _p(t), _p(info), _p(corr), _p(cov))
        return _icp_info(ok, t, info, corr, cov)

    def register_icp_normals(self, from_scan, from_normals, to_scan, to_normals, guess=None, from_is_2d=False, to_is_2d=False, max_laser_scans=0,
                             max_iterations=30, force_3dof=False, max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1, max_translation=0.2,
                             max_rotation=0.78, point_to_plane=True, min_complexity=0.02, low_complexity_strategy=1):
        """RegistrationIcpHip::computeTransformation over scans with normals ([n x 3], None: the scan has none) and the Icp/PointToPlane* keys:
        lcd_register_icp_plane for two 3-D scans with normals, register_icp's call otherwise -> (transform [12] or None, info dict with
        icp_structural_complexity)"""
        fx, tx, gs = _scan_arrays(from_scan, to_scan, guess)
        fn = None if from_normals is None else np.ascontiguousarray(from_normals, dtype=np.float32).reshape(-1, 3)
        tn = None if to_normals is None else np.ascontiguousarray(to_normals, dtype=np.float32).reshape(-1, 3)
        t, info, corr, cov = np.zeros(12, np.float32), np.zeros(4, np.float32), np.zeros(1, np.int32), np.zeros(36, np.float64)
        ok = lib().hicpp_compute(self.h, _p(fx), None if fn is None else _p(fn), fx.shape[0], int(bool(from_is_2d)), _p(tx), None if tn is None else _p(tn),
                                 tx.shape[0], int(bool(to_is_2d)), _p(gs), int(max_iterations), int(bool(force_3dof)), int(max_laser_scans),
                                 float(max_correspondence_distance), float(epsilon), float(correspondence_ratio), float(max_translation), float(max_rotation),
                                 int(bool(point_to_plane)), float(min_complexity), int(low_complexity_strategy), _p(t), _p(info), _p(corr), _p(cov))
        out = _icp_info(ok, t, info, corr, cov)
        out[1]["icp_structural_complexity"] = info[3]
        return out

    def register_icp_raw(self, from_scan, to_scan, guess=None, from_is_2d=False, to_is_2d=False, from_max_points=0, to_max_points=0, filters_enabled=3,
                         downsampling_step=1, range_min=0.0, range_max=0.0, voxel_size=0.05, point_to_plane_k=5, point_to_plane_radius=0.0,
                         ground_normals_up=0.0, max_iterations=30, force_3dof=False, max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1,
                         max_translation=0.2, max_rotation=0.78, point_to_plane=True, min_complexity=0.02, low_complexity_strategy=1):
        """RegistrationIcpHip::computeTransformation over RAW scans: lcd_filter_scans on the sides filters_enabled names, the reference's
        maxLaserScans bookkeeping, then register_icp_normals' work -> (transform [12] or None, info dict with icp_structural_complexity,
        from_rows, to_rows and max_laser_scans as the ICP got them)"""
        fx, tx, gs = _scan_arrays(from_scan, to_scan, guess)
        flt = np.array([downsampling_step, range_min, range_max, voxel_size, point_to_plane_k, point_to_plane_radius, ground_normals_up, filters_enabled], np.float32)
        t, info, corr, cov, sizes = np.zeros(12, np.float32), np.zeros(4, np.float32), np.zeros(1, np.int32), np.zeros(36, np.float64), np.zeros(3, np.int32)
        ok = lib().hicpf_compute(self.h, _p(fx), fx.shape[0], int(bool(from_is_2d)), int(from_max_points), _p(tx), tx.shape[0], int(bool(to_is_2d)),
                                 int(to_max_points), _p(gs), _p(flt), int(max_iterations), int(bool(force_3dof)), float(max_correspondence_distance),
                                 float(epsilon), float(correspondence_ratio), float(max_translation), float(max_rotation), int(bool(point_to_plane)),
                                 float(min_complexity), int(low_complexity_strategy), _p(t), _p(info), _p(corr), _p(cov), _p(sizes))
        out = _icp_info(ok, t, info, corr, cov)
        out[1].update(icp_structural_complexity=info[3], from_rows=int(sizes[0]), to_rows=int(sizes[1]), max_laser_scans=int(sizes[2]))
        return out

    def update(self):
        lib().hvwd_update(self.h)

    def add_word(self, word_id, desc):
        desc = np.ascontiguousarray(desc).reshape(-1)
        lib().hvwd_add_word(self.h, word_id, _p(desc), desc.shape[0], _type_of(desc))

    def add_word_ref(self, word_id, sig_id):
        return bool(lib().hvwd_add_word_ref(self.h, word_id, sig_id))

    def remove_all_word_ref(self, word_id, sig_id):
        lib().hvwd_remove_all_word_ref(self.h, word_id, sig_id)

    def get_unused_word_ids(self):
        n = lib().hvwd_get_unused_word_ids(self.h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        lib().hvwd_get_unused_word_ids(self.h, _p(out), n)
        return out[:n].tolist()

    def delete_unused_words(self):
        lib().hvwd_delete_unused_words(self.h)

    def clear(self):
        lib().hvwd_clear(self.h)

    def rebuild_engine(self):
        """VWDictionaryHip::rebuildEngine: a fresh device handle, replayed from the host maps (recovery after a device fault)"""
        return bool(lib().hvwd_rebuild_engine(self.h))

    def stat(self, which):
        return int(lib().hvwd_stat(self.h, which))

    visual_words = property(lambda s: s.stat(0))
    not_indexed_words = property(lambda s: s.stat(1))
    indexed_words = property(lambda s: s.stat(2))
    total_active_references = property(lambda s: s.stat(3))
    unused_words = property(lambda s: s.stat(5))

    def word_refs(self, word_id):
        n = lib().hvwd_get_word_refs(self.h, word_id, None, None, 0)
        if n < 0:
            return None
        s = np.zeros(max(n, 1), np.int32)
        c = np.zeros(max(n, 1), np.int32)
        lib().hvwd_get_word_refs(self.h, word_id, _p(s), _p(c), n)
        return dict(zip(s[:n].tolist(), c[:n].tolist()))

    def index_ids(self):
        n = lib().hvwd_index_ids(self.h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        lib().hvwd_index_ids(self.h, _p(out), n)
        return out[:n].tolist()

    def export_text(self, refs_path, desc_path):
        return lib().hvwd_export_text(self.h, (refs_path or "").encode(), (desc_path or "").encode())


class MemoryHip:
    def __init__(self, strategy=kNNBruteForceHIP, incremental=True, nndr=0.8, new_words_compared_together=True,
                 dictionary_path="", device=0, stm_size=10, _handle=None, _owner=None, max_features=None, grid_rows=1, grid_cols=1,
                 min_depth=None, max_depth=0.0, ssc=False):
        self._owner = _owner                    # a RtabmapHip owns its memory
        if _handle is not None:
            self.h = _handle
        elif min_depth is not None:             # ... and Kp/MinDepth, Kp/MaxDepth: update_depth() honours them
            self.h = lib().hmem_create_depth(strategy, int(incremental), float(nndr), int(new_words_compared_together), device, int(stm_size),
                                             int(500 if max_features is None else max_features), int(grid_rows), int(grid_cols), float(min_depth), float(max_depth))
        elif max_features is not None:          # Kp/MaxFeatures, Kp/GridRows, Kp/GridCols: update_select() honours them
            self.h = lib().hmem_create_select_ssc(strategy, int(incremental), float(nndr), int(new_words_compared_together), device, int(stm_size),
                                                  int(max_features), int(grid_rows), int(grid_cols), int(bool(ssc)))
        else:
            self.h = lib().hmem_create_stm(
                strategy, int(incremental), float(nndr), int(new_words_compared_together), dictionary_path.encode(), device, int(stm_size))
        self.vwd = VWDictionaryHip(_handle=lib().hmem_vwd(self.h), _owner=self)

    def close(self):
        if self.h and self._owner is None:
            lib().hmem_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, desc, nq=None):
        desc = np.ascontiguousarray(desc)
        rows = desc.shape[0]
        out = np.zeros(max(rows, 1), np.int32)
        sid = lib().hmem_update(self.h, _p(desc), rows, desc.shape[1], _type_of(desc), -1 if nq is None else nq, _p(out))
        return sid, out[:rows].tolist()

    def update_select(self, desc, responses, points=None, image_size=(0, 0)):
        """MemoryHip::update with the reference's own selection (Kp/MaxFeatures, Kp/GridRows, Kp/GridCols, Kp/SSC) -> (signature id, one id
        per descriptor); id 0: refused (select_error())"""
        desc = np.ascontiguousarray(desc)
        rows = desc.shape[0]
        r = np.ascontiguousarray(responses, dtype=np.float32).reshape(-1)
        p = None if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        if r.shape[0] != rows or (p is not None and p.shape[0] != rows):
            raise ValueError("update_select: one response (and one point) per descriptor")
        out = np.zeros(max(rows, 1), np.int32)
        sid = lib().hmem_update_select(self.h, _p(desc), rows, desc.shape[1], _type_of(desc), _p(r), _p(p), int(image_size[0]), int(image_size[1]), _p(out))
        return sid, out[:rows].tolist()

    def update_depth(self, desc, responses, points, image_size, depth, cameras, width=None):
        """MemoryHip::update for an RGB-D frame: the depth stage (Kp/MinDepth, Kp/MaxDepth), then the selection, the frame and the expansion
        -> (signature id, one id per KEPT feature, their 3-D points [k x 3], their indices); id 0: refused (select_error())"""
        desc = np.ascontiguousarray(desc)
        rows = desc.shape[0]
        r = np.ascontiguousarray(responses, dtype=np.float32).reshape(-1)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        if r.shape[0] != rows or p.shape[0] != rows:
            raise ValueError("update_depth: one response and one point per descriptor")
        d, dargs = _depth_args(depth, width)
        cams = _cameras_flat(cameras)
        ids, xyz, kept = np.zeros(max(rows, 1), np.int32), np.zeros((max(rows, 1), 3), np.float32), np.zeros(max(rows, 1), np.int32)
        k = C.c_int(0)
        sid = lib().hmem_update_depth(self.h, _p(desc), rows, desc.shape[1], _type_of(desc), _p(r), _p(p), int(image_size[0]), int(image_size[1]),
                                      *dargs, _p(cams), cams.shape[0], _p(ids), _p(xyz), _p(kept), C.addressof(k))
        return sid, ids[:k.value].tolist(), xyz[:k.value].copy(), kept[:k.value].copy()

    def set_stereo_params(self, params=None):
        """the Stereo/* parameters update_stereo() honours (a dict over STEREO_DEFAULTS)"""
        sp = _stereo_params_flat(params)
        lib().hmem_set_stereo_params(self.h, _p(sp))

    def update_stereo(self, desc, responses, points, image_size, left, right, camera, width=None):
        """MemoryHip::update for a stereo frame: the stereo stage (Stereo/*, Kp/MinDepth, Kp/MaxDepth), then the selection, the frame and the
        expansion -> (signature id, one id per KEPT feature, their 3-D points [k x 3], their indices); id 0: refused (select_error())"""
        desc = np.ascontiguousarray(desc)
        rows = desc.shape[0]
        r = np.ascontiguousarray(responses, dtype=np.float32).reshape(-1)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        if r.shape[0] != rows or p.shape[0] != rows:
            raise ValueError("update_stereo: one response and one point per descriptor")
        l, largs, w, h = _gray_args(left, width)
        rt, rargs, rw, rh = _gray_args(right, width)
        if (w, h) != (rw, rh):
            raise ValueError("update_stereo: the images differ in size")
        c, t = _stereo_camera_flat(camera)
        ids, xyz, kept = np.zeros(max(rows, 1), np.int32), np.zeros((max(rows, 1), 3), np.float32), np.zeros(max(rows, 1), np.int32)
        k = C.c_int(0)
        sid = lib().hmem_update_stereo(self.h, _p(desc), rows, desc.shape[1], _type_of(desc), _p(r), _p(p), int(image_size[0]), int(image_size[1]),
                                       *largs, *rargs, w, h, _p(c), _p(t), _p(ids), _p(xyz), _p(kept), C.addressof(k))
        return sid, ids[:k.value].tolist(), xyz[:k.value].copy(), kept[:k.value].copy()

    def select_error(self):
        return lib().hmem_select_error(self.h).decode()

    def add_signature(self, word_ids, sig_id=0):
        a = np.ascontiguousarray(word_ids, dtype=np.int32)
        return lib().hmem_add_signature(self.h, sig_id, _p(a), a.shape[0])

    def forget(self, sig_id):
        lib().hmem_forget(self.h, sig_id)

    STAT_NAMES = ("TimingMem/Pre_update/ms", "TimingMem/Joining_dictionary_update/ms", "TimingMem/Add_new_words/ms",
                  "Timing/Likelihood_computation/ms", "Timing/Forgetting/ms", "Keypoint/Dictionary_size/words",
                  "Keypoint/Current_frame/words", "Keypoint/Indexed_words/words", "Keypoint/Index_memory_usage/KB")

    def statistics(self, refresh=False):
        """MemoryHip::getStatistics(): the reference's statistic names (Statistics.h:178-212) -> value of the last frame."""
        out = {}
        for k, name in enumerate(self.STAT_NAMES):
            out[name] = float(lib().hmem_statistic(self.h, name.encode(), 1 if (refresh and k == 0) else 0))
        return out

    def set_engine_option(self, key, value):
        return int(lib().hmem_set_engine_option(self.h, key.encode(), int(value)))

    def load_data_from_db(self, path, last_state_only=True):
        """Memory::loadDataFromDb from a RTAB-Map database file (MemoryHip::loadDataFromDb, rtabmap_amd/host/DbLoaderHip.h): the
        dictionary indexed by one update(), every signature's references registered on the device in one bulk call.
        Returns the number of signatures loaded; raises with the loader's message on failure."""
        n = lib().hmem_load_data_from_db(self.h, str(path).encode(), int(last_state_only))
        if n < 0:
            raise RuntimeError("loadDataFromDb: " + lib().hmem_load_error(self.h).decode())
        return n

    def time_loop(self, frames, steps):
        """update + computeLikelihood against every signature + forget(oldest) per frame, looped and timed in C++ -> ms per frame"""
        f = np.ascontiguousarray(frames)
        return float(lib().hmem_time_loop(self.h, _p(f), f.shape[0], f.shape[1], f.shape[2], _type_of(f), int(steps)))

    def time_loop_modes(self, frames, steps, mode):
        """The same loop with the caller's list of ids kept from frame to frame; mode 0: std::map by value (the reference's signature),
        1: into a caller-owned std::map updated in place, 2: flat vectors.  -> ms per frame {step, update, likelihood, forget}"""
        f = np.ascontiguousarray(frames)
        out = np.zeros(4, np.float64)
        if lib().hmem_time_loop_modes(self.h, _p(f), f.shape[0], f.shape[1], f.shape[2], _type_of(f), int(steps), int(mode), _p(out)) != 0:
            raise RuntimeError("hmem_time_loop_modes failed: " + self.vwd.last_error())
        return dict(zip(("step", "update", "likelihood", "forget"), out.tolist()))

    def fast_frame_device_ms(self):
        """mean ms a device-resident update() spent inside lcd_frame_host (the rest of update() is the mirror's std::map bookkeeping)"""
        return float(lib().hmem_fast_frame_device_ms(self.h))

    def set_device_frames(self, on):
        """MemoryHip::setDeviceFrames: update() as ONE device call (lcd_frame_host) that also brings the likelihood back (default), or the
        call-by-call path (lcd_quantize / lcd_sig_add / lcd_likelihood)."""
        lib().hmem_set_device_frames(self.h, int(bool(on)))

    def set_tfidf_likelihood_used(self, on):
        """Kp/TfIdfLikelihoodUsed.  False: compute_likelihood / compute_likelihood_of answer with Signature::compareTo's words branch
        (Memory.cpp:2179-2214, lcd_similarity) instead of TF-IDF."""
        lib().hmem_set_tfidf_likelihood_used(self.h, int(bool(on)))

    def compare_to(self, sig_a, sig_b):
        """sigA->compareTo(*sigB) for two signatures in memory (what Memory::rehearsal compares, Memory.cpp:4245): by their global
        descriptors where both carry one of type 1 on the same channel, by their words otherwise"""
        return float(lib().hmem_compare_to(self.h, int(sig_a), int(sig_b)))

    def set_global_descriptors(self, sig_id, descs):
        """SensorData::setGlobalDescriptors of a signature in memory: descs[i] is channel i, a float row (type 1) or (type, row or None);
        an empty list clears them.  False: refused (no such signature, too many or too long)."""
        types, dims, rows = [], [], []
        for d in descs:
            typ, row = d if isinstance(d, tuple) else (1, d)
            row = np.zeros(0, np.float32) if row is None else np.ascontiguousarray(row, dtype=np.float32).reshape(-1)
            types.append(int(typ)); dims.append(row.shape[0]); rows.append(row)
        t, m = np.asarray(types, np.int32), np.asarray(dims, np.int32)
        data = np.concatenate(rows) if rows else np.zeros(0, np.float32)
        return bool(lib().hmem_set_global_descriptors(self.h, int(sig_id), len(types), _p(t), _p(m), _p(data)))

    def num_global_descriptors(self, sig_id):
        return int(lib().hmem_num_global_descriptors(self.h, int(sig_id)))

    def add_signatures_bulk(self, words, first_id=1):
        """n signatures (rows of `words`) through Memory::addSignature in C++, then ONE bulk registration on the device"""
        w = np.ascontiguousarray(words, dtype=np.int32)
        n = lib().hmem_add_signatures_bulk(self.h, _p(w), w.shape[0], w.shape[1], int(first_id))
        if n != w.shape[0]:
            raise RuntimeError("add_signatures_bulk failed: " + self.vwd.last_error())
        return n

    def compute_likelihood_of(self, sig_id, ids):
        """Memory::computeLikelihood(signature id, ids) -> (ids ascending, values)"""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        oi, ov = np.zeros(max(a.shape[0], 1), np.int32), np.zeros(max(a.shape[0], 1), np.float32)
        n = lib().hmem_compute_likelihood_of(self.h, int(sig_id), _p(a), a.shape[0], _p(oi), _p(ov))
        return oi[:n], ov[:n]

    def compute_likelihood_flat(self, sig_id, cap=1 << 21):
        oi, ov = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        n = lib().hmem_compute_likelihood_flat(self.h, int(sig_id), _p(oi), _p(ov), cap)
        if n < 0:
            return None
        return oi[:n], ov[:n]

    def get_ni(self, sig_id):
        return lib().hmem_get_ni(self.h, sig_id)

    def num_signatures(self):
        return int(lib().hmem_num_signatures(self.h))

    def add_link(self, a, b, neighbor=False):
        """Memory::addLink for a global loop closure between two signatures in memory (neighbor=True: an odometry link of a
        signature replayed from the database)."""
        return bool(lib().hmem_add_link(self.h, a, b, 0 if neighbor else 1))

    def get_neighbors_id(self, sig_id, max_graph_depth):
        cap = 4096
        ids, mg = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = lib().hmem_get_neighbors_id(self.h, sig_id, max_graph_depth, _p(ids), _p(mg), cap)
        assert n <= cap
        return dict(zip(ids[:n].tolist(), mg[:n].tolist()))

    def _ids(self, which):
        n = lib().hmem_ids(self.h, which, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        lib().hmem_ids(self.h, which, _p(out), n)
        return out[:n].tolist()

    def st_mem(self):
        return self._ids(0)

    def working_mem(self):
        """Ids of the working memory, the virtual place (-1) first, as Memory::getWorkingMem()."""
        return self._ids(1)

    def compute_likelihood(self, words, ids):
        w = np.ascontiguousarray(words, dtype=np.int32)
        i = np.ascontiguousarray(ids, dtype=np.int32)
        oid = np.zeros(max(i.shape[0], 1), np.int32)
        out = np.zeros(max(i.shape[0], 1), np.float32)
        n = lib().hmem_compute_likelihood(self.h, _p(w), w.shape[0], _p(i), i.shape[0], _p(oid), _p(out))
        return oid[:n], out[:n]


class BayesFilterHip:
    """rtabmap::BayesFilter's interface over the device filter (rtabmap_amd/host/BayesFilterHip.h)."""

    def __init__(self, prediction_lc="", virtual_place_prior=0.9, full_prediction_update=False):
        self.h = lib().hbayes_create(prediction_lc.encode(), float(virtual_place_prior), int(full_prediction_update))
        self.highest_hypothesis = (0, 0.0)

    def close(self):
        if self.h:
            lib().hbayes_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        lib().hbayes_reset(self.h)

    def set_prediction_lc(self, s):
        lib().hbayes_set_prediction_lc(self.h, s.encode())

    def get_prediction_lc(self):
        out = np.zeros(64, np.float64)
        n = lib().hbayes_get_prediction_lc(self.h, _p(out), 64)
        return out[:n].copy()

    def compute_posterior(self, memory, ids, values):
        """likelihood = {ids[i]: values[i]}; returns (ids, posterior) in std::map order."""
        i = np.ascontiguousarray(ids, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float32)
        cap = max(i.shape[0], 1) + 8
        oid, out = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        hid, hv = C.c_int(0), C.c_float(0.0)
        n = lib().hbayes_compute_posterior(self.h, memory.h, _p(i), _p(v), i.shape[0], _p(oid), _p(out), cap, C.byref(hid), C.byref(hv))
        self.highest_hypothesis = (hid.value, hv.value)
        return oid[:n].copy(), out[:n].copy()

    def last_error(self):
        return lib().hbayes_last_error(self.h).decode()


class RtabmapHip:
    """The loop-closure detection block of Rtabmap::process (rtabmap_amd/host/RtabmapHip.h): one frame of descriptors in, the highest
    hypothesis and the accepted loop closure out."""

    def __init__(self, loop_thr=0.11, loop_ratio=0.0, virtual_place_likelihood_ratio=0, stm_size=10, prediction_lc="",
                 virtual_place_prior=0.9, device=0, epipolar=None):
        """epipolar: None, or dict(enabled, match_count_min, ransac_param1) -- VhEp/Enabled, VhEp/MatchCountMin, VhEp/RansacParam1"""
        if epipolar is None:
            self.h = lib().hrtab_create(float(loop_thr), float(loop_ratio), int(virtual_place_likelihood_ratio), int(stm_size),
                                        prediction_lc.encode(), float(virtual_place_prior), device)
        else:
            self.h = lib().hrtab_create_epipolar(float(loop_thr), float(loop_ratio), int(virtual_place_likelihood_ratio), int(stm_size),
                                                 prediction_lc.encode(), float(virtual_place_prior), device, 1 if epipolar.get("enabled", True) else 0,
                                                 int(epipolar.get("match_count_min", 8)), float(epipolar.get("ransac_param1", 3.0)))
        self.memory = MemoryHip(_handle=lib().hrtab_memory(self.h), _owner=self)

    def close(self):
        if self.h:
            self.memory.h = None
            lib().hrtab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, desc, keypoints=None):
        """keypoints: None, or [rows x 2] positions for the epipolar check (VhEp/Enabled) -> dict(id, highest=(id, value), loop=(id, value))"""
        desc = np.ascontiguousarray(desc)
        out4 = np.zeros(4, np.int32)
        val2 = np.zeros(2, np.float32)
        if keypoints is None:
            lib().hrtab_process(self.h, _p(desc), desc.shape[0], desc.shape[1], _type_of(desc), _p(out4), _p(val2))
        else:
            kp = np.ascontiguousarray(keypoints, dtype=np.float32).reshape(-1, 2)
            if kp.shape[0] != desc.shape[0]:
                raise ValueError("one keypoint per descriptor row")
            lib().hrtab_process_keypoints(self.h, _p(desc), desc.shape[0], desc.shape[1], _type_of(desc), _p(kp), _p(out4), _p(val2))
        return {"id": int(out4[0]), "highest": (int(out4[1]), float(val2[0])), "loop": (int(out4[2]), float(val2[1])), "ok": bool(out4[3])}

    def epipolar_kept(self):
        """the number of signatures whose word ids and keypoints are kept for the epipolar check"""
        return int(lib().hrtab_epipolar_kept(self.h))

    def vector(self, which):
        """which: "raw" | "likelihood" | "posterior" of the last frame -> (ids, values) in std::map order"""
        w = {"raw": 0, "likelihood": 1, "posterior": 2}[which]
        n = lib().hrtab_vector(self.h, w, None, None, 0)
        ids, out = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
        lib().hrtab_vector(self.h, w, _p(ids), _p(out), n)
        return ids[:n].copy(), out[:n].copy()

    def last_word_ids(self):
        out = np.zeros(16384, np.int32)
        n = lib().hrtab_last_word_ids(self.h, _p(out), 16384)
        return out[:n].tolist()
