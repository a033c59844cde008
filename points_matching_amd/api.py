"""Python mirror of include/pm.h over ctypes (plumbing for tests and bench.py, not the product).

The product is libpm_hip.so (HIP kernels behind a C ABI) driven by the C++ host in host/;
this module only forwards numpy arrays / torch device pointers to that ABI.  There is NO CPU
fallback: if the library is missing or a call fails, PmError is raised.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PM_LIB_PATH") or os.path.join(_HERE, "libpm_hip.so")   # override: experiments only

MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"),
                        ("distance", "<f4")])
PM_MAX_K = 16
PM_KNN_FORCE_EXACT = 1
PM_KNN_FORCE_F32 = 2
PM_KNN_HINT_INTEGER = 4
PM_KNN_HINT_U8 = 8
PM_KNN_HINT_UNIT_NORM = 16
PM_CROSS_RATIO_FWD = 1     # cross-check (S41): + ratio test on the forward row
PM_CROSS_RATIO_REV = 2     # ... on the reverse row
PM_GUIDE_F_SAMPSON = 0     # guided matching (S48): gate kinds
PM_GUIDE_F_SYM = 1
PM_GUIDE_H = 2
PM_ERR_SAMPSON = 0
PM_ERR_SYM_EPIPOLAR = 1
PM_ERR_REPROJ = 2          # robust homography and affine (pm_ransac_homography*, pm_ransac_affine*)
PM_AFFINE_FULL = 0         # 6 DOF (cv::estimateAffine2D)
PM_AFFINE_PARTIAL = 1      # 4 DOF: rotation, uniform scale, translation (cv::estimateAffinePartial2D)
PM_OK, PM_E_INVALID, PM_E_TOO_FEW, PM_E_NO_MODEL, PM_E_HIP, PM_E_NOMEM, PM_E_UNSUPPORTED = \
    0, -1, -2, -3, -4, -5, -6

# every extern "C" symbol include/pm.h declares (tests check the library exports all of them)
EXPORTS = [
    "pm_ctx_create", "pm_ctx_destroy", "pm_ctx_set_stream", "pm_ctx_synchronize",
    "pm_ctx_timing_enable", "pm_ctx_timing_reset", "pm_ctx_timing_get", "pm_ctx_knn_diag_enable", "pm_ctx_knn_stats", "pm_ctx_knn_route",
    "pm_ctx_filter_fusion_status", "pm_ctx_scratch_info",
    "pm_last_error",
    "pm_status_string", "pm_version",
    "pm_bf_knn_l2_f32", "pm_bf_knn_l2_f32_dev", "pm_bf_knn_hamming_u8", "pm_bf_knn_hamming_u8_dev",
    "pm_filter_midpoint", "pm_filter_ratio", "pm_match_indices", "pm_gather_points",
    "pm_format_match_list",
    "pm_filter_ratio_gather_dev", "pm_filter_midpoint_gather_dev", "pm_concat_points_dev",
    "pm_ransac_fundamental", "pm_ransac_score_dev", "pm_ransac_score_devn", "pm_ransac_model_from_hyp",
    "pm_ransac_model_from_key_dev", "pm_ransac_run_dev", "pm_ransac_shard_parts_dev", "pm_ransac_finish_parts_dev",
    "pm_ctx_set_option", "pm_ctx_get_option", "pm_bf_knn_l2_ratio_dev",
    "pm_flann_build", "pm_flann_destroy", "pm_flann_knn_l2_f32", "pm_flann_knn_l2_f32_dev", "pm_flann_export",
    "pm_mgpu_create", "pm_mgpu_destroy", "pm_mgpu_size", "pm_mgpu_ctx", "pm_mgpu_ransac_fundamental", "pm_mgpu_match_ransac",
    "pm_mgpu_lane_ctx", "pm_mgpu_set_lanes", "pm_mgpu_set_train", "pm_mgpu_set_train_dev", "pm_mgpu_submit_dev", "pm_mgpu_collect",
    "pm_mgpu_allgather_latency", "pm_mgpu_batch_run", "pm_mgpu_batch_set_option",
    "pm_batch_create", "pm_batch_destroy", "pm_batch_run", "pm_batch_set_option", "pm_batch_set_desc_type", "pm_batch_set_host_threads",
    "pm_bf_knn_l2_u8", "pm_bf_knn_l2_u8_dev", "pm_bf_knn_l2_u8_ratio_dev", "pm_host_register", "pm_host_unregister",
    "pm_lmeds_fundamental", "pm_lmeds_fundamental_dev", "pm_lmeds_default_iters", "pm_ransac7_adaptive",
    "pm_epipolar_residuals", "pm_f_scale_f33", "pm_epilines", "pm_epiline_endpoints",
    "pm_ransac_homography", "pm_ransac_homography_run_dev", "pm_ransac_homography_from_hyp",
    "pm_homography_refine", "pm_homography_refine_dev", "pm_ransac_homography_refined",
    "pm_ransac_affine", "pm_ransac_affine_from_hyp", "pm_ransac_affine_run_dev", "pm_affine_refine", "pm_affine_refine_dev",
    "pm_estimate_affine",
    "pm_ransac_essential", "pm_ransac_essential_from_hyp", "pm_ransac_essential_run_dev", "pm_recover_pose",
    "pm_recover_pose_dev", "pm_estimate_pose",
    "pm_fundamental_refine", "pm_fundamental_refine_dev", "pm_ransac_fundamental_refined",
    "pm_pose_refine", "pm_pose_refine_dev", "pm_estimate_pose_refined",
    "pm_ransac_pnp", "pm_ransac_pnp_from_hyp", "pm_ransac_pnp_run_dev", "pm_pnp_refine", "pm_pnp_refine_dev",
    "pm_solve_pnp_ransac", "pm_gather_pnp_dev", "pm_triangulate_dev", "pm_triangulate",
    "pm_bundle_adjust_workspace", "pm_bundle_adjust_dev", "pm_bundle_adjust",
    "pm_pose_graph_workspace", "pm_pose_graph_optimize_dev", "pm_pose_graph_optimize", "pm_pgo_move_points_dev",
    "pm_pgo_move_points",
    "pm_ransac_align3d", "pm_ransac_align3d_from_hyp", "pm_ransac_align3d_run_dev", "pm_align3d_refine",
    "pm_align3d_refine_dev", "pm_estimate_align3d", "pm_transform_points3_dev", "pm_transform_points3",
    "pm_gather_align3d_dev",
    "pm_vocab_create", "pm_vocab_destroy", "pm_vocab_set", "pm_vocab_set_dev", "pm_vocab_get", "pm_vocab_init_stride_dev",
    "pm_vocab_train_dev", "pm_vocab_train", "pm_vocab_assign_dev", "pm_vocab_assign",
    "pm_bowdb_create", "pm_bowdb_destroy", "pm_bowdb_clear_dev", "pm_bowdb_add_dev", "pm_bowdb_add", "pm_bowdb_set_weights",
    "pm_bowdb_get_weights", "pm_bowdb_idf_dev", "pm_bowdb_query_dev", "pm_bowdb_query", "pm_bowdb_get",
    "pm_filter_cross", "pm_filter_cross_gather_dev",
    "pm_bf_match_cross_l2_f32_dev", "pm_bf_match_cross_l2_u8_dev", "pm_bf_match_cross_hamming_u8_dev",
    "pm_bf_match_cross_l2_f32", "pm_bf_match_cross_l2_u8", "pm_bf_match_cross_hamming_u8",
    "pm_bf_knn_guided_l2_f32_dev", "pm_bf_knn_guided_l2_u8_dev", "pm_bf_knn_guided_hamming_u8_dev",
    "pm_bf_match_guided_l2_f32_dev", "pm_bf_match_guided_l2_u8_dev", "pm_bf_match_guided_hamming_u8_dev",
    "pm_bf_knn_guided_l2_f32", "pm_bf_knn_guided_l2_u8", "pm_bf_knn_guided_hamming_u8",
    "pm_pad_rows_u8", "pm_pad_rows_u8_dev",
    "pm_detect_describe_dev", "pm_detect_describe", "pm_detect_level_get", "pm_detect_tables",
    "pm_detect_describe_bits_dev", "pm_detect_describe_bits", "pm_detect_bits_table",
    "pm_pyramid_create", "pm_pyramid_destroy", "pm_pyramid_build_dev", "pm_pyramid_level_get",
    "pm_track_lk_dev", "pm_track_lk_gather_dev", "pm_track_lk",
    "pm_corners_dev", "pm_corners_replenish_dev", "pm_corners",
    "pm_describe_points_dev", "pm_describe_points_gather_dev", "pm_describe_points", "pm_describe_points_tables",
    "pm_warp_dev", "pm_warp", "pm_transform_points_dev", "pm_transform_points",
    "pm_undistort_points_dev", "pm_undistort_points", "pm_distort_points_dev", "pm_distort_points",
    "pm_undistort_dev", "pm_undistort", "pm_undistort_map_dev", "pm_remap_dev", "pm_remap",
    "pm_stereo_rectify", "pm_stereo_bm_dev", "pm_stereo_bm", "pm_stereo_lr_check_dev", "pm_stereo_points_dev", "pm_stereo_points",
    "pm_stereo_sgm_dev", "pm_stereo_sgm",
    "pm_device_alloc", "pm_device_free", "pm_device_upload", "pm_device_download",
]


class PmError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("pm status %d: %s" % (status, msg))
        self.status = status


class RansacParams(C.Structure):
    _fields_ = [("hyp_begin", C.c_int64), ("hyp_end", C.c_int64), ("seed", C.c_uint64),
                ("thresh_px", C.c_float), ("error_kind", C.c_int32)]


class PointsView(C.Structure):
    """pm_points_view: `parts` padded blocks of correspondences with device-side counts (include/pm.h)."""
    _fields_ = [("xy1", C.c_void_p), ("xy2", C.c_void_p), ("counts", C.c_void_p), ("parts", C.c_int32),
                ("cap", C.c_int32), ("pitch_xy", C.c_int64), ("pitch_cnt", C.c_int32), ("reserved", C.c_int32)]


class LkParams(C.Structure):
    """pm_lk_params (include/pm.h, SPEC S61-S66); lk_params() fills it with OpenCV's defaults."""
    _fields_ = [("win_radius", C.c_int32), ("max_level", C.c_int32), ("max_iters", C.c_int32), ("eps", C.c_float),
                ("min_eig", C.c_float), ("fb_thresh", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


PM_LK_USE_INITIAL = 1


def lk_params(win_radius=10, max_level=3, max_iters=30, eps=0.01, min_eig=1e-4, fb_thresh=0.0, flags=0):
    return LkParams(win_radius, max_level, max_iters, eps, min_eig, fb_thresh, flags, 0)


class CornerParams(C.Structure):
    """pm_corner_params (include/pm.h, SPEC S67-S70); corner_params() fills it."""
    _fields_ = [("block_radius", C.c_int32), ("min_eig", C.c_float), ("quality", C.c_float), ("min_dist", C.c_float),
                ("capacity", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


def corner_params(block_radius=10, min_eig=1e-4, quality=0.01, min_dist=8.0, capacity=0):
    """block_radius: use the tracker's win_radius to share its eigenvalue; quality, min_dist: OpenCV's qualityLevel, minDistance."""
    return CornerParams(block_radius, min_eig, quality, min_dist, capacity, 0, (C.c_int32 * 2)(0, 0))


class DescribeParams(C.Structure):
    """pm_describe_params (include/pm.h, SPEC S71-S74); describe_params() fills it."""
    _fields_ = [("level", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


PM_DESCRIBE_UPRIGHT = 1


def describe_params(level=0, flags=0):
    """level: the pyramid level the points are described on; flags: 0 or PM_DESCRIBE_UPRIGHT."""
    return DescribeParams(level, flags, (C.c_int32 * 2)(0, 0))


class WarpParams(C.Structure):
    """pm_warp_params (include/pm.h, SPEC S75-S77); warp_params() fills it."""
    _fields_ = [("flags", C.c_int32), ("border_value", C.c_int32), ("reserved", C.c_int32 * 2)]


class WarpInfo(C.Structure):
    """pm_warp_info: status 0 ok, 1 singular or non-finite model, 2 the zero model; n_valid = valid output pixels."""
    _fields_ = [("status", C.c_int32), ("n_valid", C.c_int32)]


PM_WARP_INVERT, PM_WARP_REPLICATE, PM_WARP_AFFINE = 1, 2, 4


def warp_params(flags=0, border_value=0):
    """flags: PM_WARP_INVERT | PM_WARP_REPLICATE | PM_WARP_AFFINE; border_value: 0 .. 255."""
    return WarpParams(flags, border_value, (C.c_int32 * 2)(0, 0))


class Camera(C.Structure):
    """pm_camera: one pinhole camera shared by both views (fx, fy, cx, cy; no distortion: see Lens and undistort_points)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


def _camera(K):
    """A Camera from a Camera, (fx, fy, cx, cy) or a 3 x 3 intrinsic matrix."""
    if isinstance(K, Camera):
        return K
    k = np.asarray(K, np.float64)
    if k.shape == (3, 3):
        return Camera(k[0, 0], k[1, 1], k[0, 2], k[1, 2])
    return Camera(*[float(v) for v in k.reshape(4)])


class Lens(C.Structure):
    """pm_lens: OpenCV's first five distortion coefficients in distCoeffs order (SPEC S79); lens() fills it."""
    _fields_ = [("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double)]


def lens(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """k1, k2, k3 radial, p1, p2 tangential."""
    return Lens(float(k1), float(k2), float(p1), float(p2), float(k3))


def _lens(d):
    """A Lens from a Lens, up to five coefficients (k1, k2, p1, p2, k3), or None (no distortion: NULL)."""
    if d is None or isinstance(d, Lens):
        return d
    return lens(*[float(v) for v in np.asarray(d, np.float64).reshape(-1)])


def _lens_model(K, dist, R, K_new):
    """The four model arguments of the S79-S83 calls as ctypes values (None -> NULL); the tuple keeps them alive."""
    k, d = _camera(K), _lens(dist)
    n = None if K_new is None else _camera(K_new)
    r = None
    if R is not None:
        r = np.ascontiguousarray(R, np.float64).reshape(-1)
        if r.size != 9:
            raise ValueError("R must hold 9 doubles")
    return C.byref(k), (C.byref(d) if d is not None else None), _p(r), (C.byref(n) if n is not None else None), (k, d, r, n)


class StereoParams(C.Structure):
    """pm_stereo_params (include/pm.h, SPEC S85); stereo_params() fills it."""
    _fields_ = [("min_disp", C.c_int32), ("num_disp", C.c_int32), ("radius", C.c_int32), ("uniqueness", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class StereoInfo(C.Structure):
    """pm_stereo_info: status always 0; n_valid = pixels of the map that are not PM_STEREO_INVALID."""
    _fields_ = [("status", C.c_int32), ("n_valid", C.c_int32)]


PM_STEREO_INVALID = -32768
PM_STEREO_FROM_RIGHT = 1


def stereo_params(num_disp=64, radius=4, min_disp=0, uniqueness=0, flags=0):
    """Disparities min_disp .. min_disp + num_disp - 1, window (2 radius + 1)^2, uniqueness in per cent (0 rejects nothing),
    flags: 0 or PM_STEREO_FROM_RIGHT."""
    return StereoParams(min_disp, num_disp, radius, uniqueness, flags, (C.c_int32 * 3)(0, 0, 0))


class SgmParams(C.Structure):
    """pm_sgm_params (include/pm.h, SPEC S89-S92); sgm_params() fills it."""
    _fields_ = [("min_disp", C.c_int32), ("num_disp", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("paths", C.c_int32),
                ("uniqueness", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


def sgm_params(num_disp=64, p1=4, p2=24, paths=8, min_disp=0, uniqueness=0, flags=0):
    """Disparities min_disp .. min_disp + num_disp - 1, penalties 0 <= p1 <= p2 <= 1023 on the 0..62 census cost, paths 4 or 8,
    uniqueness in per cent (0 rejects nothing), flags: 0 or PM_STEREO_FROM_RIGHT."""
    return SgmParams(min_disp, num_disp, p1, p2, paths, uniqueness, flags, 0)


def stereo_rectify(R, t):
    """Host only (SPEC S84): the pose x2 ~ R x1 + t -> (rc, R1 (3, 3), R2 (3, 3), baseline, left_is_view2); rc is PM_OK,
    PM_E_NO_MODEL or PM_E_UNSUPPORTED (outputs zero), anything else raises PmError."""
    R = np.ascontiguousarray(R, np.float64).reshape(-1)
    t = np.ascontiguousarray(t, np.float64).reshape(-1)
    if R.size != 9 or t.size != 3:
        raise ValueError("R must hold 9 doubles and t 3")
    R1, R2, b, flag = np.zeros(9), np.zeros(9), C.c_double(0.0), C.c_int(0)
    rc = lib().pm_stereo_rectify(_p(R), _p(t), _p(R1), _p(R2), C.byref(b), C.byref(flag))
    if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_UNSUPPORTED):
        _check(rc)
    return rc, R1.reshape(3, 3), R2.reshape(3, 3), b.value, flag.value


class PnpView(C.Structure):
    """pm_pnp_view: world points (cap x 3) and pixels (cap x 2) on the device with an optional device-side count."""
    _fields_ = [("xyz", C.c_void_p), ("uv", C.c_void_p), ("count", C.c_void_p), ("cap", C.c_int32), ("reserved", C.c_int32)]


PM_ALIGN3D_RIGID, PM_ALIGN3D_SIMILARITY = 0, 1


class XyzView(C.Structure):
    """pm_xyz_view: rows of two frames (cap x 3 each) on the device with an optional device-side count."""
    _fields_ = [("xyz1", C.c_void_p), ("xyz2", C.c_void_p), ("count", C.c_void_p), ("cap", C.c_int32), ("reserved", C.c_int32)]


PM_TRI_MAX_VIEWS = 8
PM_TRI_USE_INITIAL = 1
PM_TRI_OK, PM_TRI_FEW_VIEWS, PM_TRI_DEGENERATE, PM_TRI_DEPTH, PM_TRI_PARALLAX, PM_TRI_REPROJ = 0, 1, 2, 3, 4, 5


class TriViews(C.Structure):
    """pm_tri_views: per view a device array of cap x 2 pixels and a device pose of 12 doubles (NULL: [I|0]), with an
    optional device-side count; tri_views() fills it."""
    _fields_ = [("uv", C.c_void_p * PM_TRI_MAX_VIEWS), ("Rt", C.c_void_p * PM_TRI_MAX_VIEWS), ("count", C.c_void_p),
                ("n_views", C.c_int32), ("cap", C.c_int32)]


class TriParams(C.Structure):
    """pm_tri_params (include/pm.h, SPEC S93-S96); tri_params() fills it."""
    _fields_ = [("max_reproj_px", C.c_double), ("max_cos_parallax", C.c_double), ("max_depth", C.c_double),
                ("max_iters", C.c_int32), ("flags", C.c_int32)]


def tri_params(max_reproj_px=3.0, max_cos_parallax=0.9998, max_depth=float("inf"), max_iters=10, flags=0):
    """max_cos_parallax 1 switches the parallax test off; max_iters 0 keeps the linear solution; flags: 0 or
    PM_TRI_USE_INITIAL."""
    return TriParams(max_reproj_px, max_cos_parallax, max_depth, max_iters, flags)


def tri_views(uv_ptrs, Rt_ptrs, cap, count_ptr=None):
    """A TriViews from device pointers: uv_ptrs[v] the pixels of view v, Rt_ptrs[v] its pose (None or 0: [I|0])."""
    if len(uv_ptrs) != len(Rt_ptrs) or len(uv_ptrs) > PM_TRI_MAX_VIEWS:
        raise ValueError("one pose per view, at most %d views" % PM_TRI_MAX_VIEWS)
    v = TriViews()
    for i, (u, r) in enumerate(zip(uv_ptrs, Rt_ptrs)):
        v.uv[i] = u or None
        v.Rt[i] = r or None
    v.count, v.n_views, v.cap = count_ptr or None, len(uv_ptrs), cap
    return v


PM_BA_MAX_POINTS = 65536


class BaParams(C.Structure):
    """pm_ba_params (include/pm.h, SPEC S113-S117); ba_params() fills it."""
    _fields_ = [("gate_px", C.c_double), ("max_iters", C.c_int32), ("fixed_mask", C.c_uint32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class BaInfo(C.Structure):
    """pm_ba_info (include/pm.h): costs in px^2 over the used observations, counts, status 0/1/2."""
    _fields_ = [("cost_in", C.c_double), ("cost_out", C.c_double), ("n_points", C.c_int32), ("n_obs", C.c_int32),
                ("iters", C.c_int32), ("accepted", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


BA_INFO_DTYPE = np.dtype([("cost_in", "<f8"), ("cost_out", "<f8"), ("n_points", "<i4"), ("n_obs", "<i4"), ("iters", "<i4"),
                          ("accepted", "<i4"), ("status", "<i4"), ("reserved", "<i4")])   # the same record, 40 bytes


def ba_params(fixed_mask=1, max_iters=10, gate_px=0.0, flags=0):
    """fixed_mask: bit v holds pose v (at least one held, one free); max_iters 0 only evaluates; gate_px 0 keeps every
    observation."""
    return BaParams(gate_px, max_iters, fixed_mask, flags, 0)


def bundle_adjust_workspace(n_views, cap):
    """Bytes of device workspace for bundle_adjust_dev; 0 for bad arguments.  Needs no GPU."""
    return int(lib().pm_bundle_adjust_workspace(n_views, cap))


PM_PGO_RIGID, PM_PGO_SIM3 = 0, 1
PM_PGO_MAX_NODES, PM_PGO_MAX_EDGES = 16384, 131072


class PgoParams(C.Structure):
    """pm_pgo_params (include/pm.h, SPEC S118-S123); pgo_params() fills it."""
    _fields_ = [("model", C.c_int32), ("max_iters", C.c_int32), ("cg_iters", C.c_int32), ("flags", C.c_int32),
                ("cg_tol", C.c_double), ("reserved", C.c_int32), ("reserved2", C.c_int32)]


class PgoInfo(C.Structure):
    """pm_pgo_info (include/pm.h): costs over the used edges, counts, status 0/1/2."""
    _fields_ = [("cost_in", C.c_double), ("cost_out", C.c_double), ("n_edges_used", C.c_int32), ("n_nodes_free", C.c_int32),
                ("iters", C.c_int32), ("accepted", C.c_int32), ("cg_total", C.c_int32), ("status", C.c_int32)]


PGO_INFO_DTYPE = np.dtype([("cost_in", "<f8"), ("cost_out", "<f8"), ("n_edges_used", "<i4"), ("n_nodes_free", "<i4"),
                           ("iters", "<i4"), ("accepted", "<i4"), ("cg_total", "<i4"), ("status", "<i4")])   # the same record, 40 bytes


def pgo_params(model=PM_PGO_SIM3, max_iters=10, cg_iters=50, cg_tol=1e-6, flags=0):
    """model: PM_PGO_SIM3 (7 parameters per node) or PM_PGO_RIGID (6, scales untouched); max_iters 0 only evaluates; cg_iters
    bounds the conjugate-gradient iterations of one step, cg_tol its relative stop (0: run them all)."""
    return PgoParams(model, max_iters, cg_iters, flags, cg_tol, 0, 0)


def pose_graph_workspace(n_nodes, n_edges, model=PM_PGO_SIM3):
    """Bytes of device workspace for pose_graph_optimize_dev; 0 for bad arguments.  Needs no GPU."""
    return int(lib().pm_pose_graph_workspace(n_nodes, n_edges, model))


class HRefineInfo(C.Structure):
    """pm_h_refine_info (include/pm.h): costs in px^2, inliers used, LM iterations, status 0/1/2."""
    _fields_ = [("cost_in", C.c_double), ("cost_out", C.c_double), ("n_used", C.c_int32), ("iters", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


H_REFINE_INFO_DTYPE = np.dtype([("cost_in", "<f8"), ("cost_out", "<f8"), ("n_used", "<i4"), ("iters", "<i4"),
                                ("status", "<i4"), ("reserved", "<i4")])   # the same record, 32 bytes

RANSAC_RECORD_DTYPE = np.dtype([("key", "<u8"), ("F", "<f8", (9,))])       # pm_ransac_record, 80 bytes
PM_MAX_PARTS = 64
PM_OPT_RANSAC_PATH, PM_OPT_SCORE_OPERANDS, PM_OPT_HAMMING_ROUTE, PM_OPT_KNN_F16_WAVES, PM_OPT_FILTER_FUSION = 1, 2, 3, 4, 5
PM_OPT_KNN_STAGING = 6
PM_OPT_KNN_WG_PER_CU = 7
PM_OPT_KNN_XCD_TILE = 8
PM_OPT_KNN_GENERAL_F16 = 9
PM_OPT_KNN_SEEDED = 10
PM_OPT_KNN_U8_GROUP = 11
PM_OPT_KNN_RING = 12
PM_OPT_KNN_U8_REFINE = 13
PM_OPT_KNN_RING_PROLOGUE = 14
PM_OPT_KNN_WIDE = 15
PM_OPT_KNN_PREP_ROWS = 16
PM_OPT_RANSAC_FORM = 17
PM_OPT_RANSAC_WG_IDS = 18
PM_OPT_HAMMING_REFINE = 19
PM_OPT_KNN_SUPERTILE = 20
PM_OPT_FEAT_CAPACITY = 21   # candidate capacity of pm_detect_describe[_dev]; 0 = max(65536, 8 * max_kp)


_lib = None


def lib():
    """Loads libpm_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PmError(PM_E_UNSUPPORTED,
                          "%s is missing: run `python -m points_matching_amd.build`" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 and cannot
        # initialise after another copy (the /opt/rocm one libpm_hip.so would pull in) has taken
        # the device.  Importing torch first makes libpm_hip.so bind to torch's runtime, which is
        # also what lets bench.py share torch streams/tensors with the library.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.pm_last_error.restype = C.c_char_p
        _lib.pm_status_string.restype = C.c_char_p
        _lib.pm_format_match_list.restype = C.c_long
        _lib.pm_bundle_adjust_workspace.restype = C.c_size_t
        _lib.pm_pose_graph_workspace.restype = C.c_size_t
    return _lib


def _check(rc):
    if rc != PM_OK:
        raise PmError(rc, (lib().pm_last_error() or b"").decode() or
                      lib().pm_status_string(rc).decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _pair(xy1, xy2):
    """Correspondences as contiguous float32 (n, 2) arrays, and n; raises ValueError unless both have n rows."""
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    if xy2.shape[0] != xy1.shape[0]:
        raise ValueError("xy1 and xy2 must have the same length")
    return xy1, xy2, xy1.shape[0]


def _outcome(rc):
    """rc when it is a data outcome (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW); raises PmError on anything else."""
    if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
        _check(rc)
    return rc


def ransac_key(inliers, hyp):
    return (int(inliers) << 32) | (0xFFFFFFFF - int(hyp))


def ransac_key_hyp(key):
    return 0xFFFFFFFF - (int(key) & 0xFFFFFFFF)


def ransac_key_inliers(key):
    return int(key) >> 32


# ---- host-side stages (no GPU needed) ---------------------------------------------------------

def filter_midpoint(m):
    """main.cpp:49-69.  Returns (good, minMatch, maxMatch)."""
    m = np.ascontiguousarray(m, MATCH_DTYPE).reshape(-1)
    out = np.zeros(max(m.size, 1), MATCH_DTYPE)
    mn, mx, n = C.c_double(), C.c_double(), C.c_int()
    _check(lib().pm_filter_midpoint(_p(m), m.size, C.byref(mn), C.byref(mx), _p(out), C.byref(n)))
    return out[:n.value].copy(), mn.value, mx.value


def filter_ratio(knn, ratio):
    knn = np.ascontiguousarray(knn, MATCH_DTYPE)
    nq, k = knn.shape
    out = np.zeros(max(nq, 1), MATCH_DTYPE)
    n = C.c_int()
    _check(lib().pm_filter_ratio(_p(knn), nq, k, C.c_float(ratio), _p(out), C.byref(n)))
    return out[:n.value].copy()


def filter_cross(fwd, rev, cross_flags=0, ratio=0.8):
    """Cross-check (SPEC S41): fwd (nq, kf) records of the matcher on (q, t), rev (nt, kr) records on (t, q)."""
    fwd = np.ascontiguousarray(fwd, MATCH_DTYPE)
    rev = np.ascontiguousarray(rev, MATCH_DTYPE)
    nq, kf = fwd.shape
    nt, kr = rev.shape
    out = np.zeros(max(nq, 1), MATCH_DTYPE)
    n = C.c_int()
    _check(lib().pm_filter_cross(_p(fwd), nq, kf, _p(rev), nt, kr, cross_flags, C.c_float(ratio), _p(out), C.byref(n)))
    return out[:n.value].copy()


def pad_rows_u8(rows, dst_bytes):
    """pm_pad_rows_u8: (n, bytes) uint8 rows copied into rows of dst_bytes >= bytes bytes with a zeroed tail (AKAZE's 61
    bytes -> 64: every Hamming distance is unchanged)."""
    rows = np.ascontiguousarray(rows, np.uint8)
    assert rows.ndim == 2
    out = np.empty((rows.shape[0], int(dst_bytes)), np.uint8)
    _check(lib().pm_pad_rows_u8(_p(rows), rows.shape[0], rows.shape[1], _p(out), int(dst_bytes)))
    return out


def match_indices(m):
    m = np.ascontiguousarray(m, MATCH_DTYPE).reshape(-1)
    qi = np.zeros(m.size, np.int32)
    ti = np.zeros(m.size, np.int32)
    _check(lib().pm_match_indices(_p(m), m.size, _p(qi), _p(ti)))
    return qi, ti


def gather_points(kp_xy, idx):
    kp_xy = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    idx = np.ascontiguousarray(idx, np.int32)
    out = np.zeros((idx.size, 2), np.float32)
    _check(lib().pm_gather_points(_p(kp_xy), kp_xy.shape[0], _p(idx), idx.size, _p(out)))
    return out


def format_match_list(m):
    m = np.ascontiguousarray(m, MATCH_DTYPE).reshape(-1)
    need = lib().pm_format_match_list(_p(m), m.size, None, C.c_size_t(0))
    buf = C.create_string_buffer(need + 1)
    lib().pm_format_match_list(_p(m), m.size, buf, C.c_size_t(need + 1))
    return buf.value.decode()


def epipolar_residuals(xy1, xy2, F, transposed=1):
    xy1 = np.ascontiguousarray(xy1, np.float32)
    xy2 = np.ascontiguousarray(xy2, np.float32)
    F = np.ascontiguousarray(F, np.float64).reshape(9)
    n = xy1.shape[0]
    r = np.zeros(max(n, 1), np.float64)
    mean = C.c_double()
    _check(lib().pm_epipolar_residuals(_p(xy1), _p(xy2), n, _p(F), transposed, _p(r), C.byref(mean)))
    return r[:n], mean.value


def f_scale_f33(F):
    F = np.ascontiguousarray(F, np.float64).reshape(9).copy()
    _check(lib().pm_f_scale_f33(_p(F)))
    return F.reshape(3, 3)


def epilines(xy, which_image, F):
    xy = np.ascontiguousarray(xy, np.float32)
    F = np.ascontiguousarray(F, np.float64).reshape(9)
    lines = np.zeros((xy.shape[0], 3), np.float32)
    _check(lib().pm_epilines(_p(xy), xy.shape[0], which_image, _p(F), _p(lines)))
    return lines


def epiline_endpoints(lines, cols):
    lines = np.ascontiguousarray(lines, np.float32)
    out = np.zeros((lines.shape[0], 4), np.int32)
    _check(lib().pm_epiline_endpoints(_p(lines), lines.shape[0], cols, _p(out)))
    return out


def detect_tables():
    """pm_detect_tables: the host-computed tables of the feature front end (SPEC S53, S56); no GPU needed."""
    tap_r = np.zeros(6, np.int32)
    taps = np.zeros((6, 25), np.float64)
    ori_w = np.zeros((3, 393), np.float64)
    rad = np.zeros(3, np.int32)
    r2 = np.zeros(3, np.int32)
    cs = np.zeros((2, 36), np.float64)
    _check(lib().pm_detect_tables(_p(tap_r), _p(taps), _p(ori_w), _p(rad), _p(r2), _p(cs)))
    return {"tap_radius": tap_r, "taps": taps, "ori_weight": ori_w, "ori_radius": rad, "desc_radius": r2, "cos": cs[0], "sin": cs[1]}


def detect_bits_table():
    """pm_detect_bits_table: the 256 tests (256, 4) and their steered offsets (3, 36, 256, 4), int8 (SPEC S58, S59); no GPU needed."""
    base = np.zeros((256, 4), np.int8)
    steer = np.zeros((3, 36, 256, 4), np.int8)
    _check(lib().pm_detect_bits_table(_p(base), _p(steer)))
    return base, steer


def describe_points_tables():
    """pm_describe_points_tables: (cos_sin_q20 (72,) int32 = C[0..35] then S[0..35], steered (37, 256, 4) int8) of SPEC S72, S73;
    no GPU needed."""
    q20 = np.zeros(72, np.int32)
    steer = np.zeros((37, 256, 4), np.int8)
    _check(lib().pm_describe_points_tables(_p(q20), _p(steer)))
    return q20, steer


# ---- GPU context ------------------------------------------------------------------------------

class Context:
    """pm_ctx wrapper: one HIP device + stream + scratch arena."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().pm_ctx_create(device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_handle):
        _check(lib().pm_ctx_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    def synchronize(self):
        _check(lib().pm_ctx_synchronize(self._h))

    def timing_enable(self, on=True):
        _check(lib().pm_ctx_timing_enable(self._h, int(on)))

    def timing_reset(self):
        _check(lib().pm_ctx_timing_reset(self._h))

    def timing_get(self, name):
        ms, n = C.c_double(), C.c_int()
        _check(lib().pm_ctx_timing_get(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_option(self, option, value):
        _check(lib().pm_ctx_set_option(self._h, option, value))

    def get_option(self, option):
        v = C.c_int()
        _check(lib().pm_ctx_get_option(self._h, option, C.byref(v)))
        return v.value

    def scratch_info(self):
        """(capacity of the scratch arena in bytes, blocks retired because a recorded graph may hold them): reads the
        context only, no device call."""
        cap, retired = C.c_size_t(), C.c_int()
        _check(lib().pm_ctx_scratch_info(self._h, C.byref(cap), C.byref(retired)))
        return cap.value, retired.value

    def ransac_shard_parts_dev(self, view, hyp_begin, hyp_end, thresh_px, seed, drec_ptr, kind=PM_ERR_SAMPSON):
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_shard_parts_dev(self._h, C.byref(view), C.byref(prm), C.c_void_p(drec_ptr)))

    def ransac_finish_parts_dev(self, view, thresh_px, drecs_ptr, n_records, dkey_ptr, dF_ptr, dmask_ptr, mask_len,
                                dninl_ptr, dntotal_ptr=0, kind=PM_ERR_SAMPSON):
        prm = RansacParams(0, 0, 0, thresh_px, kind)
        _check(lib().pm_ransac_finish_parts_dev(self._h, C.byref(view), C.byref(prm), C.c_void_p(drecs_ptr), n_records,
                                                C.c_void_p(dkey_ptr or 0), C.c_void_p(dF_ptr or 0), C.c_void_p(dmask_ptr),
                                                mask_len, C.c_void_p(dninl_ptr or 0), C.c_void_p(dntotal_ptr or 0)))

    def knn_diag_enable(self, on=True):
        _check(lib().pm_ctx_knn_diag_enable(self._h, int(on)))

    def filter_fusion_gave_up(self):
        g = C.c_int()
        _check(lib().pm_ctx_filter_fusion_status(self._h, C.byref(g)))
        return g.value

    def knn_stats(self):
        r, nf = C.c_int(), C.c_int()
        _check(lib().pm_ctx_knn_stats(self._h, C.byref(r), C.byref(nf)))
        rt = C.c_int()
        _check(lib().pm_ctx_knn_route(self._h, C.byref(rt)))
        return {"rescans": r.value, "nonfinite": nf.value, "route": rt.value}

    def filter_ratio_gather_dev(self, dknn_ptr, nq, k, ratio, dkp1_ptr, dkp2_ptr, dgood_ptr, dxy1_ptr,
                                dxy2_ptr, dn_ptr):
        _check(lib().pm_filter_ratio_gather_dev(self._h, C.c_void_p(dknn_ptr), nq, k, C.c_float(ratio),
                                                C.c_void_p(dkp1_ptr), C.c_void_p(dkp2_ptr),
                                                C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr),
                                                C.c_void_p(dxy2_ptr), C.c_void_p(dn_ptr)))

    def filter_cross_gather_dev(self, dfwd_ptr, nq, kf, drev_ptr, nt, kr, cross_flags, ratio, dkp1_ptr, dkp2_ptr, dgood_ptr,
                                dxy1_ptr, dxy2_ptr, dn_ptr):
        _check(lib().pm_filter_cross_gather_dev(self._h, C.c_void_p(dfwd_ptr), nq, kf, C.c_void_p(drev_ptr), nt, kr,
                                                cross_flags, C.c_float(ratio), C.c_void_p(dkp1_ptr or 0),
                                                C.c_void_p(dkp2_ptr or 0), C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr or 0),
                                                C.c_void_p(dxy2_ptr or 0), C.c_void_p(dn_ptr)))

    # -- one-call cross-check matching (SPEC S42): forward pass, reverse pass, fused filter + gather ----------------
    def bf_match_cross_l2_dev(self, dq_ptr, nq, dt_ptr, nt, dim, knn_flags, cross_flags, ratio, dkp1_ptr, dkp2_ptr, dfwd_ptr,
                              drev_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        _check(lib().pm_bf_match_cross_l2_f32_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt, dim, knn_flags,
                                                  cross_flags, C.c_float(ratio), C.c_void_p(dkp1_ptr or 0),
                                                  C.c_void_p(dkp2_ptr or 0), C.c_void_p(dfwd_ptr), C.c_void_p(drev_ptr),
                                                  C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr or 0), C.c_void_p(dxy2_ptr or 0),
                                                  C.c_void_p(dn_ptr)))

    def bf_match_cross_l2_u8_dev(self, dq_ptr, nq, dt_ptr, nt, dim, cross_flags, ratio, dkp1_ptr, dkp2_ptr, dfwd_ptr, drev_ptr,
                                 dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        _check(lib().pm_bf_match_cross_l2_u8_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt, dim, cross_flags,
                                                 C.c_float(ratio), C.c_void_p(dkp1_ptr or 0), C.c_void_p(dkp2_ptr or 0),
                                                 C.c_void_p(dfwd_ptr), C.c_void_p(drev_ptr), C.c_void_p(dgood_ptr),
                                                 C.c_void_p(dxy1_ptr or 0), C.c_void_p(dxy2_ptr or 0), C.c_void_p(dn_ptr)))

    def bf_match_cross_hamming_dev(self, dq_ptr, nq, dt_ptr, nt, nbytes, cross_flags, ratio, dkp1_ptr, dkp2_ptr, dfwd_ptr,
                                   drev_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        _check(lib().pm_bf_match_cross_hamming_u8_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt, nbytes,
                                                      cross_flags, C.c_float(ratio), C.c_void_p(dkp1_ptr or 0),
                                                      C.c_void_p(dkp2_ptr or 0), C.c_void_p(dfwd_ptr), C.c_void_p(drev_ptr),
                                                      C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr or 0),
                                                      C.c_void_p(dxy2_ptr or 0), C.c_void_p(dn_ptr)))

    def _match_cross_host(self, fn, q, t, dtype, *mid):
        q = np.ascontiguousarray(q, dtype)
        t = np.ascontiguousarray(t, dtype)
        assert q.ndim == 2 and t.ndim == 2 and t.shape[1] == q.shape[1]
        out = np.zeros(max(q.shape[0], 1), MATCH_DTYPE)
        n = C.c_int()
        _check(fn(self._h, _p(q), q.shape[0], _p(t), t.shape[0], q.shape[1], *mid, _p(out), C.byref(n)))
        return out[:n.value].copy()

    def bf_match_cross_l2(self, q, t, cross_flags=0, ratio=0.8, knn_flags=0):
        """Mutual nearest neighbours of float rows (pm_bf_match_cross_l2_f32): the survivors, in query order."""
        return self._match_cross_host(lib().pm_bf_match_cross_l2_f32, q, t, np.float32, knn_flags, cross_flags, C.c_float(ratio))

    def bf_match_cross_l2_u8(self, q, t, cross_flags=0, ratio=0.8):
        return self._match_cross_host(lib().pm_bf_match_cross_l2_u8, q, t, np.uint8, cross_flags, C.c_float(ratio))

    def bf_match_cross_hamming(self, q, t, cross_flags=0, ratio=0.8):
        return self._match_cross_host(lib().pm_bf_match_cross_hamming_u8, q, t, np.uint8, cross_flags, C.c_float(ratio))

    # -- guided matching (SPEC S48-S50): k-NN among the train keypoints a two-view model admits ---------------------
    def _knn_guided_dev(self, fn, dq_ptr, nq, dt_ptr, nt, width, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, k, dout_ptr, dnadm_ptr):
        _check(fn(self._h, C.c_void_p(dq_ptr or 0), nq, C.c_void_p(dt_ptr or 0), nt, width, C.c_void_p(dkp1_ptr or 0),
                  C.c_void_p(dkp2_ptr or 0), kind, C.c_void_p(dM_ptr or 0), C.c_float(tau), k, C.c_void_p(dout_ptr or 0),
                  C.c_void_p(dnadm_ptr or 0)))

    def bf_knn_guided_l2_dev(self, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, k, dout_ptr,
                             dnadm_ptr=0):
        """dM_ptr: DEVICE pointer to 9 doubles (the d_F / d_H of the device estimators); dnadm_ptr may be 0."""
        self._knn_guided_dev(lib().pm_bf_knn_guided_l2_f32_dev, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind, dM_ptr,
                             tau, k, dout_ptr, dnadm_ptr)

    def bf_knn_guided_l2_u8_dev(self, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, k, dout_ptr,
                                dnadm_ptr=0):
        self._knn_guided_dev(lib().pm_bf_knn_guided_l2_u8_dev, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind, dM_ptr,
                             tau, k, dout_ptr, dnadm_ptr)

    def bf_knn_guided_hamming_dev(self, dq_ptr, nq, dt_ptr, nt, nbytes, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, k, dout_ptr,
                                  dnadm_ptr=0):
        self._knn_guided_dev(lib().pm_bf_knn_guided_hamming_u8_dev, dq_ptr, nq, dt_ptr, nt, nbytes, dkp1_ptr, dkp2_ptr, kind,
                             dM_ptr, tau, k, dout_ptr, dnadm_ptr)

    def _match_guided_dev(self, fn, dq_ptr, nq, dt_ptr, nt, width, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, ratio, dknn_ptr,
                          dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        _check(fn(self._h, C.c_void_p(dq_ptr or 0), nq, C.c_void_p(dt_ptr or 0), nt, width, C.c_void_p(dkp1_ptr or 0),
                  C.c_void_p(dkp2_ptr or 0), kind, C.c_void_p(dM_ptr or 0), C.c_float(tau), C.c_float(ratio),
                  C.c_void_p(dknn_ptr or 0), C.c_void_p(dgood_ptr or 0), C.c_void_p(dxy1_ptr or 0), C.c_void_p(dxy2_ptr or 0),
                  C.c_void_p(dn_ptr or 0)))

    def bf_match_guided_l2_dev(self, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, ratio, dknn_ptr,
                               dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        """One-call guided matching (S50): guided 2-NN into dknn_ptr, ratio filter, compaction, gather."""
        self._match_guided_dev(lib().pm_bf_match_guided_l2_f32_dev, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind,
                               dM_ptr, tau, ratio, dknn_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr)

    def bf_match_guided_l2_u8_dev(self, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, ratio, dknn_ptr,
                                  dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        self._match_guided_dev(lib().pm_bf_match_guided_l2_u8_dev, dq_ptr, nq, dt_ptr, nt, dim, dkp1_ptr, dkp2_ptr, kind,
                               dM_ptr, tau, ratio, dknn_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr)

    def bf_match_guided_hamming_dev(self, dq_ptr, nq, dt_ptr, nt, nbytes, dkp1_ptr, dkp2_ptr, kind, dM_ptr, tau, ratio,
                                    dknn_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr):
        self._match_guided_dev(lib().pm_bf_match_guided_hamming_u8_dev, dq_ptr, nq, dt_ptr, nt, nbytes, dkp1_ptr, dkp2_ptr,
                               kind, dM_ptr, tau, ratio, dknn_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr)

    def _knn_guided_host(self, fn, q, t, dtype, kp1, kp2, kind, M, tau, k):
        q = np.ascontiguousarray(q, dtype)
        t = np.ascontiguousarray(t, dtype).reshape(-1, q.shape[1])
        kp1 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        kp2 = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        if kp1.shape[0] != q.shape[0] or kp2.shape[0] != t.shape[0]:
            raise ValueError("one keypoint per descriptor row")
        M = np.ascontiguousarray(M, np.float64).reshape(9)
        out = np.zeros((q.shape[0], max(k, 1)), MATCH_DTYPE)
        adm = np.zeros(max(q.shape[0], 1), np.int32)
        _check(fn(self._h, _p(q), q.shape[0], _p(t), t.shape[0], q.shape[1], _p(kp1), _p(kp2), kind, _p(M), C.c_float(tau), k,
                  _p(out), _p(adm)))
        return out, adm[:q.shape[0]]

    def bf_knn_guided_l2(self, q, t, kp1, kp2, kind, M, tau, k):
        """Guided k-NN of float rows, host arrays (pm_bf_knn_guided_l2_f32): (records nq x k, n_admitted)."""
        return self._knn_guided_host(lib().pm_bf_knn_guided_l2_f32, q, t, np.float32, kp1, kp2, kind, M, tau, k)

    def bf_knn_guided_l2_u8(self, q, t, kp1, kp2, kind, M, tau, k):
        return self._knn_guided_host(lib().pm_bf_knn_guided_l2_u8, q, t, np.uint8, kp1, kp2, kind, M, tau, k)

    def bf_knn_guided_hamming(self, q, t, kp1, kp2, kind, M, tau, k):
        return self._knn_guided_host(lib().pm_bf_knn_guided_hamming_u8, q, t, np.uint8, kp1, kp2, kind, M, tau, k)

    def filter_midpoint_gather_dev(self, dm_ptr, n, k, dkp1_ptr, dkp2_ptr, dgood_ptr, dxy1_ptr, dxy2_ptr, dn_ptr,
                                   dminmax_ptr=0):
        _check(lib().pm_filter_midpoint_gather_dev(self._h, C.c_void_p(dm_ptr), n, k, C.c_void_p(dkp1_ptr),
                                                   C.c_void_p(dkp2_ptr), C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr),
                                                   C.c_void_p(dxy2_ptr), C.c_void_p(dn_ptr),
                                                   C.c_void_p(dminmax_ptr or 0)))

    def concat_points_dev(self, dxy1_parts, dxy2_parts, dcounts, parts, stride, dxy1, dxy2, dn_total):
        _check(lib().pm_concat_points_dev(self._h, C.c_void_p(dxy1_parts), C.c_void_p(dxy2_parts),
                                          C.c_void_p(dcounts), parts, stride, C.c_void_p(dxy1),
                                          C.c_void_p(dxy2), C.c_void_p(dn_total)))

    def ransac_score_devn(self, dxy1_ptr, dxy2_ptr, n_max, dn_ptr, hyp_begin, hyp_end, thresh_px, seed,
                          dkey_ptr, kind=PM_ERR_SAMPSON):
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_score_devn(self._h, C.c_void_p(dxy1_ptr), C.c_void_p(dxy2_ptr), n_max,
                                          C.c_void_p(dn_ptr), C.byref(prm), C.c_void_p(dkey_ptr)))

    def ransac_run_dev(self, dxy1_ptr, dxy2_ptr, n_max, dn_ptr, hyp_begin, hyp_end, thresh_px, seed, dkey_ptr,
                       dF_ptr, dmask_ptr, dninl_ptr, kind=PM_ERR_SAMPSON):
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_run_dev(self._h, C.c_void_p(dxy1_ptr), C.c_void_p(dxy2_ptr), n_max,
                                       C.c_void_p(dn_ptr or 0), C.byref(prm), C.c_void_p(dkey_ptr),
                                       C.c_void_p(dF_ptr), C.c_void_p(dmask_ptr), C.c_void_p(dninl_ptr)))

    def ransac_model_from_key_dev(self, dxy1_ptr, dxy2_ptr, n_max, dn_ptr, thresh_px, seed, dkey_ptr, dF_ptr,
                                  dmask_ptr, dninl_ptr, kind=PM_ERR_SAMPSON):
        prm = RansacParams(0, 0, seed, thresh_px, kind)
        _check(lib().pm_ransac_model_from_key_dev(self._h, C.c_void_p(dxy1_ptr), C.c_void_p(dxy2_ptr), n_max,
                                                  C.c_void_p(dn_ptr or 0), C.byref(prm), C.c_void_p(dkey_ptr),
                                                  C.c_void_p(dF_ptr), C.c_void_p(dmask_ptr),
                                                  C.c_void_p(dninl_ptr)))

    # -- feature front end (main.cpp:22-26, :36-40; SPEC S53-S57) -----------------------------------------------------
    def detect_describe_dev(self, dimg_ptr, w, h, stride, max_kp, dkp_ptr, ddesc_u8_ptr, ddesc_f32_ptr, dmeta_ptr, dn_ptr,
                            contrast=0.03, edge_r=10.0):
        """Device pointers; outputs sized for max_kp rows; ddesc_u8_ptr / ddesc_f32_ptr / dmeta_ptr may be 0.  *dn = -1: the
        candidate buffer overflowed (PM_OPT_FEAT_CAPACITY) and no row was written."""
        _check(lib().pm_detect_describe_dev(self._h, C.c_void_p(dimg_ptr), w, h, stride, max_kp, C.c_float(contrast),
                                            C.c_float(edge_r), C.c_void_p(dkp_ptr), C.c_void_p(ddesc_u8_ptr or 0),
                                            C.c_void_p(ddesc_f32_ptr or 0), C.c_void_p(dmeta_ptr or 0), C.c_void_p(dn_ptr)))

    def detect_describe(self, img, max_kp=4000, contrast=0.03, edge_r=10.0):
        """8-bit grey image (h, w) -> (kp_xy (n, 2) f32, desc_u8 (n, 128), desc_f32 (n, 128), meta (n, 4)); blocking."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        kp = np.zeros((max_kp, 2), np.float32)
        du8 = np.zeros((max_kp, 128), np.uint8)
        df = np.zeros((max_kp, 128), np.float32)
        meta = np.zeros((max_kp, 4), np.float32)
        n = C.c_int32()
        _check(lib().pm_detect_describe(self._h, _p(img), w, h, w, max_kp, C.c_float(contrast), C.c_float(edge_r), _p(kp),
                                        _p(du8), _p(df), _p(meta), C.byref(n)))
        return kp[:n.value].copy(), du8[:n.value].copy(), df[:n.value].copy(), meta[:n.value].copy()

    def detect_describe_bits_dev(self, dimg_ptr, w, h, stride, max_kp, dkp_ptr, ddesc_bits_ptr, dmeta_ptr, dn_ptr, contrast=0.03,
                                 edge_r=10.0):
        """The binary form (SPEC S58-S60): ddesc_bits_ptr holds max_kp x 32 bytes; dmeta_ptr may be 0; *dn as above."""
        _check(lib().pm_detect_describe_bits_dev(self._h, C.c_void_p(dimg_ptr), w, h, stride, max_kp, C.c_float(contrast),
                                                 C.c_float(edge_r), C.c_void_p(dkp_ptr), C.c_void_p(ddesc_bits_ptr),
                                                 C.c_void_p(dmeta_ptr or 0), C.c_void_p(dn_ptr)))

    def detect_describe_bits(self, img, max_kp=4000, contrast=0.03, edge_r=10.0):
        """8-bit grey image (h, w) -> (kp_xy (n, 2) f32, desc_bits (n, 32) u8, meta (n, 4)); blocking."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        kp = np.zeros((max_kp, 2), np.float32)
        bits = np.zeros((max_kp, 32), np.uint8)
        meta = np.zeros((max_kp, 4), np.float32)
        n = C.c_int32()
        _check(lib().pm_detect_describe_bits(self._h, _p(img), w, h, w, max_kp, C.c_float(contrast), C.c_float(edge_r), _p(kp),
                                             _p(bits), _p(meta), C.byref(n)))
        return kp[:n.value].copy(), bits[:n.value].copy(), meta[:n.value].copy()

    def detect_level(self, octave, level):
        """Gaussian level of the last detect call on this context (pm_detect_level_get), as an (h, w) float32 array."""
        w, h = C.c_int(), C.c_int()
        _check(lib().pm_detect_level_get(self._h, octave, level, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        _check(lib().pm_detect_level_get(self._h, octave, level, _p(out), out.size, C.byref(w), C.byref(h)))
        return out

    # -- sparse optical-flow tracking (cv::calcOpticalFlowPyrLK; SPEC S61-S66) ------------------------------------------
    def pyramid(self, w, h, max_level=3):
        """A device image pyramid (pm_pyramid) for w x h frames; build it with Pyramid.build_dev."""
        return Pyramid(self, w, h, max_level)

    def track_lk_dev(self, prev, next_, dpts_ptr, dn_ptr, cap, prm, dout_ptr, dstatus_ptr, derr_ptr=None, dfb_ptr=None, dinit_ptr=None):
        """Device pointers; prev / next_: built Pyramids; dn_ptr (device int32 count) may be None = cap; prm: LkParams."""
        _check(lib().pm_track_lk_dev(self._h, prev._h, next_._h, C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap,
                                     C.c_void_p(dinit_ptr or 0), C.byref(prm), C.c_void_p(dout_ptr), C.c_void_p(dstatus_ptr),
                                     C.c_void_p(derr_ptr or 0), C.c_void_p(dfb_ptr or 0)))

    def track_lk_gather_dev(self, prev, next_, dpts_ptr, dn_ptr, cap, prm, dxy1_ptr, dxy2_ptr, dcount_ptr, dsrc_ptr=None, dout_ptr=None,
                            dstatus_ptr=None, dinit_ptr=None):
        """Track and keep the status-1 points in input order: {dxy1, dxy2, dcount, parts 1, cap} is a PointsView."""
        _check(lib().pm_track_lk_gather_dev(self._h, prev._h, next_._h, C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap,
                                            C.c_void_p(dinit_ptr or 0), C.byref(prm), C.c_void_p(dxy1_ptr), C.c_void_p(dxy2_ptr),
                                            C.c_void_p(dsrc_ptr or 0), C.c_void_p(dcount_ptr), C.c_void_p(dout_ptr or 0),
                                            C.c_void_p(dstatus_ptr or 0)))

    def track_lk(self, img1, img2, pts, prm=None, init=None):
        """Host form: two 8-bit grey frames (h, w), points (n, 2) -> (out (n, 2) f32, status (n,) u8, err (n,), fb (n,))."""
        img1 = np.ascontiguousarray(img1, np.uint8)
        img2 = np.ascontiguousarray(img2, np.uint8)
        if img1.shape != img2.shape or img1.ndim != 2:
            raise ValueError("img1 and img2 must be 2-D arrays of one shape")
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        if init is not None:
            init = np.ascontiguousarray(init, np.float32).reshape(-1, 2)
            if init.shape[0] != n:
                raise ValueError("pts and init must have the same length")
        prm = prm or lk_params()
        h, w = img1.shape
        out, status = np.zeros((max(n, 1), 2), np.float32), np.zeros(max(n, 1), np.uint8)
        err, fb = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        _check(lib().pm_track_lk(self._h, _p(img1), _p(img2), w, h, w, _p(pts), n, _p(init), C.byref(prm), _p(out), _p(status),
                                 _p(err), _p(fb)))
        return out[:n], status[:n], err[:n], fb[:n]

    # -- corners to start and replenish tracks (cv::goodFeaturesToTrack with a mask; SPEC S67-S70) -------------------------
    def corners_dev(self, pyr, prm, max_corners, dxy_ptr, dn_ptr, dscore_ptr=None, dkeep_ptr=None, dn_keep_ptr=None, cap_keep=0):
        """Device pointers; pyr: a built Pyramid (level 0 is read); prm: CornerParams.  dkeep_ptr: cap_keep x 2 float obstacles,
        dn_keep_ptr their device int32 count (None = cap_keep).  *dn = the number of rows written, -1 on overflow."""
        _check(lib().pm_corners_dev(self._h, pyr._h, C.byref(prm), C.c_void_p(dkeep_ptr or 0), C.c_void_p(dn_keep_ptr or 0), cap_keep,
                                    max_corners, C.c_void_p(dxy_ptr), C.c_void_p(dscore_ptr or 0), C.c_void_p(dn_ptr)))

    def corners_replenish_dev(self, pyr, prm, dpts_ptr, dcount_ptr, cap, target, dscore_ptr=None, dn_new_ptr=None):
        """In place: rows [0, *dcount) of dpts are the obstacles; corners are appended until min(target, cap) rows."""
        _check(lib().pm_corners_replenish_dev(self._h, pyr._h, C.byref(prm), C.c_void_p(dpts_ptr), C.c_void_p(dcount_ptr), cap, target,
                                              C.c_void_p(dscore_ptr or 0), C.c_void_p(dn_new_ptr or 0)))

    def corners(self, img, max_corners=1000, prm=None, keep=None, w=None):
        """Host form: 8-bit grey image (h, w), keep points (n, 2) -> (xy (m, 2) f32, score (m,) f32).  With w given, img holds
        h rows of img.shape[1] >= w bytes (a row stride) and only the first w columns are the image."""
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim != 2:
            raise ValueError("img must be a 2-D array")
        h = img.shape[0]
        w = img.shape[1] if w is None else w
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.float32).reshape(-1, 2)
        n_keep = 0 if keep is None else keep.shape[0]
        prm = prm or corner_params()
        rows = max(max_corners, 1)
        xy, score, n = np.zeros((rows, 2), np.float32), np.zeros(rows, np.float32), C.c_int32()
        _check(lib().pm_corners(self._h, _p(img), w, h, img.shape[1], C.byref(prm), _p(keep) if n_keep else None, n_keep, max_corners,
                                _p(xy), _p(score), C.byref(n)))
        return xy[:n.value].copy(), score[:n.value].copy()

    # -- describe given points: oriented 256-bit descriptors on a pyramid level (SPEC S71-S74) -----------------------------
    def describe_points_dev(self, pyr, dpts_ptr, dn_ptr, cap, prm, ddesc_ptr, dvalid_ptr=None, dbin_ptr=None):
        """Device pointers; pyr: a built Pyramid; dn_ptr (device int32 count) may be None = cap; prm: DescribeParams.  Writes
        rows [0, n) of ddesc (cap x 32 bytes), dvalid and dbin (cap bytes each, either may be None)."""
        _check(lib().pm_describe_points_dev(self._h, pyr._h, C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap, C.byref(prm),
                                            C.c_void_p(ddesc_ptr), C.c_void_p(dvalid_ptr or 0), C.c_void_p(dbin_ptr or 0)))

    def describe_points_gather_dev(self, pyr, dpts_ptr, dn_ptr, cap, prm, dxy_ptr, ddesc_ptr, dcount_ptr, dsrc_ptr=None):
        """Describe and keep the valid rows in input order: dxy (cap x 2), ddesc (cap x 32) and *dcount feed the Hamming matchers."""
        _check(lib().pm_describe_points_gather_dev(self._h, pyr._h, C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap, C.byref(prm),
                                                   C.c_void_p(dxy_ptr), C.c_void_p(ddesc_ptr), C.c_void_p(dsrc_ptr or 0),
                                                   C.c_void_p(dcount_ptr)))

    def describe_points(self, img, pts, prm=None, w=None):
        """Host form: 8-bit grey image (h, w), points (n, 2) in level-0 pixels -> (desc (n, 32) u8, valid (n,) u8, bin (n,) u8).
        With w given, img holds h rows of img.shape[1] >= w bytes (a row stride)."""
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim != 2:
            raise ValueError("img must be a 2-D array")
        h = img.shape[0]
        w = img.shape[1] if w is None else w
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        prm = prm or describe_params()
        desc, valid, bins = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        _check(lib().pm_describe_points(self._h, _p(img), w, h, img.shape[1], _p(pts), n, C.byref(prm), _p(desc), _p(valid), _p(bins)))
        return desc[:n], valid[:n], bins[:n]

    # -- apply a 2-D model: image warp by H or A, point transform (SPEC S75-S78) -------------------------------------------
    def warp_dev(self, dsrc_ptr, sw, sh, sstride, dM_ptr, prm, ddst_ptr, dw, dh, dstride, dvalid_ptr=None, dinfo_ptr=None):
        """Device pointers; dM: 9 doubles (6 with PM_WARP_AFFINE) read on the device; prm: WarpParams.  dvalid (dw x dh bytes) and
        dinfo (a WarpInfo, 8 bytes) may be None."""
        _check(lib().pm_warp_dev(self._h, C.c_void_p(dsrc_ptr), sw, sh, sstride, C.c_void_p(dM_ptr), C.byref(prm) if prm is not None else None,
                                 C.c_void_p(ddst_ptr), dw, dh, dstride, C.c_void_p(dvalid_ptr or 0), C.c_void_p(dinfo_ptr or 0)))

    def warp(self, src, M, prm=None, dw=None, dh=None, sw=None):
        """Host form: 8-bit grey image (sh, sw), M (3, 3) or with PM_WARP_AFFINE (2, 3) -> (dst (dh, dw) u8, valid (dh, dw) u8,
        status, n_valid).  With sw given, src holds rows of src.shape[1] >= sw bytes (a row stride)."""
        src = np.ascontiguousarray(src, np.uint8)
        if src.ndim != 2:
            raise ValueError("src must be a 2-D array")
        sh = src.shape[0]
        sw = src.shape[1] if sw is None else sw
        dw = sw if dw is None else dw
        dh = sh if dh is None else dh
        prm = prm or warp_params()
        M = np.ascontiguousarray(M, np.float64).reshape(-1)
        if M.size != (6 if prm.flags & PM_WARP_AFFINE else 9):
            raise ValueError("M must hold 9 doubles, or 6 with PM_WARP_AFFINE")
        dst, valid = np.zeros((max(dh, 1), max(dw, 1)), np.uint8), np.zeros((max(dh, 1), max(dw, 1)), np.uint8)
        info = WarpInfo()
        _check(lib().pm_warp(self._h, _p(src), sw, sh, src.shape[1], _p(M), C.byref(prm), _p(dst), dw, dh, dst.shape[1], _p(valid),
                             C.byref(info)))
        return dst, valid, info.status, info.n_valid

    def transform_points_dev(self, dM_ptr, flags, dpts_ptr, dn_ptr, cap, dout_ptr):
        """Device pointers; dn_ptr (device int32 count) may be None = cap; dout may equal dpts."""
        _check(lib().pm_transform_points_dev(self._h, C.c_void_p(dM_ptr), flags, C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap,
                                             C.c_void_p(dout_ptr)))

    def transform_points(self, M, pts, flags=0):
        """Host form: points (n, 2) through M (3, 3), or (2, 3) with PM_WARP_AFFINE -> (n, 2) f32 (cv::perspectiveTransform)."""
        M = np.ascontiguousarray(M, np.float64).reshape(-1)
        if M.size != (6 if flags & PM_WARP_AFFINE else 9):
            raise ValueError("M must hold 9 doubles, or 6 with PM_WARP_AFFINE")
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = np.zeros((max(n, 1), 2), np.float32)
        _check(lib().pm_transform_points(self._h, _p(M), flags, _p(pts), n, _p(out)))
        return out[:n]

    # -- lens distortion: points both ways, undistort an image, map + remap (SPEC S79-S83) -------------------------------
    # K, K_new: a Camera, (fx, fy, cx, cy) or a 3 x 3 matrix (K_new None = K); dist: a Lens, up to five coefficients or None;
    # R: 3 x 3 or None.  All four are host values read at call time.
    def undistort_points_dev(self, K, dist, R, K_new, iters, tol_px, dpts_ptr, dn_ptr, cap, dout_ptr):
        """Device pointers; dn_ptr (device int32 count) may be None = cap; dout may equal dpts.  Rejected rows are NaN pairs."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        _check(lib().pm_undistort_points_dev(self._h, k, d, r, n, iters, C.c_double(tol_px), C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap,
                                             C.c_void_p(dout_ptr)))

    def undistort_points(self, K, dist, pts, R=None, K_new=None, iters=20, tol_px=1e-3):
        """Host form: distorted pixels (n, 2) under K -> ideal pixels under K_new, (n, 2) f32 (cv::undistortPoints with P)."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        cnt = pts.shape[0]
        out = np.zeros((max(cnt, 1), 2), np.float32)
        _check(lib().pm_undistort_points(self._h, k, d, r, n, iters, C.c_double(tol_px), _p(pts), cnt, _p(out)))
        return out[:cnt]

    def distort_points_dev(self, K, dist, R, K_new, dpts_ptr, dn_ptr, cap, dout_ptr):
        """Device pointers, as undistort_points_dev: ideal pixels under K_new -> distorted pixels under K."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        _check(lib().pm_distort_points_dev(self._h, k, d, r, n, C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap, C.c_void_p(dout_ptr)))

    def distort_points(self, K, dist, pts, R=None, K_new=None):
        """Host form: ideal pixels (n, 2) under K_new -> distorted pixels under K, (n, 2) f32."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        cnt = pts.shape[0]
        out = np.zeros((max(cnt, 1), 2), np.float32)
        _check(lib().pm_distort_points(self._h, k, d, r, n, _p(pts), cnt, _p(out)))
        return out[:cnt]

    def undistort_dev(self, dsrc_ptr, sw, sh, sstride, K, dist, R, K_new, prm, ddst_ptr, dw, dh, dstride, dvalid_ptr=None, dinfo_ptr=None):
        """Device pointers; prm: WarpParams (PM_WARP_REPLICATE is the only flag).  dvalid (dw x dh bytes) and dinfo (a WarpInfo)
        may be None."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        _check(lib().pm_undistort_dev(self._h, C.c_void_p(dsrc_ptr), sw, sh, sstride, k, d, r, n, C.byref(prm) if prm is not None else None,
                                      C.c_void_p(ddst_ptr), dw, dh, dstride, C.c_void_p(dvalid_ptr or 0), C.c_void_p(dinfo_ptr or 0)))

    def undistort(self, src, K, dist, R=None, K_new=None, prm=None, dw=None, dh=None, sw=None, dst=None):
        """Host form: 8-bit grey image (sh, sw) -> (dst (dh, dw) u8, valid (dh, dw) u8, n_valid) (cv::undistort; with R and
        K_new cv::initUndistortRectifyMap + cv::remap).  With sw given, src holds rows of src.shape[1] >= sw bytes; with dst (a
        contiguous (dh, dstride >= dw) u8 array) given it is written in place and returned."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        src = np.ascontiguousarray(src, np.uint8)
        if src.ndim != 2:
            raise ValueError("src must be a 2-D array")
        sh = src.shape[0]
        sw = src.shape[1] if sw is None else sw
        dw = sw if dw is None else dw
        dh = sh if dh is None else dh
        prm = prm or warp_params()
        if dst is None:
            dst = np.zeros((max(dh, 1), max(dw, 1)), np.uint8)
        if dst.dtype != np.uint8 or dst.ndim != 2 or not dst.flags.c_contiguous or dst.shape[0] != max(dh, 1):
            raise ValueError("dst must be a contiguous (dh, dstride) uint8 array")
        valid = np.zeros((max(dh, 1), max(dw, 1)), np.uint8)
        info = WarpInfo()
        _check(lib().pm_undistort(self._h, _p(src), sw, sh, src.shape[1], k, d, r, n, C.byref(prm), _p(dst), dw, dh, dst.shape[1], _p(valid),
                                  C.byref(info)))
        return dst, valid, info.n_valid

    def undistort_map_dev(self, K, dist, R, K_new, dw, dh, dmap_ptr):
        """dmap: dw * dh int32 pairs (qx, qy) in 1/32 pixel, (INT32_MIN, INT32_MIN) = no usable position; 8-byte aligned."""
        k, d, r, n, keep = _lens_model(K, dist, R, K_new)
        _check(lib().pm_undistort_map_dev(self._h, k, d, r, n, dw, dh, C.c_void_p(dmap_ptr)))

    def remap_dev(self, dsrc_ptr, sw, sh, sstride, dmap_ptr, prm, ddst_ptr, dw, dh, dstride, dvalid_ptr=None, dinfo_ptr=None):
        """Device pointers; dmap as undistort_map_dev writes it (any int32 pairs are legal)."""
        _check(lib().pm_remap_dev(self._h, C.c_void_p(dsrc_ptr), sw, sh, sstride, C.c_void_p(dmap_ptr), C.byref(prm) if prm is not None else None,
                                  C.c_void_p(ddst_ptr), dw, dh, dstride, C.c_void_p(dvalid_ptr or 0), C.c_void_p(dinfo_ptr or 0)))

    def remap(self, src, qmap, prm=None, sw=None):
        """Host form: src (sh, sw) u8, qmap (dh, dw, 2) int32 -> (dst (dh, dw) u8, valid (dh, dw) u8, n_valid)."""
        src = np.ascontiguousarray(src, np.uint8)
        qmap = np.ascontiguousarray(qmap, np.int32)
        if src.ndim != 2 or qmap.ndim != 3 or qmap.shape[2] != 2:
            raise ValueError("src must be 2-D and qmap (dh, dw, 2)")
        sh = src.shape[0]
        sw = src.shape[1] if sw is None else sw
        dh, dw = qmap.shape[:2]
        prm = prm or warp_params()
        dst, valid = np.zeros((max(dh, 1), max(dw, 1)), np.uint8), np.zeros((max(dh, 1), max(dw, 1)), np.uint8)
        info = WarpInfo()
        _check(lib().pm_remap(self._h, _p(src), sw, sh, src.shape[1], _p(qmap), C.byref(prm), _p(dst), dw, dh, dst.shape[1], _p(valid),
                              C.byref(info)))
        return dst, valid, info.n_valid

    # -- dense stereo on a rectified pair: block matching, left-right check, depth at points (SPEC S85-S87) ----------------
    def stereo_bm_dev(self, dleft_ptr, dright_ptr, w, h, lstride, rstride, prm, ddisp_ptr, dstride, dinfo_ptr=None):
        """Device pointers; prm: StereoParams; ddisp: int16 rows of dstride elements; dinfo (a StereoInfo, 8 bytes) may be None."""
        _check(lib().pm_stereo_bm_dev(self._h, C.c_void_p(dleft_ptr), C.c_void_p(dright_ptr), w, h, lstride, rstride,
                                      C.byref(prm) if prm is not None else None, C.c_void_p(ddisp_ptr), dstride, C.c_void_p(dinfo_ptr or 0)))

    def stereo_bm(self, left, right, prm=None, lr_max_diff16=-1, w=None, disp=None):
        """Host form: a rectified 8-bit pair (h, w) -> (disp (h, w) int16 in 1/16 pixel, n_valid) (cv::StereoBM without its
        pre-filter).  lr_max_diff16 >= 0 adds the FROM_RIGHT pass and the left-right check.  With w given, the images hold rows of
        shape[1] >= w bytes; with disp (a contiguous (h, dstride >= w) int16 array) given it is written in place and returned."""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        if left.ndim != 2 or right.ndim != 2 or left.shape[0] != right.shape[0]:
            raise ValueError("left and right must be 2-D arrays of one height")
        h = left.shape[0]
        w = left.shape[1] if w is None else w
        prm = prm or stereo_params()
        if disp is None:
            disp = np.zeros((max(h, 1), max(w, 1)), np.int16)
        if disp.dtype != np.int16 or disp.ndim != 2 or not disp.flags.c_contiguous or disp.shape[0] != max(h, 1):
            raise ValueError("disp must be a contiguous (h, dstride) int16 array")
        info = StereoInfo()
        _check(lib().pm_stereo_bm(self._h, _p(left), _p(right), w, h, left.shape[1], right.shape[1], C.byref(prm), lr_max_diff16, _p(disp),
                                  disp.shape[1], C.byref(info)))
        return disp, info.n_valid

    def stereo_sgm_dev(self, dleft_ptr, dright_ptr, w, h, lstride, rstride, prm, ddisp_ptr, dstride, dinfo_ptr=None):
        """Semi-global matching (SPEC S89-S92) on device pointers; prm: SgmParams; the map and dinfo as for stereo_bm_dev."""
        _check(lib().pm_stereo_sgm_dev(self._h, C.c_void_p(dleft_ptr), C.c_void_p(dright_ptr), w, h, lstride, rstride,
                                       C.byref(prm) if prm is not None else None, C.c_void_p(ddisp_ptr), dstride, C.c_void_p(dinfo_ptr or 0)))

    def stereo_sgm(self, left, right, prm=None, lr_max_diff16=-1, w=None, disp=None):
        """Host form of stereo_sgm_dev: a rectified 8-bit pair (h, w) -> (disp (h, w) int16 in 1/16 pixel, n_valid)
        (cv::StereoSGBM's place in the chain).  lr_max_diff16, w and disp as for stereo_bm."""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        if left.ndim != 2 or right.ndim != 2 or left.shape[0] != right.shape[0]:
            raise ValueError("left and right must be 2-D arrays of one height")
        h = left.shape[0]
        w = left.shape[1] if w is None else w
        prm = prm or sgm_params()
        if disp is None:
            disp = np.zeros((max(h, 1), max(w, 1)), np.int16)
        if disp.dtype != np.int16 or disp.ndim != 2 or not disp.flags.c_contiguous or disp.shape[0] != max(h, 1):
            raise ValueError("disp must be a contiguous (h, dstride) int16 array")
        info = StereoInfo()
        _check(lib().pm_stereo_sgm(self._h, _p(left), _p(right), w, h, left.shape[1], right.shape[1], C.byref(prm), lr_max_diff16, _p(disp),
                                   disp.shape[1], C.byref(info)))
        return disp, info.n_valid

    def stereo_lr_check_dev(self, dleft_ptr, dright_ptr, w, h, lstride, rstride, max_diff16, dinfo_ptr=None):
        """Device pointers to the two int16 maps (strides in elements); the left map is checked in place."""
        _check(lib().pm_stereo_lr_check_dev(self._h, C.c_void_p(dleft_ptr), C.c_void_p(dright_ptr), w, h, lstride, rstride, max_diff16,
                                            C.c_void_p(dinfo_ptr or 0)))

    def stereo_points_dev(self, ddisp_ptr, w, h, dstride, K_rect, baseline, R, dpts_ptr, dn_ptr, cap, dxyz_ptr):
        """Device pointers; K_rect as the other cameras, R (3 x 3 or None) a host value; dn_ptr (device int32 count) may be None =
        cap.  Rows without a depth are three NaNs."""
        k = _camera(K_rect)
        r = None if R is None else np.ascontiguousarray(R, np.float64).reshape(-1)
        if r is not None and r.size != 9:
            raise ValueError("R must hold 9 doubles")
        _check(lib().pm_stereo_points_dev(self._h, C.c_void_p(ddisp_ptr), w, h, dstride, C.byref(k), C.c_double(baseline), _p(r),
                                          C.c_void_p(dpts_ptr), C.c_void_p(dn_ptr or 0), cap, C.c_void_p(dxyz_ptr)))

    def stereo_points(self, disp, K_rect, baseline, pts, R=None, w=None):
        """Host form: disp (h, w) int16, pts (n, 2) in the rectified left image -> (n, 3) f32 (cv::reprojectImageTo3D at pts)."""
        disp = np.ascontiguousarray(disp, np.int16)
        if disp.ndim != 2:
            raise ValueError("disp must be a 2-D array")
        h = disp.shape[0]
        w = disp.shape[1] if w is None else w
        k = _camera(K_rect)
        r = None if R is None else np.ascontiguousarray(R, np.float64).reshape(-1)
        if r is not None and r.size != 9:
            raise ValueError("R must hold 9 doubles")
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = np.zeros((max(n, 1), 3), np.float32)
        _check(lib().pm_stereo_points(self._h, _p(disp), w, h, disp.shape[1], C.byref(k), C.c_double(baseline), _p(r), _p(pts), n, _p(out)))
        return out[:n]

    def bf_knn_l2_u8(self, q, t, k):
        """u8 descriptor rows, host arrays (pm_bf_knn_l2_u8)."""
        q = np.ascontiguousarray(q, np.uint8)
        t = np.ascontiguousarray(t, np.uint8)
        nq, dim = q.shape
        out = np.zeros((nq, k), MATCH_DTYPE)
        _check(lib().pm_bf_knn_l2_u8(self._h, _p(q), nq, _p(t), t.shape[0], dim, k, _p(out)))
        return out

    def bf_knn_l2_u8_dev(self, dq_ptr, nq, dt_ptr, nt, dim, k, dout_ptr):
        _check(lib().pm_bf_knn_l2_u8_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt, dim, k, C.c_void_p(dout_ptr)))

    def bf_knn_l2_u8_ratio_dev(self, dq_ptr, nq, dt_ptr, nt, dim, ratio, dkp1_ptr, dkp2_ptr, dknn_ptr, dgood_ptr, dxy1_ptr,
                               dxy2_ptr, dn_ptr):
        _check(lib().pm_bf_knn_l2_u8_ratio_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt, dim, C.c_float(ratio),
                                               C.c_void_p(dkp1_ptr or 0), C.c_void_p(dkp2_ptr or 0), C.c_void_p(dknn_ptr),
                                               C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr or 0), C.c_void_p(dxy2_ptr or 0),
                                               C.c_void_p(dn_ptr)))

    # -- matcher (main.cpp:46) -------------------------------------------------------------------
    def bf_knn_l2(self, q, t, k, flags=0):
        q = np.ascontiguousarray(q, np.float32)
        t = np.ascontiguousarray(t, np.float32)
        dim = q.shape[1]
        assert t.ndim == 2 and t.shape[1] == dim
        out = np.zeros((q.shape[0], k), MATCH_DTYPE)
        _check(lib().pm_bf_knn_l2_f32(self._h, _p(q), q.shape[0], _p(t), t.shape[0], dim, k, flags,
                                      _p(out)))
        return out

    def bf_knn_l2_dev(self, dq_ptr, nq, dt_ptr, nt, dim, k, dout_ptr, flags=0):
        _check(lib().pm_bf_knn_l2_f32_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt,
                                          dim, k, flags, C.c_void_p(dout_ptr)))

    def bf_knn_l2_ratio_dev(self, dq_ptr, nq, dt_ptr, nt, dim, flags, ratio, dkp1_ptr, dkp2_ptr, dknn_ptr, dgood_ptr,
                            dxy1_ptr, dxy2_ptr, dn_ptr):
        _check(lib().pm_bf_knn_l2_ratio_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr), nt, dim, flags,
                                            C.c_float(ratio), C.c_void_p(dkp1_ptr or 0), C.c_void_p(dkp2_ptr or 0),
                                            C.c_void_p(dknn_ptr or 0), C.c_void_p(dgood_ptr), C.c_void_p(dxy1_ptr or 0),
                                            C.c_void_p(dxy2_ptr or 0), C.c_void_p(dn_ptr)))

    def bf_knn_hamming(self, q, t, k):
        q = np.ascontiguousarray(q, np.uint8)
        t = np.ascontiguousarray(t, np.uint8)
        nbytes = q.shape[1]
        assert t.ndim == 2 and t.shape[1] == nbytes
        out = np.zeros((q.shape[0], k), MATCH_DTYPE)
        _check(lib().pm_bf_knn_hamming_u8(self._h, _p(q), q.shape[0], _p(t), t.shape[0], nbytes, k,
                                          _p(out)))
        return out

    def pad_rows_u8_dev(self, dsrc_ptr, n, nbytes, ddst_ptr, dst_bytes):
        _check(lib().pm_pad_rows_u8_dev(self._h, C.c_void_p(dsrc_ptr or 0), n, nbytes, C.c_void_p(ddst_ptr or 0), dst_bytes))

    def bf_knn_hamming_dev(self, dq_ptr, nq, dt_ptr, nt, nbytes, k, dout_ptr):
        _check(lib().pm_bf_knn_hamming_u8_dev(self._h, C.c_void_p(dq_ptr), nq, C.c_void_p(dt_ptr),
                                              nt, nbytes, k, C.c_void_p(dout_ptr)))

    # -- robust F (main.cpp:95-98) ---------------------------------------------------------------
    def ransac_fundamental(self, xy1, xy2, iters, thresh_px, seed, kind=PM_ERR_SAMPSON,
                           hyp_begin=0):
        """Returns (status, F(3x3), mask, n_inliers, best_key); raises on anything other than
        PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW (those are data outcomes, reported as status)."""
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
        xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        n = xy1.shape[0]
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        F = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = lib().pm_ransac_fundamental(self._h, _p(xy1), _p(xy2), n, C.byref(prm), _p(F), _p(mask),
                                         C.byref(ninl), C.byref(key))
        if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
            _check(rc)
        return rc, F.reshape(3, 3), mask[:n], ninl.value, key.value

    def ransac_model_from_hyp(self, xy1, xy2, hyp, thresh_px, seed, kind=PM_ERR_SAMPSON):
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
        xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        n = xy1.shape[0]
        prm = RansacParams(0, 0, seed, thresh_px, kind)
        F = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl = C.c_int()
        rc = lib().pm_ransac_model_from_hyp(self._h, _p(xy1), _p(xy2), n, C.byref(prm),
                                            C.c_int64(hyp), _p(F), _p(mask), C.byref(ninl))
        if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
            _check(rc)
        return rc, F.reshape(3, 3), mask[:n], ninl.value

    def ransac_score_dev(self, dxy1_ptr, dxy2_ptr, n, hyp_begin, hyp_end, thresh_px, seed,
                         dkey_ptr, kind=PM_ERR_SAMPSON):
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_score_dev(self._h, C.c_void_p(dxy1_ptr), C.c_void_p(dxy2_ptr), n,
                                         C.byref(prm), C.c_void_p(dkey_ptr)))

    # -- robust H (cv::findHomography(..., RANSAC, thr), sibling of main.cpp:95-98) -----------------
    def ransac_homography(self, xy1, xy2, iters, thresh_px, seed, hyp_begin=0, kind=PM_ERR_REPROJ):
        """Hypotheses [hyp_begin, iters).  Returns (status, H(3x3), mask, n_inliers, best_key); raises on anything other
        than PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW (those are data outcomes, reported as status)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        H = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = _outcome(lib().pm_ransac_homography(self._h, _p(xy1), _p(xy2), n, C.byref(prm), _p(H), _p(mask),
                                                 C.byref(ninl), C.byref(key)))
        return rc, H.reshape(3, 3), mask[:n], ninl.value, key.value

    def ransac_homography_from_hyp(self, xy1, xy2, hyp, thresh_px, seed, kind=PM_ERR_REPROJ):
        """H, mask and count of one hypothesis id: (status, H(3x3), mask, n_inliers)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(0, 0, seed, thresh_px, kind)
        H = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl = C.c_int()
        rc = _outcome(lib().pm_ransac_homography_from_hyp(self._h, _p(xy1), _p(xy2), n, C.byref(prm), C.c_int64(hyp),
                                                          _p(H), _p(mask), C.byref(ninl)))
        return rc, H.reshape(3, 3), mask[:n], ninl.value

    def ransac_homography_run_dev(self, view, hyp_begin, hyp_end, thresh_px, seed, dkey_ptr, dH_ptr, dmask_ptr, mask_len,
                                  dninl_ptr, kind=PM_ERR_REPROJ):
        """Device-resident run over a PointsView (count read on the device); outputs are device pointers."""
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_homography_run_dev(self._h, C.byref(view), C.byref(prm), C.c_void_p(dkey_ptr),
                                                  C.c_void_p(dH_ptr), C.c_void_p(dmask_ptr), mask_len,
                                                  C.c_void_p(dninl_ptr)))

    # -- refinement of the robust H on its inliers (DLT refit + LM, SPEC S23-S25) ------------------------------------
    def homography_refine(self, xy1, xy2, mask, H_in, max_iters=10):
        """Returns (status, H(3x3), HRefineInfo); raises on anything other than PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW."""
        xy1, xy2, n = _pair(xy1, xy2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("xy1, xy2 and mask must have the same length")
        Hin = np.ascontiguousarray(H_in, np.float64).reshape(9)
        H = np.zeros(9, np.float64)
        info = HRefineInfo()
        rc = _outcome(lib().pm_homography_refine(self._h, _p(xy1), _p(xy2), n, _p(mask), _p(Hin), max_iters, _p(H),
                                                 C.byref(info)))
        return rc, H.reshape(3, 3), info

    def homography_refine_dev(self, view, dmask_ptr, dHin_ptr, max_iters, dHout_ptr, dinfo_ptr=None):
        """Device form over a PointsView; dinfo_ptr (32 bytes, H_REFINE_INFO_DTYPE) may be None."""
        _check(lib().pm_homography_refine_dev(self._h, C.byref(view), C.c_void_p(dmask_ptr), C.c_void_p(dHin_ptr),
                                              max_iters, C.c_void_p(dHout_ptr), C.c_void_p(dinfo_ptr)))

    def ransac_homography_refined(self, xy1, xy2, iters, thresh_px, seed, max_iters=10, hyp_begin=0, kind=PM_ERR_REPROJ):
        """RANSAC-H + refinement, one synchronisation: (status, H(3x3), mask, n_inliers, best_key, HRefineInfo)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        H = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        info = HRefineInfo()
        rc = _outcome(lib().pm_ransac_homography_refined(self._h, _p(xy1), _p(xy2), n, C.byref(prm), max_iters, _p(H),
                                                         _p(mask), C.byref(ninl), C.byref(key), C.byref(info)))
        return rc, H.reshape(3, 3), mask[:n], ninl.value, key.value, info


    # -- refinement of the robust F on its inliers (8-point refit + rank-2 LM, SPEC S43-S45) ----------------------------
    def fundamental_refine(self, xy1, xy2, mask, F_in, max_iters=10):
        """Returns (status, F(3x3), HRefineInfo); raises on anything other than PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW."""
        xy1, xy2, n = _pair(xy1, xy2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("xy1, xy2 and mask must have the same length")
        Fin = np.ascontiguousarray(F_in, np.float64).reshape(9)
        F = np.zeros(9, np.float64)
        info = HRefineInfo()
        rc = _outcome(lib().pm_fundamental_refine(self._h, _p(xy1), _p(xy2), n, _p(mask), _p(Fin), max_iters, _p(F),
                                                  C.byref(info)))
        return rc, F.reshape(3, 3), info

    def fundamental_refine_dev(self, view, dmask_ptr, dFin_ptr, max_iters, dFout_ptr, dinfo_ptr=None):
        """Device form over a PointsView; dinfo_ptr (32 bytes, H_REFINE_INFO_DTYPE) may be None."""
        _check(lib().pm_fundamental_refine_dev(self._h, C.byref(view), C.c_void_p(dmask_ptr), C.c_void_p(dFin_ptr),
                                               max_iters, C.c_void_p(dFout_ptr), C.c_void_p(dinfo_ptr)))

    def ransac_fundamental_refined(self, xy1, xy2, iters, thresh_px, seed, max_iters=10, hyp_begin=0, kind=PM_ERR_SAMPSON):
        """RANSAC-F + refinement, one synchronisation: (status, F(3x3), mask, n_inliers, best_key, HRefineInfo)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        F = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        info = HRefineInfo()
        rc = _outcome(lib().pm_ransac_fundamental_refined(self._h, _p(xy1), _p(xy2), n, C.byref(prm), max_iters, _p(F),
                                                          _p(mask), C.byref(ninl), C.byref(key), C.byref(info)))
        return rc, F.reshape(3, 3), mask[:n], ninl.value, key.value, info

    # -- robust 2D affine / similarity (cv::estimateAffine2D / estimateAffinePartial2D, SPEC S26-S30) -------------------
    # model: PM_AFFINE_FULL (6 DOF) or PM_AFFINE_PARTIAL (4 DOF).  A is returned as a 2 x 3 float64 array.
    def ransac_affine(self, xy1, xy2, iters, thresh_px, seed, model=PM_AFFINE_FULL, hyp_begin=0, kind=PM_ERR_REPROJ):
        """Hypotheses [hyp_begin, iters).  Returns (status, A(2x3), mask, n_inliers, best_key); raises on anything other
        than PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW (those are data outcomes, reported as status)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        A = np.zeros(6, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = _outcome(lib().pm_ransac_affine(self._h, model, _p(xy1), _p(xy2), n, C.byref(prm), _p(A), _p(mask),
                                             C.byref(ninl), C.byref(key)))
        return rc, A.reshape(2, 3), mask[:n], ninl.value, key.value

    def ransac_affine_from_hyp(self, xy1, xy2, hyp, thresh_px, seed, model=PM_AFFINE_FULL, kind=PM_ERR_REPROJ):
        """A, mask and count of one hypothesis id: (status, A(2x3), mask, n_inliers)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(0, 0, seed, thresh_px, kind)
        A = np.zeros(6, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl = C.c_int()
        rc = _outcome(lib().pm_ransac_affine_from_hyp(self._h, model, _p(xy1), _p(xy2), n, C.byref(prm), C.c_int64(hyp),
                                                      _p(A), _p(mask), C.byref(ninl)))
        return rc, A.reshape(2, 3), mask[:n], ninl.value

    def ransac_affine_run_dev(self, view, hyp_begin, hyp_end, thresh_px, seed, dkey_ptr, dA_ptr, dmask_ptr, mask_len,
                              dninl_ptr, model=PM_AFFINE_FULL, kind=PM_ERR_REPROJ):
        """Device-resident run over a PointsView (count read on the device); outputs are device pointers (A: 6 doubles)."""
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_affine_run_dev(self._h, model, C.byref(view), C.byref(prm), C.c_void_p(dkey_ptr),
                                              C.c_void_p(dA_ptr), C.c_void_p(dmask_ptr), mask_len, C.c_void_p(dninl_ptr)))

    def affine_refine(self, xy1, xy2, mask, A_in, model=PM_AFFINE_FULL):
        """Least-squares refit on the inliers: (status, A(2x3), HRefineInfo); raises on anything other than PM_OK /
        PM_E_NO_MODEL / PM_E_TOO_FEW."""
        xy1, xy2, n = _pair(xy1, xy2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("xy1, xy2 and mask must have the same length")
        Ain = np.ascontiguousarray(A_in, np.float64).reshape(6)
        A = np.zeros(6, np.float64)
        info = HRefineInfo()
        rc = _outcome(lib().pm_affine_refine(self._h, model, _p(xy1), _p(xy2), n, _p(mask), _p(Ain), _p(A),
                                             C.byref(info)))
        return rc, A.reshape(2, 3), info

    def affine_refine_dev(self, view, dmask_ptr, dAin_ptr, dAout_ptr, dinfo_ptr=None, model=PM_AFFINE_FULL):
        """Device form over a PointsView; dinfo_ptr (32 bytes, H_REFINE_INFO_DTYPE) may be None."""
        _check(lib().pm_affine_refine_dev(self._h, model, C.byref(view), C.c_void_p(dmask_ptr), C.c_void_p(dAin_ptr),
                                          C.c_void_p(dAout_ptr), C.c_void_p(dinfo_ptr)))

    def estimate_affine(self, xy1, xy2, iters, thresh_px, seed, model=PM_AFFINE_FULL, refine=True, hyp_begin=0,
                        kind=PM_ERR_REPROJ):
        """RANSAC-A + (refine) refit, one synchronisation: (status, A(2x3), mask, n_inliers, best_key, HRefineInfo)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        A = np.zeros(6, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        info = HRefineInfo()
        rc = _outcome(lib().pm_estimate_affine(self._h, model, _p(xy1), _p(xy2), n, C.byref(prm), 1 if refine else 0,
                                               _p(A), _p(mask), C.byref(ninl), C.byref(key), C.byref(info)))
        return rc, A.reshape(2, 3), mask[:n], ninl.value, key.value, info

    # -- calibrated relative pose (cv::findEssentialMat + cv::recoverPose, SPEC S31-S35) ---------------------------------
    # K: a Camera, (fx, fy, cx, cy) or a 3 x 3 intrinsic matrix.  E and R are returned as 3 x 3 float64 arrays.
    def ransac_essential(self, xy1, xy2, K, iters, thresh_px, seed, hyp_begin=0, kind=PM_ERR_SAMPSON):
        """Samples [hyp_begin, iters).  Returns (status, E(3x3), mask, n_inliers, best_key); raises on anything other than
        PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW (those are data outcomes, reported as status)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        E = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = _outcome(lib().pm_ransac_essential(self._h, _p(xy1), _p(xy2), n, C.byref(_camera(K)), C.byref(prm), _p(E),
                                                _p(mask), C.byref(ninl), C.byref(key)))
        return rc, E.reshape(3, 3), mask[:n], ninl.value, key.value

    def ransac_essential_from_hyp(self, xy1, xy2, K, hyp, thresh_px, seed, kind=PM_ERR_SAMPSON):
        """All candidates of one sample id: (status, E(10x3x3), counts(10; -1 = unused slot), n_models)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(0, 0, seed, thresh_px, kind)
        E = np.zeros(90, np.float64)
        counts = np.zeros(10, np.int32)
        nm = C.c_int()
        rc = _outcome(lib().pm_ransac_essential_from_hyp(self._h, _p(xy1), _p(xy2), n, C.byref(_camera(K)), C.byref(prm),
                                                         C.c_int64(hyp), _p(E), _p(counts), C.byref(nm)))
        return rc, E.reshape(10, 3, 3), counts, nm.value

    def ransac_essential_run_dev(self, view, K, hyp_begin, hyp_end, thresh_px, seed, dkey_ptr, dE_ptr, dmask_ptr, mask_len,
                                 dninl_ptr, kind=PM_ERR_SAMPSON):
        """Device-resident run over a PointsView (count read on the device); outputs are device pointers (E: 9 doubles)."""
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_essential_run_dev(self._h, C.byref(view), C.byref(_camera(K)), C.byref(prm),
                                                 C.c_void_p(dkey_ptr), C.c_void_p(dE_ptr), C.c_void_p(dmask_ptr), mask_len,
                                                 C.c_void_p(dninl_ptr)))

    def recover_pose(self, xy1, xy2, K, E, mask=None, dist=50.0, points=False):
        """Pose from E on the masked correspondences: (status, R(3x3), t(3), pose mask, n_good, points n x 4 or None)."""
        xy1, xy2, n = _pair(xy1, xy2)
        Ein = np.ascontiguousarray(E, np.float64).reshape(9)
        mi = None
        if mask is not None:
            mi = np.ascontiguousarray(mask, np.uint8).reshape(-1)
            if mi.shape[0] != n:
                raise ValueError("xy1, xy2 and mask must have the same length")
        R, t = np.zeros(9, np.float64), np.zeros(3, np.float64)
        mo = np.zeros(max(n, 1), np.uint8)
        pts = np.zeros((max(n, 1), 4), np.float32) if points else None
        ng = C.c_int()
        rc = _outcome(lib().pm_recover_pose(self._h, _p(xy1), _p(xy2), n, C.byref(_camera(K)), _p(Ein), _p(mi),
                                            C.c_double(dist), _p(R), _p(t), _p(mo), C.byref(ng), _p(pts)))
        return rc, R.reshape(3, 3), t, mo[:n], ng.value, (pts[:n] if points else None)

    def recover_pose_dev(self, view, K, dE_ptr, dmask_in_ptr, dR_ptr, dt_ptr, dmask_out_ptr, dngood_ptr, dpoints_ptr=None,
                         dist=50.0):
        """Device form over a PointsView; dmask_in_ptr and dpoints_ptr may be None."""
        _check(lib().pm_recover_pose_dev(self._h, C.byref(view), C.byref(_camera(K)), C.c_void_p(dE_ptr),
                                         C.c_void_p(dmask_in_ptr), C.c_double(dist), C.c_void_p(dR_ptr), C.c_void_p(dt_ptr),
                                         C.c_void_p(dmask_out_ptr), C.c_void_p(dngood_ptr), C.c_void_p(dpoints_ptr)))

    def estimate_pose(self, xy1, xy2, K, iters, thresh_px, seed, dist=50.0, hyp_begin=0, kind=PM_ERR_SAMPSON):
        """RANSAC-E + pose recovery, one synchronisation: (status, E, R, t, pose mask, n_inliers, n_good, best_key)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        E, R, t = np.zeros(9, np.float64), np.zeros(9, np.float64), np.zeros(3, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, ng, key = C.c_int(), C.c_int(), C.c_uint64()
        rc = _outcome(lib().pm_estimate_pose(self._h, _p(xy1), _p(xy2), n, C.byref(_camera(K)), C.byref(prm),
                                             C.c_double(dist), _p(E), _p(R), _p(t), _p(mask), C.byref(ninl), C.byref(ng),
                                             C.byref(key)))
        return rc, E.reshape(3, 3), R.reshape(3, 3), t, mask[:n], ninl.value, ng.value, key.value

    # -- refinement of the relative pose on its inliers (5-parameter LM on the Sampson distance, SPEC S46-S47) -----------
    def pose_refine(self, xy1, xy2, K, mask, R_in, t_in, max_iters=20):
        """Returns (status, R(3x3), t(3), E(3x3) of the refined pose, HRefineInfo); raises on anything other than PM_OK /
        PM_E_NO_MODEL / PM_E_TOO_FEW."""
        xy1, xy2, n = _pair(xy1, xy2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("xy1, xy2 and mask must have the same length")
        Rin = np.ascontiguousarray(R_in, np.float64).reshape(9)
        tin = np.ascontiguousarray(t_in, np.float64).reshape(3)
        R, t, E = np.zeros(9, np.float64), np.zeros(3, np.float64), np.zeros(9, np.float64)
        info = HRefineInfo()
        rc = _outcome(lib().pm_pose_refine(self._h, _p(xy1), _p(xy2), n, C.byref(_camera(K)), _p(mask), _p(Rin), _p(tin),
                                           max_iters, _p(R), _p(t), _p(E), C.byref(info)))
        return rc, R.reshape(3, 3), t, E.reshape(3, 3), info

    def pose_refine_dev(self, view, K, dmask_ptr, dRt_in_ptr, max_iters, dRt_out_ptr, dE_out_ptr=None, dinfo_ptr=None):
        """Device form over a PointsView; Rt: 12 doubles (R, then t); dE_out_ptr (9 doubles) and dinfo_ptr (32 bytes,
        H_REFINE_INFO_DTYPE) may be None."""
        _check(lib().pm_pose_refine_dev(self._h, C.byref(view), C.byref(_camera(K)), C.c_void_p(dmask_ptr),
                                        C.c_void_p(dRt_in_ptr), max_iters, C.c_void_p(dRt_out_ptr), C.c_void_p(dE_out_ptr),
                                        C.c_void_p(dinfo_ptr)))

    def estimate_pose_refined(self, xy1, xy2, K, iters, thresh_px, seed, max_iters=20, dist=50.0, hyp_begin=0,
                              kind=PM_ERR_SAMPSON):
        """RANSAC-E + pose recovery + refinement, one synchronisation: (status, E of the refined pose, R, t, pose mask,
        n_inliers, n_good, best_key, HRefineInfo)."""
        xy1, xy2, n = _pair(xy1, xy2)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        E, R, t = np.zeros(9, np.float64), np.zeros(9, np.float64), np.zeros(3, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, ng, key = C.c_int(), C.c_int(), C.c_uint64()
        info = HRefineInfo()
        rc = _outcome(lib().pm_estimate_pose_refined(self._h, _p(xy1), _p(xy2), n, C.byref(_camera(K)), C.byref(prm),
                                                     C.c_double(dist), max_iters, _p(E), _p(R), _p(t), _p(mask),
                                                     C.byref(ninl), C.byref(ng), C.byref(key), C.byref(info)))
        return rc, E.reshape(3, 3), R.reshape(3, 3), t, mask[:n], ninl.value, ng.value, key.value, info

    # -- absolute camera pose (cv::solvePnPRansac with SOLVEPNP_P3P, SPEC S36-S39) -------------------------------------
    # xyz: n x 3 world points, uv: n x 2 pixels; K as for the calibrated pose.  R is returned as 3 x 3, t as 3 float64.
    def ransac_pnp(self, xyz, uv, K, iters, thresh_px, seed, hyp_begin=0, kind=PM_ERR_REPROJ):
        """Samples [hyp_begin, iters).  Returns (status, R(3x3), t(3), mask, n_inliers, best_key); raises on anything other
        than PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW (those are data outcomes, reported as status)."""
        xyz, uv, n = _pnp_pair(xyz, uv)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        R, t = np.zeros(9, np.float64), np.zeros(3, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = _outcome(lib().pm_ransac_pnp(self._h, _p(xyz), _p(uv), n, C.byref(_camera(K)), C.byref(prm), _p(R), _p(t),
                                          _p(mask), C.byref(ninl), C.byref(key)))
        return rc, R.reshape(3, 3), t, mask[:n], ninl.value, key.value

    def ransac_pnp_from_hyp(self, xyz, uv, K, hyp, thresh_px, seed, kind=PM_ERR_REPROJ):
        """All candidates of one sample id: (status, Rt(4 x 12: R row-major, then t), counts(4; -1 = unused slot),
        n_models)."""
        xyz, uv, n = _pnp_pair(xyz, uv)
        prm = RansacParams(0, 0, seed, thresh_px, kind)
        Rt = np.zeros(48, np.float64)
        counts = np.zeros(4, np.int32)
        nm = C.c_int()
        rc = _outcome(lib().pm_ransac_pnp_from_hyp(self._h, _p(xyz), _p(uv), n, C.byref(_camera(K)), C.byref(prm),
                                                   C.c_int64(hyp), _p(Rt), _p(counts), C.byref(nm)))
        return rc, Rt.reshape(4, 12), counts, nm.value

    def ransac_pnp_run_dev(self, view, K, hyp_begin, hyp_end, thresh_px, seed, dkey_ptr, dRt_ptr, dmask_ptr, mask_len,
                           dninl_ptr, kind=PM_ERR_REPROJ):
        """Device-resident run over a PnpView (count read on the device); outputs are device pointers (Rt: 12 doubles)."""
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh_px, kind)
        _check(lib().pm_ransac_pnp_run_dev(self._h, C.byref(view), C.byref(_camera(K)), C.byref(prm), C.c_void_p(dkey_ptr),
                                           C.c_void_p(dRt_ptr), C.c_void_p(dmask_ptr), mask_len, C.c_void_p(dninl_ptr)))

    def pnp_refine(self, xyz, uv, K, mask, R_in, t_in, max_iters=20):
        """LM refinement of a pose on its inliers (SPEC S40): (status, R(3x3), t(3), HRefineInfo); raises on anything other
        than PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW."""
        xyz, uv, n = _pnp_pair(xyz, uv)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("xyz, uv and mask must have the same length")
        Rin = np.ascontiguousarray(R_in, np.float64).reshape(9)
        tin = np.ascontiguousarray(t_in, np.float64).reshape(3)
        R, t = np.zeros(9, np.float64), np.zeros(3, np.float64)
        info = HRefineInfo()
        rc = _outcome(lib().pm_pnp_refine(self._h, _p(xyz), _p(uv), n, C.byref(_camera(K)), _p(mask), _p(Rin), _p(tin),
                                          max_iters, _p(R), _p(t), C.byref(info)))
        return rc, R.reshape(3, 3), t, info

    def pnp_refine_dev(self, view, K, dmask_ptr, dRt_in_ptr, max_iters, dRt_out_ptr, dinfo_ptr=None):
        """Device form over a PnpView; Rt: 12 doubles (R, then t); dinfo_ptr (32 bytes, H_REFINE_INFO_DTYPE) may be None."""
        _check(lib().pm_pnp_refine_dev(self._h, C.byref(view), C.byref(_camera(K)), C.c_void_p(dmask_ptr),
                                       C.c_void_p(dRt_in_ptr), max_iters, C.c_void_p(dRt_out_ptr), C.c_void_p(dinfo_ptr)))

    def solve_pnp_ransac(self, xyz, uv, K, iters, thresh_px, seed, max_iters=20, hyp_begin=0, kind=PM_ERR_REPROJ):
        """RANSAC-PnP + refinement, one synchronisation: (status, R(3x3), t(3), mask, n_inliers, best_key, HRefineInfo)."""
        xyz, uv, n = _pnp_pair(xyz, uv)
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        R, t = np.zeros(9, np.float64), np.zeros(3, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        info = HRefineInfo()
        rc = _outcome(lib().pm_solve_pnp_ransac(self._h, _p(xyz), _p(uv), n, C.byref(_camera(K)), C.byref(prm), max_iters,
                                                _p(R), _p(t), _p(mask), C.byref(ninl), C.byref(key), C.byref(info)))
        return rc, R.reshape(3, 3), t, mask[:n], ninl.value, key.value, info

    def lmeds_fundamental_dev(self, dxy1_ptr, dxy2_ptr, n, hyp_begin, hyp_end, seed, dF_ptr, dmask_ptr, dninl_ptr,
                              dbest_ptr, dmed_ptr):
        """Device-resident 7-point + LMedS (SPEC S13-S15): inputs and outputs are device pointers (F 9 doubles, mask n
        bytes, int32 count, int64 model id, double median; any output may be None).  Asynchronous on the context's
        stream.  No winning model is not an error here: the outputs are F = 0, mask = 0, count 0, id -1, median +inf."""
        prm = LmedsParams(hyp_begin, hyp_end, seed)
        _check(lib().pm_lmeds_fundamental_dev(self._h, C.c_void_p(dxy1_ptr), C.c_void_p(dxy2_ptr), n, C.byref(prm),
                                              C.c_void_p(dF_ptr), C.c_void_p(dmask_ptr), C.c_void_p(dninl_ptr),
                                              C.c_void_p(dbest_ptr), C.c_void_p(dmed_ptr)))

    def gather_pnp_dev(self, dmatches_ptr, dcount_ptr, cap, dkp_ptr, n_kp, dobj_ptr, n_obj, duv_ptr, dxyz_ptr):
        """Compacted matches -> PnP rows on the device (uv = keypoint of queryIdx, xyz = map point of trainIdx)."""
        _check(lib().pm_gather_pnp_dev(self._h, C.c_void_p(dmatches_ptr), C.c_void_p(dcount_ptr), cap, C.c_void_p(dkp_ptr),
                                       n_kp, C.c_void_p(dobj_ptr), n_obj, C.c_void_p(duv_ptr), C.c_void_p(dxyz_ptr)))

    # -- 3-D to 3-D alignment x2 = s R x1 + t (rigid or similarity, SPEC S97-S101) -----------------------------------------
    # xyz1, xyz2: n x 3 rows; model: PM_ALIGN3D_RIGID or PM_ALIGN3D_SIMILARITY.  T is returned as 13 float64: R (9,
    # row-major), t (3), s.
    def ransac_align3d(self, xyz1, xyz2, iters, thresh, seed, model=PM_ALIGN3D_RIGID, hyp_begin=0, kind=PM_ERR_REPROJ):
        """Samples [hyp_begin, iters).  Returns (status, T(13), mask, n_inliers, best_key); raises on anything other than
        PM_OK / PM_E_NO_MODEL / PM_E_TOO_FEW (those are data outcomes, reported as status)."""
        xyz1, xyz2, n = _xyz_pair(xyz1, xyz2)
        prm = RansacParams(hyp_begin, iters, seed, thresh, kind)
        T = np.zeros(13, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = _outcome(lib().pm_ransac_align3d(self._h, model, _p(xyz1), _p(xyz2), n, C.byref(prm), _p(T), _p(mask),
                                              C.byref(ninl), C.byref(key)))
        return rc, T, mask[:n], ninl.value, key.value

    def ransac_align3d_from_hyp(self, xyz1, xyz2, hyp, thresh, seed, model=PM_ALIGN3D_RIGID, kind=PM_ERR_REPROJ):
        """T, mask and count of one sample id: (status, T(13), mask, n_inliers)."""
        xyz1, xyz2, n = _xyz_pair(xyz1, xyz2)
        prm = RansacParams(0, 0, seed, thresh, kind)
        T = np.zeros(13, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl = C.c_int()
        rc = _outcome(lib().pm_ransac_align3d_from_hyp(self._h, model, _p(xyz1), _p(xyz2), n, C.byref(prm), C.c_int64(hyp),
                                                       _p(T), _p(mask), C.byref(ninl)))
        return rc, T, mask[:n], ninl.value

    def ransac_align3d_run_dev(self, view, hyp_begin, hyp_end, thresh, seed, dkey_ptr, dT_ptr, dmask_ptr, mask_len, dninl_ptr,
                               model=PM_ALIGN3D_RIGID, kind=PM_ERR_REPROJ):
        """Device-resident run over an XyzView (count read on the device); outputs are device pointers (T: 13 doubles)."""
        prm = RansacParams(hyp_begin, hyp_end, seed, thresh, kind)
        _check(lib().pm_ransac_align3d_run_dev(self._h, model, C.byref(view), C.byref(prm), C.c_void_p(dkey_ptr),
                                               C.c_void_p(dT_ptr), C.c_void_p(dmask_ptr), mask_len, C.c_void_p(dninl_ptr)))

    def align3d_refine(self, xyz1, xyz2, mask, T_in, model=PM_ALIGN3D_RIGID):
        """Closed-form refit on the inliers (SPEC S101): (status, T(13), HRefineInfo); raises on anything other than PM_OK /
        PM_E_NO_MODEL / PM_E_TOO_FEW."""
        xyz1, xyz2, n = _xyz_pair(xyz1, xyz2)
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mask.shape[0] != n:
            raise ValueError("xyz1, xyz2 and mask must have the same length")
        Tin = np.ascontiguousarray(T_in, np.float64).reshape(13)
        T = np.zeros(13, np.float64)
        info = HRefineInfo()
        rc = _outcome(lib().pm_align3d_refine(self._h, model, _p(xyz1), _p(xyz2), n, _p(mask), _p(Tin), _p(T), C.byref(info)))
        return rc, T, info

    def align3d_refine_dev(self, view, dmask_ptr, dTin_ptr, dTout_ptr, dinfo_ptr=None, model=PM_ALIGN3D_RIGID):
        """Device form over an XyzView; dinfo_ptr (32 bytes, H_REFINE_INFO_DTYPE) may be None."""
        _check(lib().pm_align3d_refine_dev(self._h, model, C.byref(view), C.c_void_p(dmask_ptr), C.c_void_p(dTin_ptr),
                                           C.c_void_p(dTout_ptr), C.c_void_p(dinfo_ptr)))

    def estimate_align3d(self, xyz1, xyz2, iters, thresh, seed, model=PM_ALIGN3D_RIGID, refine=True, hyp_begin=0,
                         kind=PM_ERR_REPROJ):
        """RANSAC + (refine) refit, one synchronisation: (status, T(13), mask, n_inliers, best_key, HRefineInfo)."""
        xyz1, xyz2, n = _xyz_pair(xyz1, xyz2)
        prm = RansacParams(hyp_begin, iters, seed, thresh, kind)
        T = np.zeros(13, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        info = HRefineInfo()
        rc = _outcome(lib().pm_estimate_align3d(self._h, model, _p(xyz1), _p(xyz2), n, C.byref(prm), 1 if refine else 0,
                                                _p(T), _p(mask), C.byref(ninl), C.byref(key), C.byref(info)))
        return rc, T, mask[:n], ninl.value, key.value, info

    def transform_points3_dev(self, dT_ptr, dxyz_ptr, dn_ptr, cap, dout_ptr):
        """Device pointers; dT: 13 doubles; dn_ptr (device int32 count) may be None = cap; dout may equal dxyz."""
        _check(lib().pm_transform_points3_dev(self._h, C.c_void_p(dT_ptr), C.c_void_p(dxyz_ptr), C.c_void_p(dn_ptr or 0), cap,
                                              C.c_void_p(dout_ptr)))

    def transform_points3(self, T, xyz):
        """Host form: rows (n, 3) through the 13-double model T -> (n, 3) f32; NaN rows stay NaN."""
        T = np.ascontiguousarray(T, np.float64).reshape(13)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        out = np.zeros((max(n, 1), 3), np.float32)
        _check(lib().pm_transform_points3(self._h, _p(T), _p(xyz), n, _p(out)))
        return out[:n]

    def gather_align3d_dev(self, dmatches_ptr, dcount_ptr, cap, dtab1_ptr, n1, dtab2_ptr, n2, dxyz1_ptr, dxyz2_ptr):
        """Compacted matches -> two row arrays on the device (xyz1 = table 1 at queryIdx, xyz2 = table 2 at trainIdx)."""
        _check(lib().pm_gather_align3d_dev(self._h, C.c_void_p(dmatches_ptr), C.c_void_p(dcount_ptr), cap, C.c_void_p(dtab1_ptr),
                                           n1, C.c_void_p(dtab2_ptr), n2, C.c_void_p(dxyz1_ptr), C.c_void_p(dxyz2_ptr)))

    # -- triangulation (cv::triangulatePoints + refinement + the map builder's gates, SPEC S93-S96) ----------------------
    def triangulate_dev(self, views, K, params, dxyz_ptr, dstatus_ptr, dpoints4_ptr=None, derr2_ptr=None, dngood_ptr=None):
        """Device form over a TriViews: d_xyz cap x 3 f32 (NaN unless PM_TRI_OK; read under PM_TRI_USE_INITIAL), d_status
        cap bytes, optional d_points4 (cap x 4 f32), d_err2 (cap f32) and *d_n_good (int32).  Asynchronous on the stream."""
        _check(lib().pm_triangulate_dev(self._h, C.byref(views), C.byref(_camera(K)), C.byref(params), C.c_void_p(dxyz_ptr),
                                        C.c_void_p(dstatus_ptr), C.c_void_p(dpoints4_ptr), C.c_void_p(derr2_ptr),
                                        C.c_void_p(dngood_ptr)))

    def triangulate(self, uv, Rt, K, params=None, xyz0=None):
        """uv: one (n, 2) pixel array per view (a NaN row: not seen there); Rt: one pose per view (12 doubles, R row-major
        then t, or None for [I|0]).  xyz0: the start under PM_TRI_USE_INITIAL.  Returns (xyz (n, 3), status (n), points4
        (n, 4), err2 (n), n_good); points4 is zero under PM_TRI_USE_INITIAL."""
        params = params if params is not None else tri_params()
        uv = [np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in uv]
        n = uv[0].shape[0] if uv else 0
        if any(u.shape[0] != n for u in uv) or len(Rt) != len(uv):
            raise ValueError("every view needs n pixel rows and a pose")
        poses = [None if r is None else np.ascontiguousarray(r, np.float64).reshape(12) for r in Rt]
        up = (C.c_void_p * max(len(uv), 1))(*[_p(u) for u in uv])
        rp = (C.c_void_p * max(len(uv), 1))(*[_p(r) for r in poses])
        xyz = np.zeros((max(n, 1), 3), np.float32)
        if xyz0 is not None:
            xyz[:n] = np.asarray(xyz0, np.float32).reshape(-1, 3)
        status, p4, e2 = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 4), np.float32), np.zeros(max(n, 1), np.float32)
        ng = C.c_int()
        _check(lib().pm_triangulate(self._h, up, rp, len(uv), n, C.byref(_camera(K)), C.byref(params), _p(xyz), _p(status),
                                    _p(p4), _p(e2), C.byref(ng)))
        return xyz[:n], status[:n], p4[:n], e2[:n], ng.value

    # -- local bundle adjustment (joint poses and points, Schur LM in one launch, SPEC S113-S117) -------------------------
    def bundle_adjust_dev(self, views, K, params, dRt_out_ptr, dxyz_ptr, dused_ptr, dwork_ptr, work_bytes, dinfo_ptr):
        """Device form over the TriViews of triangulate_dev: d_Rt_out n_views x 12 f64 (may be the input poses), d_xyz cap x 3
        f32 read and written, optional d_used (cap bytes), a workspace of bundle_adjust_workspace(n_views, cap) bytes and
        *d_info (BA_INFO_DTYPE).  Asynchronous on the stream."""
        _check(lib().pm_bundle_adjust_dev(self._h, C.byref(views), C.byref(_camera(K)), C.byref(params), C.c_void_p(dRt_out_ptr),
                                          C.c_void_p(dxyz_ptr), C.c_void_p(dused_ptr), C.c_void_p(dwork_ptr),
                                          C.c_size_t(work_bytes), C.c_void_p(dinfo_ptr)))

    def bundle_adjust(self, uv, Rt, K, xyz, params=None):
        """uv: one (n, 2) pixel array per view (a NaN row: not seen there); Rt: one pose per view (12 doubles or None for
        [I|0]); xyz: the map rows (n, 3), NaN rows allowed.  Returns (Rt_out (V, 12), xyz (n, 3) f32, used (n) u8, info (a
        BA_INFO_DTYPE record))."""
        params = params if params is not None else ba_params()
        uv = [np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in uv]
        n = uv[0].shape[0] if uv else 0
        if any(u.shape[0] != n for u in uv) or len(Rt) != len(uv):
            raise ValueError("every view needs n pixel rows and a pose")
        poses = [None if r is None else np.ascontiguousarray(r, np.float64).reshape(12) for r in Rt]
        up = (C.c_void_p * max(len(uv), 1))(*[_p(u) for u in uv])
        rp = (C.c_void_p * max(len(uv), 1))(*[_p(r) for r in poses])
        out = np.zeros((max(len(uv), 1), 12), np.float64)
        rows = np.zeros((max(n, 1), 3), np.float32)
        rows[:n] = np.asarray(xyz, np.float32).reshape(-1, 3)[:n]
        used = np.zeros(max(n, 1), np.uint8)
        info = np.zeros(1, BA_INFO_DTYPE)
        _check(lib().pm_bundle_adjust(self._h, up, rp, len(uv), n, C.byref(_camera(K)), C.byref(params), _p(out), _p(rows),
                                      _p(used), _p(info)))
        return out[:len(uv)], rows[:n], used[:n], info[0]

    # -- pose-graph optimisation (SE(3) / Sim(3) loop correction in one launch, SPEC S118-S123) ----------------------------
    def pose_graph_optimize_dev(self, dpose_in_ptr, n_nodes, dfixed_ptr, dab_ptr, dZ_ptr, dw_ptr, dcount_ptr, cap_edges, params,
                                dpose_out_ptr, dused_ptr, dwork_ptr, work_bytes, dinfo_ptr):
        """Device pointers: poses n_nodes x 13 f64 (out may be in), fixed n_nodes bytes, edges as ab (cap_edges x 2 i32), Z
        (cap_edges x 13 f64, row e as pm_align3d_refine_dev writes it) and w (cap_edges x 3 f64), an optional device-side edge
        count, optional d_edge_used (cap_edges bytes), a workspace of pose_graph_workspace(n_nodes, cap_edges, model) bytes
        and *d_info (PGO_INFO_DTYPE).  Asynchronous on the stream."""
        _check(lib().pm_pose_graph_optimize_dev(self._h, C.c_void_p(dpose_in_ptr), n_nodes, C.c_void_p(dfixed_ptr),
                                                C.c_void_p(dab_ptr), C.c_void_p(dZ_ptr), C.c_void_p(dw_ptr),
                                                C.c_void_p(dcount_ptr or 0), cap_edges, C.byref(params), C.c_void_p(dpose_out_ptr),
                                                C.c_void_p(dused_ptr or 0), C.c_void_p(dwork_ptr), C.c_size_t(work_bytes),
                                                C.c_void_p(dinfo_ptr)))

    def pose_graph_optimize(self, pose, fixed, ab, Z, w, params=None):
        """pose (N, 13), fixed (N) bytes, ab (E, 2), Z (E, 13), w (E, 3).  Returns (pose_out (N, 13), used (E) u8, info (a
        PGO_INFO_DTYPE record))."""
        params = params if params is not None else pgo_params()
        pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 13)
        fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
        ab = np.ascontiguousarray(ab, np.int32).reshape(-1, 2)
        Z = np.ascontiguousarray(Z, np.float64).reshape(-1, 13)
        w = np.ascontiguousarray(w, np.float64).reshape(-1, 3)
        N, E = pose.shape[0], ab.shape[0]
        if fixed.shape[0] != N or Z.shape[0] != E or w.shape[0] != E:
            raise ValueError("one fixed byte per node; one measurement and one weight row per edge")
        ab, Z, w = (v if E else np.zeros((1, v.shape[1]), v.dtype) for v in (ab, Z, w))
        out = np.zeros((max(N, 1), 13), np.float64)
        used = np.zeros(max(E, 1), np.uint8)
        info = np.zeros(1, PGO_INFO_DTYPE)
        _check(lib().pm_pose_graph_optimize(self._h, _p(pose), N, _p(fixed), _p(ab), _p(Z), _p(w), E, C.byref(params), _p(out),
                                            _p(used), _p(info)))
        return out[:N], used[:E], info[0]

    def pgo_move_points_dev(self, dpose_old_ptr, dpose_new_ptr, n_nodes, danchor_ptr, dxyz_ptr, dn_ptr, cap, dout_ptr):
        """Device pointers; poses n_nodes x 13 f64 before and after the graph, anchor cap i32, rows cap x 3 f32; dn_ptr (device
        int32 count) may be None = cap; dout may equal dxyz."""
        _check(lib().pm_pgo_move_points_dev(self._h, C.c_void_p(dpose_old_ptr), C.c_void_p(dpose_new_ptr), n_nodes,
                                            C.c_void_p(danchor_ptr), C.c_void_p(dxyz_ptr), C.c_void_p(dn_ptr or 0), cap,
                                            C.c_void_p(dout_ptr)))

    def pgo_move_points(self, pose_old, pose_new, anchor, xyz):
        """Host form: rows (n, 3) moved with their anchor keyframes -> (n, 3) f32; NaN rows stay NaN."""
        po = np.ascontiguousarray(pose_old, np.float64).reshape(-1, 13)
        pn = np.ascontiguousarray(pose_new, np.float64).reshape(-1, 13)
        anchor = np.ascontiguousarray(anchor, np.int32).reshape(-1)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        if po.shape != pn.shape or anchor.shape[0] != n:
            raise ValueError("old and new poses of the same nodes; one anchor per row")
        out = np.zeros((max(n, 1), 3), np.float32)
        _check(lib().pm_pgo_move_points(self._h, _p(po), _p(pn), po.shape[0], _p(anchor), _p(xyz), n, _p(out)))
        return out[:n]


class Pyramid:
    """pm_pyramid: the device image pyramid of one frame (SPEC S61).  A video loop keeps one per frame."""

    def __init__(self, ctx, w, h, max_level=3):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.w, self.h = w, h
        _check(lib().pm_pyramid_create(ctx._h, w, h, max_level, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pm_pyramid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_dev(self, dimg_ptr, stride=None):
        """Enqueues the build from a device image of h rows of `stride` (default w) bytes; no synchronisation."""
        _check(lib().pm_pyramid_build_dev(self._ctx._h, self._h, C.c_void_p(dimg_ptr), self.w if stride is None else stride))
        return self

    @property
    def levels(self):
        n = C.c_int()
        _check(lib().pm_pyramid_level_get(self._ctx._h, self._h, -1, None, 0, C.byref(n), None))
        return n.value

    def level(self, l):
        """Level l as an (h, w) uint8 array (pm_pyramid_level_get; synchronises)."""
        w, h = C.c_int(), C.c_int()
        _check(lib().pm_pyramid_level_get(self._ctx._h, self._h, l, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().pm_pyramid_level_get(self._ctx._h, self._h, l, _p(out), out.size, C.byref(w), C.byref(h)))
        return out


PM_VOCAB_L2_U8 = 0         # visual vocabularies (S102): rows of u8 values, squared L2
PM_VOCAB_BITS = 1          # rows of bits, Hamming
VOCAB_ITER_DTYPE = np.dtype([("n_changed", "<i4"), ("n_empty", "<i4"), ("n_moved", "<i4"), ("reserved", "<i4"),
                             ("cost", "<u8")])                             # pm_vocab_iter, 24 bytes


class Vocab:
    """pm_vocab: K words of `nbytes` bytes on the device, trained by k-means (u8 rows) or k-majority (bit rows) and used to
    encode row sets as bag-of-words histograms (SPEC S102-S106).  Owns its device memory; rows of a call: at most max_rows."""

    def __init__(self, ctx, kind, nbytes, K, max_rows):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.kind, self.nbytes, self.K, self.max_rows = kind, nbytes, K, max_rows
        _check(lib().pm_vocab_create(ctx._h, kind, nbytes, K, max_rows, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pm_vocab_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, rows):
        rows = np.ascontiguousarray(rows, np.uint8)
        if rows.ndim != 2 or rows.shape[1] != self.nbytes:
            raise PmError(PM_E_INVALID, "rows must be (n, %d) uint8" % self.nbytes)
        return rows

    def set(self, words):
        words = self._rows(words)
        if words.shape[0] != self.K:
            raise PmError(PM_E_INVALID, "need %d words" % self.K)
        _check(lib().pm_vocab_set(self._ctx._h, self._h, _p(words)))

    def set_dev(self, dwords_ptr):
        _check(lib().pm_vocab_set_dev(self._ctx._h, self._h, C.c_void_p(dwords_ptr)))

    def get(self):
        """The (K, nbytes) uint8 words; synchronises."""
        words = np.zeros((self.K, self.nbytes), np.uint8)
        _check(lib().pm_vocab_get(self._ctx._h, self._h, _p(words)))
        return words

    def init_stride_dev(self, drows_ptr, n):
        _check(lib().pm_vocab_init_stride_dev(self._ctx._h, self._h, C.c_void_p(drows_ptr), n))

    def train_dev(self, drows_ptr, n, iters, dlabels_ptr=0, dinfo_ptr=0):
        """Enqueues `iters` iterations; dlabels_ptr (n int32) and dinfo_ptr (iters x 24 bytes) may be 0."""
        _check(lib().pm_vocab_train_dev(self._ctx._h, self._h, C.c_void_p(drows_ptr), n, iters, C.c_void_p(dlabels_ptr or 0),
                                        C.c_void_p(dinfo_ptr or 0)))

    def train(self, rows, iters):
        """Blocking: (labels int32 (n,), records VOCAB_ITER_DTYPE (iters,)); the words stay in the object (get())."""
        rows = self._rows(rows)
        labels = np.zeros(rows.shape[0], np.int32)
        info = np.zeros(iters, VOCAB_ITER_DTYPE)
        _check(lib().pm_vocab_train(self._ctx._h, self._h, _p(rows), rows.shape[0], iters, _p(labels), _p(info)))
        return labels, info

    def assign_dev(self, drows_ptr, n, dn_ptr=0, dwords_ptr=0, ddist_ptr=0, dhist_ptr=0):
        """Enqueues the encoding of n rows (dn_ptr: device count, 0 = all n); every output pointer may be 0."""
        _check(lib().pm_vocab_assign_dev(self._ctx._h, self._h, C.c_void_p(drows_ptr), n, C.c_void_p(dn_ptr or 0),
                                         C.c_void_p(dwords_ptr or 0), C.c_void_p(ddist_ptr or 0), C.c_void_p(dhist_ptr or 0)))

    def assign(self, rows):
        """Blocking: (words int32 (n,), dist float32 (n,), hist uint32 (K,))."""
        rows = self._rows(rows)
        n = rows.shape[0]
        words, dist, hist = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(self.K, np.uint32)
        _check(lib().pm_vocab_assign(self._ctx._h, self._h, _p(rows), n, _p(words), _p(dist), _p(hist)))
        return words, dist, hist


class BowDb:
    """pm_bowdb: an append-only database of bag-of-words histograms over K words on the device, scored by DBoW2's L1 score
    under per-word weights and queried for its best `top` images (SPEC S107-S112).  Owns its device memory."""

    def __init__(self, ctx, K, max_images, max_entries):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.K, self.max_images, self.max_entries = K, max_images, max_entries
        _check(lib().pm_bowdb_create(ctx._h, K, max_images, max_entries, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pm_bowdb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _hist(self, hist):
        hist = np.ascontiguousarray(hist, np.uint32).reshape(-1)
        if hist.size != self.K:
            raise PmError(PM_E_INVALID, "need %d counts" % self.K)
        return hist

    def clear_dev(self):
        _check(lib().pm_bowdb_clear_dev(self._ctx._h, self._h))

    def add_dev(self, dhist_ptr, did_ptr=0):
        """Enqueues the add of a device histogram (K uint32); did_ptr (one int32: the id, -1 or -2) may be 0."""
        _check(lib().pm_bowdb_add_dev(self._ctx._h, self._h, C.c_void_p(dhist_ptr), C.c_void_p(did_ptr or 0)))

    def add(self, hist):
        """Blocking: the id of the image, -1 (empty or more than 65535 rows) or -2 (full)."""
        hist = self._hist(hist)
        i = C.c_int32(-9)
        _check(lib().pm_bowdb_add(self._ctx._h, self._h, _p(hist), C.byref(i)))
        return i.value

    def set_weights(self, weights):
        _check(lib().pm_bowdb_set_weights(self._ctx._h, self._h, _p(self._hist(weights))))

    def get_weights(self):
        w = np.zeros(self.K, np.uint32)
        _check(lib().pm_bowdb_get_weights(self._ctx._h, self._h, _p(w)))
        return w

    def idf_dev(self):
        _check(lib().pm_bowdb_idf_dev(self._ctx._h, self._h))

    def query_dev(self, dhist_ptr, top, excl_lo=0, excl_hi=0, dids_ptr=0, dscores_ptr=0, dcount_ptr=0, dall_ptr=0):
        """Enqueues a query; dids_ptr (top int32), dscores_ptr (top float64), dcount_ptr (one int32) and dall_ptr (a float64
        per image) may each be 0."""
        _check(lib().pm_bowdb_query_dev(self._ctx._h, self._h, C.c_void_p(dhist_ptr), top, excl_lo, excl_hi, C.c_void_p(dids_ptr or 0),
                                        C.c_void_p(dscores_ptr or 0), C.c_void_p(dcount_ptr or 0), C.c_void_p(dall_ptr or 0)))

    def query(self, hist, top, excl_lo=0, excl_hi=0, all_scores=False):
        """Blocking: (ids int32 (count,), scores float64 (count,)) and, with all_scores, the score of every image."""
        hist = self._hist(hist)
        ids, scores, count = np.zeros(top, np.int32), np.zeros(top, np.float64), C.c_int32(0)
        n_images = self.counts()[0] if all_scores else 0
        every = np.zeros(max(n_images, 1), np.float64) if all_scores else None
        _check(lib().pm_bowdb_query(self._ctx._h, self._h, _p(hist), top, excl_lo, excl_hi, _p(ids), _p(scores), C.byref(count), _p(every)))
        n = count.value
        if all_scores:
            return ids[:n].copy(), scores[:n].copy(), every[:n_images].copy()
        return ids[:n].copy(), scores[:n].copy()

    def counts(self):
        """(images, entries); synchronises."""
        n, e = C.c_int32(), C.c_int32()
        _check(lib().pm_bowdb_get(self._ctx._h, self._h, C.byref(n), C.byref(e), None, None, None, None, None, None))
        return n.value, e.value

    def get(self):
        """The whole database as a dict: n_images, n_entries, offsets (n_images + 1), words, tfs (n_entries), norms (n_images),
        df, weights (K); synchronises."""
        n, e = self.counts()
        d = dict(n_images=n, n_entries=e, offsets=np.zeros(n + 1, np.uint32), words=np.zeros(e, np.uint32), tfs=np.zeros(e, np.uint16),
                 norms=np.zeros(n, np.uint32), df=np.zeros(self.K, np.uint32), weights=np.zeros(self.K, np.uint32))
        _check(lib().pm_bowdb_get(self._ctx._h, self._h, None, None, _p(d["offsets"]), _p(d["words"]), _p(d["tfs"]), _p(d["norms"]),
                                  _p(d["df"]), _p(d["weights"])))
        return d


def _xyz_pair(xyz1, xyz2):
    """3D-3D correspondences as contiguous float32 (n, 3) arrays, and n."""
    xyz1 = np.ascontiguousarray(xyz1, np.float32).reshape(-1, 3)
    xyz2 = np.ascontiguousarray(xyz2, np.float32).reshape(-1, 3)
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("xyz1 and xyz2 must have the same length")
    return xyz1, xyz2, xyz1.shape[0]


def _pnp_pair(xyz, uv):
    """2D-3D correspondences as contiguous float32 (n, 3) and (n, 2) arrays, and n."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    if xyz.shape[0] != uv.shape[0]:
        raise ValueError("xyz and uv must have the same length")
    return xyz, uv, xyz.shape[0]


class LmedsParams(C.Structure):
    _fields_ = [("hyp_begin", C.c_int64), ("hyp_end", C.c_int64), ("seed", C.c_uint64)]


class AdaptiveParams(C.Structure):
    _fields_ = [("max_iters", C.c_int64), ("confidence", C.c_double), ("thresh_px", C.c_float), ("reserved", C.c_int32),
                ("seed", C.c_uint64)]


def ransac7_adaptive(ctx, xy1, xy2, max_iters, confidence, thresh_px, seed):
    """Adaptive-iteration RANSAC over 7-point models (SPEC S16).
    Returns (status, F(3x3), mask, n_inliers, best_model, iters_run)."""
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    n = xy1.shape[0]
    prm = AdaptiveParams(max_iters, confidence, thresh_px, 0, seed)
    F = np.zeros(9, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    ninl, best, it = C.c_int(), C.c_int64(), C.c_int()
    rc = lib().pm_ransac7_adaptive(ctx._h, _p(xy1), _p(xy2), n, C.byref(prm), _p(F), _p(mask), C.byref(ninl),
                                   C.byref(best), C.byref(it))
    if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
        _check(rc)
    return rc, F.reshape(3, 3), mask[:n], ninl.value, best.value, it.value


def lmeds_default_iters(confidence=0.99, outlier_ratio=0.45):
    return lib().pm_lmeds_default_iters(C.c_double(confidence), C.c_double(outlier_ratio))


def lmeds_fundamental(ctx, xy1, xy2, iters, seed, hyp_begin=0):
    """7-point + LMedS (SPEC S13-S15).  Returns (status, F(3x3), mask, n_inliers, best_model, median)."""
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    n = xy1.shape[0]
    prm = LmedsParams(hyp_begin, iters, seed)
    F = np.zeros(9, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    ninl, best, med = C.c_int(), C.c_int64(), C.c_double()
    rc = lib().pm_lmeds_fundamental(ctx._h, _p(xy1), _p(xy2), n, C.byref(prm), _p(F), _p(mask), C.byref(ninl),
                                    C.byref(best), C.byref(med))
    if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
        _check(rc)
    return rc, F.reshape(3, 3), mask[:n], ninl.value, best.value, med.value


# ---- batch of image pairs (BASELINE config C5) ---------------------------------------------------

class PairJob(C.Structure):
    _fields_ = [("desc1", C.c_void_p), ("desc2", C.c_void_p), ("kp1_xy", C.c_void_p), ("kp2_xy", C.c_void_p),
                ("n1", C.c_int32), ("n2", C.c_int32)]


class PairResult(C.Structure):
    _fields_ = [("F", C.c_double * 9), ("best_key", C.c_uint64), ("n_good", C.c_int32), ("n_inliers", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class PairBatch:
    """pm_batch wrapper: `n_lanes` streams, each running whole pairs (H2D -> match -> ratio+gather ->
    RANSAC-F -> D2H).  Jobs are (desc1_ptr, n1, desc2_ptr, n2, kp1_ptr, kp2_ptr) with HOST addresses
    (ideally page-locked: torch pinned tensors, or host_register())."""

    def __init__(self, device, n_lanes, max_n1, max_n2, dim):
        self._h = C.c_void_p()
        self.max_n1, self.dim = max_n1, dim
        _check(lib().pm_batch_create(device, n_lanes, max_n1, max_n2, dim, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pm_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        _check(lib().pm_batch_set_option(self._h, option, value))

    def set_desc_u8(self, on=True):
        """the jobs' desc1 / desc2 point at uint8 rows"""
        _check(lib().pm_batch_set_desc_type(self._h, int(bool(on))))

    def set_host_threads(self, n):
        """0 = automatic (two host threads with >= 4 lanes), 1, 2"""
        _check(lib().pm_batch_set_host_threads(self._h, int(n)))

    @staticmethod
    def make_jobs(jobs):
        arr = (PairJob * len(jobs))()
        for a, (d1, n1, d2, n2, k1, k2) in zip(arr, jobs):
            a.desc1, a.n1, a.desc2, a.n2, a.kp1_xy, a.kp2_xy = d1, n1, d2, n2, k1, k2
        return arr

    def run(self, jobs, ratio, iters, thresh_px, seed, knn_flags=0, kind=PM_ERR_SAMPSON, want_good=False,
            want_masks=False):
        """jobs: list of tuples or a prepared (PairJob * n) array.  Returns (results array, good, masks)."""
        arr = jobs if isinstance(jobs, C.Array) else self.make_jobs(jobs)
        n = len(arr)
        res = (PairResult * n)()
        good = np.zeros((n, self.max_n1), MATCH_DTYPE) if want_good else None
        masks = np.zeros((n, self.max_n1), np.uint8) if want_masks else None
        prm = RansacParams(0, iters, seed, thresh_px, kind)
        _check(lib().pm_batch_run(self._h, arr, n, C.c_float(ratio), knn_flags, C.byref(prm), res,
                                  _p(good) if want_good else None, _p(masks) if want_masks else None))
        return res, good, masks


def host_register(arr):
    _check(lib().pm_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes))


def host_unregister(arr):
    _check(lib().pm_host_unregister(C.c_void_p(arr.ctypes.data)))


# ---- the path over the GPUs of one node (single process, RCCL behind the C ABI) ----------------------

class MultiGpu:
    """pm_mgpu wrapper."""

    def __init__(self, n_dev, devices=None):
        self._h = C.c_void_p()
        arr = (C.c_int * n_dev)(*devices) if devices is not None else None
        _check(lib().pm_mgpu_create(n_dev, arr, C.byref(self._h)))
        self.n = n_dev

    def close(self):
        if self._h:
            lib().pm_mgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ransac_fundamental(self, xy1, xy2, iters, thresh_px, seed, kind=PM_ERR_SAMPSON, hyp_begin=0):
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
        xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        n = xy1.shape[0]
        prm = RansacParams(hyp_begin, iters, seed, thresh_px, kind)
        F = np.zeros(9, np.float64)
        mask = np.zeros(max(n, 1), np.uint8)
        ninl, key = C.c_int(), C.c_uint64()
        rc = lib().pm_mgpu_ransac_fundamental(self._h, _p(xy1), _p(xy2), n, C.byref(prm), _p(F), _p(mask), C.byref(ninl),
                                              C.byref(key))
        if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
            _check(rc)
        return rc, F.reshape(3, 3), mask[:n], ninl.value, key.value

    def match_ransac(self, desc1, desc2, kp1, kp2, ratio, iters, thresh_px, seed, knn_flags=0, kind=PM_ERR_SAMPSON):
        """Returns (status, good, F(3x3), mask, n_inliers, best_key)."""
        binary = desc1.dtype == np.uint8
        desc1 = np.ascontiguousarray(desc1, np.uint8 if binary else np.float32)
        desc2 = np.ascontiguousarray(desc2, desc1.dtype)
        kp1 = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        kp2 = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        n1, dim = desc1.shape
        prm = RansacParams(0, iters, seed, thresh_px, kind)
        good = np.zeros(n1, MATCH_DTYPE)
        F = np.zeros(9, np.float64)
        mask = np.zeros(n1, np.uint8)
        ngood, ninl, key = C.c_int(), C.c_int(), C.c_uint64()
        rc = lib().pm_mgpu_match_ransac(self._h, _p(desc1), n1, _p(desc2), desc2.shape[0], dim, int(binary), _p(kp1), _p(kp2),
                                        C.c_float(ratio), knn_flags, C.byref(prm), _p(good), C.byref(ngood), _p(F), _p(mask),
                                        C.byref(ninl), C.byref(key))
        if rc not in (PM_OK, PM_E_NO_MODEL, PM_E_TOO_FEW):
            _check(rc)
        return rc, good[:ngood.value].copy(), F.reshape(3, 3), mask[:ngood.value].copy(), ninl.value, key.value


    # ---- streamed form: resident train side, device pointers in, tickets out -------------------------------------
    def set_lanes(self, n_lanes):
        _check(lib().pm_mgpu_set_lanes(self._h, n_lanes))

    def set_option(self, option, value):
        _check(lib().pm_mgpu_batch_set_option(self._h, option, value))

    def set_train(self, desc2, kp2):
        binary = desc2.dtype == np.uint8
        desc2 = np.ascontiguousarray(desc2, np.uint8 if binary else np.float32)
        kp2 = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        _check(lib().pm_mgpu_set_train(self._h, _p(desc2), desc2.shape[0], desc2.shape[1], int(binary), _p(kp2)))

    def set_train_dev(self, desc2_ptrs, n2, dim, binary, kp2_ptrs):
        """per-device device pointers (the caller keeps the buffers alive)"""
        a = (C.c_void_p * self.n)(*desc2_ptrs)
        b = (C.c_void_p * self.n)(*kp2_ptrs)
        _check(lib().pm_mgpu_set_train_dev(self._h, a, n2, dim, int(binary), b))

    def submit_dev(self, desc1_ptrs, rows, kp1_ptrs, ratio, iters, thresh_px, seed, knn_flags=0, kind=PM_ERR_SAMPSON):
        a = (C.c_void_p * self.n)(*desc1_ptrs)
        b = (C.c_void_p * self.n)(*kp1_ptrs)
        r = (C.c_int32 * self.n)(*rows)
        prm = RansacParams(0, iters, seed, thresh_px, kind)
        t = C.c_int()
        _check(lib().pm_mgpu_submit_dev(self._h, a, r, b, C.c_float(ratio), knn_flags, C.byref(prm), C.byref(t)))
        return t.value

    def collect(self, ticket, n1=0, want_good=False, want_mask=False):
        """Returns (PairResult, good records or None, mask or None); n1 = total query rows of the pair (buffer sizes)."""
        res = PairResult()
        good = np.zeros(max(n1, 1), MATCH_DTYPE) if want_good else None
        mask = np.zeros(max(n1, 1), np.uint8) if want_mask else None
        _check(lib().pm_mgpu_collect(self._h, ticket, C.byref(res), _p(good) if want_good else None, _p(mask) if want_mask else None))
        ng = max(res.n_good, 0)
        return res, (good[:ng].copy() if want_good else None), (mask[:ng].copy() if want_mask else None)

    def allgather_latency(self, bytes_per_device, reps=200):
        us = C.c_double()
        _check(lib().pm_mgpu_allgather_latency(self._h, bytes_per_device, reps, C.byref(us)))
        return us.value

    def batch_run(self, jobs, n_lanes, max_n1, max_n2, dim, ratio, iters, thresh_px, seed, knn_flags=0, kind=PM_ERR_SAMPSON,
                  want_good=False, want_masks=False):
        """BASELINE config C5 over the devices (pair p -> device p mod n): like PairBatch.run."""
        arr = jobs if isinstance(jobs, C.Array) else PairBatch.make_jobs(jobs)
        n = len(arr)
        res = (PairResult * n)()
        good = np.zeros((n, max_n1), MATCH_DTYPE) if want_good else None
        masks = np.zeros((n, max_n1), np.uint8) if want_masks else None
        prm = RansacParams(0, iters, seed, thresh_px, kind)
        _check(lib().pm_mgpu_batch_run(self._h, n_lanes, max_n1, max_n2, dim, arr, n, C.c_float(ratio), knn_flags, C.byref(prm), res,
                                       _p(good) if want_good else None, _p(masks) if want_masks else None))
        return res, good, masks


# ---- FlannBasedMatcher-compatible approximate matcher (main.cpp:44; SPEC S17) ---------------------------

class FlannParams(C.Structure):
    _fields_ = [("trees", C.c_int32), ("checks", C.c_int32), ("seed", C.c_uint64)]


FLANN_NODE_DTYPE = np.dtype([("child1", "<i4"), ("child2", "<i4"), ("divfeat", "<i4"), ("divval", "<f4")])


class FlannIndex:
    """pm_flann_index wrapper: kd-forest of the train descriptors (built on the host, searched on the GPU)."""

    def __init__(self, ctx, train, trees=4, checks=32, seed=0):
        self._ctx = ctx
        self.train = np.ascontiguousarray(train, np.float32)
        self.trees, self.checks = trees, checks
        self._h = C.c_void_p()
        prm = FlannParams(trees, checks, seed)
        _check(lib().pm_flann_build(ctx._h, _p(self.train), self.train.shape[0], self.train.shape[1], C.byref(prm),
                                    C.byref(self._h)))

    def close(self):
        if self._h:
            lib().pm_flann_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def knn(self, q, k=1):
        q = np.ascontiguousarray(q, np.float32)
        out = np.zeros((q.shape[0], k), MATCH_DTYPE)
        _check(lib().pm_flann_knn_l2_f32(self._ctx._h, self._h, _p(q), q.shape[0], k, _p(out)))
        return out

    def knn_dev(self, dq_ptr, nq, k, dout_ptr):
        _check(lib().pm_flann_knn_l2_f32_dev(self._ctx._h, self._h, C.c_void_p(dq_ptr), nq, k, C.c_void_p(dout_ptr)))

    def export(self):
        """(nodes structured array, roots int32[trees])"""
        n = C.c_int32()
        roots = np.zeros(16, np.int32)
        _check(lib().pm_flann_export(self._h, C.byref(n), _p(roots), None, 0))
        nodes = np.zeros(n.value, FLANN_NODE_DTYPE)
        _check(lib().pm_flann_export(self._h, C.byref(n), _p(roots), _p(nodes), n.value))
        return nodes, roots[:self.trees].copy()
