"""ctypes binding of ``include/calibba.h`` (libcalibba.so).

This is the only place the shared library is loaded.  Loading fails loudly when the library has
not been built (``python -c 'import __graft_entry__ as g; g.build()'``); compute calls fail loudly
(``CbaError`` with ``CBA_ERR_NO_DEVICE``) when no GPU is visible.  Nothing here falls back to a CPU
implementation.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

CBA_OK, CBA_ERR_INVALID_ARGUMENT, CBA_ERR_RUNTIME, CBA_ERR_NO_DEVICE, CBA_ERR_HIP, CBA_ERR_INTERNAL = range(6)
CHAIN_INTRINSIC, CHAIN_EXTRINSIC, CHAIN_BUNDLE = 0, 1, 2
# cba_estimate_bundle_seed: per-camera status, initial-target source (calibba.h)
HANDEYE_DLT, HANDEYE_GIVEN, HANDEYE_TOO_FEW_VIEWS, HANDEYE_NO_PAIRS, HANDEYE_SINGULAR = range(5)
TARGET_ESTIMATED, TARGET_CONFIG, TARGET_IDENTITY = range(3)
# cba_estimate_intrinsics_linear(_iterative)_batch: per-problem status (calibba.h)
LINEAR_OK, LINEAR_TOO_FEW, LINEAR_DEGENERATE = range(3)
LINEAR_MAX_ITERATIONS = 65536
CAMERA_PINHOLE_BC, CAMERA_SCHEIMPFLUG = 0, 1
# cba_undistort_map_apply: image element types (calibba.h)
DTYPE_U8, DTYPE_F32 = 0, 1
IMAGE_MAX_SIDE = 32768
# cba_triangulate: per-point status (calibba.h)
TRI_OK, TRI_NOT_CONVERGED, TRI_BEHIND, TRI_DEGENERATE, TRI_TOO_FEW = range(5)
TRI_MAX_CAMS = 16
TERM_CONVERGENCE, TERM_NO_CONVERGENCE, TERM_FAILURE = 0, 1, 2
RCCL_UNIQUE_ID_BYTES = 128

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_uint8_p = C.POINTER(C.c_uint8)
c_uint32_p = C.POINTER(C.c_uint32)


class CbaOptions(C.Structure):
    """``cba_options`` — OptimOptions (optimize.h:24-33) + per-stage switches."""

    _fields_ = [
        ("optimizer", C.c_int32),
        ("max_iterations", C.c_int32),
        ("huber_delta", C.c_double),
        ("epsilon", C.c_double),
        ("compute_covariance", C.c_int32),
        ("verbose", C.c_int32),
        ("optimize_intrinsics", C.c_int32),
        ("optimize_skew", C.c_int32),
        ("optimize_extrinsics", C.c_int32),
        ("optimize_target_pose", C.c_int32),
    ]


class CbaSummary(C.Structure):
    """``cba_summary`` — OptimResult (optimize.h:35-40) without the covariance matrix."""

    _fields_ = [
        ("success", C.c_int32),
        ("termination", C.c_int32),
        ("iterations", C.c_int32),
        ("successful_steps", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("solve_seconds", C.c_double),
        ("report", C.c_char * 192),
    ]


class CbaReprojProblem(C.Structure):
    """``cba_reproj_problem`` — one reprojection bundle problem in SoA form."""

    _fields_ = [
        ("chain", C.c_int32),
        ("camera_model", C.c_int32),
        ("n_blocks", C.c_int32),
        ("n_cams", C.c_int32),
        ("n_views", C.c_int32),
        ("reserved0", C.c_int32),
        ("first_view_global", C.c_int64),
        ("blk_offset", c_int64_p),
        ("blk_cam", c_int32_p),
        ("blk_view", c_int32_p),
        ("blk_b_T_g", c_double_p),
        ("X", c_double_p),
        ("Y", c_double_p),
        ("u", c_double_p),
        ("v", c_double_p),
        ("intr", c_double_p),
        ("cam_pose", c_double_p),
        ("view_pose", c_double_p),
        ("target_pose", c_double_p),
    ]


class CbaPlaneFitOptions(C.Structure):
    """``cba_plane_fit_options`` — LineScanPlaneFitOptions (linescan.h:30-33) with RansacOptions (ransac.h:23-30) inlined."""

    _fields_ = [
        ("use_ransac", C.c_int32),
        ("max_iters", C.c_int32),
        ("thresh", C.c_double),
        ("min_inliers", C.c_int32),
        ("refit_on_inliers", C.c_int32),
        ("confidence", C.c_double),
        ("seed", C.c_uint64),
    ]


class CbaRansacOptions(C.Structure):
    """``cba_ransac_options`` — RansacOptions (ransac.h:23-30)."""

    _fields_ = [
        ("max_iters", C.c_int32),
        ("thresh", C.c_double),
        ("min_inliers", C.c_int32),
        ("refit_on_inliers", C.c_int32),
        ("confidence", C.c_double),
        ("seed", C.c_uint64),
    ]


class CbaLaserPlaneResult(C.Structure):
    """``cba_laser_plane_result`` — LineScanCalibrationResult (linescan.h) without the (zero) covariance."""

    _fields_ = [
        ("plane", C.c_double * 4),
        ("homography", C.c_double * 9),
        ("rms_error", C.c_double),
        ("inlier_count", C.c_int64),
        ("n_points", C.c_int64),
        ("n_views_used", C.c_int32),
        ("iters", C.c_int32),
        ("summary", C.c_char * 16),
    ]


class CbaTriangulateOptions(C.Structure):
    """``cba_triangulate_options`` (calibba.h)."""

    _fields_ = [
        ("max_iterations", C.c_int32),
        ("step_tolerance", C.c_double),
        ("min_cams", C.c_int32),
        ("max_reproj_px", C.c_double),
    ]


class CbaLaserScanOptions(C.Structure):
    """``cba_laser_scan_options`` (calibba.h)."""

    _fields_ = [
        ("axis", C.c_int32),
        ("roi_begin", C.c_int32),
        ("roi_end", C.c_int32),
        ("half_window", C.c_int32),
        ("floor_level", C.c_double),
        ("min_peak", C.c_double),
    ]


class CbaSlOptions(C.Structure):
    """``cba_sl_options`` (calibba.h)."""

    _fields_ = [
        ("proj_width", C.c_int32),
        ("proj_height", C.c_int32),
        ("axes", C.c_int32),
        ("gray_skip_bits", C.c_int32),
        ("phase_steps", C.c_int32),
        ("phase_period", C.c_int32),
        ("min_contrast", C.c_int32),
        ("min_bit_diff", C.c_int32),
        ("min_modulation", C.c_double),
    ]


class CbaIcpOptions(C.Structure):
    """``cba_icp_options`` (calibba.h)."""

    _fields_ = [
        ("metric", C.c_int32),
        ("max_distance", C.c_double),
        ("max_iterations", C.c_int32),
        ("step_tolerance", C.c_double),
        ("min_pairs", C.c_int32),
    ]


class CbaIcpResult(C.Structure):
    """``cba_icp_result`` (calibba.h)."""

    _fields_ = [
        ("pose7", C.c_double * 7),
        ("rms", C.c_double),
        ("H", C.c_double * 36),
        ("g", C.c_double * 6),
        ("n_pairs", C.c_int64),
        ("iterations", C.c_int32),
        ("status", C.c_int32),
    ]


ICP_OK, ICP_NOT_CONVERGED, ICP_TOO_FEW, ICP_DEGENERATE = 0, 1, 2, 3
CLOUD_MAX_CELLS = 1 << 24
ALIGN_MAX_SCANS, ALIGN_MAX_EDGES = 64, 1024


class CbaAlignOptions(C.Structure):
    """``cba_align_options`` (calibba.h)."""

    _fields_ = [("icp", CbaIcpOptions), ("fixed", C.c_int32)]


class CbaAlignEdge(C.Structure):
    """``cba_align_edge`` (calibba.h)."""

    _fields_ = [
        ("H", C.c_double * 36),
        ("g", C.c_double * 6),
        ("ss", C.c_double),
        ("n_pairs", C.c_int64),
        ("used", C.c_int32),
    ]


class CbaAlignResult(C.Structure):
    """``cba_align_result`` (calibba.h)."""

    _fields_ = [
        ("rms", C.c_double),
        ("n_pairs", C.c_int64),
        ("n_used_edges", C.c_int32),
        ("iterations", C.c_int32),
        ("status", C.c_int32),
    ]


class CbaTsdfOptions(C.Structure):
    """``cba_tsdf_options`` (calibba.h)."""

    _fields_ = [("voxel_size", C.c_double), ("truncation", C.c_double), ("max_weight", C.c_double), ("max_depth", C.c_double)]


TSDF_MAX_VOXELS = 1 << 28


class CbaTsdfRaycastOptions(C.Structure):
    """``cba_tsdf_raycast_options`` (calibba.h)."""

    _fields_ = [("step", C.c_double), ("skip", C.c_double), ("near_depth", C.c_double), ("far_depth", C.c_double), ("min_weight", C.c_double)]


TSDF_MAX_RAYS = 1 << 26
TSDF_RAY_MAX_SAMPLES = 65536
TSDF_RAY_MISS, TSDF_RAY_HIT, TSDF_RAY_BEHIND, TSDF_RAY_NO_RAY = 0, 1, 2, 3


class CbaStereoRectifyOptions(C.Structure):
    """``cba_stereo_rectify_options`` (calibba.h)."""

    _fields_ = [("focal", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class CbaStereoMatchOptions(C.Structure):
    """``cba_stereo_match_options`` (calibba.h)."""

    _fields_ = [
        ("min_disparity", C.c_int32),
        ("num_disparities", C.c_int32),
        ("half_window", C.c_int32),
        ("uniqueness_percent", C.c_int32),
        ("lr_max_diff", C.c_int32),
        ("subpixel", C.c_int32),
    ]


class CbaSgmOptions(C.Structure):
    """``cba_sgm_options`` (calibba.h)."""

    _fields_ = [
        ("min_disparity", C.c_int32),
        ("num_disparities", C.c_int32),
        ("p1", C.c_int32),
        ("p2", C.c_int32),
        ("paths", C.c_int32),
        ("uniqueness_percent", C.c_int32),
        ("lr_max_diff", C.c_int32),
        ("subpixel", C.c_int32),
        ("workspace_mb", C.c_int32),
    ]


class CbaDisparityFilterOptions(C.Structure):
    """``cba_disparity_filter_options`` (calibba.h)."""

    _fields_ = [("median_half", C.c_int32), ("speckle_max_size", C.c_int32), ("speckle_max_diff", C.c_double)]


class CbaStereoGeometry(C.Structure):
    """``cba_stereo_geometry`` (calibba.h)."""

    _fields_ = [("focal", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("baseline", C.c_double)]


class CbaCornerOptions(C.Structure):
    """``cba_corner_options`` (calibba.h)."""

    _fields_ = [
        ("min_response", C.c_int32),
        ("nms_radius", C.c_int32),
        ("cog_radius", C.c_int32),
        ("refine", C.c_int32),
        ("refine_half_window", C.c_int32),
        ("refine_iterations", C.c_int32),
    ]


class CbaBlobOptions(C.Structure):
    """``cba_blob_options`` (calibba.h)."""

    _fields_ = [
        ("polarity", C.c_int32),
        ("inner_half", C.c_int32),
        ("outer_half", C.c_int32),
        ("min_contrast", C.c_int32),
        ("nms_radius", C.c_int32),
        ("max_radius", C.c_int32),
        ("rounds", C.c_int32),
        ("reserved", C.c_int32),
        ("max_fit_error", C.c_double),
        ("max_axis_ratio", C.c_double),
        ("min_radius", C.c_double),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, c_double_p, C.c_int64, C.c_void_p)


class CbaError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libcalibba status {status}: {message}")
        self.status = status
        self.message = message


class CbaInvalidArgument(CbaError, ValueError):
    """Maps the reference's std::invalid_argument."""


def dptr(a: Optional[np.ndarray]):
    if a is None:
        return C.cast(None, c_double_p)
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def i32ptr(a: Optional[np.ndarray]):
    if a is None:
        return C.cast(None, c_int32_p)
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_int32_p)


def u8ptr(a: Optional[np.ndarray]):
    if a is None:
        return C.cast(None, c_uint8_p)
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_uint8_p)


def i64ptr(a: Optional[np.ndarray]):
    if a is None:
        return C.cast(None, c_int64_p)
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_int64_p)


def library_path() -> str:
    return os.environ.get("CALIBBA_LIBRARY", os.path.join(_HERE, "lib", "libcalibba.so"))


_LIB = None

# name -> (restype, argtypes); every symbol include/calibba.h declares
PROTOTYPES = {
    "cba_version": (C.c_char_p, []),
    "cba_last_error": (C.c_char_p, []),
    "cba_device_count": (C.c_int32, []),
    "cba_trim_cache": (None, []),
    "cba_set_device": (C.c_int32, [C.c_int32]),
    "cba_get_device": (C.c_int32, []),
    "cba_options_default": (None, [C.POINTER(CbaOptions)]),
    "cba_intrinsics_size": (C.c_int32, [C.c_int32]),
    "cba_local_columns": (C.c_int32, [C.c_int32, C.c_int32]),
    "cba_pose_from_matrix": (None, [c_double_p, c_double_p]),
    "cba_pose_to_matrix": (None, [c_double_p, c_double_p]),
    "cba_reproj_create": (C.c_int32, [C.POINTER(CbaReprojProblem), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_reproj_create_aos": (C.c_int32, [C.POINTER(CbaReprojProblem), C.POINTER(c_double_p), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_reproj_destroy": (None, [C.c_void_p]),
    "cba_reproj_set_params": (C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "cba_reproj_get_params": (C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "cba_reproj_num_observations": (C.c_int64, [C.c_void_p]),
    "cba_reproj_eval": (C.c_int32, [C.c_void_p]),
    "cba_reproj_eval_fetch": (C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    "cba_reproj_eval_fetch_blocks": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_double_p, c_double_p]),
    "cba_reproj_eval_timed": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_double_p]),
    "cba_reproj_normal_eq_timed": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_double_p]),
    "cba_reproj_set_scalar": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cba_reproj_eval_fetch_f32": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cba_reproj_cost": (C.c_int32, [C.c_void_p, C.c_double, c_double_p]),
    "cba_reproj_residual_stats": (C.c_int32, [C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "cba_reproj_residuals_fetch_blocks": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, c_double_p, c_uint8_p]),
    "cba_reproj_residual_stats_timed": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, c_double_p]),
    "cba_reproj_block_normal_eq": (C.c_int32, [C.c_void_p, c_double_p]),
    "cba_reproj_block_normal_eq_size": (C.c_int64, [C.c_void_p]),
    "cba_reproj_solve": (C.c_int32, [C.c_void_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary)]),
    "cba_reproj_set_lm_mode": (C.c_int32, [C.c_void_p, C.c_int32]),
    "cba_reproj_solve_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64)]),
    "cba_reproj_covariance_dim": (C.c_int64, [C.c_void_p]),
    "cba_reproj_covariance": (C.c_int32, [C.c_void_p, C.POINTER(CbaOptions), c_double_p]),
    "cba_reproj_covariance_shared_dim": (C.c_int64, [C.c_void_p]),
    "cba_reproj_covariance_shared": (C.c_int32, [C.c_void_p, C.POINTER(CbaOptions), c_double_p]),
    "cba_reproj_covariance_views": (C.c_int32, [C.c_void_p, C.POINTER(CbaOptions), C.c_int32, c_int32_p, c_double_p]),
    "cba_reproj_set_allreduce": (C.c_int32, [C.c_void_p, ALLREDUCE_FN, C.c_void_p, C.c_int32, C.c_int32]),
    "cba_rccl_unique_id": (C.c_int32, [C.POINTER(C.c_uint8)]),
    "cba_reproj_init_rccl": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]),
    "cba_optimize_intrinsics": (
        C.c_int32,
        [C.c_int32, C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
         C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p],
    ),
    "cba_optimize_extrinsics": (
        C.c_int32,
        [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int64_p, c_int32_p, c_int32_p, c_double_p, c_double_p,
         c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary),
         c_double_p],
    ),
    "cba_optimize_bundle": (
        C.c_int32,
        [C.c_int32, C.c_int32, C.c_int32, c_int64_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
         c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p],
    ),
    "cba_optimize_planar_pose": (
        C.c_int32,
        [C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, c_double_p, C.POINTER(CbaOptions),
         C.POINTER(CbaSummary), c_double_p, c_double_p, c_double_p],
    ),
    "cba_optimize_planar_pose_batch": (
        C.c_int32,
        [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, c_double_p,
         C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p, c_double_p, c_double_p],
    ),
    "cba_optimize_homography": (
        C.c_int32,
        [C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary),
         c_double_p],
    ),
    "cba_optimize_homography_batch": (
        C.c_int32,
        [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(CbaOptions),
         C.POINTER(CbaSummary), c_double_p],
    ),
    "cba_optimize_intrinsics_semidlt": (
        C.c_int32,
        [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, c_double_p, c_double_p,
         c_int32_p, c_double_p, C.c_int32, C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p, c_double_p, c_double_p],
    ),
    "cba_optimize_intrinsics_semidlt_sharded": (
        C.c_int32,
        [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32, c_double_p, c_double_p, C.c_int32,
         c_double_p, c_double_p, c_int32_p, c_double_p, C.c_int32, C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p, c_double_p,
         c_double_p, ALLREDUCE_FN, C.c_void_p, C.c_int32, C.c_int32, C.c_int32],
    ),
    "cba_optimize_intrinsics_semidlt_rccl": (
        C.c_int32,
        [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32, c_double_p, c_double_p, C.c_int32,
         c_double_p, c_double_p, c_int32_p, c_double_p, C.c_int32, C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p, c_double_p,
         c_double_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32],
    ),
    "cba_estimate_homography_batch": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "cba_estimate_planar_pose_batch": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "cba_estimate_handeye_dlt": (C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_double, c_double_p]),
    "cba_estimate_and_optimize_handeye": (
        C.c_int32,
        [C.c_int32, c_double_p, c_double_p, C.c_double, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p],
    ),
    "cba_estimate_and_optimize_handeye_sharded": (
        C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_double, C.c_int32, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary),
                    c_double_p, ALLREDUCE_FN, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "cba_estimate_and_optimize_handeye_rccl": (
        C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_double, C.c_int32, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary),
                    c_double_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32]),
    "cba_optimize_handeye": (
        C.c_int32,
        [C.c_int32, c_double_p, c_double_p, c_double_p, C.POINTER(CbaOptions), C.POINTER(CbaSummary), c_double_p],
    ),
    "cba_plane_fit_options_default": (None, [C.POINTER(CbaPlaneFitOptions)]),
    "cba_calibrate_laser_plane": (
        C.c_int32,
        [C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int64_p,
         c_double_p, c_double_p, C.POINTER(CbaPlaneFitOptions), C.POINTER(CbaLaserPlaneResult), c_double_p, c_uint8_p],
    ),
    "cba_fit_plane": (
        C.c_int32, [C.c_int64, c_double_p, C.POINTER(CbaPlaneFitOptions), c_double_p, c_double_p, c_int64_p, c_uint8_p]),
    "cba_invert_brown_conrady": (C.c_int32, [C.c_int32, c_double_p, c_double_p]),
    "cba_ransac_options_default": (None, [C.POINTER(CbaRansacOptions)]),
    "cba_estimate_homography_ransac_batch": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(CbaRansacOptions), c_double_p,
                    c_int32_p, c_int32_p, c_double_p, c_uint8_p]),
    "cba_estimate_intrinsics": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.POINTER(CbaRansacOptions),
                    c_double_p, c_double_p, C.c_int32, c_int32_p, c_double_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p,
                    c_int32_p, c_uint8_p]),
    "cba_zhang_intrinsics_from_hs": (C.c_int32, [C.c_int32, c_double_p, c_double_p, c_int32_p]),
    "cba_pose_from_homography": (C.c_int32, [c_double_p, c_double_p, c_double_p, c_int32_p, c_double_p, c_double_p]),
    "cba_sanitize_intrinsics": (C.c_int32, [c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "cba_estimate_extrinsic_dlt": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, c_int64_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p,
                    c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "cba_estimate_bundle_seed": (
        C.c_int32, [C.c_int32, C.c_int32, c_int64_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                    C.c_double, c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_int32_p, c_double_p, c_int32_p, c_double_p,
                    c_int32_p]),
    "cba_fit_distortion_batch": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32, c_int32_p,
                    c_double_p, C.c_int32, c_double_p, c_double_p, c_int32_p, c_double_p]),
    "cba_estimate_intrinsics_linear_batch": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, c_double_p,
                    c_int32_p, c_int32_p]),
    "cba_estimate_intrinsics_linear_iterative_batch": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p,
                    c_double_p, c_int32_p, c_int32_p, c_int32_p]),
    "cba_camera_project": (C.c_int32, [C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p]),
    "cba_camera_unproject": (C.c_int32, [C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int64, c_double_p, c_double_p]),
    "cba_undistort_map_create": (
        C.c_int32, [C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_undistort_map_fetch": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cba_undistort_map_apply": (
        C.c_int32, [C.c_void_p, C.c_int32, c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "cba_undistort_map_destroy": (None, [C.c_void_p]),
    "cba_triangulate_options_default": (None, [C.POINTER(CbaTriangulateOptions)]),
    "cba_triangulate": (
        C.c_int32, [C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p, C.c_int64, c_double_p,
                    C.POINTER(CbaTriangulateOptions), c_double_p, c_double_p, c_uint32_p, c_int32_p, c_double_p]),
    "cba_laser_scan_options_default": (None, [C.POINTER(CbaLaserScanOptions)]),
    "cba_laser_points": (
        C.c_int32, [C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p, C.c_int64, c_double_p, C.c_int32, c_int64_p, c_double_p,
                    c_double_p, c_double_p]),
    "cba_laser_scanner_create": (
        C.c_int32, [C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p, C.c_int32, C.c_int32, C.c_int32,
                    C.POINTER(CbaLaserScanOptions), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_laser_scanner_process": (
        C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "cba_laser_scanner_destroy": (None, [C.c_void_p]),
    "cba_sl_options_default": (None, [C.POINTER(CbaSlOptions)]),
    "cba_sl_image_count": (C.c_int32, [C.POINTER(CbaSlOptions), c_int32_p]),
    "cba_sl_patterns": (C.c_int32, [C.POINTER(CbaSlOptions), c_uint8_p]),
    "cba_sl_decoder_create": (C.c_int32, [C.POINTER(CbaSlOptions), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_sl_decoder_set_rig": (
        C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p, C.POINTER(CbaTriangulateOptions)]),
    "cba_sl_decoder_process": (
        C.c_int32, [C.c_void_p, C.c_int32, c_uint8_p, c_double_p, c_double_p, c_uint8_p, c_double_p, c_double_p, c_int32_p]),
    "cba_sl_decoder_destroy": (None, [C.c_void_p]),
    "cba_point_normals": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, C.c_double, c_double_p]),
    "cba_cloud_index_create": (C.c_int32, [C.c_int64, c_double_p, c_double_p, C.c_double, C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_cloud_nearest": (C.c_int32, [C.c_void_p, C.c_int64, c_double_p, C.c_double, c_int64_p, c_double_p]),
    "cba_icp_options_default": (None, [C.POINTER(CbaIcpOptions)]),
    "cba_cloud_register": (
        C.c_int32, [C.c_void_p, C.c_int32, c_int64_p, c_double_p, c_double_p, C.POINTER(CbaIcpOptions), C.POINTER(CbaIcpResult)]),
    "cba_cloud_index_destroy": (None, [C.c_void_p]),
    "cba_cloud_set_create": (
        C.c_int32, [C.c_int32, c_int64_p, c_double_p, c_double_p, C.c_double, C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_align_options_default": (None, [C.POINTER(CbaAlignOptions)]),
    "cba_cloud_align": (
        C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), c_double_p, C.POINTER(CbaAlignOptions), c_double_p,
                    C.POINTER(CbaAlignEdge), C.POINTER(CbaAlignResult)]),
    "cba_cloud_set_destroy": (None, [C.c_void_p]),
    "cba_tsdf_options_default": (None, [C.POINTER(CbaTsdfOptions)]),
    "cba_tsdf_volume_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, c_double_p, C.POINTER(CbaTsdfOptions), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_tsdf_integrate": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p]),
    "cba_tsdf_fetch": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cba_tsdf_upload": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cba_tsdf_reset": (C.c_int32, [C.c_void_p]),
    "cba_tsdf_extract": (C.c_int32, [C.c_void_p, C.c_double, c_int64_p]),
    "cba_tsdf_extract_fetch": (C.c_int32, [C.c_void_p, c_double_p, c_double_p]),
    "cba_tsdf_mesh": (C.c_int32, [C.c_void_p, C.c_double, c_int64_p, c_int64_p]),
    "cba_tsdf_mesh_fetch": (C.c_int32, [C.c_void_p, c_int32_p]),
    "cba_tsdf_raycast_options_default": (None, [C.POINTER(CbaTsdfRaycastOptions)]),
    "cba_tsdf_raycast": (
        C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, C.POINTER(CbaTsdfRaycastOptions)]),
    "cba_tsdf_raycast_fetch": (C.c_int32, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_uint8_p, c_double_p]),
    "cba_tsdf_integrate_colour": (
        C.c_int32, [C.c_void_p, C.c_int32, c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_uint8_p, c_double_p]),
    "cba_tsdf_has_colour": (C.c_int32, [C.c_void_p, c_int32_p]),
    "cba_tsdf_colour_fetch": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float)]),
    "cba_tsdf_colour_upload": (C.c_int32, [C.c_void_p, C.POINTER(C.c_float)]),
    "cba_tsdf_extract_fetch_colour": (C.c_int32, [C.c_void_p, c_uint8_p]),
    "cba_tsdf_raycast_fetch_colour": (C.c_int32, [C.c_void_p, c_uint8_p]),
    "cba_tsdf_volume_destroy": (None, [C.c_void_p]),
    "cba_stereo_match_options_default": (None, [C.POINTER(CbaStereoMatchOptions)]),
    "cba_stereo_rectify": (
        C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_int32, C.c_int32, C.POINTER(CbaStereoRectifyOptions), c_double_p, c_double_p,
                    c_double_p, c_double_p]),
    "cba_stereo_matcher_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CbaStereoMatchOptions), C.POINTER(CbaStereoGeometry), c_double_p, C.c_int32,
                    C.POINTER(C.c_void_p)]),
    "cba_stereo_matcher_process": (
        C.c_int32, [C.c_void_p, C.c_int32, c_uint8_p, c_uint8_p, C.POINTER(C.c_float), c_int32_p, C.POINTER(C.c_float)]),
    "cba_stereo_matcher_destroy": (None, [C.c_void_p]),
    "cba_stereo_points": (C.c_int32, [C.POINTER(CbaStereoGeometry), c_double_p, C.c_int64, c_double_p, c_double_p]),
    "cba_sgm_options_default": (None, [C.POINTER(CbaSgmOptions)]),
    "cba_sgm_matcher_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CbaSgmOptions), C.POINTER(CbaStereoGeometry), c_double_p, C.c_int32,
                    C.POINTER(C.c_void_p)]),
    "cba_sgm_matcher_process": (
        C.c_int32, [C.c_void_p, C.c_int32, c_uint8_p, c_uint8_p, C.POINTER(C.c_float), c_int32_p, C.POINTER(C.c_float)]),
    "cba_sgm_matcher_destroy": (None, [C.c_void_p]),
    "cba_disparity_filter_options_default": (None, [C.POINTER(CbaDisparityFilterOptions)]),
    "cba_disparity_filter_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CbaDisparityFilterOptions), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_disparity_filter_process": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), c_int64_p]),
    "cba_disparity_filter_destroy": (None, [C.c_void_p]),
    "cba_stereo_matcher_set_filter": (C.c_int32, [C.c_void_p, C.POINTER(CbaDisparityFilterOptions)]),
    "cba_sgm_matcher_set_filter": (C.c_int32, [C.c_void_p, C.POINTER(CbaDisparityFilterOptions)]),
    "cba_corner_options_default": (None, [C.POINTER(CbaCornerOptions)]),
    "cba_corner_detector_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(CbaCornerOptions), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_corner_detector_process": (
        C.c_int32, [C.c_void_p, C.c_int32, c_uint8_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_int32_p, c_int32_p]),
    "cba_corner_detector_destroy": (None, [C.c_void_p]),
    "cba_chessboard_order": (C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_int32, C.c_int32, c_int32_p]),
    "cba_blob_options_default": (None, [C.POINTER(CbaBlobOptions)]),
    "cba_blob_detector_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(CbaBlobOptions), C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_blob_detector_process": (
        C.c_int32, [C.c_void_p, C.c_int32, c_uint8_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p, c_int32_p]),
    "cba_blob_detector_destroy": (None, [C.c_void_p]),
    "cba_circle_grid_order": (
        C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
}


def bind(lib, prototypes=None):
    for name, (res, args) in (prototypes or PROTOTYPES).items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library(path: Optional[str] = None):
    """Load libcalibba.so and bind every symbol of calibba.h.  Raises if it is not built."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or library_path()
    # PyTorch-ROCm wheels bundle their own libamdhip64 / librccl / libhsa-runtime64 (same SONAMEs as the
    # system ROCm libraries libcalibba.so links).  If libcalibba is loaded first and torch later, glibc maps
    # BOTH copies (torch asks for the unversioned file names) and the process ends up with two HIP runtimes.
    # Importing torch first makes libcalibba bind to the copies torch already mapped: one HIP runtime, and
    # the same RCCL that torch.distributed's "nccl" backend uses.
    try:
        import torch  # noqa: F401
    except ImportError:  # a host without PyTorch: the system ROCm libraries are used
        pass
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
            "calibration_amd has no CPU fallback."
        )
    lib = bind(C.CDLL(p, mode=C.RTLD_GLOBAL))
    if path is None:
        _LIB = lib
    return lib


def check(lib, status: int):
    if status == CBA_OK:
        return
    msg = lib.cba_last_error()
    msg = msg.decode("utf-8", "replace") if msg else ""
    if status == CBA_ERR_INVALID_ARGUMENT:
        raise CbaInvalidArgument(status, msg)
    raise CbaError(status, msg)


class Handle:
    """The life cycle of a library handle: ``_lib``, ``_h`` (a ``c_void_p`` a create call fills through ``_out()``; None when none is
    open) and ``_DESTROY``, the name of the function that frees it.  A subclass whose create call raised closes cleanly."""

    _DESTROY = ""
    _h = None

    def _out(self, lib=None):
        """binds the library (default: load_library()); the byref argument of the create call"""
        self._lib = lib or load_library()
        self._h = C.c_void_p()
        return C.byref(self._h)

    def _require_open(self, message: str):
        if not self._h:
            raise ValueError(message)
        return self._h

    def close(self):
        if self._h:
            getattr(self._lib, self._DESTROY)(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def u8_batch(a, name: str, height: int, width: int, n_name: str = "n", max_n: Optional[int] = None, count_message: str = "") -> np.ndarray:
    """A batch of uint8 images [n][height][width] (one [height][width] image is promoted) as a contiguous array.  n_name: how the
    messages call the first dimension.  With max_n: n <= max_n, else ValueError(count_message.format(n)); the matchers compare their
    two batches first and check the count themselves."""
    img = np.asarray(a)
    if img.dtype != np.uint8:
        raise ValueError(f"{name} must be uint8, got {img.dtype}")
    if img.ndim == 2:
        img = img[None]
    if img.ndim != 3 or img.shape[1:] != (height, width):
        raise ValueError(f"{name} must have shape [{n_name}][{height}][{width}], got {img.shape}")
    if max_n is not None and img.shape[0] > max_n:
        raise ValueError(count_message.format(img.shape[0]))
    return np.ascontiguousarray(img)


def default_options(lib=None) -> CbaOptions:
    o = CbaOptions()
    (lib or load_library()).cba_options_default(C.byref(o))
    return o


# ---- ChArUco boards (cba_charuco_detector, cba_marker_dictionary_generate, cba_chessboard_lattice, cba_charuco_match) -------------
class CbaCharucoBoard(C.Structure):
    """``cba_charuco_board`` (calibba.h)."""

    _fields_ = [
        ("squares_x", C.c_int32),
        ("squares_y", C.c_int32),
        ("marker_bits", C.c_int32),
        ("n_markers", C.c_int32),
        ("square", C.c_double),
        ("marker_ratio", C.c_double),
    ]


class CbaCharucoOptions(C.Structure):
    """``cba_charuco_options`` (calibba.h)."""

    _fields_ = [
        ("arm_lengths", C.c_double * 2),
        ("arm_offset", C.c_double),
        ("arm_fan_deg", C.c_double),
        ("min_arm_contrast", C.c_double),
        ("min_marker_contrast", C.c_double),
        ("min_component", C.c_int32),
        ("cell_samples", C.c_int32),
        ("max_border_errors", C.c_int32),
        ("max_correction", C.c_int32),
        ("min_markers", C.c_int32),
        ("reserved", C.c_int32),
    ]


# ``cba_marker_reading`` as a numpy record
MARKER_READING = np.dtype([("code", np.uint64), ("level_min", np.float64), ("level_max", np.float64), ("flags", np.int32), ("id", np.int32),
                           ("rotation", np.int32), ("distance", np.int32), ("second_distance", np.int32), ("border_errors", np.int32)])
assert MARKER_READING.itemsize == 48
c_uint64_p = C.POINTER(C.c_uint64)


def u64ptr(a: Optional[np.ndarray]):
    if a is None:
        return C.cast(None, c_uint64_p)
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_uint64_p)


def recptr(a: Optional[np.ndarray]):
    """a MARKER_READING array as ``cba_marker_reading*``"""
    if a is None:
        return C.c_void_p(None)
    assert a.dtype == MARKER_READING and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


PROTOTYPES.update({
    "cba_charuco_options_default": (None, [C.POINTER(CbaCharucoOptions)]),
    "cba_charuco_detector_create": (
        C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(CbaCornerOptions), C.POINTER(CbaCharucoOptions),
                    C.POINTER(CbaCharucoBoard), c_uint64_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "cba_charuco_detector_process": (
        C.c_int32, [C.c_void_p, C.c_int32, c_uint8_p, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p,
                    C.c_void_p]),
    "cba_charuco_detector_arms": (C.c_int32, [C.c_void_p, C.c_int32, c_double_p, c_double_p]),
    "cba_charuco_detector_read": (C.c_int32, [C.c_void_p, C.c_int32, c_int32_p, c_double_p, C.c_void_p]),
    "cba_charuco_detector_destroy": (None, [C.c_void_p]),
    "cba_marker_dictionary_generate": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, c_uint64_p, c_int32_p]),
    "cba_chessboard_lattice": (C.c_int32, [C.c_int32, c_double_p, c_double_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p]),
    "cba_charuco_match": (
        C.c_int32, [C.POINTER(CbaCharucoBoard), C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_double_p, C.c_int32, c_int32_p, c_int32_p,
                    c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_int32_p]),
})
