"""Linear seed and calibration of a multi-camera rig: the reference's ``estimate_extrinsic_dlt``
(include/calib/estimation/linear/extrinsics.h:27-78) on the C ABI (``cba_estimate_extrinsic_dlt``), and the numerical body of
``StereoCalibrationFacade::calibrate`` and ``MultiCameraCalibrationFacade::calibrate`` (src/pipeline/facades/extrinsics.cpp:39-131,
134-229): keep the views every camera sees with at least 4 points, seed with the cameras' K, refine with ``optimize_extrinsics``.

``views[v][c]`` is an (N, 4) array [X, Y, u, v] of view v in camera c, as ``optim.optimize_extrinsics`` takes it.  Poses are 4x4
matrices: c_se3_r maps the reference (camera 0) frame to camera c, r_se3_t the target of view v to the reference.  Reading detection
files and matching image names is not done here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .capi import dptr, i32ptr, i64ptr
from .geometry import quat_to_rotmat
from .optim import ExtrinsicOptimizationResult, ExtrinsicOptions, optimize_extrinsics


@dataclass
class ExtrinsicPoses:  # extrinsics.h:22-25
    c_se3_r: List[np.ndarray] = field(default_factory=list)  # reference -> camera
    r_se3_t: List[np.ndarray] = field(default_factory=list)  # target -> reference


@dataclass
class ExtrinsicDltBlocks:
    """Everything cba_estimate_extrinsic_dlt returns, as pose7 rows [qw, qx, qy, qz, tx, ty, tz]."""
    c_T_r: np.ndarray    # [n_cams][7]
    r_T_t: np.ndarray    # [n_views][7]
    blk_pose: np.ndarray  # [n_blocks][7]: each block's planar pose c_T_t
    blk_ok: np.ndarray    # [n_blocks]: 0 for fewer than 4 points or a failed fit (the pose is then the identity)


@dataclass
class RigCalibrationResult:
    """The numerical part of StereoCalibrationRunResult / MultiCameraCalibrationRunResult."""
    requested_views: int
    used_views: int
    view_status: List[str]  # per requested view: "ok", "missing_image" or "insufficient_points"
    initial_guess: Optional[ExtrinsicPoses]
    optimization: Optional[ExtrinsicOptimizationResult]  # None when no view is used (no solve runs)
    success: bool


def pose7_to_matrix(p) -> np.ndarray:
    """pose7 -> 4x4 without renormalising the quaternion (the seed's quaternions are unit)."""
    p = np.asarray(p, dtype=np.float64).reshape(7)
    T = np.eye(4)
    T[:3, :3] = quat_to_rotmat(p[:4])
    T[:3, 3] = p[4:]
    return T


def _kmtx5(cam) -> np.ndarray:
    c = np.asarray(cam, dtype=np.float64).reshape(-1)
    if c.size < 5:
        raise capi.CbaInvalidArgument(capi.CBA_ERR_INVALID_ARGUMENT, "a camera needs at least [fx, fy, cx, cy, skew]")
    return c[:5]


def estimate_extrinsic_dlt_blocks(n_cams: int, n_views: int, blk_offset, blk_view, blk_cam, X, Y, u, v, kmtx5) -> ExtrinsicDltBlocks:
    """cba_estimate_extrinsic_dlt on the blocked layout of cba_optimize_extrinsics."""
    lib = capi.load_library()
    off = np.ascontiguousarray(blk_offset, dtype=np.int64)
    bv = np.ascontiguousarray(blk_view, dtype=np.int32)
    bc = np.ascontiguousarray(blk_cam, dtype=np.int32)
    cols = [np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, u, v)]
    K = np.ascontiguousarray(np.asarray(kmtx5, dtype=np.float64).reshape(-1, 5))
    nb = len(off) - 1
    cr = np.zeros((max(n_cams, 1), 7))
    rt = np.zeros((max(n_views, 1), 7))
    bp = np.zeros((max(nb, 1), 7))
    ok = np.zeros(max(nb, 1), dtype=np.int32)
    capi.check(lib, lib.cba_estimate_extrinsic_dlt(int(n_cams), int(n_views), nb, i64ptr(off), i32ptr(bv), i32ptr(bc),
                                                   *(dptr(a) for a in cols), dptr(K), dptr(cr), dptr(rt), dptr(bp), i32ptr(ok)))
    return ExtrinsicDltBlocks(cr[:n_cams], rt[:n_views], bp[:nb], ok[:nb])


def _check_views(views, n_cams: int):
    if len(views) == 0 or n_cams == 0:  # extrinsics.h:31-33
        raise capi.CbaError(capi.CBA_ERR_RUNTIME, "Empty views or cameras provided")
    for i, mv in enumerate(views):  # extrinsics.h:42-47
        if len(mv) != n_cams:
            raise capi.CbaError(capi.CBA_ERR_RUNTIME,
                                f"View {i} has wrong number of cameras: expected {n_cams}, got {len(mv)}")


def estimate_extrinsic_dlt(views: Sequence[Sequence[Optional[np.ndarray]]], cameras: Sequence) -> ExtrinsicPoses:
    """estimate_extrinsic_dlt (extrinsics.h:27-78).  ``cameras``: intrinsic vectors (10 or 12) or [fx, fy, cx, cy, skew]; only K is
    read, distortion is ignored as in the reference.  An empty (or None) views[v][c] is an absent block."""
    _check_views(views, len(cameras))
    K = np.stack([_kmtx5(c) for c in cameras])
    off, bv, bc, parts = [0], [], [], []
    for vi, mv in enumerate(views):
        for ci, pv in enumerate(mv):
            a = np.zeros((0, 4)) if pv is None else np.asarray(pv, dtype=np.float64).reshape(-1, 4)
            if a.shape[0] == 0:
                continue
            parts.append(a)
            bv.append(vi)
            bc.append(ci)
            off.append(off[-1] + a.shape[0])
    allp = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4))
    r = estimate_extrinsic_dlt_blocks(len(cameras), len(views), off, bv, bc, *(allp[:, k] for k in range(4)), K)
    return ExtrinsicPoses([pose7_to_matrix(p) for p in r.c_T_r], [pose7_to_matrix(p) for p in r.r_T_t])


def calibrate_rig(views: Sequence[Sequence[Optional[np.ndarray]]], cameras: Sequence, opts: Optional[ExtrinsicOptions] = None,
                  device: int = 0) -> RigCalibrationResult:
    """The numerical body of the stereo (two cameras) and multi-camera facades (extrinsics.cpp:39-131, 134-229).  views[v][c] is None
    when camera c has no image for view v.  A view is used only when every camera sees it with at least 4 points; the used views are
    seeded by estimate_extrinsic_dlt with the cameras' K and refined by optimize_extrinsics from the full ``cameras``."""
    opts = opts or ExtrinsicOptions()
    n_cams = len(cameras)
    status, kept = [], []
    for i, mv in enumerate(views):
        if len(mv) != n_cams:
            raise capi.CbaError(capi.CBA_ERR_RUNTIME,
                                f"View {i} has wrong number of cameras: expected {n_cams}, got {len(mv)}")
        if any(pv is None for pv in mv):
            status.append("missing_image")
            continue
        arrs = [np.asarray(pv, dtype=np.float64).reshape(-1, 4) for pv in mv]
        if any(a.shape[0] < 4 for a in arrs):
            status.append("insufficient_points")
            continue
        status.append("ok")
        kept.append(arrs)
    if not kept:
        return RigCalibrationResult(len(views), 0, status, None, None, False)
    guess = estimate_extrinsic_dlt(kept, cameras)
    res = optimize_extrinsics(kept, [np.asarray(c, dtype=np.float64) for c in cameras], guess.c_se3_r, guess.r_se3_t, opts, device)
    return RigCalibrationResult(len(views), len(kept), status, guess, res, bool(res.core.success))
