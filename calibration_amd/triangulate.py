"""Multi-camera triangulation on the GPU (``cba_triangulate``): matched pixels of several calibrated cameras -> 3D points in the
reference frame, by the ray seed and the Levenberg-Marquardt refinement through the full camera model that calibba.h states.

The cameras and poses are what a rig calibration returns: ``RigCalibrationResult.optimization.cameras`` / ``.c_se3_r`` (4x4
matrices) or the pose7 rows of ``ExtrinsicDltBlocks.c_T_r`` pass straight in.  The reference has no triangulation.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi
from .capi import CbaTriangulateOptions, dptr, i32ptr
from .geometry import poses_from_matrices
from .linescan import _camera


@dataclass
class TriangulateOptions:
    """``cba_triangulate_options``: LM steps after the seed, the relative step that ends the iteration, the cameras a point needs
    (never fewer than 2) and the per-camera pixel error above which the worst camera is dropped (inf: off)."""
    max_iterations: int = 10
    step_tolerance: float = 1e-12
    min_cams: int = 2
    max_reproj_px: float = float("inf")


@dataclass
class TriangulationResult:
    xyz: np.ndarray      # [n][3], reference frame; NaN rows where status is TRI_DEGENERATE or TRI_TOO_FEW
    rms_px: np.ndarray   # [n]: sqrt(sum over the used cameras of (e_u^2 + e_v^2) / n_used)
    used: np.ndarray     # bool [n][n_cams]
    status: np.ndarray   # int32 [n]: capi.TRI_OK, TRI_NOT_CONVERGED, TRI_BEHIND, TRI_DEGENERATE, TRI_TOO_FEW
    cov: Optional[np.ndarray] = None  # [n][3][3] = (J^T J)^-1 at the solution (unit pixel sigma), with covariance=True


def _pose7_rows(c_se3_r, n_cams: int) -> np.ndarray:
    p = np.asarray(c_se3_r, dtype=np.float64)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        p = poses_from_matrices(p)
    if p.ndim != 2 or p.shape != (n_cams, 7):
        raise ValueError(f"c_se3_r must be {n_cams} 4x4 matrices or pose7 rows, got shape {p.shape}")
    return np.ascontiguousarray(p)


def triangulate(cameras, c_se3_r, uv, inverse_coeffs=None, opts: Optional[TriangulateOptions] = None,
                covariance: bool = False) -> TriangulationResult:
    """Triangulate n points seen by the cameras of a calibrated rig.

    cameras: n_cams parameter vectors of one model (10: pinhole + Brown-Conrady, 12: Scheimpflug); c_se3_r: the reference -> camera
    poses, as [n_cams][4][4] matrices or [n_cams][7] pose7 rows; uv: pixels [n_cams][n][2], NaN where a camera did not see a point;
    inverse_coeffs: optional [n_cams][m] DualDistortion inverses for the seed's unprojection (None: the 5-step fixed point)."""
    lib = capi.load_library()
    parsed = [_camera(c, None) for c in cameras]
    n_cams = len(parsed)
    if n_cams == 0 or any(p[0] != parsed[0][0] for p in parsed):
        raise ValueError("triangulate needs cameras of one model")
    model = parsed[0][0]
    intr = np.ascontiguousarray(np.stack([p[1] for p in parsed]))
    poses = _pose7_rows(c_se3_r, n_cams)
    px = np.asarray(uv, dtype=np.float64)
    if px.ndim != 3 or px.shape[0] != n_cams or px.shape[2] != 2:
        raise ValueError(f"uv must have shape [{n_cams}][n][2], got {px.shape}")
    px = np.ascontiguousarray(px)
    n = px.shape[1]
    inv, n_inv = None, 0
    if inverse_coeffs is not None:
        inv = np.ascontiguousarray(np.asarray(inverse_coeffs, dtype=np.float64).reshape(n_cams, -1))
        n_inv = inv.shape[1]
    o = opts or TriangulateOptions()
    co = CbaTriangulateOptions(int(o.max_iterations), float(o.step_tolerance), int(o.min_cams), float(o.max_reproj_px))
    xyz = np.empty((n, 3))
    rms = np.empty(n)
    mask = np.empty(n, dtype=np.uint32)
    status = np.empty(n, dtype=np.int32)
    cov6 = np.empty((n, 6)) if covariance else None
    capi.check(lib, lib.cba_triangulate(model, n_cams, dptr(intr), n_inv, dptr(inv), dptr(poses), n, dptr(px), C.byref(co), dptr(xyz),
                                        dptr(rms), mask.ctypes.data_as(capi.c_uint32_p), i32ptr(status), dptr(cov6)))
    used = ((mask[:, None] >> np.arange(n_cams, dtype=np.uint32)[None, :]) & 1).astype(bool)
    cov = None
    if covariance:
        idx = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
        cov = cov6[:, idx]
    return TriangulationResult(xyz, rms, used, status, cov)
