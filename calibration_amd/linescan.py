"""Laser-plane calibration of a line-scan rig: the reference's ``calibrate_laser_plane``
(include/calib/estimation/linear/linescan.h:39-144), ``fit_plane_svd`` / ``fit_plane_ransac`` (planefit.cpp),
``invert_brown_conrady`` (distortion.h:165-195) and ``LinescanCalibrationFacade`` (src/pipeline/linescan.cpp), on top of
the C ABI (``cba_calibrate_laser_plane``, ``cba_fit_plane``, ``cba_invert_brown_conrady``).

A camera is its parameter vector: 10 entries [fx, fy, cx, cy, skew, k1, k2, k3, p1, p2] (pinhole + Brown-Conrady) or 12
(+ tau_x, tau_y: Scheimpflug).  ``inverse_coeffs`` selects DualDistortion's one-step undistortion ([k1..k_nr, p1, p2] of
the inverse model); without it, undistortion is BrownConrady's 5-step fixed point.  A view is a ``LineScanView``: its
target correspondences [X, Y, u, v] and its laser pixels [u, v].  Planes are [nx, ny, nz, d] with n.p + d = 0 and the
sign convention of calibba.h (d > 0).

Laser profile scanning, which the reference does not have (``cba_laser_points``, ``cba_laser_scanner``): ``laser_points`` puts
caller pixels on the calibrated plane, ``LaserScanner`` turns frames into sub-pixel line centres and 3D profiles.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import capi
from .capi import CbaLaserPlaneResult, CbaLaserScanOptions, CbaPlaneFitOptions, dptr, i64ptr, u8ptr


# cba_calibrate_laser_plane's message when fewer than 3 points survive (linescan.h:113-115)
NOT_ENOUGH_POINTS = "Not enough laser points to fit a plane"


@dataclass
class RansacOptions:  # ransac.h:23-30
    max_iters: int = 1000
    thresh: float = 2.0
    min_inliers: int = 12
    confidence: float = 0.99  # accepted, unused: every hypothesis is scored
    seed: int = 1234567
    refit_on_inliers: bool = True


@dataclass
class LineScanPlaneFitOptions:  # linescan.h:30-33
    use_ransac: bool = False
    ransac_options: RansacOptions = field(default_factory=RansacOptions)


@dataclass
class LineScanView:
    target_view: np.ndarray  # [n][4] = X, Y, u, v
    laser_uv: np.ndarray     # [m][2]


@dataclass
class LineScanCalibrationResult:
    plane: np.ndarray
    homography: np.ndarray
    rms_error: float
    inlier_count: int
    summary: str
    n_points: int
    n_views_used: int
    covariance: np.ndarray = field(default_factory=lambda: np.zeros((3, 3)))
    points: Optional[np.ndarray] = None       # [n_laser][3], NaN rows for views whose homography failed
    inlier_mask: Optional[np.ndarray] = None  # [n_laser] bool


@dataclass
class PlaneRansacResult:  # planefit.h
    success: bool
    plane: np.ndarray
    inliers: np.ndarray
    inlier_rms: float


def _options(opts: Optional[LineScanPlaneFitOptions]) -> CbaPlaneFitOptions:
    opts = opts or LineScanPlaneFitOptions()
    r = opts.ransac_options
    return CbaPlaneFitOptions(int(bool(opts.use_ransac)), int(r.max_iters), float(r.thresh), int(r.min_inliers), int(bool(r.refit_on_inliers)),
                              float(r.confidence), int(r.seed))


def _camera(camera, inverse_coeffs):
    intr = np.ascontiguousarray(np.asarray(camera, dtype=np.float64).reshape(-1))
    if intr.size == 10:
        model = capi.CAMERA_PINHOLE_BC
    elif intr.size == 12:
        model = capi.CAMERA_SCHEIMPFLUG
    else:
        raise ValueError(f"camera parameter vector must have 10 or 12 entries, got {intr.size}")
    inv = None if inverse_coeffs is None else np.ascontiguousarray(np.asarray(inverse_coeffs, dtype=np.float64).reshape(-1))
    return model, intr, inv


def _flatten(views: Sequence[LineScanView]):
    tv = [np.asarray(v.target_view, dtype=np.float64).reshape(-1, 4) for v in views]
    lv = [np.asarray(v.laser_uv, dtype=np.float64).reshape(-1, 2) for v in views]
    toff = np.zeros(len(views) + 1, dtype=np.int64)
    loff = np.zeros(len(views) + 1, dtype=np.int64)
    np.cumsum([t.shape[0] for t in tv], out=toff[1:])
    np.cumsum([t.shape[0] for t in lv], out=loff[1:])
    T = np.concatenate(tv, axis=0) if tv else np.zeros((0, 4))
    L = np.concatenate(lv, axis=0) if lv else np.zeros((0, 2))
    cols = [np.ascontiguousarray(T[:, k]) for k in range(4)] + [np.ascontiguousarray(L[:, k]) for k in range(2)]
    return toff, loff, cols


def calibrate_laser_plane(views: Sequence[LineScanView], camera, opts: Optional[LineScanPlaneFitOptions] = None, inverse_coeffs=None,
                          return_points: bool = False, return_mask: bool = False) -> LineScanCalibrationResult:
    """calibrate_laser_plane (linescan.h:101-144) on the GPU.  Raises CbaInvalidArgument where the reference throws
    std::invalid_argument and CbaError (CBA_ERR_RUNTIME) where RANSAC fails."""
    lib = capi.load_library()
    model, intr, inv = _camera(camera, inverse_coeffs)
    toff, loff, (X, Y, u, v, lu, lv) = _flatten(views)
    n_l = int(loff[-1])
    pts = np.empty((max(n_l, 1), 3)) if return_points else None
    mask = np.empty(max(n_l, 1), dtype=np.uint8) if return_mask else None
    o = _options(opts)
    res = CbaLaserPlaneResult()
    capi.check(lib, lib.cba_calibrate_laser_plane(model, dptr(intr), 0 if inv is None else int(inv.size), dptr(inv), len(views), i64ptr(toff),
                                                  dptr(X), dptr(Y), dptr(u), dptr(v), i64ptr(loff), dptr(lu), dptr(lv), C.byref(o),
                                                  C.byref(res), dptr(pts), u8ptr(mask)))
    return LineScanCalibrationResult(
        plane=np.array(res.plane[:]), homography=np.array(res.homography[:]).reshape(3, 3), rms_error=float(res.rms_error),
        inlier_count=int(res.inlier_count), summary=res.summary.decode(), n_points=int(res.n_points), n_views_used=int(res.n_views_used),
        points=None if pts is None else pts[:n_l], inlier_mask=None if mask is None else mask[:n_l].astype(bool))


def points_from_view(view: LineScanView, camera, inverse_coeffs=None) -> np.ndarray:
    """points_from_view (linescan.h:63-91): the camera-frame points of one view's laser pixels; an empty [0][3] array when
    the view's homography fails.  Runs through cba_calibrate_laser_plane (which needs two views and three points): the view
    is paired with a copy of itself whose laser pixels are its target pixels."""
    tv = np.asarray(view.target_view, dtype=np.float64).reshape(-1, 4)
    lu = np.asarray(view.laser_uv, dtype=np.float64).reshape(-1, 2)
    if tv.shape[0] < 4:
        raise capi.CbaInvalidArgument(capi.CBA_ERR_INVALID_ARGUMENT, "Each view requires >=4 target correspondences")
    helper = LineScanView(tv, tv[:, 2:4])
    try:
        r = calibrate_laser_plane([view, helper], camera, inverse_coeffs=inverse_coeffs, return_points=True)
    except capi.CbaInvalidArgument as e:
        if e.message != NOT_ENOUGH_POINTS:
            raise
        return np.zeros((0, 3))  # no point from either copy: the homography failed
    if r.n_views_used == 0:
        return np.zeros((0, 3))
    return r.points[: lu.shape[0]].copy()


def _fit(points, opts: CbaPlaneFitOptions, want_mask: bool):
    lib = capi.load_library()
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    plane = np.zeros(4)
    rms = C.c_double(0.0)
    cnt = C.c_int64(0)
    mask = np.empty(max(p.shape[0], 1), dtype=np.uint8) if want_mask else None
    capi.check(lib, lib.cba_fit_plane(p.shape[0], dptr(p), C.byref(opts), dptr(plane), C.byref(rms), C.byref(cnt), u8ptr(mask)))
    return plane, rms.value, cnt.value, None if mask is None else mask[: p.shape[0]].astype(bool)


def fit_plane_svd(points) -> np.ndarray:
    """fit_plane_svd (planefit.cpp:68-85) on the GPU."""
    return _fit(points, _options(LineScanPlaneFitOptions(use_ransac=False)), False)[0]


def plane_rms(points, plane) -> float:
    """plane_rms (linescan.h:93-99), host arithmetic."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r = p @ np.asarray(plane[:3]) + plane[3]
    return float(np.sqrt(np.mean(r * r)))


def fit_plane_ransac(points, opts: Optional[RansacOptions] = None) -> PlaneRansacResult:
    """fit_plane_ransac (planefit.cpp:87-114) on the GPU.  success = False where the reference returns an unsuccessful result."""
    n = np.asarray(points).reshape(-1, 3).shape[0]
    if n < 3:
        return PlaneRansacResult(False, np.zeros(4), np.zeros(0, dtype=np.int64), float("inf"))
    try:
        plane, rms, _, mask = _fit(points, _options(LineScanPlaneFitOptions(True, opts or RansacOptions())), True)
    except capi.CbaError as e:
        if e.status != capi.CBA_ERR_RUNTIME:
            raise
        return PlaneRansacResult(False, np.zeros(4), np.zeros(0, dtype=np.int64), float("inf"))
    return PlaneRansacResult(True, plane, np.flatnonzero(mask), rms)


def invert_brown_conrady(forward) -> np.ndarray:
    """invert_brown_conrady (distortion.h:165-195): host-only, needs no GPU."""
    lib = capi.load_library()
    f = np.ascontiguousarray(np.asarray(forward, dtype=np.float64).reshape(-1))
    out = np.zeros(max(f.size, 1))
    capi.check(lib, lib.cba_invert_brown_conrady(int(f.size), dptr(f), dptr(out)))
    return out[: f.size]


@dataclass
class LinescanCalibrationRunResult:  # src/pipeline/linescan.cpp
    success: bool
    used_views: int
    result: Optional[LineScanCalibrationResult]


class LinescanCalibrationFacade:
    """LinescanCalibrationFacade::calibrate (src/pipeline/linescan.cpp): the pinhole + Brown-Conrady camera becomes a
    DualDistortion camera (invert_brown_conrady), then calibrate_laser_plane; any failure gives success = False."""

    def calibrate(self, camera, views: Sequence[LineScanView], opts: Optional[LineScanPlaneFitOptions] = None) -> LinescanCalibrationRunResult:
        intr = np.asarray(camera, dtype=np.float64).reshape(-1)
        if intr.size != 10:
            raise ValueError("the facade takes a pinhole + Brown-Conrady camera (10 parameters)")
        try:
            res = calibrate_laser_plane(views, intr, opts, inverse_coeffs=invert_brown_conrady(intr[5:10]))
            return LinescanCalibrationRunResult(True, len(views), res)
        except capi.CbaError:
            return LinescanCalibrationRunResult(False, len(views), None)


# ---- laser profile scanning (cba_laser_points, cba_laser_scanner; no counterpart in the reference) ----------------------------------
@dataclass
class LaserScanOptions:
    """``cba_laser_scan_options``: axis 0 = one peak per column (1: per row); the ROI [roi_begin, roi_end) along the search direction
    (0, 0: the whole side); the half window of the centre of gravity; the floor subtracted from the samples; the least valid peak."""
    axis: int = 0
    roi_begin: int = 0
    roi_end: int = 0
    half_window: int = 5
    floor_level: float = 0.0
    min_peak: float = 1.0


@dataclass
class LaserProfiles:
    centre: np.ndarray     # [n_frames][n_lines] sub-pixel line position, NaN for an invalid line
    amplitude: np.ndarray  # [n_frames][n_lines] the line's maximum
    width_px: np.ndarray   # [n_frames][n_lines] equivalent width sum g / (m - floor)
    xyz: np.ndarray        # [n_frames][n_lines][3] points on the laser plane (moved by the frame poses when given)


def _plane(plane) -> np.ndarray:
    if isinstance(plane, LineScanCalibrationResult):
        plane = plane.plane
    p = np.ascontiguousarray(np.asarray(plane, dtype=np.float64).reshape(-1))
    if p.size != 4:
        raise ValueError(f"a plane has 4 entries [nx, ny, nz, d], got {p.size}")
    return p


def _frame_poses(frame_poses, n_frames: int) -> np.ndarray:
    from .geometry import poses_from_matrices

    p = np.asarray(frame_poses, dtype=np.float64)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        p = poses_from_matrices(p)
    if p.ndim != 2 or p.shape != (n_frames, 7):
        raise ValueError(f"frame_poses must be {n_frames} 4x4 matrices or pose7 rows, got shape {p.shape}")
    return np.ascontiguousarray(p)


def laser_points(uv, camera, plane, frame_offset=None, frame_poses=None, inverse_coeffs=None, want_plane_xy: bool = False):
    """Pixels uv [n][2] -> points [n][3] on the laser plane (camera frame), by the rule of calibba.h.  plane: [nx, ny, nz, d] or a
    LineScanCalibrationResult.  frame_offset [n_frames + 1] and frame_poses ([n_frames][7] pose7 rows or 4x4 matrices) move each
    frame's points by its pose; frame_poses alone is one pose for all pixels.  With want_plane_xy the result is (xyz, plane_xy): the
    in-plane coordinates the calibration's homography promises."""
    lib = capi.load_library()
    model, intr, inv = _camera(camera, inverse_coeffs)
    pl = _plane(plane)
    px = np.asarray(uv, dtype=np.float64)
    if px.ndim != 2 or px.shape[1] != 2:
        raise ValueError(f"uv must have shape [n][2], got {px.shape}")
    px = np.ascontiguousarray(px)
    n = px.shape[0]
    off, n_frames = None, 0
    if frame_offset is not None:
        off = np.ascontiguousarray(np.asarray(frame_offset, dtype=np.int64).reshape(-1))
        if off.size < 1:
            raise ValueError("frame_offset needs n_frames + 1 entries")
        n_frames = off.size - 1
    poses = None
    if frame_poses is not None:
        if off is None:
            n_frames = 1
            frame_poses = np.asarray(frame_poses, dtype=np.float64)
            if frame_poses.shape in ((7,), (4, 4)):
                frame_poses = frame_poses[None]
        poses = _frame_poses(frame_poses, n_frames)
    xyz = np.empty((n, 3))
    pxy = np.empty((n, 2)) if want_plane_xy else None
    capi.check(lib, lib.cba_laser_points(model, dptr(intr), 0 if inv is None else int(inv.size), dptr(inv), dptr(pl), n, dptr(px), n_frames,
                                         i64ptr(off), dptr(poses), dptr(xyz), dptr(pxy)))
    return (xyz, pxy) if want_plane_xy else xyz


class LaserScanner(capi.Handle):
    """``cba_laser_scanner``: frames of one size in, laser profiles out, one kernel launch per ``process``.  The device buffers are
    sized for max_frames at construction.  Use as a context manager or call ``close()``."""

    _DESTROY = "cba_laser_scanner_destroy"

    def __init__(self, camera, plane, width: int, height: int, max_frames: int = 1, opts: Optional[LaserScanOptions] = None,
                 inverse_coeffs=None, device: int = 0):
        out = self._out()
        model, intr, inv = _camera(camera, inverse_coeffs)
        pl = _plane(plane)
        o = opts or LaserScanOptions()
        co = CbaLaserScanOptions(int(o.axis), int(o.roi_begin), int(o.roi_end), int(o.half_window), float(o.floor_level), float(o.min_peak))
        self.width, self.height, self.max_frames, self.axis = int(width), int(height), int(max_frames), int(o.axis)
        self.n_lines = self.width if self.axis == 0 else self.height
        capi.check(self._lib, self._lib.cba_laser_scanner_create(model, dptr(intr), 0 if inv is None else int(inv.size), dptr(inv), dptr(pl),
                                                                 self.width, self.height, self.max_frames, C.byref(co), int(device), out))

    def process(self, images, frame_poses=None) -> LaserProfiles:
        """images: [n_frames][height][width] (or one [height][width] frame), uint8 or float32; C-contiguous arrays of those types are
        used as they are.  frame_poses: one pose per frame (pose7 rows or 4x4 matrices)."""
        h = self._require_open("the scanner is closed")
        img = np.asarray(images)
        if img.dtype not in (np.uint8, np.float32):
            raise ValueError(f"images must be uint8 or float32, got {img.dtype}")
        if img.ndim == 2:
            img = img[None]
        if img.ndim != 3 or img.shape[1:] != (self.height, self.width):
            raise ValueError(f"images must have shape [n_frames][{self.height}][{self.width}], got {img.shape}")
        img = np.ascontiguousarray(img)
        n_frames = img.shape[0]
        poses = None if frame_poses is None else _frame_poses(frame_poses, n_frames)
        shape = (n_frames, self.n_lines)
        centre, amplitude, width_px, xyz = np.empty(shape), np.empty(shape), np.empty(shape), np.empty(shape + (3,))
        dtype = capi.DTYPE_U8 if img.dtype == np.uint8 else capi.DTYPE_F32
        capi.check(self._lib, self._lib.cba_laser_scanner_process(h, n_frames, dtype, img.ctypes.data_as(C.c_void_p), dptr(poses),
                                                                  dptr(centre), dptr(amplitude), dptr(width_px), dptr(xyz)))
        return LaserProfiles(centre, amplitude, width_px, xyz)
