"""Linear seed of planar intrinsic calibration: the reference's ``estimate_homography``
(include/calib/estimation/linear/homography.h, src/estimation/optim/homography.cpp:31-60), ``estimate_intrinsics``
(intrinsics.h:56-58, src/estimation/linear/intrinsicsdlt.cpp:101-145), ``zhang_intrinsics_from_hs`` (zhang.cpp),
``pose_from_homography`` (posefromhomography.cpp), ``sanitize_intrinsics`` (common/intrinsics_utils.h) and the numerical
body of ``PlanarIntrinsicCalibrationFacade::calibrate`` (src/pipeline/facades/intrinsics.cpp:86-138), on top of the C ABI
(``cba_estimate_homography_ransac_batch``, ``cba_estimate_intrinsics``, ``cba_zhang_intrinsics_from_hs``,
``cba_pose_from_homography``, ``cba_sanitize_intrinsics``).

A view is an [n][4] array of correspondences [X, Y, u, v] (target plane -> pixels).  A camera matrix is
[fx, fy, cx, cy, skew].  Poses are 4x4 c_T_t matrices.  RANSAC departs from the reference as calibba.h documents: every
hypothesis is scored and the samples come from a counter-based stream, so the same seed draws different samples.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi, optim
from .capi import CbaRansacOptions, dptr, i32ptr, i64ptr, u8ptr
from .linescan import RansacOptions
from .optim import CalibrationBounds, IntrinsicsOptimOptions, IntrinsicsOptimizationResult


@dataclass
class HomographyResult:  # homography.h:15-20
    success: bool = False
    hmtx: np.ndarray = field(default_factory=lambda: np.eye(3))
    inliers: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))
    symmetric_rms_px: float = 0.0


@dataclass
class IntrinsicsEstimOptions:  # intrinsics.h:26-30
    bounds: Optional[CalibrationBounds] = None
    homography_ransac: Optional[RansacOptions] = None
    use_skew: bool = False  # accepted and unused, as in the reference


@dataclass
class ViewEstimateData:  # intrinsics.h:32-38
    view_index: int = 0
    c_se3_t: np.ndarray = field(default_factory=lambda: np.eye(4))  # det R = -1 where the reference's t_z flip leaves it
    homography: HomographyResult = field(default_factory=HomographyResult)
    forward_rms_px: float = 0.0


@dataclass
class IntrinsicsEstimateResult:  # intrinsics.h:47-54
    success: bool = False
    kmtx: np.ndarray = field(default_factory=lambda: np.zeros(5))
    dist: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0, 0.0])
    views: List[ViewEstimateData] = field(default_factory=list)
    log: str = ""


@dataclass
class PoseFromHResult:  # posefromhomography.h
    success: bool = False
    c_se3_t: np.ndarray = field(default_factory=lambda: np.eye(4))
    scale: float = 0.0
    cond_check: float = 0.0


@dataclass
class PlanarIntrinsicsCalibration:
    """The numerical part of IntrinsicCalibrationOutputs (facades/intrinsics.cpp:86-138)."""
    linear_kmtx: np.ndarray
    linear_view_indices: List[int]
    refine_result: IntrinsicsOptimizationResult
    linear: IntrinsicsEstimateResult
    used_views: int


def _ransac_options(r: Optional[RansacOptions]) -> Optional[CbaRansacOptions]:
    if r is None:
        return None
    return CbaRansacOptions(int(r.max_iters), float(r.thresh), int(r.min_inliers), int(bool(r.refit_on_inliers)), float(r.confidence),
                            int(r.seed))


def _flatten(views):
    vs = [np.asarray(v, dtype=np.float64).reshape(-1, 4) for v in views]
    off = np.zeros(len(vs) + 1, dtype=np.int64)
    np.cumsum([v.shape[0] for v in vs], out=off[1:])
    allv = np.concatenate(vs, axis=0) if vs else np.zeros((0, 4))
    return off, [np.ascontiguousarray(allv[:, k]) for k in range(4)]


def estimate_homography_batch(views: Sequence[np.ndarray], ransac_opts: Optional[RansacOptions] = None) -> List[HomographyResult]:
    """estimate_homography (homography.cpp:45-60 with RANSAC options, :31-43 without) of every view in one call.  H is returned as
    the reference returns it: no h22 rescale."""
    lib = capi.load_library()
    off, (X, Y, u, v) = _flatten(views)
    nv = len(views)
    H = np.zeros((max(nv, 1), 9))
    ok = np.zeros(max(nv, 1), dtype=np.int32)
    cnt = np.zeros(max(nv, 1), dtype=np.int32)
    rms = np.zeros(max(nv, 1))
    mask = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
    o = _ransac_options(ransac_opts)
    capi.check(lib, lib.cba_estimate_homography_ransac_batch(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v),
                                                             None if o is None else C.byref(o), dptr(H), i32ptr(ok), i32ptr(cnt),
                                                             dptr(rms), u8ptr(mask)))
    out = []
    for i in range(nv):
        m = mask[off[i]:off[i + 1]]
        out.append(HomographyResult(bool(ok[i]), H[i].reshape(3, 3).copy(), np.flatnonzero(m).astype(np.int64) if ok[i] else
                                    np.zeros(0, dtype=np.int64), float(rms[i])))
    return out


def estimate_homography(view: np.ndarray, ransac_opts: Optional[RansacOptions] = None) -> HomographyResult:
    """estimate_homography (homography.h:22-24) of one view."""
    return estimate_homography_batch([view], ransac_opts)[0]


def _bounds(b: Optional[CalibrationBounds]):
    if b is None:
        return None, None
    lo = np.array([b.fx_min, b.fy_min, b.cx_min, b.cy_min, b.skew_min], dtype=np.float64)
    hi = np.array([b.fx_max, b.fy_max, b.cx_max, b.cy_max, b.skew_max], dtype=np.float64)
    return lo, hi


def estimate_intrinsics(views: Sequence[np.ndarray], opts: Optional[IntrinsicsEstimOptions] = None) -> IntrinsicsEstimateResult:
    """estimate_intrinsics (intrinsicsdlt.cpp:101-145) as one device pipeline.  ``views`` of the result holds the views whose
    homography succeeded, in input order, each with its ``view_index``, exactly as the reference returns them."""
    opts = opts or IntrinsicsEstimOptions()
    lib = capi.load_library()
    off, (X, Y, u, v) = _flatten(views)
    nv = len(views)
    n = max(nv, 1)
    ok, pok = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    H, rms, poses = np.zeros((n, 9)), np.zeros(n), np.zeros((n, 12))
    mask = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
    K = np.zeros(5)
    success, sanitized = C.c_int32(0), C.c_int32(0)
    o = _ransac_options(opts.homography_ransac)
    lo, hi = _bounds(opts.bounds)
    capi.check(lib, lib.cba_estimate_intrinsics(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v), int(o is not None),
                                                None if o is None else C.byref(o), dptr(lo), dptr(hi), int(bool(opts.use_skew)),
                                                C.byref(success), dptr(K), C.byref(sanitized), i32ptr(ok), dptr(H), dptr(rms), dptr(poses),
                                                i32ptr(pok), u8ptr(mask)))
    res = IntrinsicsEstimateResult()
    if not success.value:
        return res
    res.success = True
    res.kmtx = K.copy()
    if sanitized.value:
        res.log = "Intrinsics sanitized by bounds."
    for i in range(nv):
        if not ok[i]:
            continue
        hres = HomographyResult(True, H[i].reshape(3, 3).copy(), np.flatnonzero(mask[off[i]:off[i + 1]]).astype(np.int64), float(rms[i]))
        pose = _rt12_to_matrix(poses[i]) if pok[i] else np.eye(4)
        res.views.append(ViewEstimateData(i, pose, hres, float(rms[i])))
    return res


def _rt12_to_matrix(rt) -> np.ndarray:
    m = np.eye(4)
    m[:3, :3] = np.asarray(rt[:9]).reshape(3, 3)
    m[:3, 3] = rt[9:12]
    return m


def _h9(h) -> np.ndarray:
    m = h.hmtx if isinstance(h, HomographyResult) else h
    return np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(9))


def zhang_intrinsics_from_hs(hs) -> Optional[np.ndarray]:
    """zhang_intrinsics_from_hs (zhang.cpp:174-206): [fx, fy, cx, cy, skew], or None where the reference returns nullopt.
    ``hs``: HomographyResult objects or 3x3 matrices."""
    lib = capi.load_library()
    h9 = np.ascontiguousarray(np.stack([_h9(h) for h in hs])) if len(hs) else np.zeros((1, 9))
    K = np.zeros(5)
    ok = C.c_int32(0)
    capi.check(lib, lib.cba_zhang_intrinsics_from_hs(len(hs), dptr(h9), dptr(K), C.byref(ok)))
    return K if ok.value else None


def pose_from_homography(kmtx, hmtx) -> PoseFromHResult:
    """pose_from_homography (posefromhomography.cpp:11-62) with K = [fx, fy, cx, cy, skew]."""
    lib = capi.load_library()
    K = np.ascontiguousarray(np.asarray(kmtx, dtype=np.float64).reshape(-1)[:5])
    H = _h9(hmtx)
    p = np.zeros(12)
    ok = C.c_int32(0)
    s, c = C.c_double(0.0), C.c_double(0.0)
    capi.check(lib, lib.cba_pose_from_homography(dptr(K), dptr(H), dptr(p), C.byref(ok), C.byref(s), C.byref(c)))
    return PoseFromHResult(bool(ok.value), _rt12_to_matrix(p) if ok.value else np.eye(4), s.value, c.value)


def sanitize_intrinsics(kmtx, bounds: Optional[CalibrationBounds]) -> Tuple[np.ndarray, bool]:
    """sanitize_intrinsics (common/intrinsics_utils.h): (K, modified); no bounds keeps K."""
    K = np.asarray(kmtx, dtype=np.float64).reshape(-1)[:5].copy()
    if bounds is None:
        return K, False
    lib = capi.load_library()
    lo, hi = _bounds(bounds)
    out = np.zeros(5)
    mod = C.c_int32(0)
    capi.check(lib, lib.cba_sanitize_intrinsics(dptr(np.ascontiguousarray(K)), dptr(lo), dptr(hi), dptr(out), C.byref(mod)))
    return out, bool(mod.value)


def calibrate_planar_intrinsics(views: Sequence[np.ndarray], opts: Optional[IntrinsicsEstimOptions] = None,
                                optim_options: Optional[IntrinsicsOptimOptions] = None, refine: bool = True) -> PlanarIntrinsicsCalibration:
    """The numerical body of PlanarIntrinsicCalibrationFacade::calibrate (facades/intrinsics.cpp:86-138): estimate_intrinsics,
    per-view estimate_planar_pose seeds at the linear K (cba_estimate_planar_pose_batch), optimize_intrinsics of a pinhole +
    Brown-Conrady camera from zero distortion; the linear K when the refinement does not converge."""
    if len(views) < 4:
        raise RuntimeError(f"Need at least 4 views. Only {len(views)} usable views.")
    linear = estimate_intrinsics(views, opts)
    if not linear.success:
        raise RuntimeError("Linear intrinsic estimation failed to converge.")
    K = np.asarray(linear.kmtx, dtype=np.float64)
    init_camera = np.r_[K, np.zeros(5)]
    if refine:
        seeds = optim.estimate_planar_pose_batch(views, K)
        res = optim.optimize_intrinsics(views, init_camera, seeds, optim_options)
        if not res.core.success:
            res.camera = init_camera.copy()
    else:
        res = IntrinsicsOptimizationResult(optim.OptimResult(success=True), init_camera.copy(), [])
    return PlanarIntrinsicsCalibration(K.copy(), [v.view_index for v in linear.views], res, linear, len(views))
