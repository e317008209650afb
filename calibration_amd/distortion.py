"""Distortion fits and the linear intrinsic estimators on the C ABI: the reference's ``fit_distortion_full``, ``fit_distortion``
and ``fit_distortion_dual`` (include/calib/models/distortion.h:229-406) and ``estimate_intrinsics_linear`` /
``estimate_intrinsics_linear_iterative`` (src/estimation/linear/intrinsicsdlt.cpp:289-368).

Observations are an (N, 4) array [x, y, u, v]: x, y normalised and undistorted, u, v pixels (the reference's Observation).
K is [fx, fy, cx, cy, skew]; coefficients are [k1 .. k_nr, p1, p2].  The batch wrappers take the flat SoA layout of the C ABI;
the reference-shaped functions return None where the reference returns nullopt.  Departures are listed in calibba.h.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi
from .capi import dptr, i32ptr, i64ptr
from .optim import CalibrationBounds


@dataclass
class DistortionWithResiduals:
    distortion: np.ndarray  # [nr + 2]
    residuals: np.ndarray   # [2 N]: design * alpha - rhs


@dataclass
class DualDistortionWithResiduals:
    forward: np.ndarray
    inverse: np.ndarray
    residuals: np.ndarray   # the forward fit's


@dataclass
class PinholeBrownConrady:
    kmtx: np.ndarray        # [fx, fy, cx, cy, skew]
    distortion: np.ndarray  # [k1 .. k_nr, p1, p2]


@dataclass
class FitBatch:
    coeffs: np.ndarray               # [P][m]
    inverse: Optional[np.ndarray]    # [P][m] (dual)
    ok: np.ndarray                   # [P]
    residuals: Optional[np.ndarray]  # [2 N]


@dataclass
class LinearBatch:
    kmtx: np.ndarray        # [P][5]
    status: np.ndarray      # [P]: capi.LINEAR_*
    fallback: np.ndarray    # [P]


@dataclass
class IterativeBatch:
    kmtx: np.ndarray        # [P][5]
    coeffs: np.ndarray      # [P][m]
    status: np.ndarray      # [P]: capi.LINEAR_*
    iterations: np.ndarray  # [P]: K refits adopted
    fallback: np.ndarray    # [P]: fits of K that took the bounds fallback


def _soa(offset, x, y, u, v):
    off = np.ascontiguousarray(offset, dtype=np.int64)
    cols = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, u, v)]
    return off, cols


def fit_distortion_batch(offset, x, y, u, v, kmtx5, num_radial=2, fixed_indices: Sequence[int] = (),
                         fixed_values: Optional[Sequence[float]] = None, dual=False, want_residuals=True, lib=None) -> FitBatch:
    """cba_fit_distortion_batch: problem p owns observations [offset[p], offset[p+1])."""
    lib = lib or capi.load_library()
    off, (x, y, u, v) = _soa(offset, x, y, u, v)
    P = off.size - 1
    m = int(num_radial) + 2
    K = np.ascontiguousarray(np.asarray(kmtx5, dtype=np.float64).reshape(P, 5))
    fi = np.ascontiguousarray(fixed_indices, dtype=np.int32).reshape(-1)
    fv = None if fixed_values is None else np.ascontiguousarray(fixed_values, dtype=np.float64).reshape(-1)
    if fv is not None and fv.size != fi.size:
        raise ValueError("fixed_values must have one entry per fixed index (or be None)")
    co = np.zeros((max(P, 0), m))
    inv = np.zeros((max(P, 0), m)) if dual else None
    ok = np.zeros(max(P, 0), np.int32)
    res = np.zeros(2 * int(off[-1]) if off.size else 0) if want_residuals else None
    capi.check(lib, lib.cba_fit_distortion_batch(P, i64ptr(off), dptr(x), dptr(y), dptr(u), dptr(v), dptr(K), int(num_radial),
                                                 int(fi.size), i32ptr(fi if fi.size else None), dptr(fv if fv is not None and fv.size else None),
                                                 1 if dual else 0, dptr(co), dptr(inv), i32ptr(ok), dptr(res)))
    return FitBatch(co, inv, ok, res)


def _bounds5(bounds: Optional[CalibrationBounds]):
    if bounds is None:
        return None, None
    lo = np.array([bounds.fx_min, bounds.fy_min, bounds.cx_min, bounds.cy_min, bounds.skew_min])
    hi = np.array([bounds.fx_max, bounds.fy_max, bounds.cx_max, bounds.cy_max, bounds.skew_max])
    return lo, hi


def estimate_intrinsics_linear_batch(offset, x, y, u, v, bounds: Optional[CalibrationBounds] = None, use_skew=False,
                                     lib=None) -> LinearBatch:
    """cba_estimate_intrinsics_linear_batch (bounds None: CalibrationBounds{})."""
    lib = lib or capi.load_library()
    off, (x, y, u, v) = _soa(offset, x, y, u, v)
    P = off.size - 1
    lo, hi = _bounds5(bounds)
    K = np.zeros((P, 5))
    st = np.zeros(P, np.int32)
    fb = np.zeros(P, np.int32)
    capi.check(lib, lib.cba_estimate_intrinsics_linear_batch(P, i64ptr(off), dptr(x), dptr(y), dptr(u), dptr(v), dptr(lo), dptr(hi),
                                                             1 if use_skew else 0, dptr(K), i32ptr(st), i32ptr(fb)))
    return LinearBatch(K, st, fb)


def estimate_intrinsics_linear_iterative_batch(offset, x, y, u, v, num_radial=2, max_iterations=5, use_skew=False,
                                               lib=None) -> IterativeBatch:
    """cba_estimate_intrinsics_linear_iterative_batch."""
    lib = lib or capi.load_library()
    off, (x, y, u, v) = _soa(offset, x, y, u, v)
    P = off.size - 1
    m = int(num_radial) + 2
    K = np.zeros((P, 5))
    co = np.zeros((P, m))
    st, it, fb = (np.zeros(P, np.int32) for _ in range(3))
    capi.check(lib, lib.cba_estimate_intrinsics_linear_iterative_batch(P, i64ptr(off), dptr(x), dptr(y), dptr(u), dptr(v), int(num_radial),
                                                                       int(max_iterations), 1 if use_skew else 0, dptr(K), dptr(co),
                                                                       i32ptr(st), i32ptr(it), i32ptr(fb)))
    return IterativeBatch(K, co, st, it, fb)


# ---- the reference's signatures (one problem) ------------------------------------------------------------------------------
def _one(observations):
    obs = np.asarray(observations, dtype=np.float64).reshape(-1, 4)
    return np.array([0, obs.shape[0]], np.int64), obs[:, 0], obs[:, 1], obs[:, 2], obs[:, 3]


def _fixed_values(fixed_indices, fixed_values):
    """The reference reads fixed_values[i] for i < size() and 0 beyond (distortion.h:305-309)."""
    vals = list(fixed_values or ())
    return [float(vals[i]) if i < len(vals) else 0.0 for i in range(len(fixed_indices))]


def fit_distortion_full(observations, intrinsics, num_radial=2, fixed_indices: Sequence[int] = (),
                        fixed_values: Sequence[float] = ()) -> Optional[DistortionWithResiduals]:
    """fit_distortion_full (distortion.h:229-363): None for fewer than 8 observations (before the fixed indices are checked, as in
    the reference)."""
    off, x, y, u, v = _one(observations)
    if off[1] < 8:
        return None
    r = fit_distortion_batch(off, x, y, u, v, np.asarray(intrinsics, float)[:5], num_radial, list(fixed_indices),
                             _fixed_values(fixed_indices, fixed_values))
    return DistortionWithResiduals(r.coeffs[0], r.residuals)


def fit_distortion(observations, intrinsics, num_radial=2, fixed_indices: Sequence[int] = (),
                   fixed_values: Sequence[float] = ()) -> Optional[DistortionWithResiduals]:
    """fit_distortion (distortion.h:365-371) = fit_distortion_full."""
    return fit_distortion_full(observations, intrinsics, num_radial, fixed_indices, fixed_values)


def fit_distortion_dual(observations, intrinsics, num_radial=2, fixed_indices: Sequence[int] = (),
                        fixed_values: Sequence[float] = ()) -> Optional[DualDistortionWithResiduals]:
    """fit_distortion_dual (distortion.h:373-406)."""
    off, x, y, u, v = _one(observations)
    if off[1] < 8:
        return None
    r = fit_distortion_batch(off, x, y, u, v, np.asarray(intrinsics, float)[:5], num_radial, list(fixed_indices),
                             _fixed_values(fixed_indices, fixed_values), dual=True)
    return DualDistortionWithResiduals(r.coeffs[0], r.inverse[0], r.residuals)


def estimate_intrinsics_linear(observations, bounds: Optional[CalibrationBounds] = None, use_skew=False) -> Optional[np.ndarray]:
    """estimate_intrinsics_linear (intrinsicsdlt.cpp:289-312): K = [fx, fy, cx, cy, skew] or None."""
    off, x, y, u, v = _one(observations)
    r = estimate_intrinsics_linear_batch(off, x, y, u, v, bounds, use_skew)
    return r.kmtx[0] if r.status[0] == capi.LINEAR_OK else None


def estimate_intrinsics_linear_iterative(observations, num_radial, max_iterations=5, use_skew=False) -> Optional[PinholeBrownConrady]:
    """estimate_intrinsics_linear_iterative (intrinsicsdlt.cpp:319-368): the camera or None."""
    off, x, y, u, v = _one(observations)
    r = estimate_intrinsics_linear_iterative_batch(off, x, y, u, v, num_radial, max_iterations, use_skew)
    if r.status[0] != capi.LINEAR_OK:
        return None
    return PinholeBrownConrady(r.kmtx[0], r.coeffs[0])
