"""Stereo depth on top of the C ABI (``cba_stereo_rectify``, ``cba_stereo_matcher``, ``cba_stereo_points``, ``cba_disparity_filter``; no counterpart in the
reference): calibrated pair -> rectified pair -> dense disparity -> 3D points.

``rectify`` takes the two cameras and their ``c_T_r`` rows as the rig entry points return them and gives the rectifying rotations, the
common camera matrix, the baseline and ``r_T_rect``; ``rectify_maps`` builds the ``UndistortMap`` of ``camera.py`` from them;
``StereoMatcher`` (block matching) and ``SgmMatcher`` (semi-global matching, ``cba_sgm_matcher``) turn rectified uint8 pairs into
disparity, cost and points, with ``filter=`` through the median and speckle filters that ``DisparityFilter`` applies to caller maps;
``stereo_points`` does the last step for caller (u, v, disparity) triples.  The rules are stated in calibba.h.  Arguments are validated here before the library sees them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi
from .camera import UndistortMap
from .capi import CbaDisparityFilterOptions, CbaSgmOptions, CbaStereoGeometry, CbaStereoMatchOptions, CbaStereoRectifyOptions, dptr, i32ptr, u8ptr
from .linescan import _camera


@dataclass
class StereoGeometry:
    """``cba_stereo_geometry``: f', cx', cy' of the rectified pair and the baseline."""
    focal: float
    cx: float
    cy: float
    baseline: float


@dataclass
class StereoRectification:
    R: np.ndarray          # [2][3][3] rect_R_r R_i^T: what UndistortMap takes
    new_K: np.ndarray      # [2][5] two identical rows [f', f', cx', cy', 0]
    baseline: float
    r_T_rect: np.ndarray   # [7] pose7: rectified frame of camera 0 -> reference frame

    @property
    def geometry(self) -> StereoGeometry:
        return StereoGeometry(float(self.new_K[0, 0]), float(self.new_K[0, 2]), float(self.new_K[0, 3]), float(self.baseline))


@dataclass
class StereoMatchOptions:
    """``cba_stereo_match_options``: disparities [min_disparity, min_disparity + num_disparities), window (2 half_window + 1)^2,
    uniqueness margin in percent (0: off), left-right tolerance (-1: off), the sub-pixel parabola step."""
    min_disparity: int = 0
    num_disparities: int = 64
    half_window: int = 4
    uniqueness_percent: int = 10
    lr_max_diff: int = 1
    subpixel: bool = True


@dataclass
class SgmOptions:
    """``cba_sgm_options``: disparities [min_disparity, min_disparity + num_disparities), the path penalties p1 <= p2, 4 or 8 paths,
    uniqueness margin in percent (0: off), left-right tolerance (-1: off), the sub-pixel parabola step, and the budget of the device
    volumes in MiB (0: 2048)."""
    min_disparity: int = 0
    num_disparities: int = 64
    p1: int = 4
    p2: int = 32
    paths: int = 8
    uniqueness_percent: int = 10
    lr_max_diff: int = 1
    subpixel: bool = True
    workspace_mb: int = 0


@dataclass
class DisparityFilterOptions:
    """``cba_disparity_filter_options``: the median window (2 median_half + 1)^2 (0: no median), the largest component that speckle
    removal deletes (0: off) and the largest difference between joined 4-neighbours."""
    median_half: int = 1
    speckle_max_size: int = 100
    speckle_max_diff: float = 1.0


def _filter_options(o) -> CbaDisparityFilterOptions:
    o = o or DisparityFilterOptions()
    m, size, diff = int(o.median_half), int(o.speckle_max_size), float(o.speckle_max_diff)
    if not 0 <= m <= 2:
        raise ValueError(f"median_half must be in 0..2, got {o.median_half}")
    if not 0 <= size <= 2**31 - 1:
        raise ValueError(f"speckle_max_size must be in 0..2^31 - 1, got {o.speckle_max_size}")
    if not (np.isfinite(diff) and diff >= 0.0):
        raise ValueError(f"speckle_max_diff must be finite and >= 0, got {o.speckle_max_diff}")
    return CbaDisparityFilterOptions(m, size, diff)


@dataclass
class StereoResult:
    disparity: np.ndarray          # [n][H][W] float32, NaN where there is no valid match
    cost: np.ndarray               # [n][H][W] int32, C(d*) (SgmMatcher: S(d*)), -1 without an admissible candidate
    xyz: Optional[np.ndarray]      # [n][H][W][3] float32 (only with a geometry)


def _pair(cameras):
    cams = np.asarray(cameras, dtype=np.float64)
    if cams.ndim != 2 or cams.shape[0] != 2:
        raise ValueError(f"expected two cameras of one model, got shape {cams.shape}")
    parsed = [_camera(c, None) for c in cams]
    return parsed[0][0], np.ascontiguousarray(np.stack([p[1] for p in parsed]))


def _pose7(pose) -> Optional[np.ndarray]:
    if pose is None:
        return None
    from .geometry import poses_from_matrices

    p = np.asarray(pose, dtype=np.float64)
    if p.shape == (4, 4):
        p = poses_from_matrices(p[None])[0]
    if p.shape != (7,):
        raise ValueError(f"a pose is a pose7 row or a 4x4 matrix, got shape {p.shape}")
    return np.ascontiguousarray(p)


def _geometry(g) -> CbaStereoGeometry:
    if isinstance(g, StereoRectification):
        g = g.geometry
    if isinstance(g, StereoGeometry):
        g = (g.focal, g.cx, g.cy, g.baseline)
    v = np.asarray(g, dtype=np.float64).reshape(-1)
    if v.size != 4:
        raise ValueError(f"a stereo geometry has 4 entries [focal, cx, cy, baseline], got {v.size}")
    return CbaStereoGeometry(*(float(x) for x in v))


def rectify(cameras, c_T_r, width: int, height: int, focal: float = 0.0, cx: float = 0.0, cy: float = 0.0) -> StereoRectification:
    """``cba_stereo_rectify``.  cameras: two parameter vectors of one model; c_T_r: [2][7] pose7 rows or two 4x4 matrices (reference
    frame -> camera).  Camera 0 becomes the left image.  focal, cx, cy: 0 selects the default (calibba.h)."""
    lib = capi.load_library()
    model, intr = _pair(cameras)
    p = np.asarray(c_T_r, dtype=np.float64)
    if p.shape == (2, 4, 4):
        from .geometry import poses_from_matrices

        p = poses_from_matrices(p)
    if p.shape != (2, 7):
        raise ValueError(f"c_T_r must be two pose7 rows or two 4x4 matrices, got shape {p.shape}")
    p = np.ascontiguousarray(p)
    o = CbaStereoRectifyOptions(float(focal), float(cx), float(cy))
    R, K, B, rt = np.empty((2, 9)), np.empty((2, 5)), np.empty(1), np.empty(7)
    capi.check(lib, lib.cba_stereo_rectify(model, dptr(intr), dptr(p), int(width), int(height), C.byref(o), dptr(R), dptr(K), dptr(B), dptr(rt)))
    return StereoRectification(R.reshape(2, 3, 3), K, float(B[0]), rt)


def rectify_maps(cameras, rectification: StereoRectification, width: int, height: int, device: int = 0) -> UndistortMap:
    """The ``UndistortMap`` of the two cameras built with the rectification's R and new_K: ``maps.apply(images, [0, 1])`` resamples a
    raw pair into a rectified one."""
    return UndistortMap(cameras, width, height, R=rectification.R, new_K=rectification.new_K, device=device)


class StereoMatcher(capi.Handle):
    """``cba_stereo_matcher``: rectified uint8 pairs of one size in, disparity, cost and (with a geometry) points out.  The device
    buffers are sized for max_pairs at construction.  geometry: a StereoGeometry, a StereoRectification or [focal, cx, cy, baseline];
    pose: pose7 or 4x4 applied to the points (r_T_rect, say).  Use as a context manager or call ``close()``."""

    _FN = "cba_stereo_matcher"  # the handle's create / process / destroy functions

    @staticmethod
    def _options(o):
        o = o or StereoMatchOptions()
        return CbaStereoMatchOptions(int(o.min_disparity), int(o.num_disparities), int(o.half_window), int(o.uniqueness_percent),
                                     int(o.lr_max_diff), int(bool(o.subpixel)))

    def __init__(self, width: int, height: int, max_pairs: int = 1, opts=None, geometry=None, pose=None, device: int = 0, filter=None):
        self._DESTROY = self._FN + "_destroy"
        out = self._out()
        co = self._options(opts)
        fo = None if filter is None else _filter_options(filter)
        if pose is not None and geometry is None:
            raise ValueError("a pose needs a geometry")
        g = None if geometry is None else _geometry(geometry)
        p = _pose7(pose)
        self.width, self.height, self.max_pairs = int(width), int(height), int(max_pairs)
        self.has_geometry = g is not None
        create = getattr(self._lib, self._FN + "_create")
        capi.check(self._lib, create(self.width, self.height, self.max_pairs, C.byref(co), None if g is None else C.byref(g), dptr(p),
                                     int(device), out))
        if fo is not None:  # None: the calls made without this keyword and nothing else
            capi.check(self._lib, getattr(self._lib, self._FN + "_set_filter")(self._h, C.byref(fo)))

    def set_filter(self, filter=None):
        """``..._set_filter``: a ``DisparityFilterOptions`` (the disparity is filtered on the device, xyz follows it), or None for none."""
        h = self._require_open("the matcher is closed")
        fo = None if filter is None else _filter_options(filter)
        capi.check(self._lib, getattr(self._lib, self._FN + "_set_filter")(h, None if fo is None else C.byref(fo)))

    def process(self, left, right, want_xyz: Optional[bool] = None) -> StereoResult:
        """left, right: [n_pairs][height][width] uint8 (or one [height][width] pair), rectified.  want_xyz: default = a geometry was
        given."""
        h = self._require_open("the matcher is closed")
        L = capi.u8_batch(left, "left", self.height, self.width, "n_pairs")
        R = capi.u8_batch(right, "right", self.height, self.width, "n_pairs")
        if L.shape != R.shape:
            raise ValueError(f"left and right differ in shape: {L.shape} and {R.shape}")
        n = L.shape[0]
        if n > self.max_pairs:
            raise ValueError(f"{n} pairs given, the matcher was created for {self.max_pairs}")
        want_xyz = self.has_geometry if want_xyz is None else bool(want_xyz)
        if want_xyz and not self.has_geometry:
            raise ValueError("xyz needs a matcher created with a geometry")
        shape = (n, self.height, self.width)
        disp, cost = np.empty(shape, np.float32), np.empty(shape, np.int32)
        xyz = np.empty(shape + (3,), np.float32) if want_xyz else None
        fp = C.POINTER(C.c_float)
        process = getattr(self._lib, self._FN + "_process")
        capi.check(self._lib, process(h, n, u8ptr(L), u8ptr(R), disp.ctypes.data_as(fp), i32ptr(cost),
                                      None if xyz is None else xyz.ctypes.data_as(fp)))
        return StereoResult(disp, cost, xyz)


class SgmMatcher(StereoMatcher):
    """``cba_sgm_matcher``: semi-global matching on a census cost (the rule is stated in calibba.h).  Same images, geometry, pose,
    ``process`` and ``StereoResult`` as ``StereoMatcher``; ``cost`` is S(d*).  opts: an ``SgmOptions``."""

    _FN = "cba_sgm_matcher"

    @staticmethod
    def _options(o):
        o = o or SgmOptions()
        if int(o.paths) not in (4, 8):
            raise ValueError(f"paths must be 4 or 8, got {o.paths}")
        if not 0 <= int(o.p1) <= int(o.p2):
            raise ValueError(f"the penalties must satisfy 0 <= p1 <= p2, got p1 = {o.p1}, p2 = {o.p2}")
        return CbaSgmOptions(int(o.min_disparity), int(o.num_disparities), int(o.p1), int(o.p2), int(o.paths), int(o.uniqueness_percent),
                             int(o.lr_max_diff), int(bool(o.subpixel)), int(o.workspace_mb))


class DisparityFilter(capi.Handle):
    """``cba_disparity_filter``: float32 disparity maps of one size in, NaN = no disparity; the median and speckle filters of calibba.h
    out.  The device buffers are sized for max_images at construction.  Use as a context manager or call ``close()``."""

    _DESTROY = "cba_disparity_filter_destroy"

    def __init__(self, width: int, height: int, max_images: int = 1, opts=None, device: int = 0):
        co = _filter_options(opts)
        out = self._out()
        self.width, self.height, self.max_images = int(width), int(height), int(max_images)
        capi.check(self._lib, self._lib.cba_disparity_filter_create(self.width, self.height, self.max_images, C.byref(co), int(device), out))

    def process(self, disparity, want_stats: bool = False):
        """disparity: [n][height][width] float32 (or one [height][width] map).  Returns the filtered maps [n][height][width]; with
        want_stats also int64 [n][3] = valid pixels read, components removed, pixels removed."""
        h = self._require_open("the filter is closed")
        d = np.asarray(disparity)
        if d.dtype != np.float32:
            raise ValueError(f"disparity must be float32, got {d.dtype}")
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3 or d.shape[1:] != (self.height, self.width):
            raise ValueError(f"disparity must have shape [n][{self.height}][{self.width}], got {d.shape}")
        if d.shape[0] > self.max_images:
            raise ValueError(f"{d.shape[0]} maps given, the filter was created for {self.max_images}")
        d = np.ascontiguousarray(d)
        out = np.empty_like(d)
        stats = np.zeros((d.shape[0], 3), np.int64) if want_stats else None
        fp = C.POINTER(C.c_float)
        capi.check(self._lib, self._lib.cba_disparity_filter_process(h, d.shape[0], d.ctypes.data_as(fp), out.ctypes.data_as(fp),
                                                                     capi.i64ptr(stats)))
        return (out, stats) if want_stats else out


def stereo_points(uvd, geometry, pose=None) -> np.ndarray:
    """``cba_stereo_points``: triples uvd [n][3] (u, v, disparity) -> points [n][3]; NaN where the disparity is not > 0."""
    lib = capi.load_library()
    g = _geometry(geometry)
    p = _pose7(pose)
    t = np.asarray(uvd, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"uvd must have shape [n][3], got {t.shape}")
    t = np.ascontiguousarray(t)
    xyz = np.empty_like(t)
    capi.check(lib, lib.cba_stereo_points(C.byref(g), dptr(p), t.shape[0], dptr(t), dptr(xyz)))
    return xyz


__all__ = ["StereoGeometry", "StereoRectification", "StereoMatchOptions", "StereoResult", "StereoMatcher", "SgmOptions", "SgmMatcher",
           "DisparityFilterOptions", "DisparityFilter", "rectify", "rectify_maps", "stereo_points"]
