"""Chessboard detection on top of the C ABI (``cba_corner_detector``, ``cba_chessboard_order``; no counterpart in the reference,
which reads corners from files): pictures of a plain chessboard -> the ``(object_xy, image_uv)`` lists that ``calibration_amd.linear``,
``calibration_amd.rig`` and ``calibration_amd.optim`` take.

``CornerDetector`` turns batches of uint8 images of one size into corners (position, angle, response, flags); ``order_chessboard``
puts one image's corners into the board's grid order on the host; ``detect_chessboard`` does both for a batch.  The rules are stated
in calibba.h.  Arguments are validated here before the library sees them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import capi
from .capi import CbaCornerOptions, dptr, i32ptr, u8ptr

REFINE_NONE, REFINE_COG, REFINE_GRADIENT = 0, 1, 2
STATUS_OVERFLOW = 1
FLAG_WINDOW, FLAG_DET, FLAG_DRIFT = 1, 2, 4


@dataclass
class CornerOptions:
    """``cba_corner_options``: lowest response of a peak, suppression radius, centre-of-gravity radius, the sub-pixel method and
    GRADIENT's half window and rounds."""
    min_response: int = 400
    nms_radius: int = 3
    cog_radius: int = 2
    refine: int = REFINE_GRADIENT
    refine_half_window: int = 5
    refine_iterations: int = 5


@dataclass
class CornerResult:
    count: np.ndarray      # [n] int32: the true number of peaks of every image
    status: np.ndarray     # [n] int32: STATUS_OVERFLOW
    xy: np.ndarray         # [n][max_corners][2] float64, NaN past the kept corners
    angle: np.ndarray      # [n][max_corners] float64, NaN past the kept corners
    response: np.ndarray   # [n][max_corners] int32
    flags: np.ndarray      # [n][max_corners] int32: FLAG_*

    def kept(self, i: int) -> int:
        return int(min(self.count[i], self.xy.shape[1]))


@dataclass
class BoardDetection:
    found: bool
    image_uv: np.ndarray    # [rows cols][2], row-major over (j, i); NaN when not found
    object_xy: np.ndarray   # [rows cols][2] = (i square, j square)
    n_corners: int = 0      # the peaks of the image

    @property
    def view(self) -> np.ndarray:
        """[rows cols][4] rows (X, Y, u, v): one view of the intrinsic and rig entry points."""
        return np.concatenate([self.object_xy, self.image_uv], axis=1)


class CornerDetector:
    """``cba_corner_detector``: uint8 images of one size in, corners out.  The device buffers are sized for max_images and
    max_corners at construction.  Use as a context manager or call ``close()``."""

    def __init__(self, width: int, height: int, max_images: int = 1, max_corners: int = 1024, opts: Optional[CornerOptions] = None,
                 device: int = 0):
        self._h = None
        self._lib = capi.load_library()
        o = opts or CornerOptions()
        co = CbaCornerOptions(int(o.min_response), int(o.nms_radius), int(o.cog_radius), int(o.refine), int(o.refine_half_window),
                              int(o.refine_iterations))
        self.width, self.height, self.max_images, self.max_corners = int(width), int(height), int(max_images), int(max_corners)
        h = C.c_void_p()
        capi.check(self._lib, self._lib.cba_corner_detector_create(self.width, self.height, self.max_images, self.max_corners, C.byref(co),
                                                                   int(device), C.byref(h)))
        self._h = h

    def process(self, images) -> CornerResult:
        """images: [n][height][width] uint8 (or one [height][width] image)."""
        if self._h is None:
            raise ValueError("the detector is closed")
        img = np.asarray(images)
        if img.dtype != np.uint8:
            raise ValueError(f"images must be uint8, got {img.dtype}")
        if img.ndim == 2:
            img = img[None]
        if img.ndim != 3 or img.shape[1:] != (self.height, self.width):
            raise ValueError(f"images must have shape [n][{self.height}][{self.width}], got {img.shape}")
        img = np.ascontiguousarray(img)
        n, m = img.shape[0], self.max_corners
        if n > self.max_images:
            raise ValueError(f"{n} images given, the detector was created for {self.max_images}")
        count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        xy, angle = np.full((n, m, 2), np.nan), np.full((n, m), np.nan)
        response, flags = np.zeros((n, m), np.int32), np.zeros((n, m), np.int32)
        capi.check(self._lib, self._lib.cba_corner_detector_process(self._h, n, u8ptr(img), i32ptr(count), i32ptr(status), dptr(xy),
                                                                    dptr(angle), i32ptr(response), i32ptr(flags)))
        return CornerResult(count, status, xy, angle, response, flags)

    def close(self):
        if self._h is not None:
            self._lib.cba_corner_detector_destroy(self._h)
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


def order_chessboard(xy, angle, rows: int, cols: int) -> Optional[np.ndarray]:
    """``cba_chessboard_order``: one image's corners xy [n][2], angle [n] -> index [rows cols] into them, row-major over (j, i), or
    None when the board is not found.  rows x cols are the board's inner corners."""
    lib = capi.load_library()
    p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64))
    a = np.ascontiguousarray(np.asarray(angle, dtype=np.float64).reshape(-1))
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] != a.shape[0]:
        raise ValueError(f"xy must have shape [n][2] and angle [n], got {p.shape} and {a.shape}")
    index = np.full(int(rows) * int(cols) if rows > 0 and cols > 0 else 1, -1, np.int32)
    capi.check(lib, lib.cba_chessboard_order(p.shape[0], dptr(p), dptr(a), int(rows), int(cols), i32ptr(index)))
    return None if index[0] < 0 else index


def detect_chessboard(images, rows: int, cols: int, square: float = 1.0, opts: Optional[CornerOptions] = None, max_corners: int = 1024,
                      device: int = 0) -> List[BoardDetection]:
    """Corners of every image on the device, grid order on the host.  images: [n][H][W] uint8; rows x cols inner corners of side
    ``square``.  Corners that carry a flag are left out before ordering."""
    img = np.asarray(images)
    if img.ndim == 2:
        img = img[None]
    if img.ndim != 3:
        raise ValueError(f"images must have shape [n][H][W], got {img.shape}")
    if rows < 2 or cols < 2:
        raise ValueError("rows and cols must be >= 2")
    jj, ii = np.divmod(np.arange(rows * cols), cols)
    obj = np.stack([ii * float(square), jj * float(square)], axis=1)
    out = []
    if img.shape[0] == 0:
        return out
    with CornerDetector(img.shape[2], img.shape[1], img.shape[0], max_corners, opts, device) as det:
        res = det.process(img)
    for i in range(img.shape[0]):
        k = res.kept(i)
        good = np.flatnonzero(res.flags[i, :k] == 0)
        index = order_chessboard(res.xy[i, good], res.angle[i, good], rows, cols) if good.size >= rows * cols else None
        if index is None:
            out.append(BoardDetection(False, np.full((rows * cols, 2), np.nan), obj.copy(), int(res.count[i])))
        else:
            out.append(BoardDetection(True, res.xy[i, good[index]].copy(), obj.copy(), int(res.count[i])))
    return out


__all__ = ["CornerOptions", "CornerResult", "BoardDetection", "CornerDetector", "order_chessboard", "detect_chessboard", "REFINE_NONE",
           "REFINE_COG", "REFINE_GRADIENT", "STATUS_OVERFLOW", "FLAG_WINDOW", "FLAG_DET", "FLAG_DRIFT"]
