"""Structured-light scanning on the GPU (``cba_sl_patterns``, ``cba_sl_decoder``): Gray-code and phase-shift patterns for a projector,
the decode of a camera's image sequence into a projector coordinate per pixel by the rule calibba.h states, and with a rig the point
map by ``cba_triangulate``'s rule.  ``projector_corners`` turns decoded views of a calibration board into projector-side corner
positions, so that a projector is calibrated as an inverse camera with the solvers that exist (``estimate_intrinsics``,
``optimize_intrinsics``, ``estimate_extrinsic_dlt``, ``optimize_extrinsics``).  The reference has no counterpart.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi
from .capi import CbaSlOptions, CbaTriangulateOptions, dptr, i32ptr, u8ptr
from .linescan import _camera
from .triangulate import TriangulateOptions, _pose7_rows

AXIS_X, AXIS_Y = 1, 2
# status bits (calibba.h: cba_sl_status_bits)
LOW_CONTRAST, X_UNCERTAIN, X_OUTSIDE, X_LOW_MODULATION, Y_UNCERTAIN, Y_OUTSIDE, Y_LOW_MODULATION = 1, 2, 4, 8, 16, 32, 64


@dataclass
class StructuredLightOptions:
    """``cba_sl_options``: the projector's size, the axes to decode (bit 0: columns -> x, bit 1: rows -> y), the Gray bits that are
    not projected, the phase steps (0: none, else 3..8) and their period in projector pixels, and the three validity thresholds."""
    proj_width: int
    proj_height: int
    axes: int = AXIS_X | AXIS_Y
    gray_skip_bits: int = 0
    phase_steps: int = 0
    phase_period: int = 16
    min_contrast: int = 10
    min_bit_diff: int = 4
    min_modulation: float = 5.0

    def _c(self) -> CbaSlOptions:
        return CbaSlOptions(int(self.proj_width), int(self.proj_height), int(self.axes), int(self.gray_skip_bits), int(self.phase_steps),
                            int(self.phase_period), int(self.min_contrast), int(self.min_bit_diff), float(self.min_modulation))


@dataclass
class Decoded:
    x: Optional[np.ndarray]           # [n_sequences][height][width] projector x, NaN where invalid; None when the axis is not decoded
    y: Optional[np.ndarray]           # ... projector y
    modulation: np.ndarray            # [n_sequences][n_axes][height][width]; NaN without phase steps
    status: np.ndarray                # uint8 [n_sequences][height][width]: 0 = every decoded axis is valid
    xyz: Optional[np.ndarray] = None         # [n_sequences][height][width][3] with want_points
    rms_px: Optional[np.ndarray] = None      # [n_sequences][height][width]
    tri_status: Optional[np.ndarray] = None  # int32 [n_sequences][height][width]: capi.TRI_*


def image_count(opts: StructuredLightOptions) -> int:
    """Images of one sequence: white, black and per axis 2 nbits Gray planes and the phase steps."""
    lib = capi.load_library()
    n = C.c_int32(0)
    capi.check(lib, lib.cba_sl_image_count(C.byref(opts._c()), C.byref(n)))
    return int(n.value)


def patterns(opts: StructuredLightOptions) -> np.ndarray:
    """The sequence to project: uint8 [n_images][proj_height][proj_width] (host only: no device is needed)."""
    lib = capi.load_library()
    n = image_count(opts)
    out = np.empty((n, int(opts.proj_height), int(opts.proj_width)), dtype=np.uint8)
    capi.check(lib, lib.cba_sl_patterns(C.byref(opts._c()), u8ptr(out)))
    return out


class StructuredLightDecoder(capi.Handle):
    """``cba_sl_decoder``: image sequences of one size in, projector coordinates (and points) out, one kernel launch per ``decode``
    (two with points).  The device buffers are sized for max_sequences at construction.  Use as a context manager or call ``close()``."""

    _DESTROY = "cba_sl_decoder_destroy"

    def __init__(self, opts: StructuredLightOptions, width: int, height: int, max_sequences: int = 1, device: int = 0):
        out = self._out()
        self.opts = opts
        self.width, self.height, self.max_sequences = int(width), int(height), int(max_sequences)
        self.n_axes = bin(int(opts.axes) & 3).count("1")
        co = opts._c()
        capi.check(self._lib, self._lib.cba_sl_decoder_create(C.byref(co), self.width, self.height, self.max_sequences, int(device), out))
        self.n_images = image_count(opts)

    def set_rig(self, camera, projector, c_se3_r, inverse_coeffs=None, opts: Optional[TriangulateOptions] = None):
        """camera, projector: parameter vectors of one model (10 | 12 entries); c_se3_r: the reference -> camera and reference ->
        projector poses ([2][4][4] or [2][7]); inverse_coeffs: optional [2][m]; opts: the triangulation's options."""
        h = self._require_open("the decoder is closed")
        parsed = [_camera(camera, None), _camera(projector, None)]
        if parsed[0][0] != parsed[1][0]:
            raise ValueError("camera and projector must be of one model")
        intr = np.ascontiguousarray(np.stack([p[1] for p in parsed]))
        poses = _pose7_rows(c_se3_r, 2)
        inv, n_inv = None, 0
        if inverse_coeffs is not None:
            inv = np.ascontiguousarray(np.asarray(inverse_coeffs, dtype=np.float64).reshape(2, -1))
            n_inv = inv.shape[1]
        o = opts or TriangulateOptions()
        co = CbaTriangulateOptions(int(o.max_iterations), float(o.step_tolerance), int(o.min_cams), float(o.max_reproj_px))
        capi.check(self._lib, self._lib.cba_sl_decoder_set_rig(h, parsed[0][0], dptr(intr), n_inv, dptr(inv), dptr(poses), C.byref(co)))

    def process(self, images, coord=True, modulation=True, status=True, xyz=False, rms_px=False, tri_status=False) -> dict:
        """The C call with each output on request: a dict of the arrays asked for (None for the others).  images:
        [n_sequences][n_images][height][width] uint8 (one [n_images][height][width] sequence is promoted)."""
        h = self._require_open("the decoder is closed")
        img = np.asarray(images)
        if img.dtype != np.uint8:
            raise ValueError(f"images must be uint8, got {img.dtype}")
        if img.ndim == 3:
            img = img[None]
        if img.ndim != 4 or img.shape[1:] != (self.n_images, self.height, self.width):
            raise ValueError(f"images must have shape [n_sequences][{self.n_images}][{self.height}][{self.width}], got {img.shape}")
        img = np.ascontiguousarray(img)
        n = img.shape[0]
        px = (n, self.height, self.width)
        maps = (n, self.n_axes, self.height, self.width)
        r = dict(coord=np.empty(maps) if coord else None, modulation=np.empty(maps) if modulation else None,
                 status=np.empty(px, np.uint8) if status else None, xyz=np.empty(px + (3,)) if xyz else None,
                 rms_px=np.empty(px) if rms_px else None, tri_status=np.empty(px, np.int32) if tri_status else None)
        capi.check(self._lib, self._lib.cba_sl_decoder_process(h, n, u8ptr(img), dptr(r["coord"]), dptr(r["modulation"]), u8ptr(r["status"]),
                                                               dptr(r["xyz"]), dptr(r["rms_px"]), i32ptr(r["tri_status"])))
        return r

    def decode(self, images, want_points: bool = False) -> Decoded:
        r = self.process(images, xyz=want_points, rms_px=want_points, tri_status=want_points)
        axes = int(self.opts.axes)
        x = r["coord"][:, 0] if axes & AXIS_X else None
        y = r["coord"][:, self.n_axes - 1] if axes & AXIS_Y else None
        return Decoded(x, y, r["modulation"], r["status"], r["xyz"], r["rms_px"], r["tri_status"])


def projector_corners(decoded_x, decoded_y, corners_uv, radius: int = 8, min_valid: int = 16):
    """The projector positions of detected board corners, by a local homography per corner.

    decoded_x, decoded_y: the decoded maps of the views, [n_views][height][width] (or one [height][width] view); corners_uv: per view
    the detected corners [n][2] in camera pixels (one array for one view).  For each corner the integer camera pixels of the window
    |du|, |dv| <= radius around rint(corner), inside the image, with both coordinates finite, are matched to their projector
    coordinates; fewer than max(min_valid, 4) of them, or a NaN corner, gives NaN.  All corners of all views form one
    ``estimate_homography_batch`` call (camera pixel -> projector coordinate, no RANSAC); the corner's projector position is
    hnormalized(H (u, v, 1)).  Returns per view [n][2] (one array for one view).

    With the board's object_xy the result is the (object_xy, image_uv) list that ``estimate_intrinsics``, ``optimize_intrinsics``,
    ``estimate_extrinsic_dlt`` and ``optimize_extrinsics`` take for the projector as a second camera."""
    from .linear import estimate_homography_batch

    X, Y = np.asarray(decoded_x, dtype=np.float64), np.asarray(decoded_y, dtype=np.float64)
    single = X.ndim == 2
    if single:
        X, Y, corners_uv = X[None], Y[None], [corners_uv]
    if X.ndim != 3 or X.shape != Y.shape or len(corners_uv) != X.shape[0]:
        raise ValueError("decoded_x and decoded_y must be [n_views][height][width] maps of one shape, with one corner list per view")
    if radius < 0:
        raise ValueError("radius must be >= 0")
    H, W = X.shape[1:]
    need = max(int(min_valid), 4)
    corners = [np.asarray(c, dtype=np.float64).reshape(-1, 2) for c in corners_uv]
    out = [np.full(c.shape, np.nan) for c in corners]
    views, where = [], []
    for vi, c in enumerate(corners):
        for ci, (u, v) in enumerate(c):
            if not (np.isfinite(u) and np.isfinite(v)):
                continue
            cu, cv = int(np.rint(u)), int(np.rint(v))
            u0, u1, v0, v1 = max(cu - radius, 0), min(cu + radius, W - 1), max(cv - radius, 0), min(cv + radius, H - 1)
            if u0 > u1 or v0 > v1:
                continue
            vv, uu = np.mgrid[v0:v1 + 1, u0:u1 + 1]
            px, py = X[vi, v0:v1 + 1, u0:u1 + 1], Y[vi, v0:v1 + 1, u0:u1 + 1]
            ok = np.isfinite(px) & np.isfinite(py)
            if ok.sum() < need:
                continue
            views.append(np.stack([uu[ok], vv[ok], px[ok], py[ok]], axis=1).astype(np.float64))
            where.append((vi, ci))
    if views:
        for (vi, ci), r in zip(where, estimate_homography_batch(views)):
            if not r.success:
                continue
            u, v = corners[vi][ci]
            q = r.hmtx @ np.array([u, v, 1.0])
            out[vi][ci] = q[:2] / q[2]
    return out[0] if single else out
