"""The camera models on the GPU: the reference's ``PinholeCamera::project`` / ``unproject`` (pinhole.h:96-113),
``ScheimpflugCamera::project`` (scheimpflug.h:139-181), ``BrownConrady::distort`` / ``undistort`` (distortion.h:119-160) and
``DualDistortion::undistort`` (distortion.h:208-218), plus undistortion / rectification maps and their application to whole
images, on top of the C ABI (``cba_camera_project``, ``cba_camera_unproject``, ``cba_undistort_map_*``).

A camera is what ``calibration_amd.linescan`` takes: the 10-entry [fx, fy, cx, cy, skew, k1, k2, k3, p1, p2] (pinhole +
Brown-Conrady) or 12-entry (+ tau_x, tau_y: Scheimpflug) parameter vector, and optional ``inverse_coeffs`` ([k1..k_nr, p1, p2]
of DualDistortion's inverse) where an inverse is needed.  The outputs of ``optimize_*`` and of the rig and line-scan facades pass
straight in.  The arithmetic (fp64; the maps rounded to float32; apply's fixed-point and fp32 rules) is stated in calibba.h.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import capi
from .capi import dptr, i32ptr
from .linescan import _camera

_IDENTITY_K = np.array([1.0, 1.0, 0.0, 0.0, 0.0])


def _points(a, width):
    p = np.asarray(a, dtype=np.float64)
    if p.ndim == 1:
        p = p.reshape(1, -1)
    if p.ndim != 2 or p.shape[1] != width:
        raise ValueError(f"expected points of shape [n][{width}], got {np.asarray(a).shape}")
    return np.ascontiguousarray(p)


def project(camera, xyz) -> np.ndarray:
    """project(xyz) of camera-frame points xyz [n][3] -> pixels [n][2]; points [n][2] are normalised (x, y): project(norm_xy).
    No masking: z <= 0 (or a Scheimpflug sensor denominator <= 0) gives whatever the division gives."""
    lib = capi.load_library()
    model, intr, _ = _camera(camera, None)
    p = np.asarray(xyz, dtype=np.float64)
    if p.ndim == 2 and p.shape[1] == 2:
        p = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1)
    p = _points(p, 3)
    uv = np.empty((p.shape[0], 2))
    capi.check(lib, lib.cba_camera_project(model, dptr(intr), p.shape[0], dptr(p), dptr(uv)))
    return uv


def unproject(camera, uv, inverse_coeffs=None) -> np.ndarray:
    """Pixels uv [n][2] -> normalised (x, y) [n][2]: the pinhole's unproject (undistortion: DualDistortion's one step with
    inverse_coeffs, else BrownConrady's 5-step fixed point); for Scheimpflug the exact inverse of project (calibba.h)."""
    lib = capi.load_library()
    model, intr, inv = _camera(camera, inverse_coeffs)
    p = _points(uv, 2)
    xy = np.empty_like(p)
    capi.check(lib, lib.cba_camera_unproject(model, dptr(intr), 0 if inv is None else int(inv.size), dptr(inv), p.shape[0], dptr(p),
                                             dptr(xy)))
    return xy


def _coeffs(coeffs):
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    if c.size in (10, 12):  # a camera vector: its distortion
        c = c[5:10]
    if c.size != 5:
        raise ValueError(f"expected the 5 Brown-Conrady coefficients [k1, k2, k3, p1, p2] or a camera vector, got {c.size} entries")
    return np.concatenate([_IDENTITY_K, c])


def distort(coeffs, xy) -> np.ndarray:
    """BrownConrady::distort of normalised points xy [n][2]: project with K = [1, 1, 0, 0, 0].  coeffs: [k1, k2, k3, p1, p2] or
    a camera vector."""
    return project(_coeffs(coeffs), _points(xy, 2))


def undistort(coeffs, xy, inverse_coeffs=None) -> np.ndarray:
    """BrownConrady::undistort (5-step fixed point) or, with inverse_coeffs, DualDistortion::undistort of distorted normalised
    points xy [n][2]: unproject with K = [1, 1, 0, 0, 0]."""
    return unproject(_coeffs(coeffs), xy, inverse_coeffs)


class UndistortMap(capi.Handle):
    """Undistortion / rectification maps of one or more cameras of one model, kept on the device.

    ``UndistortMap(cameras, width, height, R=None, new_K=None, device=0)``: cameras is one parameter vector or a list of them;
    R [n_cams][3][3] (or one 3x3 for a single camera) the rectifying rotations (None: identity); new_K [n_cams][5]
    ([fx', fy', cx', cy', skew']; None: each camera's own K).  Map pixel (u', v') of camera c is project_c(R_c^T K'^-1 (u', v', 1)),
    rounded to float32, NaN where the ray does not reach the image side.  Use it as a context manager or call ``close()``."""

    _DESTROY = "cba_undistort_map_destroy"

    def __init__(self, cameras, width: int, height: int, R=None, new_K=None, device: int = 0):
        out = self._out()
        cams = np.asarray(cameras, dtype=np.float64)
        if cams.ndim == 1:
            cams = cams.reshape(1, -1)
        parsed = [_camera(c, None) for c in cams]
        self.model = parsed[0][0]
        self.n_cams = len(parsed)
        intr = np.ascontiguousarray(np.stack([p[1] for p in parsed]))
        Rm = None if R is None else np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(self.n_cams, 9))
        Kn = None if new_K is None else np.ascontiguousarray(np.asarray(new_K, dtype=np.float64).reshape(self.n_cams, 5))
        self.width, self.height = int(width), int(height)
        capi.check(self._lib, self._lib.cba_undistort_map_create(self.model, self.n_cams, dptr(intr), dptr(Rm), dptr(Kn), self.width,
                                                                 self.height, int(device), out))

    def _handle(self):
        return self._require_open("UndistortMap is closed")

    def maps(self):
        """(map_x, map_y), each [n_cams][height][width] float32: OpenCV's remap layout."""
        mx = np.empty((self.n_cams, self.height, self.width), dtype=np.float32)
        my = np.empty_like(mx)
        fp = C.POINTER(C.c_float)
        capi.check(self._lib, self._lib.cba_undistort_map_fetch(self._handle(), mx.ctypes.data_as(fp), my.ctypes.data_as(fp)))
        return mx, my

    def apply(self, images, cams, border=0):
        """Resample images [n][h][w] or [n][h][w][channels] (uint8 or float32, channels 1..4) through the maps of cameras cams
        (one index per image, or one for all) -> [n][height][width](+[channels]) of the same dtype.  Bilinear, constant border."""
        im = np.asarray(images)
        if im.dtype == np.uint8:
            dtype = capi.DTYPE_U8
        elif im.dtype == np.float32:
            dtype = capi.DTYPE_F32
        else:
            raise ValueError(f"images must be uint8 or float32, got {im.dtype}")
        if im.ndim == 3:
            ch, shape = 1, (im.shape[0], self.height, self.width)
        elif im.ndim == 4:
            ch, shape = im.shape[3], (im.shape[0], self.height, self.width, im.shape[3])
        else:
            raise ValueError("images must be [n][h][w] or [n][h][w][channels]")
        im = np.ascontiguousarray(im)
        n = im.shape[0]
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(cams, dtype=np.int32), (n,)))
        out = np.empty(shape, dtype=im.dtype)
        capi.check(self._lib, self._lib.cba_undistort_map_apply(self._handle(), n, i32ptr(c), im.shape[2], im.shape[1], ch, dtype,
                                                                float(border), im.ctypes.data_as(C.c_void_p),
                                                                out.ctypes.data_as(C.c_void_p)))
        return out


__all__ = ["project", "unproject", "distort", "undistort", "UndistortMap"]
