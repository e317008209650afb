"""Scan fusion on the GPU (``cba_tsdf_volume``, ``cba_tsdf_integrate``, ``cba_tsdf_extract``): depth maps of one object, each with
its pose, are merged into a truncated signed distance volume, and the surface is read off it as points with normals on the lattice
edges, by the rules calibba.h states.  The reference has no counterpart.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import capi
from .capi import CbaTsdfOptions, dptr, i64ptr


def _fptr(a: Optional[np.ndarray]):
    if a is None:
        return C.cast(None, C.POINTER(C.c_float))
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_float))


@dataclass
class TsdfOptions:
    """``cba_tsdf_options``: the lattice spacing, the truncation band (in the volume's unit; a few voxel sizes), the cap of a voxel's
    weight (an integer value in [1, 2^24]) and the largest depth that is used."""
    voxel_size: float
    truncation: float
    max_weight: float = 64.0
    max_depth: float = np.inf

    def _c(self) -> CbaTsdfOptions:
        return CbaTsdfOptions(float(self.voxel_size), float(self.truncation), float(self.max_weight), float(self.max_depth))


def depth_from_xyz(xyz) -> np.ndarray:
    """The depth maps of organised point maps [...][height][width][3], as the stereo, SGM and structured-light handles write them (in
    the frame of the camera whose pixels organise them): z, NaN where any coordinate of the pixel is non-finite.  Host work."""
    p = np.asarray(xyz, dtype=np.float64)
    if p.ndim < 3 or p.shape[-1] != 3:
        raise ValueError(f"xyz must be [height][width][3] or [n_maps][height][width][3], got {p.shape}")
    return np.where(np.isfinite(p).all(axis=-1), p[..., 2], np.nan)


class TsdfVolume(capi.Handle):
    """``cba_tsdf_volume``: nx x ny x nz voxels (x fastest) whose lattice point (i, j, k) lies at origin + (i, j, k) voxel_size.  Use
    as a context manager or call ``close()``."""

    _DESTROY = "cba_tsdf_volume_destroy"

    def __init__(self, shape: Tuple[int, int, int], origin, opts: TsdfOptions, device: int = 0):
        out = self._out()
        nx, ny, nz = (int(v) for v in shape)
        self.shape, self.opts = (nx, ny, nz), opts
        self.origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
        co = opts._c()
        capi.check(self._lib, self._lib.cba_tsdf_volume_create(nx, ny, nz, dptr(self.origin), C.byref(co), int(device), out))

    def integrate(self, camera_model: int, intr, poses, depth=None, xyz=None) -> None:
        """Apply depth maps [n_maps][height][width] (or one [height][width]) in order; poses [n_maps][7]: volume frame -> camera.
        ``xyz``: organised point maps in the camera's frame instead (``depth_from_xyz``)."""
        h = self._require_open("the volume is closed")
        if (depth is None) == (xyz is None):
            raise ValueError("give depth or xyz, one of them")
        d = depth_from_xyz(xyz) if depth is None else np.asarray(depth, dtype=np.float64)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3:
            raise ValueError(f"depth must be [height][width] or [n_maps][height][width], got {d.shape}")
        d = np.ascontiguousarray(d)
        pose = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
        if pose.shape[0] != d.shape[0]:
            raise ValueError(f"{d.shape[0]} maps but {pose.shape[0]} poses")
        k = np.ascontiguousarray(np.asarray(intr, dtype=np.float64).reshape(-1))
        if k.size != (12 if camera_model == 1 else 10):
            raise ValueError(f"intr has {k.size} entries")
        capi.check(self._lib, self._lib.cba_tsdf_integrate(h, int(camera_model), dptr(k), d.shape[0], d.shape[1], d.shape[2], dptr(d), dptr(pose)))

    def fetch(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (tsdf, weight), float32 [nz][ny][nx]"""
        h = self._require_open("the volume is closed")
        nx, ny, nz = self.shape
        tsdf, weight = np.empty((nz, ny, nx), np.float32), np.empty((nz, ny, nx), np.float32)
        capi.check(self._lib, self._lib.cba_tsdf_fetch(h, _fptr(tsdf), _fptr(weight)))
        return tsdf, weight

    def upload(self, tsdf=None, weight=None) -> None:
        """Write planes [nz][ny][nx] that ``fetch`` returned (either may be None: that plane stays)."""
        h = self._require_open("the volume is closed")
        nx, ny, nz = self.shape
        planes = []
        for a in (tsdf, weight):
            if a is not None:
                a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
                if a.shape != (nz, ny, nx):
                    raise ValueError(f"a plane must be [{nz}][{ny}][{nx}], got {a.shape}")
            planes.append(a)
        capi.check(self._lib, self._lib.cba_tsdf_upload(h, _fptr(planes[0]), _fptr(planes[1])))

    def extract(self, min_weight: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
        """-> (xyz [n][3], normals [n][3]): the zero crossings on lattice edges in visiting order; a normal is NaN where there is none"""
        h = self._require_open("the volume is closed")
        n = np.zeros(1, np.int64)
        capi.check(self._lib, self._lib.cba_tsdf_extract(h, float(min_weight), i64ptr(n)))
        xyz, normals = np.empty((int(n[0]), 3)), np.empty((int(n[0]), 3))
        capi.check(self._lib, self._lib.cba_tsdf_extract_fetch(h, dptr(xyz), dptr(normals)))
        return xyz, normals

    def reset(self) -> None:
        capi.check(self._lib, self._lib.cba_tsdf_reset(self._require_open("the volume is closed")))


def fuse(shape, origin, opts: TsdfOptions, camera_model: int, intr, poses, depth=None, xyz=None, min_weight: float = 1.0, device: int = 0):
    """One volume, one integrate, one extract: -> (xyz [n][3], normals [n][3])"""
    with TsdfVolume(shape, origin, opts, device) as vol:
        vol.integrate(camera_model, intr, poses, depth=depth, xyz=xyz)
        return vol.extract(min_weight)
