"""Scan registration on the GPU (``cba_point_normals``, ``cba_cloud_index``, ``cba_cloud_nearest``, ``cba_cloud_register``): normals of
organised point maps, a uniform grid over a target cloud with an exact nearest-neighbour search inside a radius, and ICP (point to
plane or point to point) of a ragged batch of sources onto it, by the rules calibba.h states.  The reference has no counterpart.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi
from .capi import CbaIcpOptions, CbaIcpResult, dptr, i64ptr

POINT_TO_PLANE, POINT_TO_POINT = 0, 1
OK, NOT_CONVERGED, TOO_FEW, DEGENERATE = capi.ICP_OK, capi.ICP_NOT_CONVERGED, capi.ICP_TOO_FEW, capi.ICP_DEGENERATE


@dataclass
class IcpOptions:
    """``cba_icp_options``: metric (0: point to plane, 1: point to point), the correspondence gate, the cap on the updates, the step
    tolerance (rotation in rad, translation relative to the index's box diagonal) and the fewest pairs a system may have."""
    max_distance: float
    metric: int = POINT_TO_PLANE
    max_iterations: int = 30
    step_tolerance: float = 1e-9
    min_pairs: int = 6

    def _c(self) -> CbaIcpOptions:
        return CbaIcpOptions(int(self.metric), float(self.max_distance), int(self.max_iterations), float(self.step_tolerance),
                             int(self.min_pairs))


@dataclass
class IcpResult:
    pose7: np.ndarray    # [qw qx qy qz tx ty tz]: source -> target
    rms: float           # of the system at pose7; NaN without pairs
    H: np.ndarray        # [6][6], order (omega, v)
    g: np.ndarray        # [6]
    n_pairs: int
    iterations: int      # updates made
    status: int          # OK, NOT_CONVERGED, TOO_FEW, DEGENERATE

    @property
    def matrix(self) -> np.ndarray:
        """pose7 as a 4 x 4 matrix"""
        from .geometry import pose_to_matrix

        return pose_to_matrix(self.pose7)


def _points(a, name: str) -> np.ndarray:
    """[n][3] fp64, contiguous, from an [n][3] array or an organised map [...][3]"""
    p = np.asarray(a, dtype=np.float64)
    if p.ndim < 2 or p.shape[-1] != 3:
        raise ValueError(f"{name} must be an [n][3] array or an organised map [...][3], got {p.shape}")
    return np.ascontiguousarray(p.reshape(-1, 3))


def point_normals(xyz, viewpoint=None, max_jump: float = np.inf) -> np.ndarray:
    """Normals of organised point maps [height][width][3] or [n_maps][height][width][3] (NaN marks an invalid point), oriented towards
    viewpoint (default: the origin); neighbours further than max_jump from the centre are not used.  NaN where there is no normal."""
    lib = capi.load_library()
    p = np.asarray(xyz, dtype=np.float64)
    if p.ndim not in (3, 4) or p.shape[-1] != 3:
        raise ValueError(f"xyz must be [height][width][3] or [n_maps][height][width][3], got {p.shape}")
    maps = np.ascontiguousarray(p if p.ndim == 4 else p[None])
    vp = None if viewpoint is None else np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float64).reshape(3))
    out = np.empty_like(maps)
    capi.check(lib, lib.cba_point_normals(maps.shape[0], maps.shape[1], maps.shape[2], dptr(maps), dptr(vp), float(max_jump), dptr(out)))
    return out.reshape(p.shape)


class CloudIndex(capi.Handle):
    """``cba_cloud_index``: a uniform grid over a target cloud, built once on the device.  target: [n][3] or an organised map; normals:
    the same shape or None (point-to-plane needs them).  Use as a context manager or call ``close()``."""

    _DESTROY = "cba_cloud_index_destroy"

    def __init__(self, target, normals=None, cell_size: float = 0.0, device: int = 0):
        out = self._out()
        xyz = _points(target, "target")
        nrm = None
        if normals is not None:
            nrm = _points(normals, "normals")
            if nrm.shape != xyz.shape:
                raise ValueError("normals must have the target's shape")
        self.n, self.cell_size, self.has_normals = xyz.shape[0], float(cell_size), nrm is not None
        capi.check(self._lib, self._lib.cba_cloud_index_create(xyz.shape[0], dptr(xyz), dptr(nrm), self.cell_size, int(device), out))

    def nearest(self, query, max_distance: float):
        """-> (index int64 [m], dist2 [m]): the nearest valid target point within max_distance of each query; -1 and NaN when none"""
        h = self._require_open("the index is closed")
        q = _points(query, "query")
        index, dist2 = np.empty(q.shape[0], np.int64), np.empty(q.shape[0])
        capi.check(self._lib, self._lib.cba_cloud_nearest(h, q.shape[0], dptr(q), float(max_distance), i64ptr(index), dptr(dist2)))
        return index, dist2

    def register(self, sources: Sequence, opts: IcpOptions, init_pose7=None) -> list:
        """ICP of each source ([n][3] or an organised map) onto the index, all in one call.  init_pose7: [n_sources][7] or None (identities).
        -> one IcpResult per source."""
        h = self._require_open("the index is closed")
        pts = [_points(s, "source") for s in sources]
        off = np.zeros(len(pts) + 1, np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in pts])
        xyz = np.ascontiguousarray(np.concatenate(pts)) if pts else np.zeros((0, 3))
        init = None
        if init_pose7 is not None:
            init = np.ascontiguousarray(np.asarray(init_pose7, dtype=np.float64).reshape(len(pts), 7))
        res = (CbaIcpResult * max(len(pts), 1))()
        co = opts._c()
        capi.check(self._lib, self._lib.cba_cloud_register(h, len(pts), i64ptr(off), dptr(xyz), dptr(init), C.byref(co), res))
        return [IcpResult(np.array(r.pose7), float(r.rms), np.array(r.H).reshape(6, 6), np.array(r.g), int(r.n_pairs), int(r.iterations),
                          int(r.status)) for r in res[:len(pts)]]


def default_cell_size(max_distance: float) -> float:
    """the smallest cell size that admits max_distance: max_distance / 0.999, one step up where the product rounds below it"""
    cell = float(max_distance) / 0.999
    while 0.999 * cell < max_distance:
        cell = float(np.nextafter(cell, np.inf))
    return cell


def register(source, target, opts: IcpOptions, target_normals=None, init_pose7=None, cell_size: Optional[float] = None,
             viewpoint=None, device: int = 0) -> IcpResult:
    """ICP of one source onto one target ([n][3] arrays or organised maps).  cell_size defaults to max_distance / 0.999.  Point to
    plane without target_normals: the target must be an organised map, and its normals are computed by ``point_normals`` (oriented
    towards viewpoint)."""
    if target_normals is None and opts.metric == POINT_TO_PLANE:
        t = np.asarray(target)
        if t.ndim != 3:
            raise ValueError("point-to-plane needs target_normals or an organised target map")
        target_normals = point_normals(t, viewpoint)
    cell = default_cell_size(opts.max_distance) if cell_size is None else cell_size
    with CloudIndex(target, target_normals, cell, device) as index:
        return index.register([source], opts, None if init_pose7 is None else np.asarray(init_pose7, dtype=np.float64).reshape(1, 7))[0]
