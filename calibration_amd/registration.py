"""Scan registration on the GPU (``cba_point_normals``, ``cba_cloud_index``, ``cba_cloud_nearest``, ``cba_cloud_register``): normals of
organised point maps, a uniform grid over a target cloud with an exact nearest-neighbour search inside a radius, and ICP (point to
plane or point to point) of a ragged batch of sources onto it; and the alignment of many scans at once over a graph of overlapping
pairs with one pose held (``cba_cloud_set``, ``cba_cloud_align``), by the rules calibba.h states.  The reference has no counterpart.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import capi
from .capi import CbaAlignEdge, CbaAlignOptions, CbaAlignResult, CbaIcpOptions, CbaIcpResult, dptr, i32ptr, i64ptr

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


# ---- alignment of many scans --------------------------------------------------------------------------------------------------------
@dataclass
class AlignEdge:
    """``cba_align_edge``: the system of one edge (source, target) at the returned poses, in the target scan's frame"""
    H: np.ndarray    # [6][6]
    g: np.ndarray    # [6]
    ss: float
    n_pairs: int
    used: bool       # n_pairs reached the floor, so the edge is part of the system of all scans


@dataclass
class AlignResult:
    poses: np.ndarray    # [n_scans][7]: scan k -> the common frame
    rms: float           # over the used edges at poses; NaN without pairs
    n_pairs: int
    n_used_edges: int
    iterations: int      # rounds with an update
    status: int          # OK, NOT_CONVERGED, TOO_FEW, DEGENERATE
    edges: list          # one AlignEdge per edge of the call


def _edge_array(edges) -> np.ndarray:
    e = np.asarray(edges, dtype=np.int64)
    if e.size == 0:
        return np.zeros((0, 2), np.int32)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError(f"edges must be [n_edges][2] (source, target), got {e.shape}")
    if e.min() < -2 ** 31 or e.max() >= 2 ** 31:
        raise ValueError("edges must hold scan numbers")
    return np.ascontiguousarray(e.astype(np.int32))


class CloudSet(capi.Handle):
    """``cba_cloud_set``: N scans ([n][3] arrays or organised maps), each with a grid of its own on the device, and their points as
    sources.  normals: one array per scan of the scan's shape, or None (point to plane needs them).  Use as a context manager or call
    ``close()``."""

    _DESTROY = "cba_cloud_set_destroy"

    def __init__(self, scans: Sequence, normals: Optional[Sequence] = None, cell_size: float = 0.0, device: int = 0):
        out = self._out()
        pts = [_points(s, "scan") for s in scans]
        nrm = None
        if normals is not None:
            nrms = [_points(n, "normals") for n in normals]
            if [n.shape for n in nrms] != [p.shape for p in pts]:
                raise ValueError("normals must have the scans' shapes")
            nrm = np.ascontiguousarray(np.concatenate(nrms)) if nrms else np.zeros((0, 3))
        off = np.zeros(len(pts) + 1, np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in pts])
        xyz = np.ascontiguousarray(np.concatenate(pts)) if pts else np.zeros((0, 3))
        self.n_scans, self.cell_size, self.has_normals = len(pts), float(cell_size), nrm is not None
        capi.check(self._lib, self._lib.cba_cloud_set_create(len(pts), i64ptr(off), dptr(xyz), dptr(nrm), self.cell_size, int(device), out))

    def align(self, edges, opts: IcpOptions, init_pose7=None, fixed: int = 0) -> AlignResult:
        """The poses of all scans over the edges [(source, target), ...], scan ``fixed`` held.  init_pose7: [n_scans][7] or None
        (identities)."""
        h = self._require_open("the set is closed")
        e = _edge_array(edges)
        init = None
        if init_pose7 is not None:
            init = np.ascontiguousarray(np.asarray(init_pose7, dtype=np.float64).reshape(self.n_scans, 7))
        poses = np.empty((self.n_scans, 7))
        out = (CbaAlignEdge * max(e.shape[0], 1))()
        res = CbaAlignResult()
        co = CbaAlignOptions(opts._c(), int(fixed))
        capi.check(self._lib, self._lib.cba_cloud_align(h, e.shape[0], i32ptr(e), dptr(init), C.byref(co), dptr(poses), out, C.byref(res)))
        return AlignResult(poses, float(res.rms), int(res.n_pairs), int(res.n_used_edges), int(res.iterations), int(res.status),
                           [AlignEdge(np.array(o.H).reshape(6, 6), np.array(o.g), float(o.ss), int(o.n_pairs), bool(o.used))
                            for o in out[:e.shape[0]]])

    def overlaps(self, poses, max_distance: float, metric: int = POINT_TO_POINT) -> np.ndarray:
        """[n_scans][n_scans] pair counts at the given poses: entry (a, b) is how many points of scan a have a neighbour in scan b
        within max_distance (with metric 0: one that has a normal).  A composition: all ordered pairs as edges with
        max_iterations = 0, in calls of at most 1024 edges."""
        n = self.n_scans
        pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
        counts = np.zeros((n, n), np.int64)
        opts = IcpOptions(max_distance, metric=metric, max_iterations=0)
        for first in range(0, len(pairs), capi.ALIGN_MAX_EDGES):
            part = pairs[first:first + capi.ALIGN_MAX_EDGES]
            for (a, b), e in zip(part, self.align(part, opts, init_pose7=poses).edges):
                counts[a, b] = e.n_pairs
        return counts


def edges_from_overlaps(counts, min_pairs: int) -> list:
    """The directed edges (a, b), a != b, whose pair count reaches min_pairs, in row-major order"""
    c = np.asarray(counts)
    return [(int(a), int(b)) for a in range(c.shape[0]) for b in range(c.shape[1]) if a != b and c[a, b] >= min_pairs]


def align(scans: Sequence, edges, opts: IcpOptions, normals: Optional[Sequence] = None, init_pose7=None, fixed: int = 0,
          cell_size: Optional[float] = None, viewpoint=None, device: int = 0) -> AlignResult:
    """One-shot alignment of scans over edges.  cell_size defaults to max_distance / 0.999.  Point to plane without normals: the
    scans must be organised maps, and their normals are computed by ``point_normals`` (oriented towards viewpoint, in each scan's
    own frame)."""
    if normals is None and opts.metric == POINT_TO_PLANE:
        if any(np.asarray(s).ndim != 3 for s in scans):
            raise ValueError("point-to-plane needs normals or organised scan maps")
        normals = [point_normals(s, viewpoint) for s in scans]
    cell = default_cell_size(opts.max_distance) if cell_size is None else cell_size
    with CloudSet(scans, normals, cell, device) as cloud_set:
        return cloud_set.align(edges, opts, init_pose7, fixed)
