"""Scan fusion on the GPU (``cba_tsdf_volume``, ``cba_tsdf_integrate``, ``cba_tsdf_extract``, ``cba_tsdf_mesh``, ``cba_tsdf_raycast``):
depth maps of one object, each with its pose, are merged into a truncated signed distance volume, and the surface is read off it as
points with normals on the lattice edges, as triangles over those points, and as what a camera at a given pose sees of it (depth,
points and normals per pixel), by the rules calibba.h states.  With the cameras' images behind the depth maps
(``cba_tsdf_integrate_colour``) the volume also keeps a colour per voxel, and the points, the mesh and the ray cast carry it.  ``track`` registers a new scan against the model's ray cast.  The
reference has no counterpart.  The mesh statistics, the PLY files and the clouds of a ray cast are host work in numpy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from . import capi
from .capi import CbaTsdfOptions, CbaTsdfRaycastOptions, dptr, i32ptr, i64ptr, u8ptr
from .geometry import quat_to_rotmat


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


@dataclass
class RayCastOptions:
    """``cba_tsdf_raycast_options``: the march's step (0: half a voxel; at least voxel_size / 16), the share of F times the truncation
    that a valid sample may advance by (in [0, 1]; 0: fixed steps), the depth range of the rays, and the weight all eight voxels of a
    sampled cell must have."""
    step: float = 0.0
    skip: float = 0.5
    near_depth: float = 0.0
    far_depth: float = np.inf
    min_weight: float = 1.0

    def _c(self) -> CbaTsdfRaycastOptions:
        return CbaTsdfRaycastOptions(float(self.step), float(self.skip), float(self.near_depth), float(self.far_depth), float(self.min_weight))


MISS, HIT, BEHIND, NO_RAY = capi.TSDF_RAY_MISS, capi.TSDF_RAY_HIT, capi.TSDF_RAY_BEHIND, capi.TSDF_RAY_NO_RAY


def rgba_maps(colour, shape: Tuple[int, int, int]) -> np.ndarray:
    """The images behind depth maps of shape = (n_maps, height, width) as uint8 [n_maps][height][width][4]: grey [n][H][W] is
    replicated, and grey and [n][H][W][3] get A = 255; [n][H][W][4] is taken as it is (A == 0: the pixel has no colour).  One image
    may be given for one map.  Host work."""
    c = np.asarray(colour)
    if c.dtype != np.uint8:
        raise ValueError(f"colour must be uint8, got {c.dtype}")
    n, H, W = shape
    if n == 1 and c.shape in ((H, W), (H, W, 3), (H, W, 4)) and c.shape[:3] != (n, H, W):
        c = c[None]
    if c.shape == (n, H, W):
        c = np.repeat(c[..., None], 3, axis=-1)
    if c.shape == (n, H, W, 3):
        c = np.concatenate([c, np.full((n, H, W, 1), 255, np.uint8)], axis=-1)
    if c.shape != (n, H, W, 4):
        raise ValueError(f"colour must be [{n}][{H}][{W}], [..][3] or [..][4], got {c.shape}")
    return np.ascontiguousarray(c)


def _rigid(pose7) -> Tuple[np.ndarray, np.ndarray]:
    """R, t of a rigid pose7 (the quaternion normalised)"""
    p = np.asarray(pose7, dtype=np.float64).reshape(7)
    return quat_to_rotmat(p[:4] / np.linalg.norm(p[:4])), p[4:]


def pose_inverse(pose7) -> np.ndarray:
    """The inverse of a rigid pose7."""
    p = np.asarray(pose7, dtype=np.float64).reshape(7)
    q = p[:4] / np.linalg.norm(p[:4]) * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([q, -(quat_to_rotmat(q) @ p[4:])])


@dataclass
class RayCast:
    """What cameras at n_views poses see of a volume: depth [n_views][height][width], xyz and normals [..][3] in each camera's frame
    (organised maps, NaN where a pixel is no hit; a hit's normal is NaN where there is none), status uint8 [..] (MISS, HIT, BEHIND,
    NO_RAY) and the rays table [height][width][2]; rgba uint8 [n_views][height][width][4] when the volume has colour (A = 255 where
    a hit has a colour, all four 0 elsewhere)."""
    depth: np.ndarray
    xyz: np.ndarray
    normals: np.ndarray
    status: np.ndarray
    rays: np.ndarray
    rgba: Optional[np.ndarray] = None

    @property
    def hits(self) -> np.ndarray:
        return self.status == HIT

    def cloud(self, view: int, pose7) -> Tuple[np.ndarray, np.ndarray]:
        """-> (xyz [n][3], normals [n][3]) of view's hits in the volume frame, in row-major pixel order; pose7: that view's rigid pose,
        volume frame -> camera"""
        R, t = _rigid(pose7)
        m = self.hits[view]
        return (self.xyz[view][m] - t) @ R, self.normals[view][m] @ R


@dataclass
class Mesh:
    """Indexed triangles over surface points: xyz [n][3], normals [n][3] (NaN where a point has none), triangles int32 [m][3].
    (p1 - p0) x (p2 - p0) of a triangle points into positive D: out of the scanned object.  colours: uint8 [n][4] = R, G, B, A of the
    points when the volume has colour (A = 0: the point has none)."""
    xyz: np.ndarray
    normals: np.ndarray
    triangles: np.ndarray
    colours: Optional[np.ndarray] = None

    def _corners(self) -> np.ndarray:
        return self.xyz[self.triangles.astype(np.int64)]

    def area(self) -> float:
        p = self._corners()
        return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())

    def volume(self) -> float:
        """The volume the surface encloses, by the divergence theorem (the sum of p0 . (p1 x p2) / 6): meaningful for a closed mesh."""
        p = self._corners()
        return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)

    def boundary_edges(self) -> np.ndarray:
        """The directed edges u -> v [n][2] that occur more often than their reverse v -> u, each once per surplus occurrence, sorted:
        empty for a closed oriented mesh."""
        t = self.triangles.astype(np.int64)
        h = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        if len(h) == 0:
            return np.zeros((0, 2), np.int64)
        both = np.concatenate([h, h[:, ::-1]])
        sign = np.concatenate([np.ones(len(h), np.int64), -np.ones(len(h), np.int64)])
        uniq, inv = np.unique(both, axis=0, return_inverse=True)
        net = np.bincount(inv.ravel(), weights=sign, minlength=len(uniq)).astype(np.int64)
        return np.repeat(uniq, np.maximum(net, 0), axis=0)

    def compact(self) -> "Mesh":
        """Without the points no triangle refers to, renumbered, in the same order."""
        used = np.zeros(len(self.xyz), bool)
        used[self.triangles.ravel()] = True
        new = (np.cumsum(used) - 1).astype(np.int32)
        return Mesh(self.xyz[used], self.normals[used], new[self.triangles.astype(np.int64)].reshape(-1, 3),
                    None if self.colours is None else self.colours[used])


_PLY_XYZ = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
_PLY_NORMAL = [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
_PLY_COLOUR = [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, mesh: Mesh, normals: Optional[bool] = None) -> None:
    """A binary little-endian PLY file: vertices as float64 x y z, then nx ny nz when ``normals`` is True or, by default, when every
    normal is finite, then uchar red green blue alpha when ``mesh.colours`` is set; faces as ``list uchar int``."""
    if normals is None:
        normals = bool(np.isfinite(mesh.normals).all())
    colours = mesh.colours is not None
    fields = _PLY_XYZ + (_PLY_NORMAL if normals else []) + (_PLY_COLOUR if colours else [])
    v = np.empty(len(mesh.xyz), np.dtype(fields))
    for c, (name, _) in enumerate(_PLY_XYZ):
        v[name] = mesh.xyz[:, c]
    if normals:
        for c, (name, _) in enumerate(_PLY_NORMAL):
            v[name] = mesh.normals[:, c]
    if colours:
        for c, (name, _) in enumerate(_PLY_COLOUR):
            v[name] = mesh.colours[:, c]
    f = np.empty(len(mesh.triangles), _PLY_FACE)
    f["n"], f["v"] = 3, mesh.triangles
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'uchar' if kind == 'u1' else 'double'} {name}" for name, kind in fields]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def read_ply(path) -> Mesh:
    """What ``write_ply`` wrote, and only that dialect; normals are NaN and colours None when the file has none."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    if head[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError("not a binary little-endian PLY file")
    names, kinds, n_vertex, n_face = [], [], None, None
    for line in head[2:]:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            n_vertex = int(w[2])
        elif w[:2] == ["element", "face"]:
            n_face = int(w[2])
        elif w[:2] in (["property", "double"], ["property", "uchar"]) and len(w) == 3 and n_face is None:
            names.append(w[2])
            kinds.append(w[1])
        elif w and w != ["end_header"] and w != ["property", "list", "uchar", "int", "vertex_indices"]:
            raise ValueError(f"not the dialect write_ply writes: {line!r}")
    with_colours = names[-4:] == [n for n, _ in _PLY_COLOUR]
    geometry = names[:-4] if with_colours else names
    with_normals = geometry == [n for n, _ in _PLY_XYZ + _PLY_NORMAL]
    fields = _PLY_XYZ + (_PLY_NORMAL if with_normals else []) + (_PLY_COLOUR if with_colours else [])
    if n_vertex is None or n_face is None or not (with_normals or geometry == [n for n, _ in _PLY_XYZ]) or \
            kinds != ["uchar" if kind == "u1" else "double" for _, kind in fields]:
        raise ValueError("not the dialect write_ply writes")
    vt = np.dtype(fields)
    if len(data) != end + n_vertex * vt.itemsize + n_face * _PLY_FACE.itemsize:
        raise ValueError("the file's length does not match its header")
    v = np.frombuffer(data, vt, n_vertex, end)
    f = np.frombuffer(data, _PLY_FACE, n_face, end + n_vertex * vt.itemsize)
    if not (f["n"] == 3).all():
        raise ValueError("a face is not a triangle")
    xyz = np.stack([v[n] for n, _ in _PLY_XYZ], axis=1) if n_vertex else np.zeros((0, 3))
    nrm = np.stack([v[n] for n, _ in _PLY_NORMAL], axis=1) if with_normals and n_vertex else np.full((n_vertex, 3), np.nan)
    colours = np.stack([v[n] for n, _ in _PLY_COLOUR], axis=1).reshape(-1, 4) if with_colours else None
    return Mesh(np.ascontiguousarray(xyz), np.ascontiguousarray(nrm), np.ascontiguousarray(f["v"]).reshape(-1, 3), colours)


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

    def integrate(self, camera_model: int, intr, poses, depth=None, xyz=None, colour=None) -> None:
        """Apply depth maps [n_maps][height][width] (or one [height][width]) in order; poses [n_maps][7]: volume frame -> camera.
        ``xyz``: organised point maps in the camera's frame instead (``depth_from_xyz``).  ``colour``: the camera's images on the
        maps' pixel grid, uint8 [n_maps][height][width], [..][3] or [..][4] (``rgba_maps``): the volume takes colour too."""
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
        if colour is None:
            capi.check(self._lib, self._lib.cba_tsdf_integrate(h, int(camera_model), dptr(k), d.shape[0], d.shape[1], d.shape[2], dptr(d), dptr(pose)))
            return
        rgba = rgba_maps(colour, d.shape)
        capi.check(self._lib, self._lib.cba_tsdf_integrate_colour(h, int(camera_model), dptr(k), d.shape[0], d.shape[1], d.shape[2], dptr(d),
                                                                  u8ptr(rgba), dptr(pose)))

    @property
    def has_colour(self) -> bool:
        out = np.zeros(1, np.int32)
        capi.check(self._lib, self._lib.cba_tsdf_has_colour(self._require_open("the volume is closed"), i32ptr(out)))
        return bool(out[0])

    def fetch_colour(self) -> np.ndarray:
        """-> the {R, G, B, Wc} records, float32 [nz][ny][nx][4]; the volume must have colour"""
        h = self._require_open("the volume is closed")
        nx, ny, nz = self.shape
        colour = np.empty((nz, ny, nx, 4), np.float32)
        capi.check(self._lib, self._lib.cba_tsdf_colour_fetch(h, _fptr(colour)))
        return colour

    def upload_colour(self, colour) -> None:
        """Write records [nz][ny][nx][4] that ``fetch_colour`` returned; a volume without colour has it afterwards."""
        h = self._require_open("the volume is closed")
        nx, ny, nz = self.shape
        a = np.ascontiguousarray(np.asarray(colour, dtype=np.float32))
        if a.shape != (nz, ny, nx, 4):
            raise ValueError(f"colour must be [{nz}][{ny}][{nx}][4], got {a.shape}")
        capi.check(self._lib, self._lib.cba_tsdf_colour_upload(h, _fptr(a)))

    def _point_colours(self, h, n: int) -> np.ndarray:
        rgba = np.empty((n, 4), np.uint8)
        capi.check(self._lib, self._lib.cba_tsdf_extract_fetch_colour(h, u8ptr(rgba)))
        return rgba

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

    def extract(self, min_weight: float = 1.0, colour: bool = False):
        """-> (xyz [n][3], normals [n][3]): the zero crossings on lattice edges in visiting order; a normal is NaN where there is none.
        ``colour``: -> (xyz, normals, rgba uint8 [n][4]); the volume must have colour"""
        h = self._require_open("the volume is closed")
        n = np.zeros(1, np.int64)
        capi.check(self._lib, self._lib.cba_tsdf_extract(h, float(min_weight), i64ptr(n)))
        xyz, normals = np.empty((int(n[0]), 3)), np.empty((int(n[0]), 3))
        capi.check(self._lib, self._lib.cba_tsdf_extract_fetch(h, dptr(xyz), dptr(normals)))
        return (xyz, normals, self._point_colours(h, int(n[0]))) if colour else (xyz, normals)

    def mesh(self, min_weight: float = 1.0, compact: bool = False) -> Mesh:
        """The surface as triangles over the points ``extract(min_weight)`` gives: a cell of eight voxels that all have W >= min_weight
        is cut by the rule calibba.h states.  Points that no such cell touches stay in the list unreferenced; ``compact`` drops them."""
        h = self._require_open("the volume is closed")
        n, m = np.zeros(1, np.int64), np.zeros(1, np.int64)
        capi.check(self._lib, self._lib.cba_tsdf_mesh(h, float(min_weight), i64ptr(n), i64ptr(m)))
        xyz, normals, tri = np.empty((int(n[0]), 3)), np.empty((int(n[0]), 3)), np.empty((int(m[0]), 3), np.int32)
        capi.check(self._lib, self._lib.cba_tsdf_extract_fetch(h, dptr(xyz), dptr(normals)))
        capi.check(self._lib, self._lib.cba_tsdf_mesh_fetch(h, i32ptr(tri)))
        out = Mesh(xyz, normals, tri, self._point_colours(h, int(n[0])) if self.has_colour else None)
        return out.compact() if compact else out

    def raycast(self, camera_model: int, intr, poses, shape: Tuple[int, int], opts: Optional[RayCastOptions] = None) -> RayCast:
        """The model as cameras at poses [n_views][7] (volume frame -> camera) see it, in views of shape = (height, width)."""
        h = self._require_open("the volume is closed")
        H, W = (int(v) for v in shape)
        pose = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
        k = np.ascontiguousarray(np.asarray(intr, dtype=np.float64).reshape(-1))
        if k.size != (12 if camera_model == 1 else 10):
            raise ValueError(f"intr has {k.size} entries")
        co = (opts or RayCastOptions())._c()
        capi.check(self._lib, self._lib.cba_tsdf_raycast(h, int(camera_model), dptr(k), pose.shape[0], H, W, dptr(pose), C.byref(co)))
        n = pose.shape[0]
        out = RayCast(np.empty((n, H, W)), np.empty((n, H, W, 3)), np.empty((n, H, W, 3)), np.empty((n, H, W), np.uint8), np.empty((H, W, 2)))
        if n > 0:
            capi.check(self._lib, self._lib.cba_tsdf_raycast_fetch(h, dptr(out.depth), dptr(out.xyz), dptr(out.normals), u8ptr(out.status),
                                                                   dptr(out.rays)))
            if self.has_colour:
                out.rgba = np.empty((n, H, W, 4), np.uint8)
                capi.check(self._lib, self._lib.cba_tsdf_raycast_fetch_colour(h, u8ptr(out.rgba)))
        else:
            out.rays[:] = np.nan  # no work was done: there is no table
        return out

    def reset(self) -> None:
        capi.check(self._lib, self._lib.cba_tsdf_reset(self._require_open("the volume is closed")))


def fuse(shape, origin, opts: TsdfOptions, camera_model: int, intr, poses, depth=None, xyz=None, min_weight: float = 1.0, device: int = 0,
         mesh: bool = False, colour=None) -> Union[Tuple[np.ndarray, ...], Mesh]:
    """One volume, one integrate, one extract: -> (xyz [n][3], normals [n][3]); with ``mesh=True`` one mesh instead: -> Mesh.
    ``colour``: the images behind the maps (``TsdfVolume.integrate``): -> (xyz, normals, rgba uint8 [n][4]), or a Mesh with colours"""
    with TsdfVolume(shape, origin, opts, device) as vol:
        vol.integrate(camera_model, intr, poses, depth=depth, xyz=xyz, colour=colour)
        if mesh:
            return vol.mesh(min_weight)
        if colour is None:
            return vol.extract(min_weight)
        if not vol.has_colour:  # no maps: no work was done and nothing was allocated; there are no points either
            return vol.extract(min_weight) + (np.zeros((0, 4), np.uint8),)
        return vol.extract(min_weight, colour=True)


def track(vol: TsdfVolume, camera_model: int, intr, init_pose7, depth=None, xyz=None, icp=None, opts: Optional[RayCastOptions] = None):
    """Frame-to-model registration of one new scan (a depth map [height][width], or an organised map ``xyz`` in the camera's frame):
    the model is ray cast at init_pose7 (volume frame -> camera), a ``CloudIndex`` is put over that view's hits in the volume frame,
    and the scan's points are registered onto it from the inverse of init_pose7.  icp: ``IcpOptions`` (default: point to plane within
    two voxels).  -> (the refined pose7 volume frame -> camera, the ``IcpResult``, whose pose7 maps the camera to the volume frame)."""
    from .registration import CloudIndex, IcpOptions, default_cell_size

    if (depth is None) == (xyz is None):
        raise ValueError("give depth or xyz, one of them")
    init = np.asarray(init_pose7, dtype=np.float64).reshape(7)
    if depth is not None:
        d = np.asarray(depth, dtype=np.float64)
        if d.ndim != 2:
            raise ValueError(f"depth must be [height][width], got {d.shape}")
        shape = d.shape
    else:
        pts = np.asarray(xyz, dtype=np.float64)
        if pts.ndim != 3 or pts.shape[-1] != 3:
            raise ValueError(f"xyz must be [height][width][3], got {pts.shape}")
        shape = pts.shape[:2]
    icp = icp or IcpOptions(2.0 * vol.opts.voxel_size)
    cast = vol.raycast(camera_model, intr, init[None], shape, opts)
    if depth is not None:
        pts = np.concatenate([cast.rays * d[..., None], d[..., None]], axis=-1)  # the scan's points on the model's own rays
    src = pts.reshape(-1, 3)
    src = src[np.isfinite(src).all(axis=1)]
    target, normals = cast.cloud(0, init)
    with CloudIndex(target, normals, default_cell_size(icp.max_distance)) as index:
        res = index.register([src], icp, init_pose7=pose_inverse(init)[None])[0]
    return pose_inverse(res.pose7), res
