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


class _Detector(capi.Handle):
    """What the two detector handles share: the create call, the image batch, the outputs every detector has and the process call.
    A subclass names its functions (``_FN``) and states its options struct (``_options``), its own outputs as (trailing shape, ...)
    in the order of the C call between xy and response (``_EXTRA``) and its result type (``_RESULT``: count, status, xy, the extra
    outputs, response, flags)."""

    def __init__(self, width: int, height: int, max_images: int, max_items: int, opts, device: int):
        self._DESTROY = self._FN + "_destroy"
        out = self._out()
        co = self._options(opts)
        self.width, self.height, self.max_images, self._max_items = int(width), int(height), int(max_images), int(max_items)
        capi.check(self._lib, getattr(self._lib, self._FN + "_create")(self.width, self.height, self.max_images, self._max_items,
                                                                       C.byref(co), int(device), out))

    def process(self, images):
        """images: [n][height][width] uint8 (or one [height][width] image)."""
        h = self._require_open("the detector is closed")
        img = capi.u8_batch(images, "images", self.height, self.width, "n", self.max_images,
                            "{} images given, the detector was created for " + str(self.max_images))
        n, m = img.shape[0], self._max_items
        count, status, xy = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full((n, m, 2), np.nan)
        extra = [np.full((n, m) + tail, np.nan) for tail in self._EXTRA]
        response, flags = np.zeros((n, m), np.int32), np.zeros((n, m), np.int32)
        capi.check(self._lib, getattr(self._lib, self._FN + "_process")(h, n, u8ptr(img), i32ptr(count), i32ptr(status), dptr(xy),
                                                                        *[dptr(e) for e in extra], i32ptr(response), i32ptr(flags)))
        return self._RESULT(count, status, xy, *extra, response, flags)


class CornerDetector(_Detector):
    """``cba_corner_detector``: uint8 images of one size in, corners out.  The device buffers are sized for max_images and
    max_corners at construction.  Use as a context manager or call ``close()``."""

    _FN, _EXTRA, _RESULT = "cba_corner_detector", ((),), CornerResult  # angle [n][max_corners]

    def __init__(self, width: int, height: int, max_images: int = 1, max_corners: int = 1024, opts: Optional[CornerOptions] = None,
                 device: int = 0):
        super().__init__(width, height, max_images, max_corners, opts, device)
        self.max_corners = self._max_items

    @staticmethod
    def _options(o):
        o = o or CornerOptions()
        return CbaCornerOptions(int(o.min_response), int(o.nms_radius), int(o.cog_radius), int(o.refine), int(o.refine_half_window),
                                int(o.refine_iterations))


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


# ---- circle grids (cba_blob_detector, cba_circle_grid_order) ---------------------------------------------------------------------------
BLOB_DARK, BLOB_BRIGHT = 0, 1
CIRCLES_SYMMETRIC, CIRCLES_ASYMMETRIC = 0, 1
BLOB_FLAG_WINDOW, BLOB_FLAG_NO_EDGE, BLOB_FLAG_DEGENERATE, BLOB_FLAG_SHAPE, BLOB_FLAG_RATIO, BLOB_FLAG_SIZE, BLOB_FLAG_DUPLICATE = (
    1, 2, 4, 8, 16, 32, 64)


@dataclass
class BlobOptions:
    """``cba_blob_options``: polarity, the half sides of the inner and outer box, the lowest contrast of a peak in grey levels, the
    suppression radius, the longest ray, the centroid rounds and the three limits behind FLAG_SHAPE, FLAG_RATIO and FLAG_SIZE."""
    polarity: int = BLOB_DARK
    inner_half: int = 2
    outer_half: int = 12
    min_contrast: int = 30
    nms_radius: int = 4
    max_radius: int = 20
    rounds: int = 3
    max_fit_error: float = 0.2
    max_axis_ratio: float = 3.0
    min_radius: float = 1.5


@dataclass
class BlobResult:
    count: np.ndarray      # [n] int32: the true number of peaks of every image
    status: np.ndarray     # [n] int32: STATUS_OVERFLOW
    xy: np.ndarray         # [n][max_blobs][2] float64, NaN past the kept blobs
    shape: np.ndarray      # [n][max_blobs][3] float64 (m_xx, m_xy, m_yy) of the ellipse {d : d^T M^-1 d = 1}; NaN when flagged early
    fit_error: np.ndarray  # [n][max_blobs] float64
    response: np.ndarray   # [n][max_blobs] int32
    flags: np.ndarray      # [n][max_blobs] int32: BLOB_FLAG_*

    def kept(self, i: int) -> int:
        return int(min(self.count[i], self.xy.shape[1]))

    @property
    def semi_axes(self) -> np.ndarray:
        """[n][max_blobs][2] (major, minor): the square roots of the eigenvalues of M"""
        h, d = 0.5 * (self.shape[..., 0] + self.shape[..., 2]), 0.5 * (self.shape[..., 0] - self.shape[..., 2])
        s = np.sqrt(d * d + self.shape[..., 1] ** 2)
        return np.stack([np.sqrt(h + s), np.sqrt(h - s)], axis=-1)

    @property
    def angle(self) -> np.ndarray:
        """[n][max_blobs]: direction of the major axis, in (-pi/2, pi/2], x right and y down"""
        return 0.5 * np.arctan2(2.0 * self.shape[..., 1], self.shape[..., 0] - self.shape[..., 2])


class BlobDetector(_Detector):
    """``cba_blob_detector``: uint8 images of one size in, blobs out.  The device buffers are sized for max_images and max_blobs at
    construction.  Use as a context manager or call ``close()``."""

    _FN, _EXTRA, _RESULT = "cba_blob_detector", ((3,), ()), BlobResult  # shape [n][max_blobs][3], fit_error [n][max_blobs]

    def __init__(self, width: int, height: int, max_images: int = 1, max_blobs: int = 1024, opts: Optional[BlobOptions] = None,
                 device: int = 0):
        super().__init__(width, height, max_images, max_blobs, opts, device)
        self.max_blobs = self._max_items

    @staticmethod
    def _options(o):
        o = o or BlobOptions()
        return capi.CbaBlobOptions(int(o.polarity), int(o.inner_half), int(o.outer_half), int(o.min_contrast), int(o.nms_radius),
                                   int(o.max_radius), int(o.rounds), 0, float(o.max_fit_error), float(o.max_axis_ratio), float(o.min_radius))


def circle_grid_points(rows: int, cols: int, spacing: float = 1.0, pattern: int = CIRCLES_ASYMMETRIC) -> np.ndarray:
    """[rows cols][2], row-major over (j, i): SYMMETRIC (i, j) spacing; ASYMMETRIC ((2 i + j mod 2) spacing, j spacing)"""
    jj, ii = np.divmod(np.arange(rows * cols), cols)
    x = ii if pattern == CIRCLES_SYMMETRIC else 2 * ii + jj % 2
    return np.stack([x * float(spacing), jj * float(spacing)], axis=1)


def order_circle_grid(xy, shape, pattern: int, rows: int, cols: int):
    """``cba_circle_grid_order``: one image's blobs xy [n][2] and their shapes [n][3] (or None: the identity metric) -> (index
    [rows cols] into them, row-major over (j, i), or None when the grid is not found; unique: whether exactly one labelling fits)."""
    lib = capi.load_library()
    p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64))
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"xy must have shape [n][2], got {p.shape}")
    m = None
    if shape is not None:
        m = np.ascontiguousarray(np.asarray(shape, dtype=np.float64))
        if m.shape != (p.shape[0], 3):
            raise ValueError(f"shape must have shape [{p.shape[0]}][3], got {m.shape}")
    index = np.full(int(rows) * int(cols) if rows > 0 and cols > 0 else 1, -1, np.int32)
    unique = np.zeros(1, np.int32)
    capi.check(lib, lib.cba_circle_grid_order(p.shape[0], dptr(p), None if m is None else dptr(m), int(pattern), int(rows), int(cols),
                                              i32ptr(index), i32ptr(unique)))
    return (None, False) if index[0] < 0 else (index, bool(unique[0]))


def _dlt_homography(obj: np.ndarray, uv: np.ndarray) -> np.ndarray:
    """normalised DLT, obj [n][2] -> uv [n][2]"""
    def norm(p):
        m = p.mean(axis=0)
        s = np.sqrt(2.0) / np.linalg.norm(p - m, axis=1).mean()
        return np.array([[s, 0.0, -s * m[0]], [0.0, s, -s * m[1]], [0.0, 0.0, 1.0]])

    To, Tu = norm(obj), norm(uv)
    a, b = np.c_[obj, np.ones(len(obj))] @ To.T, np.c_[uv, np.ones(len(uv))] @ Tu.T
    z = np.zeros_like(a)
    A = np.concatenate([np.c_[a, z, -b[:, :1] * a], np.c_[z, a, -b[:, 1:2] * a]], axis=0)
    h = np.linalg.svd(A)[2][-1].reshape(3, 3)
    Hm = np.linalg.inv(Tu) @ h @ To
    return Hm / Hm[2, 2]


def circle_centre_bias(H, object_xy, radius: float) -> np.ndarray:
    """The perspective bias of an ellipse's centre, [n][2] px: the circle of ``radius`` round (X, Y) is the conic C, its image under the
    board-to-image homography H is H^-T C H^-1, and the bias is that conic's centre minus the projection of (X, Y).  Lens distortion
    is ignored: H is a pinhole map, so with a distorted camera the value is the bias to first order only."""
    Hm = np.asarray(H, dtype=np.float64).reshape(3, 3)
    obj = np.asarray(object_xy, dtype=np.float64).reshape(-1, 2)
    Hi = np.linalg.inv(Hm)
    X, Y = obj[:, 0], obj[:, 1]
    one, zero = np.ones_like(X), np.zeros_like(X)
    Cm = np.stack([np.stack([one, zero, -X], 1), np.stack([zero, one, -Y], 1), np.stack([-X, -Y, X * X + Y * Y - float(radius) ** 2], 1)], 1)
    Q = Hi.T[None] @ Cm @ Hi[None]
    centre = np.linalg.solve(Q[:, :2, :2], -Q[:, :2, 2:3])[:, :, 0]
    p = np.c_[obj, one] @ Hm.T
    return centre - p[:, :2] / p[:, 2:3]


def detect_circle_grid(images, rows: int, cols: int, spacing: float = 1.0, pattern: int = CIRCLES_ASYMMETRIC,
                       opts: Optional[BlobOptions] = None, circle_radius: Optional[float] = None, max_blobs: int = 1024, device: int = 0):
    """Blobs of every image on the device, grid order on the host -> (list of BoardDetection, list of unique).  images: [n][H][W]
    uint8; rows x cols circles at ``spacing``.  Blobs that carry a flag are left out before ordering.  With ``circle_radius`` (in the
    unit of ``spacing``) the perspective bias of the ellipse centres is subtracted: H from the ordered centres by a normalised DLT,
    ``circle_centre_bias``, once more with H from the corrected centres.  Lens distortion is ignored in that correction."""
    img = np.asarray(images)
    if img.ndim == 2:
        img = img[None]
    if img.ndim != 3:
        raise ValueError(f"images must have shape [n][H][W], got {img.shape}")
    if rows < 2 or cols < 2:
        raise ValueError("rows and cols must be >= 2")
    if pattern not in (CIRCLES_SYMMETRIC, CIRCLES_ASYMMETRIC):
        raise ValueError("pattern must be CIRCLES_SYMMETRIC or CIRCLES_ASYMMETRIC")
    if circle_radius is not None and not circle_radius > 0:
        raise ValueError("circle_radius must be > 0")
    obj = circle_grid_points(rows, cols, spacing, pattern)
    out, uniq = [], []
    if img.shape[0] == 0:
        return out, uniq
    with BlobDetector(img.shape[2], img.shape[1], img.shape[0], max_blobs, opts, device) as det:
        res = det.process(img)
    for i in range(img.shape[0]):
        k = res.kept(i)
        good = np.flatnonzero(res.flags[i, :k] == 0)
        index, unique = order_circle_grid(res.xy[i, good], res.shape[i, good], pattern, rows, cols) if good.size >= rows * cols else (None, False)
        if index is None:
            out.append(BoardDetection(False, np.full((rows * cols, 2), np.nan), obj.copy(), int(res.count[i])))
        else:
            uv = res.xy[i, good[index]].copy()
            if circle_radius is not None:
                fixed = uv
                for _ in range(2):
                    fixed = uv - circle_centre_bias(_dlt_homography(obj, fixed), obj, circle_radius)
                uv = fixed
            out.append(BoardDetection(True, uv, obj.copy(), int(res.count[i])))
        uniq.append(unique)
    return out, uniq


__all__ = ["CornerOptions", "CornerResult", "BoardDetection", "CornerDetector", "order_chessboard", "detect_chessboard", "REFINE_NONE",
           "REFINE_COG", "REFINE_GRADIENT", "STATUS_OVERFLOW", "FLAG_WINDOW", "FLAG_DET", "FLAG_DRIFT", "BlobOptions", "BlobResult",
           "BlobDetector", "order_circle_grid", "detect_circle_grid", "circle_centre_bias", "circle_grid_points", "BLOB_DARK", "BLOB_BRIGHT",
           "CIRCLES_SYMMETRIC", "CIRCLES_ASYMMETRIC", "BLOB_FLAG_WINDOW", "BLOB_FLAG_NO_EDGE", "BLOB_FLAG_DEGENERATE", "BLOB_FLAG_SHAPE",
           "BLOB_FLAG_RATIO", "BLOB_FLAG_SIZE", "BLOB_FLAG_DUPLICATE"]


# ---- ChArUco boards (cba_charuco_detector, cba_marker_dictionary_generate, cba_chessboard_lattice, cba_charuco_match) -------------
CHARUCO_STATUS_CORNER_OVERFLOW, CHARUCO_STATUS_CELL_OVERFLOW = 1, 2
MARKER_FLAG_DEGENERATE, MARKER_FLAG_WINDOW, MARKER_FLAG_LOW_CONTRAST, MARKER_FLAG_BORDER, MARKER_FLAG_NO_MATCH = 1, 2, 4, 8, 16


def marker_dictionary(bits: int, count: int, min_distance: int, seed: int = 0) -> np.ndarray:
    """``cba_marker_dictionary_generate``: up to ``count`` codes of bits x bits cells, each ``min_distance`` from its own rotations
    and from every rotation of the others.  The result is shorter than ``count`` when the candidate budget ran out."""
    lib = capi.load_library()
    codes, found = np.zeros(max(int(count), 1), np.uint64), np.zeros(1, np.int32)
    capi.check(lib, lib.cba_marker_dictionary_generate(int(bits), int(count), int(min_distance), int(seed) & (2 ** 64 - 1),
                                                       capi.u64ptr(codes), i32ptr(found)))
    return codes[:int(found[0])].copy()


@dataclass
class CharucoBoard:
    """``cba_charuco_board`` with its dictionary: squares_x x squares_y squares of side ``square``, square (0, 0) dark, a marker of
    marker_bits^2 bits in every bright square, ids ascending row-major."""
    squares_x: int
    squares_y: int
    square: float
    codes: np.ndarray
    marker_bits: int = 4
    marker_ratio: float = 0.6

    @property
    def n_corners(self) -> int:
        return (self.squares_x - 1) * (self.squares_y - 1)

    @property
    def object_points(self) -> np.ndarray:
        """[n_corners][2]: inner corner (i, j), index j (squares_x - 1) + i, lies at ((i + 1) square, (j + 1) square)"""
        jj, ii = np.divmod(np.arange(self.n_corners), self.squares_x - 1)
        return np.stack([(ii + 1) * float(self.square), (jj + 1) * float(self.square)], axis=1)

    @property
    def marker_squares(self) -> np.ndarray:
        """[n][2]: the square (sx, sy) of marker id 0, 1, ..."""
        return np.array([(x, y) for y in range(self.squares_y) for x in range(self.squares_x) if (x + y) % 2 == 1], np.int32).reshape(-1, 2)

    def _c(self):
        codes = np.ascontiguousarray(np.asarray(self.codes, dtype=np.uint64).reshape(-1))
        return capi.CbaCharucoBoard(int(self.squares_x), int(self.squares_y), int(self.marker_bits), int(codes.shape[0]), float(self.square),
                                    float(self.marker_ratio)), codes


@dataclass
class CharucoOptions:
    """``cba_charuco_options``: the arm test (lengths, offset, fan, lowest score), the smallest lattice component, the marker read
    (sub-samples per cell, lowest contrast, border errors, corrected bits) and the readings a labelling needs."""
    arm_lengths: tuple = (7.0, 10.0)
    arm_offset: float = 2.0
    arm_fan_deg: float = 14.0
    min_arm_contrast: float = 112.0
    min_marker_contrast: float = 40.0
    min_component: int = 4
    cell_samples: int = 3
    max_border_errors: int = 1
    max_correction: int = 1
    min_markers: int = 2

    def _c(self):
        return capi.CbaCharucoOptions((C.c_double * 2)(float(self.arm_lengths[0]), float(self.arm_lengths[1])), float(self.arm_offset),
                                      float(self.arm_fan_deg), float(self.min_arm_contrast), float(self.min_marker_contrast),
                                      int(self.min_component), int(self.cell_samples), int(self.max_border_errors), int(self.max_correction),
                                      int(self.min_markers), 0)


@dataclass
class CharucoResult:
    count: np.ndarray      # [n] int32: the corners that got a board index
    status: np.ndarray     # [n] int32: CHARUCO_STATUS_*
    ids: np.ndarray        # [n][n_corners] int32 ascending, -1 past count
    xy: np.ndarray         # [n][n_corners][2] float64, NaN past count
    n_markers: np.ndarray  # [n] int32: the readings behind the labellings used
    n_corners: np.ndarray  # [n] int32: the peaks of the corner stage
    n_cells: int           # lattice cells of the call (true number)
    cells: np.ndarray      # [min(n_cells, max_cells)][4] int32: image, component, i, j
    readings: np.ndarray   # [min(n_cells, max_cells)] capi.MARKER_READING


class CharucoDetector(_Detector):
    """``cba_charuco_detector``: uint8 images of one size in, the visible inner corners of a ChArUco board with their board indices out.
    Use as a context manager or call ``close()``.  ``arms`` and ``read`` run the two device stages alone on the images of the last
    ``process``."""

    _FN = "cba_charuco_detector"

    def __init__(self, width: int, height: int, board: CharucoBoard, max_images: int = 1, max_corners: int = 1024, max_cells: int = 4096,
                 corner_opts: Optional[CornerOptions] = None, opts: Optional[CharucoOptions] = None, device: int = 0):
        self._DESTROY = self._FN + "_destroy"
        out = self._out()
        cb, codes = board._c()
        co, ch = CornerDetector._options(corner_opts), (opts or CharucoOptions())._c()
        self.width, self.height, self.max_images, self.max_corners, self.max_cells = int(width), int(height), int(max_images), int(max_corners), int(max_cells)
        self.board = board
        capi.check(self._lib, self._lib.cba_charuco_detector_create(self.width, self.height, self.max_images, self.max_corners, self.max_cells,
                                                                    C.byref(co), C.byref(ch), C.byref(cb), capi.u64ptr(codes), int(device), out))

    def process(self, images) -> CharucoResult:
        h = self._require_open("the detector is closed")
        img = capi.u8_batch(images, "images", self.height, self.width, "n", self.max_images,
                            "{} images given, the detector was created for " + str(self.max_images))
        n, nb = img.shape[0], self.board.n_corners
        count, status, nm, nc = (np.zeros(n, np.int32) for _ in range(4))
        ids, xy = np.full((n, nb), -1, np.int32), np.full((n, nb, 2), np.nan)
        n_cells, cells = np.zeros(1, np.int32), np.zeros((self.max_cells, 4), np.int32)
        readings = np.zeros(self.max_cells, capi.MARKER_READING)
        capi.check(self._lib, self._lib.cba_charuco_detector_process(h, n, u8ptr(img), i32ptr(count), i32ptr(status), i32ptr(ids), dptr(xy),
                                                                     i32ptr(nm), i32ptr(nc), i32ptr(n_cells), i32ptr(cells),
                                                                     capi.recptr(readings)))
        k = min(int(n_cells[0]), self.max_cells)
        return CharucoResult(count, status, ids, xy, nm, nc, int(n_cells[0]), cells[:k].copy(), readings[:k].copy())

    def arms(self, dirs) -> np.ndarray:
        """dirs [n][max_corners][12][2] -> scores [n][max_corners] (NaN past the kept corners); n: the images of the last process"""
        h = self._require_open("the detector is closed")
        d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64))
        if d.ndim != 4 or d.shape[1:] != (self.max_corners, 12, 2):
            raise ValueError(f"dirs must have shape [n][{self.max_corners}][12][2], got {d.shape}")
        score = np.full(d.shape[:2], np.nan)
        capi.check(self._lib, self._lib.cba_charuco_detector_arms(h, d.shape[0], dptr(d), dptr(score)))
        return score

    def read(self, cell_image, quads) -> np.ndarray:
        """cell_image [m], quads [m][4][2] -> readings [m] (capi.MARKER_READING), on the images of the last process"""
        h = self._require_open("the detector is closed")
        ci = np.ascontiguousarray(np.asarray(cell_image, dtype=np.int32).reshape(-1))
        q = np.ascontiguousarray(np.asarray(quads, dtype=np.float64))
        if q.shape != (ci.shape[0], 4, 2):
            raise ValueError(f"quads must have shape [{ci.shape[0]}][4][2], got {q.shape}")
        out = np.zeros(ci.shape[0], capi.MARKER_READING)
        capi.check(self._lib, self._lib.cba_charuco_detector_read(h, ci.shape[0], i32ptr(ci), dptr(q), capi.recptr(out)))
        return out


def arm_directions(angle, fan_deg: float = 14.0) -> np.ndarray:
    """angle [...] -> the unit vectors [...][12][2] of the arm test: direction 3 k + f at angle + pi/4 + k pi/2 + (f - 1) fan"""
    import math

    a = np.asarray(angle, dtype=np.float64)
    out = np.zeros(a.shape + (12, 2))
    fan = float(fan_deg) * (math.pi / 180.0)
    for idx in np.ndindex(a.shape):
        if not np.isfinite(a[idx]):
            continue
        for k in range(4):
            for f in range(3):
                phi = float(a[idx]) + math.pi / 4 + k * (math.pi / 2) + (f - 1) * fan
                out[idx + (3 * k + f,)] = (math.cos(phi), math.sin(phi))
    return out


def chessboard_lattice(xy, angle, min_component: int = 4):
    """``cba_chessboard_lattice``: one image's corners -> (component [n] (-1: none), ij [n][2], number of components)"""
    lib = capi.load_library()
    p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
    a = np.ascontiguousarray(np.asarray(angle, dtype=np.float64).reshape(-1))
    if p.shape[0] != a.shape[0]:
        raise ValueError(f"xy must have shape [n][2] and angle [n], got {p.shape} and {a.shape}")
    comp, ij, k = np.full(max(len(a), 1), -1, np.int32), np.zeros((max(len(a), 1), 2), np.int32), np.zeros(1, np.int32)
    capi.check(lib, lib.cba_chessboard_lattice(len(a), dptr(p), dptr(a), int(min_component), i32ptr(comp), i32ptr(ij), i32ptr(k)))
    return comp[:len(a)], ij[:len(a)], int(k[0])


def charuco_match(board: CharucoBoard, component, ij, xy, cells, flags, ids, rotations, min_markers: int = 2):
    """``cba_charuco_match``: one image's labelled corners and readings (cells [m][3] = component, i, j) -> (ids ascending, xy,
    n_markers)"""
    lib = capi.load_library()
    cb, _ = board._c()
    comp = np.ascontiguousarray(np.asarray(component, dtype=np.int32).reshape(-1))
    lab = np.ascontiguousarray(np.asarray(ij, dtype=np.int32).reshape(-1, 2))
    p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
    ce = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 3))
    fl, mid, rot = (np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1)) for v in (flags, ids, rotations))
    if not (len(comp) == len(lab) == len(p)) or not (len(ce) == len(fl) == len(mid) == len(rot)):
        raise ValueError("component, ij and xy need one row per corner; cells, flags, ids and rotations one per reading")
    nb = board.n_corners
    count, nm, out_ids, out_xy = np.zeros(1, np.int32), np.zeros(1, np.int32), np.full(nb, -1, np.int32), np.full((nb, 2), np.nan)
    capi.check(lib, lib.cba_charuco_match(C.byref(cb), int(min_markers), len(comp), i32ptr(comp), i32ptr(lab), dptr(p), len(ce), i32ptr(ce),
                                          i32ptr(fl), i32ptr(mid), i32ptr(rot), i32ptr(count), i32ptr(out_ids), dptr(out_xy), i32ptr(nm)))
    k = int(count[0])
    return out_ids[:k].copy(), out_xy[:k].copy(), int(nm[0])


@dataclass
class CharucoDetection:
    found: bool
    ids: np.ndarray         # [k] board indices, ascending
    object_xy: np.ndarray   # [k][2]
    image_uv: np.ndarray    # [k][2]
    n_markers: int = 0

    @property
    def view(self) -> np.ndarray:
        """[k][4] rows (X, Y, u, v) of the found corners: one view of the intrinsic and rig entry points."""
        return np.concatenate([self.object_xy, self.image_uv], axis=1)


def detect_charuco(images, board: CharucoBoard, opts: Optional[CharucoOptions] = None, corner_opts: Optional[CornerOptions] = None,
                   min_corners: int = 6, max_corners: int = 1024, max_cells: int = 4096, device: int = 0) -> List[CharucoDetection]:
    """The visible inner corners of a ChArUco board in every image, with their board indices.  images: [n][H][W] uint8.  ``found``:
    at least ``min_corners`` corners got an index."""
    img = np.asarray(images)
    if img.ndim == 2:
        img = img[None]
    if img.ndim != 3:
        raise ValueError(f"images must have shape [n][H][W], got {img.shape}")
    out = []
    if img.shape[0] == 0:
        return out
    with CharucoDetector(img.shape[2], img.shape[1], board, img.shape[0], max_corners, max_cells, corner_opts, opts, device) as det:
        res = det.process(img)
    obj = board.object_points
    for i in range(img.shape[0]):
        k = int(res.count[i])
        ids = res.ids[i, :k].copy()
        out.append(CharucoDetection(k >= min_corners, ids, obj[ids], res.xy[i, :k].copy(), int(res.n_markers[i])))
    return out


__all__ += ["marker_dictionary", "CharucoBoard", "CharucoOptions", "CharucoResult", "CharucoDetector", "CharucoDetection", "arm_directions",
            "chessboard_lattice", "charuco_match", "detect_charuco", "CHARUCO_STATUS_CORNER_OVERFLOW", "CHARUCO_STATUS_CELL_OVERFLOW",
            "MARKER_FLAG_DEGENERATE", "MARKER_FLAG_WINDOW", "MARKER_FLAG_LOW_CONTRAST", "MARKER_FLAG_BORDER", "MARKER_FLAG_NO_MATCH"]
