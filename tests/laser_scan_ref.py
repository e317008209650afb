"""Independent numpy restatement of laser profile scanning as calibba.h states it (cba_laser_points, cba_laser_scanner): the peak of
one line (maximum, lowest position, plateau, window, centre of gravity), the ray-plane intersection and the frame pose.  Unprojection
comes from tests/camera_ref.py.  Also the scene maker of the laser-scan tests, the plants of their edge cases and the wrappers of the host
build (tests/laser_scan_cpu).  Test infrastructure: the host build and the device are checked against it."""
import numpy as np

from tests import camera_ref as R
from tests.host_build import ptr

SIGMA = 2.0        # px, the rendered line's Gaussian cross-section along the search axis
AMPLITUDE = 200.0  # its height (uint8: rounded to the nearest integer)


class Options:  # cba_laser_scan_options
    def __init__(self, axis=0, roi_begin=0, roi_end=0, half_window=5, floor_level=0.0, min_peak=1.0):
        self.axis, self.roi_begin, self.roi_end = axis, roi_begin, roi_end
        self.half_window, self.floor_level, self.min_peak = half_window, floor_level, min_peak

    def roi(self, W, H):
        side = H if self.axis == 0 else W
        return (0, side) if self.roi_begin == 0 and self.roi_end == 0 else (self.roi_begin, self.roi_end)


# ---- the peak of one line ----------------------------------------------------------------------------------------------------------
def peak_line(I, pb, pe, hw, floor_level, min_peak):
    """I: the samples of one line along the search direction (uint8 or float32) -> (centre, amplitude, width_px)"""
    nan = float("nan")
    u8 = I.dtype == np.uint8
    roi = I[pb:pe]
    good = np.ones(roi.shape, bool) if u8 else ~np.isnan(roi)
    if not good.any():
        return nan, nan, nan
    m = roi[good].max()
    p0 = pb + int(np.flatnonzero(good & (roi == m))[0])
    p1 = p0
    while p1 + 1 < pe and I[p1 + 1] == m:
        p1 += 1
    amp = float(m)
    level = float(np.clip(np.rint(floor_level), 0, 255)) if u8 else float(floor_level)
    if amp < min_peak:
        return nan, amp, nan
    lo, hi = max(p0 - hw, pb), min(p1 + hw, pe - 1)
    p = np.arange(lo, hi + 1)
    if u8:
        g = np.maximum(I[lo:hi + 1].astype(np.int64) - int(level), 0)
        sg, sgp = float(int(g.sum())), float(int((g * p).sum()))  # exact integers, each converted once
    else:
        w = I[lo:hi + 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            g = np.where(np.isnan(w), 0.0, np.maximum(w - level, 0.0))
            sg, sgp = float(np.cumsum(g)[-1]), float(np.cumsum(g * p)[-1])  # cumsum adds in ascending order
    if sg == 0.0:
        return nan, amp, nan
    with np.errstate(all="ignore"):
        return float(np.float64(sgp) / np.float64(sg)), amp, float(np.float64(sg) / np.float64(amp - level))


def quat_to_rotmat(q):  # the quaternion's matrix without normalisation (Eigen's toRotationMatrix)
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def plane_homography(plane):  # build_plane_homography: the inverse of [e1 e2 p0]
    n = np.asarray(plane[:3], float)
    p0 = -plane[3] * n
    tmp = np.array([0.0, 0.0, 1.0]) if abs(n[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    e1 = np.cross(n, tmp)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    e2 /= np.linalg.norm(e2)
    return np.linalg.inv(np.column_stack([e1, e2, p0]))


def points(model, intr, inv, plane, uv, frame=None, poses=None, want_plane_xy=False):
    """uv [n][2] -> xyz [n][3] (and plane_xy [n][2]); frame [n]: each pixel's frame index, poses [n_frames][7]"""
    uv = np.asarray(uv, float).reshape(-1, 2)
    plane = np.asarray(plane, float)
    with np.errstate(all="ignore"):
        xy = R.unproject(model, intr, uv, inv)
        x, y = xy[:, 0], xy[:, 1]
        den = plane[0] * x + plane[1] * y + plane[2]
        s = -plane[3] / den
        ok = (den != 0.0) & (s > 0.0) & np.isfinite(s)
        P = np.where(ok[:, None], np.stack([s * x, s * y, s], axis=1), np.nan)
        if poses is not None:
            poses = np.asarray(poses, float).reshape(-1, 7)
            frame = np.zeros(len(uv), int) if frame is None else np.asarray(frame)
            out = np.empty_like(P)
            for f in range(len(poses)):
                M, t = quat_to_rotmat(poses[f, :4]), poses[f, 4:]
                k = frame == f
                for r in range(3):
                    out[k, r] = M[r, 0] * P[k, 0] + M[r, 1] * P[k, 1] + M[r, 2] * P[k, 2] + t[r]
            P = out
        if not want_plane_xy:
            return P
        Hp = plane_homography(plane)
        h = np.stack([x, y, np.ones_like(x)], axis=1) @ Hp.T
        pxy = np.where(ok[:, None], h[:, :2] / h[:, 2:3], np.nan)
    return P, pxy


def scan(model, intr, inv, plane, images, o, poses=None):
    """images [n_frames][H][W] -> dict(centre, amplitude, width_px [n_frames][n_lines], xyz [n_frames][n_lines][3])"""
    n_frames, H, W = images.shape
    pb, pe = o.roi(W, H)
    n_lines = W if o.axis == 0 else H
    out = np.empty((3, n_frames, n_lines))
    for f in range(n_frames):
        for l in range(n_lines):
            line = images[f, :, l] if o.axis == 0 else images[f, l, :]
            out[:, f, l] = peak_line(line, pb, pe, o.half_window, o.floor_level, o.min_peak)
    idx = np.broadcast_to(np.arange(n_lines, dtype=float), (n_frames, n_lines))
    uv = np.stack([idx, out[0]] if o.axis == 0 else [out[0], idx], axis=-1).reshape(-1, 2)
    xyz = points(model, intr, inv, plane, uv, np.repeat(np.arange(n_frames), n_lines), poses)
    return dict(centre=out[0], amplitude=out[1], width_px=out[2], xyz=xyz.reshape(n_frames, n_lines, 3))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
PLANE = np.r_[np.array([0.1, 0.7, -0.7]) / np.linalg.norm([0.1, 0.7, -0.7]), 0.5]  # as cba_calibrate_laser_plane returns it: d > 0


def camera(model, W, H):
    """A camera that sees the W x H image under ~45 degrees, with a distortion weak enough for the 5-step undistortion to be exact to
    rounding (contraction ~1e-3 per step), so that project(unproject(pixel)) returns the pixel to ~1e-12 px."""
    f = 1.2 * max(W, H, 8)
    intr = [f, 0.97 * f, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2, 0.1, -1e-3, 2e-4, -1e-5, 1e-4, -1e-4]
    if model == R.SCHEIMPFLUG:
        intr += [0.02, -0.015]
    return np.array(intr)


def true_positions(n_frames, n_lines, side):
    """The true sub-pixel line position of every line: smooth along the line index, different in every frame, the whole Gaussian
    (+-3 sigma) inside the side when the side has room for it."""
    t = np.arange(n_lines) / max(n_lines - 1, 1)
    mid = (side - 1) / 2
    amp = max(mid - 3 * SIGMA - 1.0, 0.0)
    f = np.arange(n_frames)[:, None]
    return mid + 0.37 * (side > 1) * min(1.0, mid) + amp * np.sin(2 * np.pi * (0.7 * t[None, :] + 0.13 * f))


def render(pos, side, axis):
    """pos [n_frames][n_lines] -> float32 images of the Gaussian cross-section along the search axis, and their uint8 quantisation"""
    p = np.arange(side, dtype=float)
    g = AMPLITUDE * np.exp(-((p[None, None, :] - pos[:, :, None]) ** 2) / (2 * SIGMA ** 2))  # [frame][line][position]
    img = np.ascontiguousarray(g.transpose(0, 2, 1) if axis == 0 else g)
    return img.astype(np.float32), np.rint(img).astype(np.uint8)


def scene(model, W, H, axis, n_frames=1):
    """(intr, plane, pos, curve, f32 images, u8 images): the curve [n_frames][n_lines][3] lies on the plane and projects to the line"""
    intr = camera(model, W, H)
    n_lines, side = (W, H) if axis == 0 else (H, W)
    pos = true_positions(n_frames, n_lines, side)
    idx = np.broadcast_to(np.arange(n_lines, dtype=float), pos.shape)
    uv = np.stack([idx, pos] if axis == 0 else [pos, idx], axis=-1).reshape(-1, 2)
    curve = points(model, intr, None, PLANE, uv).reshape(n_frames, n_lines, 3)
    f32, u8 = render(pos, side, axis)
    return intr, PLANE, pos, curve, f32, u8


def line_view(images, axis, frame, line):
    """the writable samples of one line along the search direction"""
    return images[frame, :, line] if axis == 0 else images[frame, line, :]


def frame_poses(n_frames):
    """one pose per frame; frame 1 (when there is one) has a quaternion that is not a unit quaternion"""
    rng = np.random.default_rng(11)
    q = np.c_[np.ones(n_frames), rng.uniform(-0.1, 0.1, (n_frames, 3))]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[min(1, n_frames - 1)] *= 1.05
    return np.ascontiguousarray(np.c_[q, rng.uniform(-0.2, 0.2, (n_frames, 3))])


# ---- the host build of laser_scan_math.hpp (tests/laser_scan_cpu) ------------------------------------------------------------------
def host_points(L, model, intr, inv, plane, uv, frame_offset=None, poses=None, want_plane_xy=False):
    import ctypes as C

    intr, plane, uv = (np.ascontiguousarray(a, float) for a in (intr, plane, uv))
    inv = None if inv is None else np.ascontiguousarray(inv, float)
    poses = None if poses is None else np.ascontiguousarray(poses, float).reshape(-1, 7)
    off = None if frame_offset is None else np.ascontiguousarray(frame_offset, np.int64)
    n = uv.shape[0]
    n_frames = 0 if poses is None else len(poses)
    xyz = np.empty((n, 3))
    pxy = np.empty((n, 2)) if want_plane_xy else None
    L.ls_points(C.c_int(model), ptr(intr), C.c_int(0 if inv is None else inv.size), ptr(inv), ptr(plane), C.c_int64(n), ptr(uv), C.c_int(n_frames),
                ptr(off), ptr(poses), ptr(xyz), ptr(pxy))
    return (xyz, pxy) if want_plane_xy else xyz


def host_scan(L, model, intr, inv, plane, images, o, poses=None):
    import ctypes as C

    intr, plane = np.ascontiguousarray(intr, float), np.ascontiguousarray(plane, float)
    inv = None if inv is None else np.ascontiguousarray(inv, float)
    poses = None if poses is None else np.ascontiguousarray(poses, float)
    images = np.ascontiguousarray(images)
    n_frames, H, W = images.shape
    pb, pe = o.roi(W, H)
    n_lines = W if o.axis == 0 else H
    r = {k: np.empty((n_frames, n_lines)) for k in ("centre", "amplitude", "width_px")}
    r["xyz"] = np.empty((n_frames, n_lines, 3))
    L.ls_scan(C.c_int(model), ptr(intr), C.c_int(0 if inv is None else inv.size), ptr(inv), ptr(plane), C.c_int(W), C.c_int(H), C.c_int(o.axis),
              C.c_int(pb), C.c_int(pe), C.c_int(o.half_window), C.c_double(o.floor_level), C.c_double(o.min_peak), C.c_int(n_frames),
              C.c_int(0 if images.dtype == np.uint8 else 1), ptr(images), ptr(poses), ptr(r["centre"]), ptr(r["amplitude"]), ptr(r["width_px"]),
              ptr(r["xyz"]))
    return r


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def rel(a, b):
    """max |a - b| / max(1, |b|) over the entries that are not NaN in both (the bar test_camera_gpu.py holds unproject to)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    k = ~(np.isnan(a) & np.isnan(b))
    if not k.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(a[k] - b[k]) / np.maximum(1.0, np.abs(b[k]))
    return float(np.max(np.where(np.isnan(d), np.inf, d)))


def bitwise(a, b):
    """equal to the bit, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and same_nan(a, b) and np.array_equal(np.nan_to_num(a, nan=0.0).view(np.int64), np.nan_to_num(b, nan=0.0).view(np.int64))
