"""Independent numpy restatement of structured-light decoding as calibba.h states it (cba_sl_patterns, cba_sl_decoder): the patterns,
the per-pixel decode in plain integer and fp64 array arithmetic (weights and pattern cosines from math.sin / math.cos, the C
library's), the scene renderer with its exact projector coordinates, and the ctypes wrappers of the host build (tests/sl_cpu).  Test
infrastructure: the host build and the device are checked against it."""
import math

import numpy as np

from tests import camera_ref as R
from tests import triangulate_ref as T

LOW_CONTRAST, UNCERTAIN, OUTSIDE, LOW_MODULATION = 1, 1, 2, 4  # the axis bits before their shift by 1 + 3 axis
GAIN, OFFSET, NOISE_SIGMA = 0.7, 20.0, 1.0


class Options:  # cba_sl_options
    def __init__(self, proj_width, proj_height, axes=3, s=0, N=0, T=16, min_contrast=10, min_bit_diff=4, min_modulation=5.0):
        self.proj_width, self.proj_height, self.axes, self.s, self.N, self.T = proj_width, proj_height, axes, s, N, T
        self.min_contrast, self.min_bit_diff, self.min_modulation = min_contrast, min_bit_diff, min_modulation

    def sides(self):
        """[(projector axis, P)] of the selected axes"""
        return [(a, P) for a, P in ((0, self.proj_width), (1, self.proj_height)) if self.axes >> a & 1]

    def nbits(self, P):
        return max(1, (P - 1).bit_length()) - self.s

    def allowed(self):
        return all(self.nbits(P) >= 1 for _, P in self.sides()) and (self.N == 0 or self.T >= 2 ** (self.s + 1))


def image_count(o):
    return 2 + sum(2 * o.nbits(P) + o.N for _, P in o.sides())


def pattern_line(o, P):
    """the 2 nbits + N images of one axis along that axis: int [2 nbits + N][P]"""
    j = np.arange(P)
    c = j >> o.s
    g = c ^ (c >> 1)
    nb = o.nbits(P)
    rows = []
    for b in range(nb):
        v = np.where((g >> (nb - 1 - b)) & 1, 255, 0)
        rows += [v, 255 - v]
    NT = o.N * o.T
    for k in range(o.N):
        row = []
        for jj in range(P):
            m = (jj * o.N - k * o.T) % NT
            cs = 0.0 if 4 * m == NT or 4 * m == 3 * NT else math.cos(2.0 * math.pi * m / NT)
            row.append(min(255, max(0, math.floor(127.5 * (1.0 + cs) + 0.5))))
        rows.append(np.array(row))
    return np.array(rows).reshape(2 * nb + o.N, P)


def patterns(o):
    PW, PH = o.proj_width, o.proj_height
    imgs = [np.full((PH, PW), 255), np.zeros((PH, PW), int)]
    for a, P in o.sides():
        for line in pattern_line(o, P):
            imgs.append(np.broadcast_to(line[None, :] if a == 0 else line[:, None], (PH, PW)))
    return np.array(imgs).astype(np.uint8)


def weights(N):
    return [math.sin(2.0 * math.pi * k / N) for k in range(N)], [math.cos(2.0 * math.pi * k / N) for k in range(N)]


def decode(o, images):
    """images [n_images][H][W] uint8 -> dict(coord, modulation [n_axes][H][W], status [H][W] uint8, and for the tests' conditions
    unwrap_margin = the least distance of (xg - f) / T from a half-integer over the valid pixels (inf without one) and mod_margin = the
    least |mod / min_modulation - 1| over the pixels whose modulation was evaluated)"""
    I = np.asarray(images).astype(np.int64)
    H, W = I.shape[1:]
    low = (I[0] - I[1]) < o.min_contrast
    status = np.where(low, LOW_CONTRAST, 0)
    coords, mods = [], []
    unwrap_margin, mod_margin = np.inf, np.inf
    idx = 2
    for a, P in o.sides():
        unc, b, c = np.zeros((H, W), bool), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
        for _ in range(o.nbits(P)):
            p, q = I[idx], I[idx + 1]
            idx += 2
            unc |= np.abs(p - q) < o.min_bit_diff
            b = b ^ (p > q)
            c = 2 * c + b
        xg = c * float(2 ** o.s) + (2 ** o.s - 1) / 2.0
        alive = ~low & ~unc
        outside = alive & (xg > P - 1)
        alive &= ~outside
        x, mod = np.where(alive, xg, np.nan), np.full((H, W), np.nan)
        lowmod = np.zeros((H, W), bool)
        if o.N:
            ws, wc = weights(o.N)
            S, C = np.zeros((H, W)), np.zeros((H, W))
            for k in range(o.N):
                Ik = I[idx].astype(np.float64)
                idx += 1
                S = S + Ik * ws[k]
                C = C + Ik * wc[k]
            m = (2.0 / o.N) * np.sqrt(S * S + C * C)
            mod = np.where(alive, m, np.nan)
            lowmod = alive & (m < o.min_modulation)
            phi = np.arctan2(S, C)
            phi = np.where(phi < 0.0, phi + 2.0 * math.pi, phi)
            f = phi * float(o.T) / (2.0 * math.pi)
            t = (xg - f) / float(o.T)
            x = np.where(alive & ~lowmod, np.rint(t) * float(o.T) + f, np.nan)
            ok = alive & ~lowmod
            if ok.any():
                unwrap_margin = min(unwrap_margin, np.abs(np.abs(t[ok] - np.rint(t[ok])) - 0.5).min())
            if alive.any() and o.min_modulation > 0:
                mod_margin = min(mod_margin, np.abs(m[alive] / o.min_modulation - 1.0).min())
        status = status | (np.where(~low & unc, UNCERTAIN, 0) | np.where(outside, OUTSIDE, 0) | np.where(lowmod, LOW_MODULATION, 0)) << (1 + 3 * a)
        coords.append(x)
        mods.append(mod)
    return dict(coord=np.array(coords), modulation=np.array(mods), status=status.astype(np.uint8), unwrap_margin=unwrap_margin,
                mod_margin=mod_margin)


def decode_batch(o, images):
    r = [decode(o, im) for im in images]
    return dict(coord=np.array([d["coord"] for d in r]), modulation=np.array([d["modulation"] for d in r]),
                status=np.array([d["status"] for d in r]), unwrap_margin=min(d["unwrap_margin"] for d in r),
                mod_margin=min(d["mod_margin"] for d in r))


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
def _intr(model, f, W, H, tilt):
    intr = [f, 0.97 * f, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2, 0.1, -1e-3, 2e-4, -1e-5, 1e-4, -1e-4]
    if model == R.SCHEIMPFLUG:
        intr += tilt
    return np.array(intr)


def rig(model, W, H, PW, PH):
    """(intr [2][10 | 12], poses [2][7]): the camera is the reference; the projector stands 0.25 to its right, turned towards the scene
    at depth 1, with a focal length that puts the camera's field of view on the middle 70 % of its panel.  Both have a weak
    distortion (the 5-step undistortion is then exact to rounding), the Scheimpflug model a tilted sensor and a tilted panel."""
    fc = 1.2 * max(W, H, 8)
    fp = 0.7 * min(PW / (max(W, 4) / fc), PH / (max(H, 4) / fc))
    intr = np.stack([_intr(model, fc, W, H, [0.02, -0.015]), _intr(model, fp, PW, PH, [-0.03, 0.02])])
    Rm = T._axis_angle([0.1, 1.0, 0.05], math.atan(0.25))  # reference -> projector
    centre = np.array([0.25, 0.01, 0.0])
    q = T._rotmat_to_quat(Rm)
    poses = np.array([[1.0, 0, 0, 0, 0, 0, 0], np.r_[q, -T.quat_to_rotmat(q) @ centre]])
    return intr, poses


PLANES = np.array([[0.10, -0.05, -1.0, 1.00], [-0.15, 0.08, -1.0, 1.06]])  # n.X + d = 0 in the reference frame: z about 1 and 1.06


def projector_of(model, intr, poses, uv, plane_index, shift=0.0):
    """camera pixels uv [n][2] on the planes plane_index [n] (d moved by shift): the points where their rays meet the planes and the
    points' exact projector coordinates -> (pp [n][2], X [n][3])"""
    xy = R.unproject(model, intr[0], uv)
    ray = np.c_[xy, np.ones(len(xy))]
    pl = PLANES[plane_index]
    s = -(pl[:, 3] + shift) / np.einsum("ij,ij->i", pl[:, :3], ray)
    X = s[:, None] * ray
    Rm, t = T.quat_to_rotmat(poses[1]), poses[1][4:]
    return R.project(model, intr[1], X @ Rm.T + t), X


def true_coordinates(model, intr, poses, W, H, plane_of_pixel, shift=0.0):
    """Per camera pixel: the point where its ray meets its plane, and the point's exact projector coordinates.
    -> (xp, yp [H][W], X [H][W][3])"""
    v, u = np.mgrid[0:H, 0:W]
    pp, X = projector_of(model, intr, poses, np.stack([u.ravel(), v.ravel()], axis=1).astype(float), plane_of_pixel.ravel(), shift)
    return pp[:, 0].reshape(H, W), pp[:, 1].reshape(H, W), X.reshape(H, W, 3)


def sample(pats, xp, yp):
    """bilinear samples of the patterns [n][PH][PW] at projector positions; nothing (0) where the position is more than half a pixel
    outside the panel"""
    n, PH, PW = pats.shape
    inside = (xp >= -0.5) & (xp <= PW - 0.5) & (yp >= -0.5) & (yp <= PH - 0.5)
    x, y = np.clip(xp, 0.0, PW - 1.0), np.clip(yp, 0.0, PH - 1.0)
    x0, y0 = np.minimum(np.floor(x).astype(int), max(PW - 2, 0)), np.minimum(np.floor(y).astype(int), max(PH - 2, 0))
    x1, y1 = np.minimum(x0 + 1, PW - 1), np.minimum(y0 + 1, PH - 1)
    fx, fy = x - x0, y - y0
    P = pats.astype(np.float64)
    top = P[:, y0, x0] * (1 - fx) + P[:, y0, x1] * fx
    bot = P[:, y1, x0] * (1 - fx) + P[:, y1, x1] * fx
    return np.where(inside, top * (1 - fy) + bot * fy, 0.0)


def scene(model, W, H, o, n_seq=1, two_planes=False, seed=0):
    """dict(images uint8 [n_seq][n_images][H][W], xp, yp [n_seq][H][W] exact projector coordinates, X [n_seq][H][W][3], plane_of_pixel
    [H][W], shifts [n_seq], intr, poses).  A plane, or two with a step at the image's middle column; sequence i moves the planes by
    0.01 i.  Gain 0.7, offset 20, seeded Gaussian noise of sigma 1, rounded to uint8."""
    rng = np.random.default_rng(seed)
    intr, poses = rig(model, W, H, o.proj_width, o.proj_height)
    pats = patterns(o)
    which = np.zeros((H, W), int)
    if two_planes:
        which[:, W // 2:] = 1
    out = dict(images=[], xp=[], yp=[], X=[], plane_of_pixel=which, shifts=0.01 * np.arange(n_seq), intr=intr, poses=poses)
    for i in range(n_seq):
        xp, yp, X = true_coordinates(model, intr, poses, W, H, which, out["shifts"][i])
        img = GAIN * sample(pats, xp, yp) + OFFSET + rng.normal(0.0, NOISE_SIGMA, (len(pats), H, W))
        out["images"].append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
        out["xp"].append(xp)
        out["yp"].append(yp)
        out["X"].append(X)
    for k in ("images", "xp", "yp", "X"):
        out[k] = np.ascontiguousarray(np.array(out[k]))
    return out


def plane_distance(X, plane_index, shift=0.0):
    """distance of the points X [n][3] to their planes"""
    pl = PLANES[plane_index]
    return np.abs(np.einsum("ij,ij->i", pl[:, :3], X) + pl[:, 3] + shift) / np.linalg.norm(pl[:, :3], axis=1)


def dlt_homography(src, dst):
    """the normalised DLT by SVD: dst ~ H src, [n][2] each"""
    def norm(p):
        c = p.mean(axis=0)
        k = math.sqrt(2.0) / max(np.linalg.norm(p - c, axis=1).mean(), 1e-300)
        return np.array([[k, 0, -k * c[0]], [0, k, -k * c[1]], [0, 0, 1.0]])
    Ts, Td = norm(src), norm(dst)
    a = np.c_[src, np.ones(len(src))] @ Ts.T
    b = np.c_[dst, np.ones(len(dst))] @ Td.T
    rows = []
    for (x, y, _), (u, v, _) in zip(a, b):
        rows += [[-x, -y, -1, 0, 0, 0, u * x, u * y, u], [0, 0, 0, -x, -y, -1, v * x, v * y, v]]
    h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    return np.linalg.inv(Td) @ h @ Ts


def projector_corners(x, y, corners, radius=8, min_valid=16):
    """the restatement of calibration_amd.projector_corners for one view: x, y [H][W], corners [n][2] -> [n][2]"""
    H, W = x.shape
    out = np.full((len(corners), 2), np.nan)
    for i, (u, v) in enumerate(corners):
        if not (np.isfinite(u) and np.isfinite(v)):
            continue
        cu, cv = int(np.rint(u)), int(np.rint(v))
        pts = [(a, b, x[b, a], y[b, a]) for b in range(max(cv - radius, 0), min(cv + radius, H - 1) + 1)
               for a in range(max(cu - radius, 0), min(cu + radius, W - 1) + 1) if np.isfinite(x[b, a]) and np.isfinite(y[b, a])]
        if len(pts) < max(min_valid, 4):
            continue
        pts = np.array(pts, float)
        q = dlt_homography(pts[:, :2], pts[:, 2:]) @ np.array([u, v, 1.0])
        out[i] = q[:2] / q[2]
    return out


# ---- planted pixels -------------------------------------------------------------------------------------------------------------------
def pixel_stack(o, cx, cy, white=200, black=20, hi=200, lo=20, A=110.0, B=80.0):
    """the n_images samples of one pixel whose Gray planes say the codes cx and cy and whose phase is that of the stripe's centre"""
    v = [white, black]
    for a, P in o.sides():
        c = cx if a == 0 else cy
        nb = o.nbits(P)
        g = c ^ (c >> 1)
        for b in range(nb):
            v += [hi, lo] if (g >> (nb - 1 - b)) & 1 else [lo, hi]
        xc = c * 2 ** o.s + (2 ** o.s - 1) / 2
        v += [int(round(A + B * math.cos(2 * math.pi * xc / o.T - 2 * math.pi * k / o.N))) for k in range(o.N)]
    return v


PLANT_OPTIONS = dict(proj_width=16, proj_height=17, axes=3, s=0, N=4, T=16)  # a power of two and one more: nbits 4 and 5


def plants():
    """[(name, samples of the pixel, expected status)] for Options(**PLANT_OPTIONS) with its default thresholds (10, 4, 5)"""
    o = Options(**PLANT_OPTIONS)
    nx = o.nbits(16)
    x_msb, x_lsb, y_lsb = 2, 2 + 2 * (nx - 1), 2 + 2 * nx + o.N + 2 * (o.nbits(17) - 1)

    def pair(v, at, p, q):
        v = list(v)
        v[at], v[at + 1] = p, q
        return v

    base = pixel_stack(o, 9, 5)  # x = 9 = Gray 1101: MSB set, LSB set; y = 5 = Gray 00111: LSB set
    return [
        ("clean", base, 0),
        ("contrast at the threshold", pixel_stack(o, 9, 5, white=30), 0),
        ("contrast one below", pixel_stack(o, 9, 5, white=29), LOW_CONTRAST),
        ("MSB difference at the threshold", pair(base, x_msb, 24, 20), 0),
        ("MSB difference one below", pair(base, x_msb, 23, 20), UNCERTAIN << 1),
        ("LSB difference at the threshold", pair(base, y_lsb, 104, 100), 0),
        ("LSB difference one below", pair(base, y_lsb, 100, 103), UNCERTAIN << 4),
        ("p == q", pair(base, x_lsb, 77, 77), UNCERTAIN << 1),
        ("last code of a power of two", pixel_stack(o, 15, 5), 0),
        ("stripe centre at P - 1", pixel_stack(o, 9, 16), 0),
        ("the next code: outside", pixel_stack(o, 9, 17), OUTSIDE << 4),
        ("modulation far under the threshold (just under: modulation_plant)", pixel_stack(o, 9, 5, B=3.0), LOW_MODULATION << 1 | LOW_MODULATION << 4),
        ("all 255", [255] * image_count(o), LOW_CONTRAST),
        ("all 0", [0] * image_count(o), LOW_CONTRAST),
    ]


MOD_STEP = 1e-7  # how far, relatively, modulation_plant puts the threshold from the pixel's modulation: 100 times the 1e-9 condition


def modulation_plant():
    """A pixel whose modulation lies just under the threshold, which a plant with the default threshold cannot be: with N = 4 and
    integer samples 4 mod^2 is an integer, and none lies within 1e-6 of 100.  So the threshold comes from the pixel: with m the
    restated modulation of its weaker axis,
    -> (samples, [(min_modulation, expected status)]): m (1 + MOD_STEP) -> that axis low, m (1 - MOD_STEP) -> valid.
    The other axis is stronger by more than 1e-3 relative and stays valid in both."""
    v = pixel_stack(Options(**PLANT_OPTIONS), 9, 6, B=40.0)
    m = decode(Options(**PLANT_OPTIONS, min_modulation=0.0), np.array(v, np.uint8)[:, None, None])["modulation"][:, 0, 0]
    a = int(np.argmin(m))
    assert m[1 - a] > m[a] * (1 + 1e-3) and 20.0 < m[a] < 60.0, m
    return v, [(m[a] * (1 + MOD_STEP), LOW_MODULATION << (1 + 3 * a)), (m[a] * (1 - MOD_STEP), 0)]


def planted_images(W, H, places, plant_list=None):
    """A W x H sequence of clean pixels for Options(**PLANT_OPTIONS) with plant i (of plants(), or of plant_list in
    the same form) at places[i] = (row, column):
    -> (images [n_images][H][W] uint8, expected status [H][W])"""
    o = Options(**PLANT_OPTIONS)
    img = np.empty((image_count(o), H, W), np.uint8)
    want = np.zeros((H, W), np.uint8)
    for r in range(H):
        for c in range(W):
            img[:, r, c] = pixel_stack(o, (3 * c + r) % 16, (5 * c + 2 * r) % 17)
    for (name, v, st), (r, c) in zip(plants() if plant_list is None else plant_list, places):
        img[:, r, c] = v
        want[r, c] = st
    return img, want


# ---- the host build of structured_light_math.hpp (tests/sl_cpu) ------------------------------------------------------------------------
def _opts_args(o):
    import ctypes as C

    return [C.c_int(v) for v in (o.proj_width, o.proj_height, o.axes, o.s, o.N, o.T, o.min_contrast, o.min_bit_diff)] + [C.c_double(o.min_modulation)]


def host_patterns(L, o):
    import ctypes as C

    out = np.empty((image_count(o), o.proj_height, o.proj_width), np.uint8)
    L.sl_host_patterns(*_opts_args(o), out.ctypes.data_as(C.c_void_p))
    return out


def host_decode(L, o, images):
    """images [n_seq][n_images][H][W] -> dict(coord, modulation [n_seq][n_axes][H][W], status [n_seq][H][W])"""
    import ctypes as C

    images = np.ascontiguousarray(images, np.uint8)
    n, ni, H, W = images.shape
    assert ni == image_count(o)
    na = len(o.sides())
    r = dict(coord=np.empty((n, na, H, W)), modulation=np.empty((n, na, H, W)), status=np.empty((n, H, W), np.uint8))
    L.sl_host_decode(*_opts_args(o), C.c_int(W), C.c_int(H), C.c_int(n), images.ctypes.data_as(C.c_void_p), r["coord"].ctypes.data_as(C.c_void_p),
                     r["modulation"].ctypes.data_as(C.c_void_p), r["status"].ctypes.data_as(C.c_void_p))
    return r


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def max_abs(a, b):
    d = np.abs(a - b)[~np.isnan(a) & ~np.isnan(b)]
    return d.max() if d.size else 0.0


def max_rel(a, b):
    ok = ~np.isnan(a) & ~np.isnan(b)
    return (np.abs(a - b)[ok] / np.maximum(np.abs(b[ok]), 1e-300)).max() if ok.any() else 0.0
