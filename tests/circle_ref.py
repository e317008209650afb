"""Independent numpy restatement of circle-grid detection (calibba.h: cba_blob_detector, cba_circle_grid_order), written from the
header's rule and not from blob_math.hpp / circle_grid.hpp, plus the renderer of the end-to-end scenes and the wrappers of the host
build (tests/circle_cpu).  Box sums come from integral images and shifted slices; sums whose order the rule fixes are accumulated
one term at a time."""
import math
from collections import namedtuple

import numpy as np

from tests import camera_ref as R
from tests import corner_ref as K
from tests.host_build import ptr

Options = namedtuple("Options", "polarity a b min_contrast nms_radius max_radius rounds max_fit_error max_axis_ratio min_radius")
DARK, BRIGHT = 0, 1
FLAG_WINDOW, FLAG_NO_EDGE, FLAG_DEGENERATE, FLAG_SHAPE, FLAG_RATIO, FLAG_SIZE, FLAG_DUPLICATE = 1, 2, 4, 8, 16, 32, 64
SYMMETRIC, ASYMMETRIC = 0, 1
DEFAULT = Options(DARK, 2, 12, 30, 4, 20, 3, 0.2, 3.0, 1.5)
SMALL = Options(DARK, 1, 2, 1, 1, 6, 2, 0.2, 3.0, 1.5)  # the small boxes of SIZES: 11 x 11 is legal


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def _box(img, h):
    """sum over the (2h + 1)^2 box centred on every pixel, zeros outside the image"""
    H, W = img.shape
    ii = np.zeros((H + 2 * h + 1, W + 2 * h + 1), np.int64)
    ii[h + 1:h + 1 + H, h + 1:h + 1 + W] = img
    ii = ii.cumsum(axis=0).cumsum(axis=1)
    n = 2 * h + 1
    return ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]


def response(img, o):
    """one image [H][W] uint8 -> (R [H][W] int32, S_in [H][W] uint16)"""
    H, W = img.shape
    s_in, s_out = _box(img, o.a), _box(img, o.b)
    n_in = (2 * o.a + 1) ** 2
    n_ring = (2 * o.b + 1) ** 2 - n_in
    r = n_in * (s_out - s_in) - n_ring * s_in
    if o.polarity == BRIGHT:
        r = -r
    out = np.zeros((H, W), np.int64)
    b = o.b
    if H > 2 * b and W > 2 * b:
        out[b:H - b, b:W - b] = r[b:H - b, b:W - b]
    assert np.abs(out).max(initial=0) < 2 ** 31 and s_in.max() < 2 ** 16
    return out.astype(np.int32), s_in.astype(np.uint16)


def peaks(Rm, min_response, nms, border):
    """-> [(y, x)] in row-major order: the corner detector's rule with another border"""
    H, W = Rm.shape
    b = border + nms
    if H - 2 * b < 1 or W - 2 * b < 1:
        return []
    Rl = Rm.astype(np.int64)
    core = Rl[b:H - b, b:W - b]
    ok = core >= min_response
    for dy in range(-nms, nms + 1):
        for dx in range(-nms, nms + 1):
            if dy == 0 and dx == 0:
                continue
            other = Rl[b + dy:H - b + dy, b + dx:W - b + dx]
            ok &= (core > other) if (dy < 0 or (dy == 0 and dx < 0)) else (core >= other)
    ys, xs = np.nonzero(ok)
    return [(int(y) + b, int(x) + b) for y, x in zip(ys, xs)]


def ray_table():
    return ([math.cos(2.0 * math.pi * float(k) / 32.0) for k in range(32)], [math.sin(2.0 * math.pi * float(k) / 32.0) for k in range(32)])


def _samples(img, xs, ys):
    """bilinear samples at arrays of positions -> (values, inside)"""
    H, W = img.shape
    inside = (xs >= 0.0) & (ys >= 0.0) & (xs < float(W - 1)) & (ys < float(H - 1))
    x, y = np.where(inside, xs, 0.0), np.where(inside, ys, 0.0)
    ix, iy = x.astype(np.int64), y.astype(np.int64)
    fx, fy = x - ix, y - iy
    p00, p01 = img[iy, ix].astype(np.float64), img[iy, ix + 1].astype(np.float64)
    p10, p11 = img[iy + 1, ix].astype(np.float64), img[iy + 1, ix + 1].astype(np.float64)
    top, bot = p00 + fx * (p01 - p00), p10 + fx * (p11 - p10)
    return top + fy * (bot - top), inside


def _edge(img, cx, cy, dx, dy, i0, thr, o):
    """-> (flags, r)"""
    t = np.arange(1, o.max_radius + 1, dtype=np.float64)
    v, inside = _samples(img, cx + t * dx, cy + t * dy)
    reach = (v >= thr) if o.polarity == DARK else (v <= thr)
    stop = np.flatnonzero(~inside | reach)
    if stop.size == 0:
        return FLAG_NO_EDGE, 0.0
    k = int(stop[0])
    if not inside[k]:
        return FLAG_WINDOW, 0.0
    prev, cur = (i0 if k == 0 else float(v[k - 1])), float(v[k])
    if o.polarity == DARK:
        return 0, (float(t[k]) - 1.0) + (thr - prev) / (cur - prev)
    return 0, (float(t[k]) - 1.0) + (prev - thr) / (prev - cur)


def refine(img, px, py, Rv, s_in, o, rays=None):
    """-> (x, y, (mxx, mxy, myy), fit_error, flags)"""
    cos, sin = rays or ray_table()
    n_in = (2 * o.a + 1) ** 2
    n_ring = (2 * o.b + 1) ** 2 - n_in
    num = Rv + n_ring * s_in if o.polarity == DARK else n_ring * s_in - Rv
    assert num % n_in == 0
    lo, hi = float(s_in) / float(n_in), float(num // n_in) / float(n_ring)
    thr = (lo + hi) / 2.0
    cx, cy = float(px), float(py)
    nan = float("nan")
    for rnd in range(o.rounds):
        v, inside = _samples(img, np.array([cx]), np.array([cy]))
        if not inside[0]:
            return cx, cy, (nan, nan, nan), nan, FLAG_WINDOW
        i0 = float(v[0])
        if not (i0 < thr if o.polarity == DARK else i0 > thr):
            return cx, cy, (nan, nan, nan), nan, FLAG_NO_EDGE
        ex, ey = [], []
        for k in range(32):
            f, r = _edge(img, cx, cy, cos[k], sin[k], i0, thr, o)
            if f:
                return cx, cy, (nan, nan, nan), nan, f
            ex.append(r * cos[k])
            ey.append(r * sin[k])
        s2 = sx = sy = sxx = sxy = syy = 0.0
        for k in range(32):
            xp, yp, xk, yk = ex[k], ey[k], ex[(k + 1) % 32], ey[(k + 1) % 32]
            cr = xp * yk - xk * yp
            s2 = s2 + cr
            sx = sx + (xp + xk) * cr
            sy = sy + (yp + yk) * cr
            sxx = sxx + (xp * xp + xp * xk + xk * xk) * cr
            syy = syy + (yp * yp + yp * yk + yk * yk) * cr
            sxy = sxy + (xp * yk + 2.0 * (xp * yp) + 2.0 * (xk * yk) + xk * yp) * cr
        if not s2 > 0.0:
            return cx, cy, (nan, nan, nan), nan, FLAG_DEGENERATE
        gx, gy = sx / (3.0 * s2), sy / (3.0 * s2)
        if rnd == o.rounds - 1:
            mxx, myy = 4.0 * (sxx / (6.0 * s2) - gx * gx), 4.0 * (syy / (6.0 * s2) - gy * gy)
            mxy = 4.0 * (sxy / (12.0 * s2) - gx * gy)
            det = mxx * myy - mxy * mxy
            if not det > 0.0:
                return cx, cy, (nan, nan, nan), nan, FLAG_DEGENERATE
            err = 0.0
            for k in range(32):
                dx, dy = ex[k] - gx, ey[k] - gy
                err = max(err, abs((myy * (dx * dx) - 2.0 * (mxy * (dx * dy)) + mxx * (dy * dy)) / det - 1.0))
            return cx + gx, cy + gy, (mxx, mxy, myy), err, 0
        cx, cy = cx + gx, cy + gy
    raise AssertionError("rounds >= 1")


def semi_axes(shape):
    """shape [...][3] -> (major, minor)"""
    shape = np.asarray(shape, float)
    h, d = 0.5 * (shape[..., 0] + shape[..., 2]), 0.5 * (shape[..., 0] - shape[..., 2])
    s = np.sqrt(d * d + shape[..., 1] ** 2)
    return np.sqrt(h + s), np.sqrt(h - s)


def detect(images, o, max_blobs):
    """images [n][H][W] uint8 -> dict(count, status, xy, shape, fit_error, response, flags) shaped as cba_blob_detector_process writes"""
    n = images.shape[0]
    count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xy, shape, fit = np.full((n, max_blobs, 2), np.nan), np.full((n, max_blobs, 3), np.nan), np.full((n, max_blobs), np.nan)
    resp, flags = np.zeros((n, max_blobs), np.int32), np.zeros((n, max_blobs), np.int32)
    rays = ray_table()
    thr = o.min_contrast * (2 * o.a + 1) ** 2 * ((2 * o.b + 1) ** 2 - (2 * o.a + 1) ** 2)
    for i in range(n):
        Rm, Sm = response(images[i], o)
        pk = peaks(Rm, thr, o.nms_radius, o.b)
        count[i] = len(pk)
        status[i] = 1 if len(pk) > max_blobs else 0
        for k, (py, px) in enumerate(pk[:max_blobs]):
            x, y, m, e, f = refine(images[i], px, py, int(Rm[py, px]), int(Sm[py, px]), o, rays)
            if not f:
                major, minor = (float(v) for v in semi_axes(m))
                if e > o.max_fit_error:
                    f |= FLAG_SHAPE
                if major > o.max_axis_ratio * minor:
                    f |= FLAG_RATIO
                if minor < o.min_radius:
                    f |= FLAG_SIZE
                for j in range(k):
                    if flags[i, j] == 0 and (x - xy[i, j, 0]) ** 2 + (y - xy[i, j, 1]) ** 2 <= minor * minor:
                        f |= FLAG_DUPLICATE
                        break
            xy[i, k], shape[i, k], fit[i, k], resp[i, k], flags[i, k] = (x, y), m, e, Rm[py, px], f
    return dict(count=count, status=status, xy=xy, shape=shape, fit_error=fit, response=resp, flags=flags)


_CACHE = {}


def detect_cached(key, images, o, max_blobs):
    """detect() computed once per key: the CPU and GPU tiers share the restatement's results"""
    if key not in _CACHE:
        _CACHE[key] = detect(images, o, max_blobs)
    return _CACHE[key]


# ---- grid order ------------------------------------------------------------------------------------------------------------------------
def pattern_points(pattern, rows, cols, d=1.0):
    jj, ii = np.divmod(np.arange(rows * cols), cols)
    x = ii if pattern == SYMMETRIC else 2 * ii + jj % 2
    return np.stack([x * float(d), jj * float(d)], axis=1)


def order(xy, shape, pattern, rows, cols):
    """-> (index [rows cols] row-major over (j, i), unique) or (None, 0)"""
    xy = np.asarray(xy, float).reshape(-1, 2)
    n, need = len(xy), rows * cols
    if n < need:
        return None, 0
    if shape is None:
        inv = np.tile(np.eye(2), (n, 1, 1))
    else:
        s = np.asarray(shape, float).reshape(-1, 3)
        det = s[:, 0] * s[:, 2] - s[:, 1] ** 2
        inv = np.stack([np.stack([s[:, 2] / det, -s[:, 1] / det], 1), np.stack([-s[:, 1] / det, s[:, 0] / det], 1)], 1)

    def cosine(c, v, w):
        return (v @ inv[c] @ w) / math.sqrt((v @ inv[c] @ v) * (w @ inv[c] @ w))

    cand = []
    for c in range(n):
        v = xy - xy[c]
        q = np.einsum("ni,ij,nj->n", v, inv[c], v)
        q[c] = np.inf
        near = np.argsort(q, kind="stable")[:4]
        cand.append([int(j) for j in near if q[near[0]] > 0 and q[j] <= 1.44 * q[near[0]] and j != c])
    link = [[j for j in cand[c] if c in cand[j]] for c in range(n)]
    centre = xy.mean(axis=0)
    starts = np.argsort(np.hypot(*(xy - centre).T), kind="stable")
    c30 = math.cos(math.radians(30.0))
    seen = set()
    for s in starts:
        s = int(s)
        if s in seen:
            continue
        ok = True
        lab, basis, todo = {s: (0, 0)}, {}, [s]
        seen.add(s)
        if link[s]:
            e1 = xy[link[s][0]] - xy[s]
            rest = [xy[j] - xy[s] for j in link[s][1:]]
            if rest:
                basis[s] = (e1, min(rest, key=lambda w: abs(cosine(s, e1, w))))
            else:
                ok = False
        while todo:
            c = todo.pop(0)
            if not ok:
                for j in link[c]:
                    if j not in seen:
                        seen.add(j)
                        lab[j] = None
                        todo.append(j)
                continue
            e = list(basis[c])
            for ax in range(2):
                best, carried = c30, basis[c][ax]
                for j in link[c]:
                    w = xy[j] - xy[c]
                    cs = cosine(c, carried, w)
                    if abs(cs) > best:
                        best, e[ax] = abs(cs), (w if cs > 0 else -w)
            for j in link[c]:
                w = xy[j] - xy[c]
                c1, c2 = cosine(c, e[0], w), cosine(c, e[1], w)
                first = abs(c1) >= abs(c2)
                cs = c1 if first else c2
                if not abs(cs) > c30:
                    ok = False
                    continue
                sg = 1 if cs > 0 else -1
                new = (lab[c][0] + (sg if first else 0), lab[c][1] + (0 if first else sg))
                if j in seen:
                    ok &= lab[j] == new
                    continue
                seen.add(j)
                lab[j], basis[j] = new, (e[0], e[1])
                todo.append(j)
        if not ok or len(lab) != need:
            continue
        ids = np.array(list(lab.keys()))
        P, Q = np.array([lab[i][0] for i in ids]), np.array([lab[i][1] for i in ids])
        fits = []
        for t in range(8):
            p, q = (Q, P) if t & 1 else (P, Q)
            p = -p if t & 2 else p
            q = -q if t & 4 else q
            u, v = (p - q, p + q) if pattern == ASYMMETRIC else (p, q)
            u, v = u - u.min(), v - v.min()
            if pattern == ASYMMETRIC:
                if ((u - v % 2) % 2).any():
                    continue
                u = (u - v % 2) // 2
            if u.min() < 0 or u.max() >= cols or v.max() >= rows or len(set(zip(u.tolist(), v.tolist()))) != need:
                continue
            G = np.empty((rows, cols), int)
            G[v, u] = ids
            Pt = xy[G]
            mi, mj = (Pt[:, 1:] - Pt[:, :-1]).sum(axis=(0, 1)) / (rows * (cols - 1)), (Pt[1:] - Pt[:-1]).sum(axis=(0, 1)) / ((rows - 1) * cols)
            if mi[0] * mj[1] - mi[1] * mj[0] > 0:
                fits.append(((mi[0], mi[1]), G.reshape(-1).astype(np.int32)))
        if fits:
            best = fits[0]
            for f in fits[1:]:
                if f[0] > best[0]:
                    best = f
            return best[1], int(len(fits) == 1)
    return None, 0


# ---- the perspective bias of the ellipse centre and the homography that feeds it ---------------------------------------------------------
def homography(obj, uv):
    """normalised DLT: obj [n][2] -> uv [n][2]"""
    def norm(p):
        m, s = p.mean(axis=0), math.sqrt(2.0) / np.linalg.norm(p - p.mean(axis=0), axis=1).mean()
        return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])
    To, Tu = norm(obj), norm(uv)
    a = (np.c_[obj, np.ones(len(obj))] @ To.T)
    b = (np.c_[uv, np.ones(len(uv))] @ Tu.T)
    rows = []
    for (X, Y, _), (u, v, _) in zip(a, b):
        rows.append([X, Y, 1, 0, 0, 0, -u * X, -u * Y, -u])
        rows.append([0, 0, 0, X, Y, 1, -v * X, -v * Y, -v])
    h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    Hm = np.linalg.inv(Tu) @ h @ To
    return Hm / Hm[2, 2]


def centre_bias(Hm, obj, radius):
    """centre of the image of the circle of `radius` round obj minus the image of obj, [n][2]"""
    Hi = np.linalg.inv(Hm)
    out = np.empty((len(obj), 2))
    for k, (X, Y) in enumerate(obj):
        Cm = np.array([[1.0, 0, -X], [0, 1.0, -Y], [-X, -Y, X * X + Y * Y - radius * radius]])
        Q = Hi.T @ Cm @ Hi
        c = np.linalg.solve(Q[:2, :2], -Q[:2, 2])
        p = Hm @ np.array([X, Y, 1.0])
        out[k] = c - p[:2] / p[2]
    return out


def corrected(obj, uv, radius):
    """uv minus the bias, H from the ordered centres, repeated once with H from the corrected centres"""
    out = uv
    for _ in range(2):
        out = uv - centre_bias(homography(obj, out), obj, radius)
    return out


# ---- the renderer ----------------------------------------------------------------------------------------------------------------------
ROWS, COLS, SPACING, RADIUS = 11, 4, 0.018, 0.0065
W_IMG, H_IMG, CAMERA = K.W_IMG, K.H_IMG, K.CAMERA


def grid_points(rows=ROWS, cols=COLS, d=SPACING, pattern=ASYMMETRIC):
    """object points with the grid's centre where the chessboard's centre is"""
    p = pattern_points(pattern, rows, cols, d)
    centre = np.array([(K.COLS - 1) * K.SQUARE / 2, (K.ROWS - 1) * K.SQUARE / 2])
    return p - (p.min(axis=0) + p.max(axis=0)) / 2 + centre


def render(Rm, t, rng, ss=4, blur=0.8, noise=2.0):
    """One view of the asymmetric grid: discs of 40 on a board of 210 that reaches one spacing past the outer centres, background 128;
    supersampling, blur and noise as corner_ref.render"""
    obj = grid_points()
    o0 = obj.min(axis=0)
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    us = (np.arange(W_IMG)[:, None] + sub[None, :]).reshape(-1)
    vs = (np.arange(H_IMG)[:, None] + sub[None, :]).reshape(-1)
    U, V = np.meshgrid(us, vs)
    XY = K._unproject_board(np.c_[U.reshape(-1), V.reshape(-1)], Rm, t) - o0
    X, Y = XY[:, 0], XY[:, 1]
    board = (X >= -SPACING) & (X <= (2 * COLS - 1) * SPACING + SPACING) & (Y >= -SPACING) & (Y <= (ROWS - 1) * SPACING + SPACING)
    disc = np.zeros(len(X), bool)
    j0 = np.floor(Y / SPACING)
    for dj in (0, 1):
        j = j0 + dj
        i = np.rint((X - (j % 2) * SPACING) / (2 * SPACING))
        ok = (j >= 0) & (j < ROWS) & (i >= 0) & (i < COLS)
        disc |= ok & ((X - (2 * i + j % 2) * SPACING) ** 2 + (Y - j * SPACING) ** 2 <= RADIUS ** 2)
    val = np.where(np.isfinite(X) & board, np.where(disc, 40.0, 210.0), 128.0).reshape(H_IMG * ss, W_IMG * ss)
    img = val.reshape(H_IMG, ss, W_IMG, ss).mean(axis=(1, 3))
    h = int(math.ceil(4 * blur))
    k = np.exp(-0.5 * (np.arange(-h, h + 1) / blur) ** 2)
    k /= k.sum()
    pad = np.pad(img, h, mode="edge")
    img = sum(k[i] * pad[:, i:i + W_IMG] for i in range(2 * h + 1))
    img = sum(k[i] * img[i:i + H_IMG, :] for i in range(2 * h + 1))
    img = img + noise * rng.standard_normal(img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


_SCENES = {}


def scene(seed, n_views=6):
    """-> dict(images [n][240][320] uint8, truth [n][44][2] true projections of the circle centres, poses)"""
    key = (seed, n_views)
    if key not in _SCENES:
        rng = np.random.default_rng(seed)
        imgs, truth, poses = [], [], []
        obj = np.c_[grid_points(), np.zeros(ROWS * COLS)]
        for k in range(n_views):
            Rm, t = K.view_pose(k, seed)
            imgs.append(render(Rm, t, rng))
            truth.append(R.project(R.PINHOLE, CAMERA, obj @ Rm.T + t))
            poses.append((Rm, t))
        _SCENES[key] = dict(images=np.stack(imgs), truth=np.stack(truth), poses=poses)
    return _SCENES[key]


SCENE_SEED = 3
MAX_BLOBS = 128


def restatement_boards():
    """[(found, unique, uv [44][2] or None, corrected uv or None, n_peaks, n_unflagged)] of the scene by the restatement alone"""
    if "boards" not in _CACHE:
        sc = scene(SCENE_SEED)
        d = detect_cached(("scene", SCENE_SEED), sc["images"], DEFAULT, MAX_BLOBS)
        obj = grid_points()
        out = []
        for i in range(len(sc["images"])):
            k = min(int(d["count"][i]), MAX_BLOBS)
            good = np.flatnonzero(d["flags"][i, :k] == 0)
            index, unique = order(d["xy"][i, good], d["shape"][i, good], ASYMMETRIC, ROWS, COLS)
            uv = None if index is None else d["xy"][i, good[index]]
            out.append((index is not None, unique, uv, None if uv is None else corrected(obj, uv, RADIUS), int(d["count"][i]), len(good)))
        _CACHE["boards"] = out
    return _CACHE["boards"]


def rms(uv, truth):
    e = np.linalg.norm(uv - truth, axis=1)
    return float(np.sqrt((e ** 2).mean())), float(e.max())


# ---- the host build of blob_math.hpp / circle_grid.hpp (tests/circle_cpu) ---------------------------------------------------------------
def host_detect(Lb, images, o, max_blobs, want_response=False):
    import ctypes as C

    images = np.ascontiguousarray(images)
    n, H, W = images.shape
    count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xy, shape, fit = np.empty((n, max_blobs, 2)), np.empty((n, max_blobs, 3)), np.empty((n, max_blobs))
    resp, flags = np.empty((n, max_blobs), np.int32), np.empty((n, max_blobs), np.int32)
    Rm = np.empty((n, H, W), np.int32) if want_response else None
    Sm = np.empty((n, H, W), np.uint16) if want_response else None
    Lb.cc_detect(C.c_int(W), C.c_int(H), C.c_int(n), C.c_int(max_blobs), C.c_int(o.polarity), C.c_int(o.a), C.c_int(o.b),
                 C.c_int(o.min_contrast), C.c_int(o.nms_radius), C.c_int(o.max_radius), C.c_int(o.rounds), C.c_double(o.max_fit_error),
                 C.c_double(o.max_axis_ratio), C.c_double(o.min_radius), ptr(images), ptr(count), ptr(status), ptr(xy), ptr(shape), ptr(fit),
                 ptr(resp), ptr(flags), ptr(Rm), ptr(Sm))
    return dict(count=count, status=status, xy=xy, shape=shape, fit_error=fit, response=resp, flags=flags, R=Rm, S=Sm)


def host_order(Lb, xy, shape, pattern, rows, cols):
    import ctypes as C

    xy = np.ascontiguousarray(xy, float)
    shape = None if shape is None else np.ascontiguousarray(shape, float)
    index, unique = np.full(rows * cols, -1, np.int32), C.c_int32(0)
    Lb.cc_order.restype = C.c_int
    found = Lb.cc_order(C.c_int(len(xy)), ptr(xy), ptr(shape), C.c_int(pattern), C.c_int(rows), C.c_int(cols), ptr(index), C.byref(unique))
    return (index, unique.value) if found else (None, 0)


# ---- comparisons and cases ------------------------------------------------------------------------------------------------------------
bitwise = K.bitwise


def same_result(got, ref, tol=1e-9):
    """count, status, response and flags bitwise; xy, shape and fit_error within tol with equal NaN positions"""
    for k in ("count", "status", "response", "flags"):
        if not bitwise(got[k], ref[k]):
            return False
    for k in ("xy", "shape", "fit_error"):
        na, nb = np.isnan(got[k]), np.isnan(ref[k])
        if not (np.array_equal(na, nb) and (np.abs(np.where(na, 0, got[k]) - np.where(nb, 0, ref[k])) <= tol).all()):
            return False
    return True


def blobs_random(n, H, W, seed=0, sigma=1.2):
    """n random images with structure at the scale of the small boxes, so that peaks, ties, flags and clean blobs all occur"""
    return K.smooth_random(n, H, W, seed=seed + 7, sigma=sigma)


def disc(H, W, cx, cy, r, lo=40, hi=210, ss=8):
    """a dark disc of radius r round (cx, cy) on a bright ground, area-sampled"""
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(W)[:, None] + sub[None, :]).reshape(-1)
    ys = (np.arange(H)[:, None] + sub[None, :]).reshape(-1)
    inside = ((xs[None, :] - cx) ** 2 + (ys[:, None] - cy) ** 2 <= r * r).reshape(H, ss, W, ss).mean(axis=(1, 3))
    return np.rint(hi + (lo - hi) * inside).astype(np.uint8)


def rect(H, W, x0, y0, w, h, lo=40, hi=210):
    """a dark w x h rectangle whose first pixel is (x0, y0)"""
    img = np.full((H, W), hi, np.uint8)
    img[y0:y0 + h, x0:x0 + w] = lo
    return img


# the response kernel's tile (BLB_TX x BLB_TY) and the strip height of the peak passes (BLB_SH) in csrc/blob_detect.hip;
# tests/test_circle_cpu.py holds these to the source and SIZES to them
TILE_W, TILE_H, STRIP_H = 64, 16, 16

# sizes of both tiers, (H, W, n_images), with the small boxes a = 1, b = 2, nms = 1 (smallest legal side 7).  Heights: 11; one row
# less and one more than a strip (= a tile) and than two (15, 17, 31, 33) next to whole ones (16, 32); 45 and 40 end in part strips.
# Widths: 64 k - 1, 64 k, 64 k + 1 for k = 1, 2; 23 and 70 are multiples of neither 4 nor 16 (byte staging, single stores), 96 a
# multiple of 16 with a part tile (16-byte staging, vector stores), 68 a multiple of 4 and not of 16 (byte staging, vector stores)
SIZES = [(11, 11, 1), (17, 23, 2), (15, 63, 1), (17, 64, 3), (33, 65, 2), (16, 127, 1), (31, 128, 2), (32, 129, 1), (45, 70, 3), (40, 96, 2),
         (19, 68, 2)]


def border_images(o, H=60, W=72):
    """[(image, inside)]: a disc of radius 4 whose centre pixel lies b + nms from each border (a peak) and one pixel closer (none)"""
    m = o.b + o.nms_radius
    cases = [((m, 30), True), ((m - 1, 30), False), ((36, m), True), ((36, m - 1), False), ((W - 1 - m, 30), True), ((W - m, 30), False),
             ((36, H - 1 - m), True), ((36, H - m), False)]
    return [(disc(H, W, float(cx), float(cy), 4.0), (cx, cy), ok) for (cx, cy), ok in cases]


def planted_cases():
    """[(name, images [n][H][W], Options, max_blobs)] shared by both tiers; tests/test_circle_cpu.py asserts on the restatement that each
    is what it claims"""
    o = DEFAULT._replace(b=8, nms_radius=3, max_radius=12)
    H, W = 50, 150
    tie = disc(H, W, 63.5, 15.5, 3.0)  # no wider than the inner box, so only the four pixels (63 | 64, 15 | 16) round the tile and strip corner have equal responses
    grid = np.minimum(np.minimum(disc(H, W, 30.0, 24.0, 5.0), disc(H, W, 70.0, 25.0, 4.0)), disc(H, W, 110.5, 24.5, 6.0))
    flat = np.full((H, W), 77, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    half = np.where(xx + 0.37 * yy > 80.0, 210, 40).astype(np.uint8)
    ob = DEFAULT._replace(b=6, nms_radius=2, max_radius=10)
    wide = DEFAULT._replace(a=7, b=15, nms_radius=4, max_radius=32)
    return [
        ("tie_on_tile_corner", tie[None], o, 8),
        ("constant_and_half_plane", np.stack([flat, half]), o, 64),
        ("borders", np.stack([im for im, _, _ in border_images(ob)]), ob, 4),
        # a disc cut by the upper border and wider than the outer box: peaks on its rim, whose upward rays leave the image
        ("ray_leaves_image", disc(40, 60, 30.0, 4.0, 10.0)[None], DEFAULT._replace(a=1, b=3, nms_radius=2, max_radius=32), 16),
        ("overflow", grid[None], o, 2),
        ("empty_between", np.stack([grid, flat, tie]), o, 8),
        ("bright", 255 - np.stack([grid, flat, tie]), o._replace(polarity=BRIGHT), 8),
        ("wide_disc_duplicates", disc(70, 80, 40.0, 34.0, 14.0)[None], DEFAULT._replace(b=8, nms_radius=2, max_radius=32), 64),
        ("square", rect(50, 60, 24, 19, 12, 12)[None], o._replace(max_radius=20), 8),
        ("bar", rect(50, 60, 20, 23, 20, 4)[None], o._replace(a=1, max_radius=32), 16),
        # 2 x 2 pixels, smaller than the smallest inner box: the half level lies high on the dot's flank and the moment ellipse has
        # semi-axes 1.61, so this case asks for min_radius = 2
        ("dot", rect(40, 40, 19, 19, 2, 2)[None], o._replace(a=1, b=4, min_radius=2.0), 8),
        ("widest_boxes", disc(70, 150, 60.0, 35.0, 9.0)[None], wide, 8),
    ]
