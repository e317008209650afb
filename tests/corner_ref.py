"""Independent numpy restatement of chessboard detection (calibba.h: cba_corner_detector, cba_chessboard_order), written from the
header's rule and not from corner_math.hpp / corner_grid.hpp, plus the renderer of the end-to-end scenes and the wrappers of the host
build (tests/corner_cpu).  Sums whose order the rule fixes are accumulated with np.cumsum (strictly left to right)."""
import math
from collections import namedtuple

import numpy as np

from tests import camera_ref as R
from tests.host_build import ptr

Options = namedtuple("Options", "min_response nms_radius cog_radius refine refine_half_window refine_iterations")
NONE, COG, GRADIENT = 0, 1, 2
FLAG_WINDOW, FLAG_DET, FLAG_DRIFT = 1, 2, 4
RING = [(0, -5), (2, -5), (3, -3), (5, -2), (5, 0), (5, 2), (3, 3), (2, 5), (0, 5), (-2, 5), (-3, 3), (-5, 2), (-5, 0), (-5, -2), (-3, -3),
        (-2, -5)]
DEFAULT = Options(400, 3, 2, GRADIENT, 5, 5)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def response(img):
    """one image [H][W] uint8 -> R [H][W] int16"""
    H, W = img.shape
    I = img.astype(np.int64)
    out = np.zeros((H, W), np.int64)
    if H < 11 or W < 11:
        return out.astype(np.int16)
    ring = [I[5 + dy:H - 5 + dy, 5 + dx:W - 5 + dx] for dx, dy in RING]
    sr = sum(np.abs(ring[n] + ring[n + 8] - ring[n + 4] - ring[n + 12]) for n in range(4))
    dr = sum(np.abs(ring[n] - ring[n + 8]) for n in range(8))
    s16 = sum(ring)
    s5 = I[5:H - 5, 5:W - 5] + I[5:H - 5, 4:W - 6] + I[5:H - 5, 6:W - 4] + I[4:H - 6, 5:W - 5] + I[6:H - 4, 5:W - 5]
    out[5:H - 5, 5:W - 5] = 5 * sr - 5 * dr - np.abs(5 * s16 - 16 * s5)
    return out.astype(np.int16)


def peaks(Rm, min_response, nms):
    """-> [(y, x)] in row-major order"""
    H, W = Rm.shape
    b = 5 + nms
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


def cog(Rm, px, py, c):
    win = np.maximum(Rm[py - c:py + c + 1, px - c:px + c + 1].astype(np.int64), 0)
    d = np.arange(-c, c + 1)
    s = int(win.sum())
    return px + float(int((win * d[None, :]).sum())) / float(s), py + float(int((win * d[:, None]).sum())) / float(s)


def trig_table():
    c = [(dx * dx - dy * dy) / float(dx * dx + dy * dy) for dx, dy in RING[:8]]
    s = [(2.0 * dx * dy) / float(dx * dx + dy * dy) for dx, dy in RING[:8]]
    return c, s


def weight_table(w):
    den = 2.0 * ((w / 2.0) * (w / 2.0))
    return np.array([[math.exp(-float(dx * dx + dy * dy) / den) for dx in range(-w, w + 1)] for dy in range(-w, w + 1)])


def angle_at(img, px, py):
    c, s = trig_table()
    a = b = 0.0
    for n, (dx, dy) in enumerate(RING[:8]):
        p = float(int(img[py + dy, px + dx]) + int(img[py - dy, px - dx]))
        a = a + p * c[n]
        b = b + p * s[n]
    return 0.5 * math.atan2(b, a)


def _seqsum(v):
    return float(np.cumsum(v.reshape(-1))[-1])


def gradient(img, px, py, x, y, cog_radius, w, iters, wt=None):
    """-> (x, y, flags)"""
    H, W = img.shape
    wt = weight_table(w) if wt is None else wt
    lim = float(w + 2)
    inside = lambda u, v: u >= lim and u <= float(W - 1) - lim and v >= lim and v <= float(H - 1) - lim
    flags = 0 if inside(x, y) else FLAG_WINDOW
    d = np.arange(-w, w + 1, dtype=np.float64)
    ox, oy = np.broadcast_to(d[None, :], wt.shape), np.broadcast_to(d[:, None], wt.shape)
    it = 0
    while it < iters and not flags:
        it += 1
        x0, y0 = math.floor(x), math.floor(y)
        fx, fy = x - x0, y - y0
        ix, iy = int(x0), int(y0)
        # P over offsets -w-1 .. w+1 on both axes
        blk = img[iy - w - 1:iy + w + 3, ix - w - 1:ix + w + 3].astype(np.float64)
        top = blk[:-1, :-1] + fx * (blk[:-1, 1:] - blk[:-1, :-1])
        bot = blk[1:, :-1] + fx * (blk[1:, 1:] - blk[1:, :-1])
        P = top + fy * (bot - top)  # [2w+3][2w+3]
        gx = (P[1:-1, 2:] - P[1:-1, :-2]) * 0.5
        gy = (P[2:, 1:-1] - P[:-2, 1:-1]) * 0.5
        tgx, tgy = gx * wt, gy * wt
        gxx, gxy, gyy = tgx * gx, tgx * gy, tgy * gy
        a, b, c = _seqsum(gxx), _seqsum(gxy), _seqsum(gyy)
        b1, b2 = _seqsum(gxx * ox + gxy * oy), _seqsum(gxy * ox + gyy * oy)
        det, tr = a * c - b * b, a + c
        if not det > 1e-6 * (tr * tr):
            flags |= FLAG_DET
            break
        nx, ny = x + (c * b1 - b * b2) / det, y + (a * b2 - b * b1) / det
        if not inside(nx, ny):
            flags |= FLAG_WINDOW
            break
        x, y = nx, ny
    far = float(cog_radius + 1)
    if abs(x - px) > far or abs(y - py) > far:
        flags |= FLAG_DRIFT
    return x, y, flags


def detect(images, o, max_corners):
    """images [n][H][W] uint8 -> dict(count, status, xy, angle, response, flags, peaks) shaped as cba_corner_detector_process writes"""
    n = images.shape[0]
    count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xy, angle = np.full((n, max_corners, 2), np.nan), np.full((n, max_corners), np.nan)
    resp, flags = np.zeros((n, max_corners), np.int32), np.zeros((n, max_corners), np.int32)
    wt = weight_table(o.refine_half_window)
    for i in range(n):
        Rm = response(images[i])
        pk = peaks(Rm, o.min_response, o.nms_radius)
        count[i] = len(pk)
        status[i] = 1 if len(pk) > max_corners else 0
        for k, (py, px) in enumerate(pk[:max_corners]):
            x, y, f = float(px), float(py), 0
            if o.refine != NONE:
                x, y = cog(Rm, px, py, o.cog_radius)
            if o.refine == GRADIENT:
                x, y, f = gradient(images[i], px, py, x, y, o.cog_radius, o.refine_half_window, o.refine_iterations, wt)
            xy[i, k] = (x, y)
            angle[i, k] = angle_at(images[i], px, py)
            resp[i, k] = Rm[py, px]
            flags[i, k] = f
    return dict(count=count, status=status, xy=xy, angle=angle, response=resp, flags=flags)


_CACHE = {}


def detect_cached(key, images, o, max_corners):
    """detect() computed once per key: the CPU and GPU tiers share the restatement's results"""
    if key not in _CACHE:
        _CACHE[key] = detect(images, o, max_corners)
    return _CACHE[key]


# ---- grid order ------------------------------------------------------------------------------------------------------------------------
def _wrap(d, period):
    d = math.fmod(d, period)
    if d > period / 2:
        d -= period
    if d <= -period / 2:
        d += period
    return d


def order(xy, angle, rows, cols):
    """-> index [rows cols] (row-major over (j, i)) or None"""
    xy, angle = np.asarray(xy, float).reshape(-1, 2), np.asarray(angle, float).reshape(-1)
    n, need = len(xy), rows * cols
    if n < need:
        return None
    link = -np.ones((n, 4), int)
    for c in range(n):
        dist = np.hypot(*(xy - xy[c]).T)
        cand = [j for j in range(n) if j != c and abs(_wrap(angle[j] - angle[c], math.pi)) > math.pi / 4]
        if not cand:
            continue
        dmin = min(dist[j] for j in cand)
        if not dmin > 0:
            continue
        cand = [j for j in cand if dist[j] <= 1.7 * dmin]
        for k in range(4):
            phi = angle[c] + math.pi / 4 + k * (math.pi / 2)
            best = None
            for j in cand:
                psi = math.atan2(xy[j, 1] - xy[c, 1], xy[j, 0] - xy[c, 0])
                if abs(_wrap(psi - phi, 2 * math.pi)) <= math.radians(35.0) and (best is None or dist[j] < dist[best]):
                    best = j
            if best is not None:
                link[c, k] = best
    mutual = -np.ones((n, 4), int)
    for c in range(n):
        for k in range(4):
            j = link[c, k]
            if j >= 0 and c in link[j]:
                mutual[c, k] = j
    centre = xy.mean(axis=0)
    starts = np.argsort(np.hypot(*(xy - centre).T), kind="stable")
    step = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    seen = {}
    for s in starts:
        if s in seen:
            continue
        lab, ok, todo = {s: (0, 0, 0)}, True, [s]
        seen[s] = True
        while todo:
            c = todo.pop(0)
            ci, cj, co = lab[c]
            for k in range(4):
                j = mutual[c, k]
                if j < 0:
                    continue
                back = list(mutual[j]).index(c)
                t = (k + co) % 4
                new = (ci + step[t][0], cj + step[t][1], (k + co + 2 - back) % 4)
                if j in lab:
                    ok &= lab[j] == new
                    continue
                lab[j] = new
                seen[j] = True
                todo.append(j)
        if not ok or len(lab) != need:
            continue
        ii, jj = np.array([v[0] for v in lab.values()]), np.array([v[1] for v in lab.values()])
        ids = np.array(list(lab.keys()))
        ii, jj = ii - ii.min(), jj - jj.min()
        ni, nj = ii.max() + 1, jj.max() + 1
        if (ni, nj) not in ((cols, rows), (rows, cols)) or len(set(zip(ii, jj))) != need:
            continue
        best = None
        for tr in (False, True):
            a, b = (jj, ii) if tr else (ii, jj)
            if a.max() + 1 != cols or b.max() + 1 != rows:
                continue
            for fi in (False, True):
                for fj in (False, True):
                    a2 = cols - 1 - a if fi else a
                    b2 = rows - 1 - b if fj else b
                    G = np.empty((rows, cols), int)
                    G[b2, a2] = ids
                    P = xy[G]
                    mi, mj = (P[:, 1:] - P[:, :-1]).mean(axis=(0, 1)), (P[1:] - P[:-1]).mean(axis=(0, 1))
                    if not mi[0] * mj[1] - mi[1] * mj[0] > 0:
                        continue
                    if best is None or (mi[0], mi[1]) > best[0]:
                        best = ((mi[0], mi[1]), G.reshape(-1).astype(np.int32))
        if best is not None:
            return best[1]
    return None


# ---- the renderer ----------------------------------------------------------------------------------------------------------------------
CAMERA = np.array([420.0, 415.0, 158.0, 121.0, 0.0, -0.12, 0.05, 0.0, 8e-4, -5e-4])  # 320 x 240, Brown-Conrady (k1 k2 k3 p1 p2)
W_IMG, H_IMG, ROWS, COLS, SQUARE = 320, 240, 6, 9, 0.025


def rodrigues(r):
    t = np.linalg.norm(r)
    if t < 1e-12:
        return np.eye(3)
    k = r / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def board_points(rows=ROWS, cols=COLS, square=SQUARE):
    jj, ii = np.divmod(np.arange(rows * cols), cols)
    return np.stack([ii * square, jj * square], axis=1)


def view_pose(k, seed, square=SQUARE):
    """pose (R, t) of view k of a scene: tilt up to about 0.8 rad about a random in-plane axis, an in-plane turn that walks round the
    whole circle, the board's centre near the optical axis"""
    rng = np.random.default_rng(1000 * seed + k)
    turn = 2 * math.pi * k / 6 + rng.uniform(-0.3, 0.3)
    tilt = rng.uniform(0.25, 0.8)
    ax = rng.uniform(0, 2 * math.pi)
    Rm = rodrigues(tilt * np.array([math.cos(ax), math.sin(ax), 0.0])) @ rodrigues(np.array([0.0, 0.0, turn]))
    centre = np.array([(COLS - 1) * square / 2, (ROWS - 1) * square / 2, 0.0])
    t = np.array([rng.uniform(-0.012, 0.012), rng.uniform(-0.008, 0.008), rng.uniform(0.40, 0.46)]) - Rm @ centre
    return Rm, t


def _unproject_board(uv, Rm, t):
    """pixels [n][2] -> board coordinates (X, Y) [n][2] of the ray's hit with the board plane (NaN where the ray misses)"""
    xn = R.unproject(R.PINHOLE, CAMERA, uv)
    ray = np.c_[xn, np.ones(len(xn))]
    nrm, o = Rm[:, 2], t
    s = (o @ nrm) / (ray @ nrm)
    P = (ray * s[:, None] - o) @ Rm  # R^T (P_cam - t)
    return P[:, :2]


def render(Rm, t, rng, ss=4, blur=0.8, noise=2.0, square=SQUARE):
    """One view: 4 x 4 supersampling of the board seen through the pose and CAMERA (dark 40, bright 210, background 128), a Gaussian
    blur of `blur` px, noise of `noise` grey levels, rounded to uint8"""
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    us = (np.arange(W_IMG)[:, None] + sub[None, :]).reshape(-1)
    vs = (np.arange(H_IMG)[:, None] + sub[None, :]).reshape(-1)
    U, V = np.meshgrid(us, vs)
    XY = _unproject_board(np.c_[U.reshape(-1), V.reshape(-1)], Rm, t)
    ci, cj = np.floor(XY[:, 0] / square + 1), np.floor(XY[:, 1] / square + 1)  # squares -1 .. cols-1 -> 0 .. cols
    on = (ci >= 0) & (ci <= COLS) & (cj >= 0) & (cj <= ROWS)
    val = np.where(on, np.where((ci + cj) % 2 == 1, 210.0, 40.0), 128.0).reshape(H_IMG * ss, W_IMG * ss)
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


def scene(seed, n_views=6, square=SQUARE):
    """-> dict(images [n][240][320] uint8, truth [n][54][2] true projections of the inner corners, poses); square: the side of a
    square in metres at 0.40 .. 0.46 m from a camera of 420 px focal length (0.025 m: about 24 px seen frontally)"""
    key = (seed, n_views, square)
    if key not in _SCENES:
        rng = np.random.default_rng(seed)
        imgs, truth, poses = [], [], []
        obj = np.c_[board_points(square=square), np.zeros(ROWS * COLS)]
        for k in range(n_views):
            Rm, t = view_pose(k, seed, square)
            imgs.append(render(Rm, t, rng, square=square))
            truth.append(R.project(R.PINHOLE, CAMERA, obj @ Rm.T + t))
            poses.append((Rm, t))
        _SCENES[key] = dict(images=np.stack(imgs), truth=np.stack(truth), poses=poses)
    return _SCENES[key]


def match_truth(uv, truth):
    """The detected board against the true projections: the board is symmetric under a half turn, so the labelling may be the truth's
    or its half turn; -> (rms, max) of the better one"""
    e = [np.linalg.norm(uv - t, axis=1) for t in (truth, truth[::-1])]
    e = min(e, key=lambda v: v.max())
    return float(np.sqrt((e ** 2).mean())), float(e.max())


SCENE_SEED = 3  # seeds 1 and 2 set aside: in views 1, 2, 5 (seed 1) and 1, 2, 4, 5 (seed 2) a corner of the board lies closer than
#                 5 + nms_radius = 8 px to the image border or outside the image, so the plain chessboard cannot be indexed there


def restatement_boards(refine):
    """[(found, uv [54][2], n_peaks)] of the scene by the restatement alone, computed once per mode"""
    sc = scene(SCENE_SEED)
    o = DEFAULT._replace(refine=refine)
    d = detect_cached(("scene", SCENE_SEED, refine), sc["images"], o, 128)
    out = []
    for i in range(len(sc["images"])):
        k = min(int(d["count"][i]), 128)
        good = np.flatnonzero(d["flags"][i, :k] == 0)
        index = order(d["xy"][i, good], d["angle"][i, good], ROWS, COLS)
        out.append((index is not None, None if index is None else d["xy"][i, good[index]], int(d["count"][i])))
    return out


# ---- the host build of corner_math.hpp / corner_grid.hpp (tests/corner_cpu) -----------------------------------------------------------
def host_detect(Lb, images, o, max_corners, want_response=False):
    import ctypes as C

    images = np.ascontiguousarray(images)
    n, H, W = images.shape
    count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xy, angle = np.empty((n, max_corners, 2)), np.empty((n, max_corners))
    resp, flags = np.empty((n, max_corners), np.int32), np.empty((n, max_corners), np.int32)
    Rm = np.empty((n, H, W), np.int16) if want_response else None
    Lb.cr_detect(C.c_int(W), C.c_int(H), C.c_int(n), C.c_int(max_corners), C.c_int(o.min_response), C.c_int(o.nms_radius),
                 C.c_int(o.cog_radius), C.c_int(o.refine), C.c_int(o.refine_half_window), C.c_int(o.refine_iterations), ptr(images), ptr(count),
                 ptr(status), ptr(xy), ptr(angle), ptr(resp), ptr(flags), ptr(Rm))
    return dict(count=count, status=status, xy=xy, angle=angle, response=resp, flags=flags, R=Rm)


def host_order(Lb, xy, angle, rows, cols):
    import ctypes as C

    xy, angle = np.ascontiguousarray(xy, float), np.ascontiguousarray(angle, float)
    index = np.full(rows * cols, -1, np.int32)
    Lb.cr_order.restype = C.c_int
    found = Lb.cr_order(C.c_int(len(angle)), ptr(xy), ptr(angle), C.c_int(rows), C.c_int(cols), ptr(index))
    return index if found else None


# ---- comparisons and cases ------------------------------------------------------------------------------------------------------------
def bitwise(a, b):
    """equal to the bit, NaN positions equal"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.int64), np.where(nb, 0, b).view(np.int64)))


def same_result(got, ref, xy_tol=0.0):
    """count, status, response, flags and angle bitwise; xy bitwise (xy_tol == 0) or within xy_tol px with equal NaN positions"""
    for k in ("count", "status", "response", "flags", "angle"):
        if not bitwise(got[k], ref[k]):
            return False
    if xy_tol == 0.0:
        return bitwise(got["xy"], ref["xy"])
    na, nb = np.isnan(got["xy"]), np.isnan(ref["xy"])
    return bool(np.array_equal(na, nb) and (np.abs(np.where(na, 0, got["xy"]) - np.where(nb, 0, ref["xy"])) <= xy_tol).all())


def smooth_random(n, H, W, seed=0, sigma=1.5):
    """n random images with structure at the ring's scale (plain white noise has almost no positive response): Gaussian-filtered
    noise stretched to the full range, so that peaks, ties and negative responses all occur"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    t = rng.standard_normal((n, H + 12, W + 12))
    h = int(math.ceil(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-h, h + 1) / sigma) ** 2)
    t = sum(k[i] * np.roll(t, i - h, axis=1) for i in range(2 * h + 1))
    t = sum(k[i] * np.roll(t, i - h, axis=2) for i in range(2 * h + 1))[:, 6:6 + H, 6:6 + W]
    t = (t - t.min()) / (t.max() - t.min())
    return np.ascontiguousarray(np.clip(np.rint(255 * np.clip(2.0 * t - 0.5, 0, 1)), 0, 255).astype(np.uint8))


def checker(H, W, square, ox=0, oy=0, lo=40, hi=210):
    """an axis-aligned periodic chessboard filling the image: corners at (ox + k square - 0.5, oy + l square - 0.5)"""
    y, x = np.mgrid[0:H, 0:W]
    return np.where((((x - ox) // square) + ((y - oy) // square)) % 2 == 0, lo, hi).astype(np.uint8)


# the response kernel's tile (CRN_TX x CRN_TY) and the strip height of the peak passes (CRN_SH) in csrc/corner_detect.hip;
# tests/test_corner_cpu.py holds these to the source and SIZES to them, so a change of either constant cannot leave an edge uncovered
TILE_W, TILE_H, STRIP_H = 64, 16, 16

# sizes of the GPU tier, (H, W, n_images).  Heights: the smallest legal 11; one row less and one more than a strip and than two strips
# (15, 17, 31, 33) next to whole strips (16, 32); 40 and 45 end in a part strip of 8 and 13 rows.  The tile is as high as a strip, so the
# same heights are its edges.  Widths: 64 k - 1, 64 k, 64 k + 1 for k = 1, 2; 23 and 70 are multiples of neither 4 nor 16 (byte
# staging, single int16 stores), 96 a multiple of 16 with a part tile (16-byte staging, 8-byte stores), 68 a multiple of 4 and not of
# 16 (byte staging with 8-byte stores)
SIZES = [(11, 11, 1), (17, 23, 2), (15, 63, 1), (17, 64, 3), (33, 65, 2), (16, 127, 1), (31, 128, 2), (32, 129, 1), (45, 70, 3), (40, 96, 2),
         (19, 68, 2)]


def xcorner(H, W, cx, cy, lo=40, hi=210):
    """one X-junction at (cx + 0.5, cy + 0.5): the four pixels (cx | cx + 1, cy | cy + 1) have equal responses"""
    y, x = np.mgrid[0:H, 0:W]
    return np.where((x > cx) == (y > cy), lo, hi).astype(np.uint8)


def border_images(H=40, W=52, b=8):
    """[(image, expected peaks [(y, x)])]: the junction's winning pixel at the closest legal distance b = 5 + nms_radius to each
    border, and one pixel closer, where it is absent (the lowest of the four equal pixels wins; when it lies outside the legal
    region the others lose to it all the same)"""
    cases = [((b, b), [(b, b)]), ((b - 1, 20), []), ((20, b - 1), []), ((W - 1 - b, 20), [(20, W - 1 - b)]), ((W - b, 20), []),
             ((20, H - 1 - b), [(H - 1 - b, 20)]), ((20, H - b), [])]
    return [(xcorner(H, W, cx, cy), exp) for (cx, cy), exp in cases]


def planted_cases():
    """[(name, images [n][H][W], Options, max_corners)] shared by both tiers.  The tile of the response kernel is TILE_W x TILE_H = 64 x 16 and the
    strip of the peak kernels STRIP_H = 16 rows.  The periodic boards of 16-pixel squares have a junction, four pixels of
    equal response, at every (16 k - 0.5, 16 l - 0.5) (c0) or one pixel further (c1).  c0's tie at k = 4, l = 1 is the pixels
    (63 | 64, 15 | 16): it straddles the tile edge x = 64 and the tile and strip edge y = 16, two of its pixels in the same row and two in
    adjacent rows.  c1's is (64 | 65, 16 | 17): the surviving pixel is the tile's and the strip's first, and its NMS window reaches
    back into both neighbours."""
    c0, c1 = checker(50, 150, 16), checker(50, 150, 16, 1, 1)
    flat = np.full((50, 150), 77, np.uint8)
    split = np.concatenate([np.zeros((50, 75), np.uint8), np.full((50, 75), 255, np.uint8)], axis=1)
    o = Options(1, 3, 2, COG, 5, 5)
    border = np.stack([im for im, _ in border_images()])
    return [
        ("ties_on_tile_edges", np.stack([c0, c1]), o, 64),
        ("ties_gradient", np.stack([c0, c1]), o._replace(refine=GRADIENT), 64),
        ("constant_and_split", np.stack([flat, split]), o, 16),
        ("borders", border, o._replace(refine=NONE), 4),
        ("overflow", np.stack([c1, c0]), o, 3),
        ("empty_between", np.stack([c0, flat, c1]), o._replace(refine=GRADIENT), 64),
        ("gradient_window_flag", np.stack([xcorner(40, 52, 8, 8), xcorner(40, 52, 20, 20)]), Options(1, 3, 2, GRADIENT, 7, 5), 4),
    ]
