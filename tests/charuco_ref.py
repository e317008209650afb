"""Independent numpy restatement of ChArUco detection (calibba.h: cba_charuco_detector, cba_marker_dictionary_generate,
cba_chessboard_lattice, cba_charuco_match), written from the header's rule and not from marker_math.hpp / marker_board.hpp, plus the
renderer of the end-to-end scenes and the wrappers of the host build (tests/charuco_cpu).  Corners come from tests/corner_ref.py."""
import math
from collections import namedtuple

import numpy as np

from tests import camera_ref as R
from tests import corner_ref as CR
from tests.host_build import ptr

Options = namedtuple("Options", "arm_lengths arm_offset arm_fan_deg min_arm_contrast min_marker_contrast min_component cell_samples "
                                "max_border_errors max_correction min_markers")
DEFAULT = Options((7.0, 10.0), 2.0, 14.0, 112.0, 40.0, 4, 3, 1, 1, 2)
Board = namedtuple("Board", "squares_x squares_y square marker_bits marker_ratio codes")
DEGENERATE, WINDOW, LOW_CONTRAST, BORDER, NO_MATCH = 1, 2, 4, 8, 16
READING = np.dtype([("code", np.uint64), ("level_min", np.float64), ("level_max", np.float64), ("flags", np.int32), ("id", np.int32),
                    ("rotation", np.int32), ("distance", np.int32), ("second_distance", np.int32), ("border_errors", np.int32)])
M64 = (1 << 64) - 1
BUDGET = 200000
WAVES_PER_GROUP, WAVE = 4, 64  # k_marker_read in csrc/marker_read.hip; tests/test_charuco_cpu.py holds these to the source


# ---- dictionary --------------------------------------------------------------------------------------------------------------------
def rotate(code, bits):
    """a quarter-turn clockwise: cell (y, x) of the result = cell (bits - 1 - x, y) of code"""
    n2, out = bits * bits, 0
    for y in range(bits):
        for x in range(bits):
            src = (bits - 1 - x) * bits + y
            out = (out << 1) | ((code >> (n2 - 1 - src)) & 1)
    return out


def dictionary(bits, count, min_distance, seed):
    s, kept, rots = seed & M64, [], []
    for _ in range(BUDGET):
        if len(kept) >= count:
            break
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        c = z >> (64 - bits * bits)
        r = [c]
        for _k in range(3):
            r.append(rotate(r[-1], bits))
        if any(bin(c ^ q).count("1") < min_distance for q in r[1:]):
            continue
        if rots and int(np.min(popcount(np.array(rots, np.uint64) ^ np.uint64(c)))) < min_distance:
            continue
        kept.append(c)
        rots += r
    return np.array(kept, np.uint64)


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def popcount(a):
    return _POP8[np.ascontiguousarray(a, np.uint64).view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1)


def rotated_table(codes, bits):
    out = []
    for c in codes:
        c = int(c)
        for _r in range(4):
            out.append(c)
            c = rotate(c, bits)
    return np.array(out, np.uint64)


# ---- arm test ----------------------------------------------------------------------------------------------------------------------
def legal(x, y, W, H):
    return (x >= 1.0) & (x <= float(W - 2)) & (y >= 1.0) & (y <= float(H - 2))


def bilinear(img, x, y):
    """B(x, y) for arrays of legal positions"""
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    p00, p01 = img[iy, ix].astype(np.float64), img[iy, ix + 1].astype(np.float64)
    p10, p11 = img[iy + 1, ix].astype(np.float64), img[iy + 1, ix + 1].astype(np.float64)
    top, bot = p00 + fx * (p01 - p00), p10 + fx * (p11 - p10)
    return top + fy * (bot - top)


def directions(angle, fan_deg):
    d = np.zeros((12, 2))
    fan = fan_deg * (math.pi / 180.0)
    for k in range(4):
        for f in range(3):
            phi = angle + math.pi / 4 + k * (math.pi / 2) + (f - 1) * fan
            d[3 * k + f] = (math.cos(phi), math.sin(phi))
    return d


def arm_score(img, x, y, dirs, o):
    H, W = img.shape
    off, score = o.arm_offset, None
    for L in o.arm_lengths:
        P, M = [], []
        for k in range(4):
            c, s = dirs[3 * k:3 * k + 3, 0], dirs[3 * k:3 * k + 3, 1]
            px, py = x + L * c, y + L * s
            ax, ay, bx, by = px - off * s, py + off * c, px + off * s, py - off * c
            if not (legal(ax, ay, W, H).all() and legal(bx, by, W, H).all()):
                continue
            d = bilinear(img, ax, ay) - bilinear(img, bx, by)
            sg = -1.0 if k & 1 else 1.0
            P.append(float((sg * d).max()))
            M.append(float((-sg * d).max()))
        if len(P) < 2:
            return 0.0
        sl = max(min(P), min(M))
        score = sl if score is None else min(score, sl)
    return score


def arm_scores(images, det, o, max_corners):
    """scores [n][max_corners] as cba_charuco_detector_arms writes them (NaN past the kept corners)"""
    n = images.shape[0]
    out = np.full((n, max_corners), np.nan)
    for i in range(n):
        for c in range(min(int(det["count"][i]), max_corners)):
            out[i, c] = arm_score(images[i], det["xy"][i, c, 0], det["xy"][i, c, 1], directions(float(det["angle"][i, c]), o.arm_fan_deg), o)
    return out


# ---- lattice -----------------------------------------------------------------------------------------------------------------------
STEP = [(1, 0), (0, 1), (-1, 0), (0, -1)]


def _links(xy, angle):
    n = len(xy)
    link = -np.ones((n, 4), int)
    for c in range(n):
        dist = np.hypot(xy[:, 0] - xy[c, 0], xy[:, 1] - xy[c, 1])
        cand = [j for j in range(n) if j != c and abs(CR._wrap(angle[j] - angle[c], math.pi)) > math.pi / 4]
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
                if abs(CR._wrap(psi - phi, 2 * math.pi)) <= math.radians(35.0) and (best is None or dist[j] < dist[best]):
                    best = j
            if best is not None:
                link[c, k] = best
    mutual = -np.ones((n, 4), int)
    for c in range(n):
        for k in range(4):
            j = link[c, k]
            if j >= 0 and c in link[j]:
                mutual[c, k] = j
    return mutual


def _label(link, alive):
    n = len(link)
    lab = {}
    comp = -np.ones(n, int)
    k_comp = 0
    for start in range(n):
        if not alive[start] or comp[start] >= 0:
            continue
        comp[start], lab[start], todo = k_comp, (0, 0, 0), [start]
        while todo:
            c = todo.pop(0)
            ci, cj, co = lab[c]
            for k in range(4):
                j = link[c, k]
                if j < 0:
                    continue
                back = list(link[j]).index(c)
                t = (k + co) % 4
                new = (ci + STEP[t][0], cj + STEP[t][1], (k + co + 2 - back) % 4)
                if comp[j] >= 0:
                    if lab[j] != new:
                        link[c, k] = -1
                        link[j, back] = -1
                    continue
                comp[j], lab[j] = k_comp, new
                todo.append(j)
        k_comp += 1
    return comp, lab


def _twice(comp, lab):
    claims = {}
    for c in range(len(comp)):
        if comp[c] >= 0:
            claims.setdefault((comp[c], lab[c][0], lab[c][1]), []).append(c)
    return [c for v in claims.values() if len(v) > 1 for c in v]


def _unlink(link, c):
    for k in range(4):
        j = link[c, k]
        if j >= 0:
            link[j][link[j] == c] = -1
            link[c, k] = -1


def lattice(xy, angle, min_component=4):
    """-> (component [n] (-1: none), ij [n][2], number of components)"""
    xy, angle = np.asarray(xy, float).reshape(-1, 2), np.asarray(angle, float).reshape(-1)
    n = len(xy)
    out_comp, out_ij = -np.ones(n, np.int32), np.zeros((n, 2), np.int32)
    if n == 0:
        return out_comp, out_ij, 0
    link = _links(xy, angle)
    alive = np.ones(n, bool)
    comp, lab = _label(link, alive)
    tw = _twice(comp, lab)
    if tw:
        for c in tw:
            alive[c] = False
            _unlink(link, c)
        comp, lab = _label(link, alive)
        for c in _twice(comp, lab):
            comp[c] = -1
            _unlink(link, c)
    weak = [c for c in range(n) if comp[c] >= 0 and (link[c] >= 0).sum() < 2]
    for c in weak:
        comp[c] = -1
    groups = []
    for m in range(comp.max() + 1 if n else 0):
        mem = [c for c in range(n) if comp[c] == m]
        if len(mem) < min_component or not mem:
            continue
        at = {(lab[c][0], lab[c][1]): c for c in mem}
        si, sj = [], []
        for c in mem:
            i, j = lab[c][0], lab[c][1]
            if (i + 1, j) in at:
                si.append(xy[at[(i + 1, j)]] - xy[c])
            if (i, j + 1) in at:
                sj.append(xy[at[(i, j + 1)]] - xy[c])
        if not si or not sj:
            continue
        mi, mj = np.sum(si, axis=0) / len(si), np.sum(sj, axis=0) / len(sj)
        cross = mi[0] * mj[1] - mi[1] * mj[0]
        if cross == 0:
            continue
        ij = np.array([[(-lab[c][0] if cross < 0 else lab[c][0]), lab[c][1]] for c in mem])
        ij -= ij.min(axis=0)
        groups.append((mem, ij))
    groups.sort(key=lambda g: (-len(g[0]), g[0][0]))
    for r, (mem, ij) in enumerate(groups):
        out_comp[mem] = r
        out_ij[mem] = ij
    return out_comp, out_ij, len(groups)


def cells_of(xy, comp, ij):
    """-> (cells [m][3] = (component, i, j), quads [m][4][2]) by component, then j, then i"""
    at = {(int(comp[c]), int(ij[c, 0]), int(ij[c, 1])): c for c in range(len(comp)) if comp[c] >= 0}
    cells, quads = [], []
    for (k, i, j) in sorted(at, key=lambda t: (t[0], t[2], t[1])):
        idx = [at.get((k, i, j)), at.get((k, i + 1, j)), at.get((k, i + 1, j + 1)), at.get((k, i, j + 1))]
        if any(v is None for v in idx):
            continue
        cells.append((k, i, j))
        quads.append(xy[idx])
    return np.array(cells, np.int32).reshape(-1, 3), np.array(quads, float).reshape(-1, 4, 2)


# ---- marker read -------------------------------------------------------------------------------------------------------------------
def homography(q):
    """-> (a, b, c, d, e, f, g, h) or None when degenerate"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(float(p[0]), float(p[1])) for p in q]
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dy1 * dx2
    side = max((q[(k + 1) % 4][0] - q[k][0]) ** 2 + (q[(k + 1) % 4][1] - q[k][1]) ** 2 for k in range(4))
    cross = min(abs((q[(k + 1) % 4][0] - q[k][0]) * (q[(k + 3) % 4][1] - q[k][1]) - (q[(k + 1) % 4][1] - q[k][1]) * (q[(k + 3) % 4][0] - q[k][0]))
                for k in range(4))
    if not cross > 1e-12 * side:
        return None
    g, h = (sx * dy2 - sy * dx2) / den, (dx1 * sy - dy1 * sx) / den
    return (x1 - x0 + g * x1, x3 - x0 + h * x3, x0, y1 - y0 + g * y1, y3 - y0 + h * y3, y0, g, h)


def _unread(flag):
    r = np.zeros((), READING)
    r["flags"], r["id"], r["distance"], r["second_distance"] = flag, -1, -1, -1
    return r


def read_marker(img, quad, bits, ratio, table, o):
    """one reading (a READING record)"""
    H, W = img.shape
    hc = homography(np.asarray(quad, float))
    if hc is None:
        return _unread(DEGENERATE)
    a, b, c, d, e, f, g, h = hc
    side, S = bits + 2, o.cell_samples
    m0, ms = 0.5 * (1.0 - ratio), ratio / float(side)
    cell = np.arange(side, dtype=np.float64)
    loc = 0.25 + 0.5 * (np.arange(S, dtype=np.float64) + 0.5) / float(S)
    t1 = m0 + ms * (cell[:, None] + loc[None, :])  # [cell][sub]: u for (cx, kx), v for (cy, ky)
    v, u = t1[:, None, :, None], t1[None, :, None, :]  # [cy][cx][ky][kx]
    w = g * u + h * v + 1.0
    x, y = (a * u + b * v + c) / w, (d * u + e * v + f) / w
    if not legal(x, y, W, H).all():
        return _unread(WINDOW)
    smp = bilinear(img, x, y).reshape(side, side, S * S)
    mean = np.cumsum(smp, axis=2)[:, :, -1] / float(S * S)
    lo, hi = float(mean.min()), float(mean.max())
    t = (lo + hi) / 2.0
    bright = mean > t
    inner = bright[1:-1, 1:-1]
    border = int(bright.sum() - inner.sum())
    code = 0
    for bit in inner.reshape(-1):
        code = (code << 1) | int(bit)
    dist = popcount(table ^ np.uint64(code))
    key = dist.astype(np.int64) * 65536 + np.arange(len(table))
    best = int(key.min())
    bd, be = best >> 16, best & 0xffff
    other = dist[(np.arange(len(table)) >> 2) != (be >> 2)]
    flags = (LOW_CONTRAST if hi - lo < o.min_marker_contrast else 0) | (BORDER if border > o.max_border_errors else 0) | (
        NO_MATCH if bd > o.max_correction else 0)
    r = np.zeros((), READING)
    r["code"], r["level_min"], r["level_max"], r["flags"], r["id"], r["rotation"] = code, lo, hi, flags, be >> 2, be & 3
    r["distance"], r["second_distance"], r["border_errors"] = bd, (int(other.min()) if len(other) else -1), border
    return r


def read_cells(images, cell_image, quads, board, o, table=None):
    table = rotated_table(board.codes, board.marker_bits) if table is None else table
    out = np.zeros(len(cell_image), READING)
    for t in range(len(cell_image)):
        out[t] = read_marker(images[cell_image[t]], quads[t], board.marker_bits, board.marker_ratio, table, o)
    return out


# ---- board index -------------------------------------------------------------------------------------------------------------------
def marker_squares(board):
    return [(x, y) for y in range(board.squares_y) for x in range(board.squares_x) if (x + y) % 2 == 1]


def _turn(r, a, b):
    for _ in range(r):
        a, b = b, -a
    return a, b


def match(board, comp, ij, xy, cells, flags, ids, rots, min_markers=2):
    """-> (ids ascending, xy, n_markers)"""
    nx, ny = board.squares_x - 1, board.squares_y - 1
    sq = marker_squares(board)
    wins = []
    for k in range(int(comp.max()) + 1 if len(comp) else 0):
        votes = {}
        for t in range(len(cells)):
            if cells[t][0] != k or flags[t] != 0 or not 0 <= ids[t] < len(sq):
                continue
            r = int(rots[t]) & 3
            tx, ty = _turn(r, 2 * int(cells[t][1]) + 1, 2 * int(cells[t][2]) + 1)
            key = (r, (2 * sq[ids[t]][0] - 1 - tx) // 2, (2 * sq[ids[t]][1] - 1 - ty) // 2)
            votes[key] = votes.get(key, 0) + 1
        if not votes:
            continue
        top = max(votes.values())
        if top >= min_markers and list(votes.values()).count(top) == 1:
            wins.append((top, k, [key for key, v in votes.items() if v == top][0]))
    wins.sort(key=lambda w: (-w[0], w[1]))
    owner, used = {}, 0
    for top, k, (r, sx, sy) in wins:
        mine = {}
        for c in np.flatnonzero(comp == k):
            bi, bj = _turn(r, int(ij[c][0]), int(ij[c][1]))
            bi, bj = bi + sx, bj + sy
            if 0 <= bi < nx and 0 <= bj < ny:
                mine[bj * nx + bi] = c
        if any(b in owner for b in mine):
            continue
        owner.update(mine)
        used += top
    out = sorted(owner)
    return np.array(out, np.int32), np.array([xy[owner[b]] for b in out], float).reshape(-1, 2), used


# ---- the whole detector ------------------------------------------------------------------------------------------------------------
_CACHE = {}


def detect(images, board, o=DEFAULT, corner_opts=CR.DEFAULT, max_corners=1024, key=None):
    """-> per image dict(ids, xy, n_markers, n_corners, scores, comp, ij, cells, readings, good); cached per key"""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    det = CR.detect(images, corner_opts, max_corners)
    scores = arm_scores(images, det, o, max_corners)
    table = rotated_table(board.codes, board.marker_bits)
    out = []
    for i in range(images.shape[0]):
        k = min(int(det["count"][i]), max_corners)
        good = np.flatnonzero((det["flags"][i, :k] == 0) & (scores[i, :k] >= o.min_arm_contrast))
        xy, ang = det["xy"][i, good], det["angle"][i, good]
        comp, ij, _ = lattice(xy, ang, o.min_component)
        cells, quads = cells_of(xy, comp, ij)
        rd = read_cells(images, np.full(len(cells), i), quads, board, o, table)
        ids, pxy, nm = match(board, comp, ij, xy, cells, rd["flags"], rd["id"], rd["rotation"], o.min_markers)
        out.append(dict(ids=ids, xy=pxy, n_markers=nm, n_corners=int(det["count"][i]), scores=scores[i], comp=comp, ij=ij, cells=cells,
                        quads=quads, readings=rd, good=good, corners=det["xy"][i], angle=det["angle"][i], flags=det["flags"][i]))
    if key is not None:
        _CACHE[key] = out
    return out


# ---- the renderer ------------------------------------------------------------------------------------------------------------------
CAMERA = CR.CAMERA.copy()
CAMERA[:4] *= 2.0  # 640 x 480
W_IMG, H_IMG, SQUARE = 640, 480, 0.025
DARK, BRIGHT, BACK = 40.0, 210.0, 128.0


def make_board(squares_x, squares_y, bits=4, ratio=0.6, min_distance=None, seed=11, square=SQUARE):
    n = squares_x * squares_y // 2
    codes = dictionary(bits, n, bits * bits // 4 if min_distance is None else min_distance, seed)
    assert len(codes) == n
    return Board(squares_x, squares_y, square, bits, ratio, codes)


def object_points(board):
    nx = board.squares_x - 1
    jj, ii = np.divmod(np.arange(nx * (board.squares_y - 1)), nx)
    return np.stack([(ii + 1) * board.square, (jj + 1) * board.square], axis=1)


def board_value(board, X, Y):
    """grey level of the board plane at board coordinates (arrays); BACK off the board"""
    sq, n, r = board.square, board.marker_bits, board.marker_ratio
    fx, fy = X / sq, Y / sq
    sx, sy = np.floor(fx), np.floor(fy)
    on = (sx >= 0) & (sx < board.squares_x) & (sy >= 0) & (sy < board.squares_y)
    bright = ((sx + sy) % 2 == 1) & on
    ids = -np.ones((board.squares_y, board.squares_x), int)
    for k, (x, y) in enumerate(marker_squares(board)):
        ids[y, x] = k
    bitmap = np.zeros((len(board.codes), n + 2, n + 2))
    for k, c in enumerate(board.codes):
        for p in range(n * n):
            bitmap[k, 1 + p // n, 1 + p % n] = (int(c) >> (n * n - 1 - p)) & 1
    lu, lv = (fx - sx - 0.5 * (1 - r)) / r, (fy - sy - 0.5 * (1 - r)) / r
    inm = bright & (lu >= 0) & (lu < 1) & (lv >= 0) & (lv < 1)
    cu, cv = np.clip(np.floor(lu * (n + 2)), 0, n + 1).astype(int), np.clip(np.floor(lv * (n + 2)), 0, n + 1).astype(int)
    mid = ids[np.clip(sy, 0, board.squares_y - 1).astype(int), np.clip(sx, 0, board.squares_x - 1).astype(int)]
    mval = np.where(bitmap[np.maximum(mid, 0), cv, cu] > 0, BRIGHT, DARK)
    val = np.where(on, np.where(bright, BRIGHT, DARK), BACK)
    return np.where(inm, mval, val)


def view_pose(board, k, seed):
    """corner_ref.view_pose with the board's centre on the optical axis"""
    rng = np.random.default_rng(1000 * seed + k)
    turn = 2 * math.pi * k / 6 + rng.uniform(-0.3, 0.3)
    tilt = rng.uniform(0.25, 0.8)
    ax = rng.uniform(0, 2 * math.pi)
    Rm = CR.rodrigues(tilt * np.array([math.cos(ax), math.sin(ax), 0.0])) @ CR.rodrigues(np.array([0.0, 0.0, turn]))
    centre = np.array([board.squares_x * board.square / 2, board.squares_y * board.square / 2, 0.0])
    t = np.array([rng.uniform(-0.012, 0.012), rng.uniform(-0.008, 0.008), rng.uniform(0.40, 0.46)]) - Rm @ centre
    return Rm, t


def render(board, Rm, t, rng, W=W_IMG, H=H_IMG, ss=4, blur=0.8, noise=2.0):
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    us = (np.arange(W)[:, None] + sub[None, :]).reshape(-1)
    vs = (np.arange(H)[:, None] + sub[None, :]).reshape(-1)
    U, V = np.meshgrid(us, vs)
    xn = R.unproject(R.PINHOLE, CAMERA, np.c_[U.reshape(-1), V.reshape(-1)])
    ray = np.c_[xn, np.ones(len(xn))]
    nrm = Rm[:, 2]
    s = (t @ nrm) / (ray @ nrm)
    P = (ray * s[:, None] - t) @ Rm
    val = board_value(board, P[:, 0], P[:, 1]).reshape(H * ss, W * ss)
    img = val.reshape(H, ss, W, ss).mean(axis=(1, 3))
    h = int(math.ceil(4 * blur))
    k = np.exp(-0.5 * (np.arange(-h, h + 1) / blur) ** 2)
    k /= k.sum()
    pad = np.pad(img, h, mode="edge")
    img = sum(k[i] * pad[:, i:i + W] for i in range(2 * h + 1))
    img = sum(k[i] * img[i:i + H, :] for i in range(2 * h + 1))
    img = img + noise * rng.standard_normal(img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


_SCENES = {}
SCENE_SEED = 1  # no seed is set aside: seeds 1-3 of both boards meet the scene conditions (tests/test_charuco_cpu.py)


def scene(board_key, seed, n_views=6):
    """board_key: "big" (14 x 10 squares, larger than the view) or "small" (10 x 7, fully in view) -> dict(board, images, truth
    [n][n_corners][2], poses)"""
    key = (board_key, seed, n_views)
    if key not in _SCENES:
        board = make_board(14, 10) if board_key == "big" else make_board(10, 7)
        rng = np.random.default_rng(seed)
        obj = np.c_[object_points(board), np.zeros(len(object_points(board)))]
        imgs, truth, poses = [], [], []
        for k in range(n_views):
            Rm, t = view_pose(board, k, seed)
            imgs.append(render(board, Rm, t, rng))
            truth.append(R.project(R.PINHOLE, CAMERA, obj @ Rm.T + t))
            poses.append((Rm, t))
        _SCENES[key] = dict(board=board, images=np.stack(imgs), truth=np.stack(truth), poses=poses)
    return _SCENES[key]


def marker_image(code, bits, side, margin=12, turn=0, lo=DARK, hi=BRIGHT):
    """one marker with its dark border on a bright ground, `side` px wide, axis-aligned, `margin` px of ground round it, turned by
    `turn` quarter-turns clockwise -> (image, quad of the marker area (ratio 1 would sample exactly the marker))"""
    n = bits + 2
    cellmap = np.zeros((n, n))
    for p in range(bits * bits):
        cellmap[1 + p // bits, 1 + p % bits] = (int(code) >> (bits * bits - 1 - p)) & 1
    cellmap = np.rot90(cellmap, -turn)
    S = side + 2 * margin
    y, x = np.mgrid[0:S, 0:S]
    cy, cx = np.clip((y - margin) * n // side, 0, n - 1), np.clip((x - margin) * n // side, 0, n - 1)
    inside = (x >= margin) & (x < margin + side) & (y >= margin) & (y < margin + side)
    return np.where(inside & (cellmap[cy, cx] == 0), lo, hi).astype(np.uint8)


def square_quad(side, margin, ratio):
    """the quad of the square that carries marker_image's marker at `ratio`: the marker area [margin - 0.5, margin + side - 0.5] is the
    central `ratio` of it"""
    c, half = margin - 0.5 + side / 2.0, side / ratio / 2.0
    return np.array([[c - half, c - half], [c + half, c - half], [c + half, c + half], [c - half, c + half]])


# ---- the host build of marker_math.hpp / marker_board.hpp (tests/charuco_cpu) -----------------------------------------------------
def host_arms(Lb, images, xy, count, dirs, o):
    import ctypes as C

    images = np.ascontiguousarray(images)
    n, H, W = images.shape
    m = xy.shape[1]
    xy, dirs = np.ascontiguousarray(xy, float), np.ascontiguousarray(dirs, float)
    count = np.ascontiguousarray(count, np.int32)
    out = np.empty((n, m))
    Lb.ch_arms(C.c_int(W), C.c_int(H), C.c_int(n), C.c_int(m), ptr(images), ptr(count), ptr(xy), ptr(dirs), C.c_double(o.arm_lengths[0]),
               C.c_double(o.arm_lengths[1]), C.c_double(o.arm_offset), ptr(out))
    return out


def host_read(Lb, images, cell_image, quads, board, o):
    import ctypes as C

    images = np.ascontiguousarray(images)
    n, H, W = images.shape
    ci, q = np.ascontiguousarray(cell_image, np.int32), np.ascontiguousarray(quads, float)
    codes = np.ascontiguousarray(board.codes, np.uint64)
    out = np.zeros(len(ci), READING)
    Lb.ch_read(C.c_int(W), C.c_int(H), ptr(images), C.c_int(board.marker_bits), C.c_double(board.marker_ratio), C.c_int(len(codes)), ptr(codes),
               C.c_int(o.cell_samples), C.c_double(o.min_marker_contrast), C.c_int(o.max_border_errors), C.c_int(o.max_correction),
               C.c_int(len(ci)), ptr(ci), ptr(q), ptr(out))
    return out


def same_readings(a, b, tol=0.0):
    """integers, codes and flags bitwise; levels bitwise (tol == 0) or within tol grey levels"""
    for k in ("code", "flags", "id", "rotation", "distance", "second_distance", "border_errors"):
        if not np.array_equal(a[k], b[k]):
            return False
    for k in ("level_min", "level_max"):
        if not (np.array_equal(a[k], b[k]) if tol == 0.0 else (np.abs(a[k] - b[k]) <= tol).all()):
            return False
    return True


# ---- cases shared by both tiers ----------------------------------------------------------------------------------------------------
_DICTS = {}


def cached_dictionary(bits, count, min_distance, seed):
    key = (bits, count, min_distance, seed)
    if key not in _DICTS:
        _DICTS[key] = dictionary(bits, count, min_distance, seed)
        assert len(_DICTS[key]) == count
    return _DICTS[key]


CELL_PX = {3: 12, 4: 12, 5: 12, 6: 11, 7: 10}  # marker sides of 60, 72, 84, 88 and 90 px


def marker_picture(code, bits, turn=0, bright_border=0, margin=30):
    """marker_image of CELL_PX[bits] px per cell; the first `bright_border` border cells (row-major) are drawn bright"""
    side = CELL_PX[bits] * (bits + 2)
    img = marker_image(code, bits, side, margin, turn)
    n, px, k = bits + 2, CELL_PX[bits], 0
    for cy in range(n):
        for cx in range(n):
            if (cx in (0, n - 1) or cy in (0, n - 1)) and k < bright_border:
                img[margin + cy * px:margin + (cy + 1) * px, margin + cx * px:margin + (cx + 1) * px] = int(BRIGHT)
                k += 1
    return img, square_quad(side, margin, 0.6)


def turned(quad, k):
    """the same square entered k corners later: the reading turns back by k quarter-turns"""
    return np.roll(quad, -k, axis=0)


def read_cases():
    """[dict(name, images, board, opts, cell_image, quads, expect)] for cba_charuco_detector_read; expect: None or, per cell, the
    (flags, id, rotation, distance) the case is about (None entries are not claimed).  Wave edges: bits 3..7 give 25, 36, 49, 64 and 81
    marker cells (under a wavefront, exactly one, one plus 17); 16 codes are 64 table entries, exactly one stride of the match loop.
    Workgroup edges: 0, 1, 3, 4, 5 cells with four wavefronts per workgroup."""
    out = []
    o0 = DEFAULT._replace(max_correction=0, max_border_errors=0)
    for bits in (3, 4, 5, 6, 7):
        codes = cached_dictionary(bits, 17, max(1, bits * bits // 5), 3)
        pics = [marker_picture(codes[5], bits, 0), marker_picture(codes[16], bits, 1)]
        S = pics[0][0].shape[0]
        images = np.stack([pics[0][0], np.full((S, S), 77, np.uint8), pics[1][0]])
        q = pics[0][1]
        mirrored = q[[1, 0, 3, 2]]
        two_equal, collinear = q.copy(), q.copy()
        two_equal[1] = two_equal[0]
        collinear[2] = 0.5 * (collinear[1] + collinear[3])
        quads = np.stack([q, turned(q, 1), turned(q, 2), turned(q, 3), q, q, mirrored, two_equal, collinear])
        ci = np.array([0, 0, 0, 0, 2, 1, 0, 0, 0], np.int32)
        expect = [(0, 5, 0, 0), (0, 5, 3, 0), (0, 5, 2, 0), (0, 5, 1, 0), (0, 16, 1, 0), None, None, (DEGENERATE, -1, 0, -1), (DEGENERATE, -1, 0, -1)]
        for S_ in (1, 3, 5):
            out.append(dict(name=f"bits{bits}_samples{S_}", images=images, board=Board(3, 3, 1.0, bits, 0.6, codes),
                            opts=o0._replace(cell_samples=S_), cell_image=ci, quads=quads, expect=expect))
    # dictionary sizes round the stride of the match loop, 6 x 6 bits
    big = cached_dictionary(6, 1000, 8, 9)
    for n in (1, 16, 17, 250, 1000):
        codes = big[:n]
        pics = [marker_picture(codes[n - 1], 6, 2), marker_picture(codes[0], 6, 0)]
        out.append(dict(name=f"dictionary{n}", images=np.stack([p[0] for p in pics]), board=Board(3, 3, 1.0, 6, 0.6, codes), opts=o0,
                        cell_image=np.array([0, 1], np.int32), quads=np.stack([pics[0][1], pics[1][1]]),
                        expect=[(0, n - 1, 2, 0), (0, 0, 0, 0)]))
    # ties and the correction limit, 4 x 4 bits: the drawn code r lies one bit from two ids; from all rotations of one id
    r = 0b0110100110010110  # rot(r) == r
    assert rotate(r, 4) == r
    pic, q = marker_picture(r, 4)
    img1 = pic[None]
    one = np.zeros(1, np.int32)

    def case(name, codes, **kw):
        exp = kw.pop("expect")
        out.append(dict(name=name, images=img1, board=Board(3, 3, 1.0, 4, 0.6, np.array(codes, np.uint64)), opts=o0._replace(**kw),
                        cell_image=one, quads=q[None], expect=[exp]))

    case("tie_two_ids", [r ^ 0x8000, r ^ 0x0001, r ^ 0x0180], max_correction=1, expect=(0, 0, 0, 1))
    case("tie_two_ids_swapped", [r ^ 0x0180, r ^ 0x0001, r ^ 0x8000], max_correction=1, expect=(0, 1, 0, 1))
    case("tie_rotations", [r ^ 0x0400], max_correction=1, expect=(0, 0, 0, 1))
    case("correction_at_limit", [r ^ 0x0003], max_correction=2, expect=(0, 0, None, 2))
    case("correction_over_limit", [r ^ 0x0003], max_correction=1, expect=(NO_MATCH, 0, None, 2))
    case("correction_zero_exact", [r], max_correction=0, expect=(0, 0, 0, 0))
    case("correction_zero_one_bit", [r ^ 0x0010], max_correction=0, expect=(NO_MATCH, 0, None, 1))
    # border errors at the limit and one over
    picb, qb = marker_picture(r, 4, bright_border=2)
    for name, lim, fl in (("border_at_limit", 2, 0), ("border_over_limit", 1, BORDER)):
        out.append(dict(name=name, images=picb[None], board=Board(3, 3, 1.0, 4, 0.6, np.array([r], np.uint64)),
                        opts=o0._replace(max_border_errors=lim), cell_image=one, quads=qb[None], expect=[(fl, 0, 0, 0)]))
    # the closest legal samples: ratio 0.5, 6 bits, one sample per cell: u = 0.25 + (cx + 0.5) / 16, so the quad (-17, -17) .. (47, 47)
    # samples x = 1, 5, .., 29 = W - 2 exactly; half a pixel either way on either axis leaves the legal region
    rnd = CR.smooth_random(1, 31, 31, seed=5)
    base = np.array([[-17.0, -17.0], [47.0, -17.0], [47.0, 47.0], [-17.0, 47.0]])
    shifts = [(0, 0), (-0.5, 0), (0.5, 0), (0, -0.5), (0, 0.5)]
    out.append(dict(name="window_edges", images=rnd, board=Board(3, 3, 1.0, 6, 0.5, big[:16]), opts=o0._replace(cell_samples=1),
                    cell_image=np.zeros(5, np.int32), quads=np.stack([base + np.array(s) for s in shifts]),
                    expect=[None] + [(WINDOW, -1, 0, -1)] * 4))
    # cell counts round the workgroup of four wavefronts; cells of the first and last image with an image without cells between
    codes = cached_dictionary(4, 17, 3, 3)
    pa, qa = marker_picture(codes[2], 4, 3)
    pb, _ = marker_picture(codes[7], 4, 1)
    imgs = np.stack([pa, np.full_like(pa, 200), pb])
    for m in (0, 1, 3, 4, 5):
        ci = np.array([0, 2, 0, 2, 2][:m], np.int32)
        out.append(dict(name=f"cells{m}", images=imgs, board=Board(3, 3, 1.0, 4, 0.6, codes), opts=o0, cell_image=ci,
                        quads=np.stack([qa] * 5)[:m].reshape(m, 4, 2), expect=[(0, 2, 3, 0), (0, 7, 1, 0), (0, 2, 3, 0), (0, 7, 1, 0), (0, 7, 1, 0)][:m]))
    return out


def read_reference(case):
    key = ("read", case["name"])
    if key not in _CACHE:
        _CACHE[key] = read_cells(case["images"], case["cell_image"], case["quads"], case["board"], case["opts"])
    return _CACHE[key]


ARM_CORNERS = CR.Options(1, 3, 2, CR.COG, 5, 5)  # COG: positions are exact quotients, the same on every implementation


def arm_cases():
    """[(name, images, max_corners)] for cba_charuco_detector_arms with ARM_CORNERS and DEFAULT: widths and heights 23, 64, 65, 129;
    one junction 8, 9, 11 and 12 px from each border, where the arms towards it drop out one by one; both polarities; an image
    without corners, so that its slots and those past the kept corners are NaN"""
    out = []
    for H, W in ((23, 23), (64, 65), (65, 129), (129, 64)):
        out.append((f"smooth_{H}x{W}", CR.smooth_random(2, H, W, seed=3), 48))
        out.append((f"checker_{H}x{W}", np.stack([CR.checker(H, W, 11, 3, 2), CR.checker(H, W, 14, 5, 9, 210, 40)]), 96))
    for d in (8, 9, 11, 12):
        H, W = 48, 56
        pos = [(d - 1, 24), (W - 1 - d, 24), (28, d - 1), (28, H - 1 - d), (d - 1, d - 1), (W - 1 - d, H - 1 - d)]  # junction at (cx + .5, cy + .5)
        imgs = [CR.xcorner(H, W, cx, cy) for cx, cy in pos] + [CR.xcorner(H, W, cx, cy, 210, 40) for cx, cy in pos[:2]]
        out.append((f"junction_{d}px", np.stack(imgs + [np.full((H, W), 90, np.uint8)]), 4))
    return out


def arm_reference(name, images, max_corners):
    """-> (corner detection, dirs [n][max_corners][12][2], scores [n][max_corners]) by the restatement"""
    key = ("arms", name)
    if key not in _CACHE:
        det = CR.detect(images, ARM_CORNERS, max_corners)
        dirs = np.zeros(det["angle"].shape + (12, 2))
        for idx in np.ndindex(det["angle"].shape):
            if np.isfinite(det["angle"][idx]):
                dirs[idx] = directions(float(det["angle"][idx]), DEFAULT.arm_fan_deg)
        _CACHE[key] = (det, dirs, arm_scores(images, det, DEFAULT, max_corners))
    return _CACHE[key]
