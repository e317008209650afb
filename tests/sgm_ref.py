"""Independent numpy restatement of semi-global matching as calibba.h states it (cba_sgm_matcher): the census bits by shifted copies of
the zero-padded image, the Hamming cost volume, every path as a sweep over whole rows or columns of candidates arrays, the sum S, and
argmin / uniqueness / left-right check / parabola taken on the S volume.  Also the wrappers of the host build (tests/sgm_cpu), the
result cache both tiers share, and option_cases().  Test infrastructure: the host build and the device are checked against it."""
import numpy as np

from tests.host_build import ptr

from tests.stereo_ref import GEOM, POSE, bitwise, points, random_pairs, truth_pair  # noqa: F401  (scenes and comparisons)

BIG = 1 << 40  # "not admissible" in the S volume
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


class Options:  # cba_sgm_options
    def __init__(self, min_disparity=0, num_disparities=64, p1=4, p2=32, paths=8, uniqueness_percent=10, lr_max_diff=1, subpixel=1,
                 workspace_mb=0):
        self.min_disparity, self.num_disparities, self.p1, self.p2, self.paths = min_disparity, num_disparities, p1, p2, paths
        self.uniqueness_percent, self.lr_max_diff, self.subpixel, self.workspace_mb = uniqueness_percent, lr_max_diff, subpixel, workspace_mb

    def __repr__(self):
        return (f"min{self.min_disparity}_D{self.num_disparities}_p{self.p1}_{self.p2}_r{self.paths}_u{self.uniqueness_percent}"
                f"_lr{self.lr_max_diff}_s{self.subpixel}")


# ---- steps 1 and 2: census and cost -------------------------------------------------------------------------------------------------
def census_bits(I):
    """[H][W][62] bool: b(x, y; i, j) = [I(x+i, y+j) < I(x, y)], pixels outside reading 0"""
    H, W = I.shape
    P = np.zeros((H + 6, W + 8), np.int64)
    P[3:3 + H, 4:4 + W] = I
    c = I.astype(np.int64)
    return np.stack([P[3 + j:3 + j + H, 4 + i:4 + i + W] < c for j in range(-3, 4) for i in range(-4, 5) if (i, j) != (0, 0)], axis=-1)


def census_cost(L, R, dmin, D):
    """C [H][W][D] int64: the count of differing bits; the right bits are all 0 where x - d is outside the image"""
    H, W = L.shape
    cL, cR = np.packbits(census_bits(L), axis=-1), np.packbits(census_bits(R), axis=-1)  # [H][W][8]; the packing is ours, only the set counts
    C = np.empty((H, W, D), np.int64)
    for k in range(D):
        d = dmin + k
        sh = np.zeros_like(cR)
        x0, x1 = max(0, d), min(W, W + d)  # columns x with 0 <= x - d < W
        if x0 < x1:
            sh[:, x0:x1] = cR[:, x0 - d:x1 - d]
        C[:, :, k] = _POP[cL ^ sh].sum(-1)
    return C


# ---- step 3: paths ------------------------------------------------------------------------------------------------------------------
def _step(Lq, Cp, p1, p2):
    M = Lq.min(-1, keepdims=True)
    m = np.minimum(Lq, M + p2)
    if Lq.shape[-1] > 1:
        m[..., 1:] = np.minimum(m[..., 1:], Lq[..., :-1] + p1)
        m[..., :-1] = np.minimum(m[..., :-1], Lq[..., 1:] + p1)
    return Cp + m - M


def path_costs(C, dx, dy, p1, p2):
    """L_r [H][W][D] of the direction r = (dx, dy)"""
    H, W, _ = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for n, x in enumerate(xs):
            L[:, x] = C[:, x] if n == 0 else _step(L[:, x - dx], C[:, x], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    cols = np.arange(W)
    has = (cols - dx >= 0) & (cols - dx < W)  # the columns whose predecessor's column exists
    for n, y in enumerate(ys):
        L[y] = C[y]
        if n:
            L[y, cols[has]] = _step(L[y - dy, cols[has] - dx], C[y, cols[has]], p1, p2)
    return L


def aggregate(C, o):
    """(S [H][W][D], the largest L_r met)"""
    S, lmax = np.zeros_like(C), 0
    for dx, dy in DIRECTIONS[:o.paths]:
        L = path_costs(C, dx, dy, o.p1, o.p2)
        S += L
        lmax = max(lmax, int(L.max()))
    return S, lmax


# ---- step 4: selection ----------------------------------------------------------------------------------------------------------------
def select(S, o):
    """S [H][W][D] -> (disparity float32 [H][W], cost int32 [H][W])"""
    H, W, D = S.shape
    dmin = o.min_disparity
    ds = dmin + np.arange(D)
    xs = np.arange(W)
    adm = ((xs[None, :] - ds[:, None]) >= 0) & ((xs[None, :] - ds[:, None]) <= W - 1)  # [D][W]
    V = np.where(adm[:, None, :], S.transpose(2, 0, 1), BIG)  # [D][H][W]
    k, best = V.argmin(0), V.min(0)  # the first of equals: the lowest d
    any_ = best < BIG
    ks = np.arange(D)[:, None, None]
    nan_ = np.zeros((H, W), bool)
    if o.uniqueness_percent > 0:
        other = np.where(np.abs(ks - k[None]) > 1, V, BIG).min(0)
        nan_ |= (other < BIG) & (100 * other <= (100 + o.uniqueness_percent) * best)
    if o.lr_max_diff >= 0:
        VR = np.full_like(V, BIG)  # VR[d][y][x'] = S(x' + d, y, d)
        for j in range(D):
            d = dmin + j
            x0, x1 = max(0, -d), min(W, W - d)
            if x0 < x1:
                VR[j, :, x0:x1] = S[:, x0 + d:x1 + d, j]
        kr, has_r = VR.argmin(0), VR.min(0) < BIG
        yy, xx = np.nonzero(any_)
        xr = xx - (dmin + k[yy, xx])
        bad = ~has_r[yy, xr] | (np.abs(kr[yy, xr] - k[yy, xx]) > o.lr_max_diff)
        nan_[yy[bad], xx[bad]] = True
    yy, xx = np.indices((H, W))
    cm = np.where(k > 0, V[np.maximum(k - 1, 0), yy, xx], BIG)
    cp = np.where(k < D - 1, V[np.minimum(k + 1, D - 1), yy, xx], BIG)
    den = cm - 2 * best + cp
    step = bool(o.subpixel) & any_ & (cm < BIG) & (cp < BIG) & (den > 0)
    disp = (dmin + k).astype(np.float64)
    with np.errstate(all="ignore"):
        disp = np.where(step, disp + (cm - cp).astype(np.float64) / np.where(step, 2 * den, 1).astype(np.float64), disp)
    disp[~any_ | nan_] = np.nan
    return disp.astype(np.float32), np.where(any_, best, -1).astype(np.int32)


def match_pair(L, R, o):
    """one pair -> (disparity, cost, the largest S, the largest L_r)"""
    S, lmax = aggregate(census_cost(L, R, o.min_disparity, o.num_disparities), o)
    return select(S, o) + (int(S.max()), lmax)


def match(left, right, o, geom=None, pose=None):
    """left, right [n][H][W] uint8 -> dict(disparity, cost, xyz or None, smax, lmax)"""
    n, H, W = left.shape
    out = [match_pair(left[i], right[i], o) for i in range(n)]
    disp, cost = np.stack([a[0] for a in out]), np.stack([a[1] for a in out])
    xyz = None
    if geom is not None:
        yy, xx = np.indices((H, W))
        uvd = np.stack([np.broadcast_to(xx, disp.shape), np.broadcast_to(yy, disp.shape), disp.astype(np.float64)], axis=-1)
        xyz = points(uvd.reshape(-1, 3), geom, pose).astype(np.float32).reshape(n, H, W, 3)
    return dict(disparity=disp, cost=cost, xyz=xyz, smax=max(a[2] for a in out), lmax=max(a[3] for a in out))


_CACHE = {}


def match_cached(key, left, right, o, geom=None, pose=None):
    """match() computed once per key: the CPU and GPU tiers share the restatement's results"""
    if key not in _CACHE:
        _CACHE[key] = match(left, right, o, geom, pose)
    return _CACHE[key]


def same_result(got, ref):
    return all((ref[k] is None and got[k] is None) or bitwise(got[k], ref[k]) for k in ("disparity", "cost", "xyz"))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def band_scene(rows=16):
    """The 48 x 160 constant-disparity-7 scene with a band of `rows` rows wiped to 128: left columns 40-119, right columns 33-112.
    Returns (L, R, the band's rows as a slice)."""
    L, R, _ = truth_pair(lambda x, y: 7.0)
    L, R = L.copy(), R.copy()
    y0 = (48 - rows) // 2
    L[y0:y0 + rows, 40:120] = 128
    R[y0:y0 + rows, 33:113] = 128
    return L, R, slice(y0, y0 + rows)


def noise_pair(H=16, W=64, seed=5):
    """independent uint8 noise left and right"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (1, H, W), dtype=np.uint8), rng.integers(0, 256, (1, H, W), dtype=np.uint8)


# ---- the host build of sgm_math.hpp (tests/sgm_cpu) -------------------------------------------------------------------------------------
def host_match(Lb, left, right, o, geom=None, pose=None):
    import ctypes as C

    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    n, H, W = left.shape
    disp, cost = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.int32)
    xyz = np.empty((n, H, W, 3), np.float32) if geom is not None else None
    g = None if geom is None else np.ascontiguousarray(geom, float)
    p = None if pose is None else np.ascontiguousarray(pose, float)
    Lb.sgm_match(C.c_int(W), C.c_int(H), C.c_int(n), C.c_int(o.min_disparity), C.c_int(o.num_disparities), C.c_int(o.p1), C.c_int(o.p2),
                 C.c_int(o.paths), C.c_int(o.uniqueness_percent), C.c_int(o.lr_max_diff), C.c_int(o.subpixel), ptr(left), ptr(right), ptr(g), ptr(p),
                 ptr(disp), ptr(cost), ptr(xyz))
    return dict(disparity=disp, cost=cost, xyz=xyz)


# ---- the sizes and options of both tiers: every value of every option meets every size at least once, without the full product -------
SIZES = [(1, 1), (1, 9), (7, 1), (7, 9), (16, 63), (16, 64), (16, 65), (33, 130), (21, 257), (48, 160)]
MD = [(0, 1), (0, 17), (0, 24), (-5, 16), (3, 64), (0, 100), (0, 256)]
PEN = [(0, 0), (4, 32), (10, 120), (0, 1023), (1023, 1023)]


def option_cases():
    """[(H, W, n_pairs, Options, with_pose)]: at every size j runs over the seven (min, D); over j the penalties take their five
    values and paths, uniqueness, lr, sub-pixel and n_pairs both of theirs"""
    cases = []
    for si, (H, W) in enumerate(SIZES):
        for j, (dmin, D) in enumerate(MD):
            p1, p2 = PEN[(si + j) % 5]
            o = Options(dmin, D, p1, p2, 8 if (si + j // 2) % 2 else 4, 10 * ((si + j) % 2), 1 if (si + j // 2 + j // 4) % 2 else -1,
                        (j + si // 2) % 2)
            cases.append((H, W, 3 if (si + j // 3) % 2 else 1, o, (si + j) % 3 == 0))
    return cases


def case_id(c):
    return f"{c[0]}x{c[1]}_n{c[2]}_{c[3]}" + ("_pose" if c[4] else "")
