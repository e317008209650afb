"""Independent numpy restatement of stereo depth as calibba.h states it (cba_stereo_rectify, cba_stereo_matcher, cba_stereo_points):
the closed-form rectification, the whole cost volume by integral images with argmin / uniqueness / left-right check / parabola taken on
it, and disparity to 3D.  Also the scene makers of the stereo tests and the wrappers of the host build (tests/stereo_cpu).  Test
infrastructure: the host build and the device are checked against it."""
import numpy as np

from tests.host_build import ptr

BIG = 1 << 40  # "not admissible" in the cost volume


class Options:  # cba_stereo_match_options
    def __init__(self, min_disparity=0, num_disparities=64, half_window=4, uniqueness_percent=10, lr_max_diff=1, subpixel=1):
        self.min_disparity, self.num_disparities, self.half_window = min_disparity, num_disparities, half_window
        self.uniqueness_percent, self.lr_max_diff, self.subpixel = uniqueness_percent, lr_max_diff, subpixel

    def __repr__(self):
        return (f"min{self.min_disparity}_D{self.num_disparities}_r{self.half_window}_u{self.uniqueness_percent}_lr{self.lr_max_diff}"
                f"_s{self.subpixel}")


def quat_to_rotmat(q):  # the quaternion's matrix without normalisation
    w, x, y, z = q
    return np.array([[1.0 - (2.0 * y * y + 2.0 * z * z), 2.0 * y * x - 2.0 * z * w, 2.0 * z * x + 2.0 * y * w],
                     [2.0 * y * x + 2.0 * z * w, 1.0 - (2.0 * x * x + 2.0 * z * z), 2.0 * z * y - 2.0 * x * w],
                     [2.0 * z * x - 2.0 * y * w, 2.0 * z * y + 2.0 * x * w, 1.0 - (2.0 * x * x + 2.0 * y * y)]])


# ---- rectification ----------------------------------------------------------------------------------------------------------------
def rectify(intr, c_T_r, W, H, focal=0.0, cx=0.0, cy=0.0):
    """intr [2][10 | 12], c_T_r [2][7] -> dict(R [2][3][3], new_k5 [2][5], baseline, rect_R_r, o0)"""
    intr, c_T_r = np.asarray(intr, float), np.asarray(c_T_r, float)
    Rs = [quat_to_rotmat(p[:4] / np.linalg.norm(p[:4])) for p in c_T_r]
    o = [-Rm.T @ p[4:] for Rm, p in zip(Rs, c_T_r)]
    B = np.linalg.norm(o[1] - o[0])
    e1 = (o[1] - o[0]) / B
    zbar = Rs[0].T[:, 2] + Rs[1].T[:, 2]
    e2 = np.cross(zbar, e1)
    e2 /= np.linalg.norm(e2)
    e3 = np.cross(e1, e2)
    M = np.stack([e1, e2, e3])
    f = focal if focal > 0 else (intr[0, 0] + intr[0, 1] + intr[1, 0] + intr[1, 1]) / 4.0
    k = [f, f, cx if cx and cx == cx else (W - 1) / 2.0, cy if cy and cy == cy else (H - 1) / 2.0, 0.0]
    return dict(R=np.stack([M @ Rs[0].T, M @ Rs[1].T]), new_k5=np.array([k, k]), baseline=B, rect_R_r=M, o0=o[0])


# ---- matching -----------------------------------------------------------------------------------------------------------------------
def cost_volume(L, R, dmin, D, r):
    """C [D][H][W] (int64) of one pair: C(x, y, d) where admissible, BIG elsewhere"""
    H, W = L.shape
    Li, Ri = L.astype(np.int64), R.astype(np.int64)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    C = np.full((D, H, W), BIG, np.int64)
    for k in range(D):
        d = dmin + k
        ad = np.zeros((H, W), np.int64)
        x0, x1 = max(0, d), min(W, W + d)  # columns x with 0 <= x - d < W
        if x0 < x1:
            ad[:, x0:x1] = np.abs(Li[:, x0:x1] - Ri[:, x0 - d:x1 - d])
        I = np.zeros((H + 1, W + 1), np.int64)
        I[1:, 1:] = ad.cumsum(0).cumsum(1)
        adm = (ys >= r) & (ys <= H - 1 - r) & (xs >= r) & (xs <= W - 1 - r) & (xs - r - d >= 0) & (xs + r - d <= W - 1)
        yy, xx = np.nonzero(adm)
        C[k, yy, xx] = I[yy + r + 1, xx + r + 1] - I[yy - r, xx + r + 1] - I[yy + r + 1, xx - r] + I[yy - r, xx - r]
    return C


def match_pair(L, R, o):
    """one pair -> (disparity float32 [H][W], cost int32 [H][W])"""
    H, W = L.shape
    dmin, D, r = o.min_disparity, o.num_disparities, o.half_window
    C = cost_volume(L, R, dmin, D, r)
    k = C.argmin(0)  # the first of equals: the lowest d
    best = C.min(0)
    any_ = best < BIG
    ks = np.arange(D)[:, None, None]
    nan_ = np.zeros((H, W), bool)
    if o.uniqueness_percent > 0:
        other = np.where(np.abs(ks - k[None]) > 1, C, BIG).min(0)
        nan_ |= (other < BIG) & (100 * other <= (100 + o.uniqueness_percent) * best)
    if o.lr_max_diff >= 0:
        CR = np.full_like(C, BIG)  # CR[d][y][x'] = C(x' + d, y, d)
        for j in range(D):
            d = dmin + j
            x0, x1 = max(0, -d), min(W, W - d)
            if x0 < x1:
                CR[j, :, x0:x1] = C[j, :, x0 + d:x1 + d]
        kr, has_r = CR.argmin(0), CR.min(0) < BIG
        yy, xx = np.nonzero(any_)
        xr = xx - (dmin + k[yy, xx])
        bad = ~has_r[yy, xr] | (np.abs(kr[yy, xr] - k[yy, xx]) > o.lr_max_diff)
        nan_[yy[bad], xx[bad]] = True
    yy, xx = np.indices((H, W))
    cm = np.where(k > 0, C[np.maximum(k - 1, 0), yy, xx], BIG)
    cp = np.where(k < D - 1, C[np.minimum(k + 1, D - 1), yy, xx], BIG)
    den = cm - 2 * best + cp
    step = bool(o.subpixel) & any_ & (cm < BIG) & (cp < BIG) & (den > 0)
    disp = (dmin + k).astype(np.float64)
    with np.errstate(all="ignore"):
        disp = np.where(step, disp + (cm - cp).astype(np.float64) / np.where(step, 2 * den, 1).astype(np.float64), disp)
    disp[~any_ | nan_] = np.nan
    return disp.astype(np.float32), np.where(any_, best, -1).astype(np.int32)


def points(uvd, geom, pose=None):
    """uvd [n][3] -> xyz [n][3] (fp64); geom = (f, cx, cy, B)"""
    uvd = np.asarray(uvd, float).reshape(-1, 3)
    f, cx, cy, B = (float(g) for g in geom)
    u, v, d = uvd[:, 0], uvd[:, 1], uvd[:, 2]
    with np.errstate(all="ignore"):
        ok = (d > 0) & np.isfinite(d) & np.isfinite(u) & np.isfinite(v)
        s = B / d
        P = np.where(ok[:, None], np.stack([(u - cx) * s, (v - cy) * s, f * s], axis=1), np.nan)
        if pose is not None:
            pose = np.asarray(pose, float)
            M, t = quat_to_rotmat(pose[:4]), pose[4:]
            P = np.stack([M[i, 0] * P[:, 0] + M[i, 1] * P[:, 1] + M[i, 2] * P[:, 2] + t[i] for i in range(3)], axis=1)
    return P


def match(left, right, o, geom=None, pose=None):
    """left, right [n][H][W] uint8 -> dict(disparity, cost, xyz or None)"""
    n, H, W = left.shape
    out = [match_pair(left[i], right[i], o) for i in range(n)]
    disp, cost = np.stack([a for a, _ in out]), np.stack([b for _, b in out])
    xyz = None
    if geom is not None:
        yy, xx = np.indices((H, W))
        uvd = np.stack([np.broadcast_to(xx, disp.shape), np.broadcast_to(yy, disp.shape), disp.astype(np.float64)], axis=-1)
        xyz = points(uvd.reshape(-1, 3), geom, pose).astype(np.float32).reshape(n, H, W, 3)
    return dict(disparity=disp, cost=cost, xyz=xyz)


_CACHE = {}


def match_cached(key, left, right, o, geom=None, pose=None):
    """match() computed once per key: the CPU and GPU tiers share the restatement's results"""
    if key not in _CACHE:
        _CACHE[key] = match(left, right, o, geom, pose)
    return _CACHE[key]


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
GEOM = (123.5, 30.25, 11.75, 0.0875)
POSE = np.array([0.98, 0.05, -0.12, 0.07, 0.3, -0.2, 1.1])  # not a unit quaternion


def smooth_noise(rng, H, W, sigma=1.2):
    """unit Gaussian noise, Gaussian-filtered with sigma, scaled to 0..255 (float64)"""
    t = rng.standard_normal((H, W))
    h = int(np.ceil(4 * sigma))
    g = np.exp(-0.5 * (np.arange(-h, h + 1) / sigma) ** 2)
    g /= g.sum()
    t = np.apply_along_axis(lambda a: np.convolve(np.pad(a, h, mode="reflect"), g, mode="valid"), 0, t)
    t = np.apply_along_axis(lambda a: np.convolve(np.pad(a, h, mode="reflect"), g, mode="valid"), 1, t)
    return 255.0 * (t - t.min()) / (t.max() - t.min())


def truth_pair(truth, H=48, W=160, noise=0.0, seed=2):
    """The issue's ground-truth recipe: R(x, y) = T(x + 40, y), L(x, y) = T(x - d(x, y) + 40, y) sampled bilinearly along x, pixel noise
    of `noise` grey levels, rounded to uint8.  truth(x, y) -> d.  Returns (L, R, d)."""
    rng = np.random.default_rng(seed)
    T = smooth_noise(rng, H, W + 64)
    yy, xx = np.indices((H, W))
    d = truth(xx.astype(float), yy.astype(float)) + np.zeros((H, W))
    R = T[:, 40:40 + W]
    p = xx - d + 40
    p0 = np.floor(p).astype(int)
    a = p - p0
    L = (1 - a) * T[yy, p0] + a * T[yy, p0 + 1]
    if noise > 0:
        L = L + rng.normal(0, noise, L.shape)
        R = R + rng.normal(0, noise, R.shape)
    q = lambda I: np.clip(np.rint(I), 0, 255).astype(np.uint8)
    return q(L), q(R), d


def random_pairs(n, H, W, shift=3, seed=0):
    """n textured pairs of H x W: the right image is the left one moved by `shift` columns plus a little noise"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    T = smooth_noise(rng, n * H, W + 2 * abs(shift) + 2).reshape(n, H, -1)
    L = T[:, :, abs(shift):abs(shift) + W]
    R = T[:, :, abs(shift) + shift:abs(shift) + shift + W] + rng.normal(0, 1.5, (n, H, W))
    q = lambda I: np.ascontiguousarray(np.clip(np.rint(I), 0, 255).astype(np.uint8))
    return q(L), q(R)


# ---- the host build of stereo_math.hpp (tests/stereo_cpu) -----------------------------------------------------------------------
def host_rectify(Lb, intr, c_T_r, W, H, focal=0.0, cx=0.0, cy=0.0):
    import ctypes as C

    intr, c_T_r = np.ascontiguousarray(intr, float), np.ascontiguousarray(c_T_r, float)
    R, K, B, rt = np.empty((2, 9)), np.empty((2, 5)), np.empty(1), np.empty(7)
    Lb.st_rectify.restype = C.c_int
    st = Lb.st_rectify(ptr(intr), C.c_int(intr.shape[1]), ptr(c_T_r), C.c_int(W), C.c_int(H), C.c_double(focal), C.c_double(cx), C.c_double(cy),
                       ptr(R), ptr(K), ptr(B), ptr(rt))
    if st:
        raise ValueError("stereo_rectify refused the input")
    return dict(R=R.reshape(2, 3, 3), new_k5=K, baseline=float(B[0]), r_T_rect=rt)


def host_match(Lb, left, right, o, geom=None, pose=None):
    import ctypes as C

    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    n, H, W = left.shape
    disp, cost = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.int32)
    xyz = np.empty((n, H, W, 3), np.float32) if geom is not None else None
    g = None if geom is None else np.ascontiguousarray(geom, float)
    p = None if pose is None else np.ascontiguousarray(pose, float)
    Lb.st_match(C.c_int(W), C.c_int(H), C.c_int(n), C.c_int(o.min_disparity), C.c_int(o.num_disparities), C.c_int(o.half_window),
                C.c_int(o.uniqueness_percent), C.c_int(o.lr_max_diff), C.c_int(o.subpixel), ptr(left), ptr(right), ptr(g), ptr(p), ptr(disp), ptr(cost),
                ptr(xyz))
    return dict(disparity=disp, cost=cost, xyz=xyz)


def host_points(Lb, uvd, geom, pose=None):
    import ctypes as C

    uvd = np.ascontiguousarray(uvd, float).reshape(-1, 3)
    g = np.ascontiguousarray(geom, float)
    p = None if pose is None else np.ascontiguousarray(pose, float)
    xyz = np.empty_like(uvd)
    Lb.st_points(ptr(g), ptr(p), C.c_int64(len(uvd)), ptr(uvd), ptr(xyz))
    return xyz


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def bitwise(a, b):
    """equal to the bit, NaN positions equal (any NaN counting as equal to any NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    iv = np.int32 if a.dtype == np.float32 else np.int64
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(iv), np.where(nb, 0, b).view(iv)))


def same_result(got, ref):
    return all((ref[k] is None and got[k] is None) or bitwise(got[k], ref[k]) for k in ("disparity", "cost", "xyz"))


# The sizes and options of the GPU tier (the host build is held to the same): every value of every option meets every size at least
# once, without the full product.
def sizes(r):
    return [(2 * r + 1, 2 * r + 1), (16, 63), (16, 64), (16, 65), (33, 130), (21, 257), (48, 160)]


def option_cases():
    """[(H, W, n_pairs, Options)]"""
    R_ = [1, 4, 10]
    MD = [(0, 1), (0, 24), (-5, 16), (3, 64), (0, 256)]
    cases = []
    for si in range(7):
        for j in range(5):  # every (min, D) and, over j, every r, uniqueness, lr, sub-pixel and n_pairs value at this size
            r = R_[(si + j) % 3]
            H, W = sizes(r)[si]
            dmin, D = MD[j]
            cases.append((H, W, 1 if (si + j) % 2 else 3, Options(dmin, D, r, 10 * ((si + j) % 2), 1 if (si + j // 2) % 2 else -1, (j + si // 2) % 2)))
        for r in R_:  # ... and every r at this size, the remaining switches the other way round
            H, W = sizes(r)[si]
            cases.append((H, W, 3 if r != 4 else 1, Options(0, 24, r, 10 if r != 4 else 0, -1 if r == 1 else 1, 1 if r != 10 else 0)))
    return cases
