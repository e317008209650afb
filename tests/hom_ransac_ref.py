"""numpy restatement of the linear seed of planar intrinsic calibration, written from the reference's equations with SVDs where
the reference takes them: HomographyEstimator (homographyestimator.cpp), ransac<> (common/ransac.h) with the library's
counter-based sampler, Zhang (zhang.cpp), pose_from_homography (posefromhomography.cpp) and symmetric_rms_px
(intrinsicsdlt.cpp:21-30).  The oracle of tests/test_hom_ransac_cpu.py and tests/test_hom_ransac_gpu.py."""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample(seed, k, n):
    """Hypothesis k's four distinct indices in [0, n) (hom_ransac_math.hpp hr_sample)."""
    base = ((seed ^ 0x5851F42D4C957F2D) + 4 * k) & M64
    taken, out = [], []
    for j in range(4):
        r = (splitmix64((base + j) & M64) * (n - j)) >> 64
        for t in sorted(taken):
            if r >= t:
                r += 1
        out.append(r)
        taken.append(r)
    return out


def normalize_points(p):
    c = p.mean(axis=0)
    md = np.linalg.norm(p - c, axis=1).mean()
    s = np.sqrt(2.0) / md if md > 0 else 1.0
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    return (p - c) * s, T


def dlt(src, dst):
    """normalize_and_estimate_homography (homographyestimator.cpp:61-70): SVD null vector of the normalised 2N x 9 design."""
    sn, Ts = normalize_points(src)
    dn, Td = normalize_points(dst)
    n = src.shape[0]
    A = np.zeros((2 * n, 9))
    x, y, u, v = sn[:, 0], sn[:, 1], dn[:, 0], dn[:, 1]
    A[0::2] = np.stack([-x, -y, -np.ones(n), 0 * x, 0 * x, 0 * x, u * x, u * y, u], axis=1)
    A[1::2] = np.stack([0 * x, 0 * x, 0 * x, -x, -y, -np.ones(n), v * x, v * y, v], axis=1)
    h = np.linalg.svd(A)[2][-1]
    Hn = h.reshape(3, 3) / h[8]
    return np.linalg.inv(Td) @ Hn @ Ts


def fit(view, idx):
    """HomographyEstimator::fit: None where H(0,0) is not finite (homographyestimator.cpp:139)."""
    with np.errstate(all="ignore"):
        H = dlt(view[idx, :2], view[idx, 2:])
    return H if np.isfinite(H[0, 0]) else None


def degenerate(view, idx):
    """has_near_collinear_triplet (homographyestimator.cpp:100-119) on the object points."""
    P = view[idx, :2]
    for i in range(4):
        for j in range(i + 1, 4):
            for k in range(j + 1, 4):
                a, b, c = P[i], P[j], P[k]
                if abs((b - a)[0] * (c - a)[1] - (b - a)[1] * (c - a)[0]) < 1e-6:
                    return True
    return False


def residuals(H, view):
    """symmetric_transfer_error (homographyestimator.cpp:80-94) of every correspondence."""
    with np.errstate(all="ignore"):
        xy1 = np.c_[view[:, :2], np.ones(len(view))]
        uv1 = np.c_[view[:, 2:], np.ones(len(view))]
        q = xy1 @ H.T
        s = uv1 @ np.linalg.inv(H).T
        e1 = np.linalg.norm(view[:, 2:] - q[:, :2] / q[:, 2:], axis=1)
        e2 = np.linalg.norm(view[:, :2] - s[:, :2] / s[:, 2:], axis=1)
        return np.sqrt(0.5 * (e1 * e1 + e2 * e2))


def ransac(view, max_iters=1000, thresh=2.0, min_inliers=12, seed=1234567, refit=True):
    """ransac<HomographyEstimator> with every hypothesis scored and the counter-based sampler.
    -> (success, H, inliers, rms, winning k)."""
    n = len(view)
    best = None
    if n < 4:
        return False, np.eye(3), np.zeros(0, dtype=np.int64), np.inf, -1
    for k in range(max_iters):
        idx = sample(seed, k, n)
        if degenerate(view, idx):
            continue
        H = fit(view, idx)
        if H is None:
            continue
        r = residuals(H, view)
        inl = np.flatnonzero(r <= thresh)
        if len(inl) < min_inliers:
            continue
        Hf, fin, rf = H, inl, r[inl]
        if refit and len(inl) >= 4:
            H2 = fit(view, inl)
            if H2 is not None:
                r2 = residuals(H2, view)
                Hf, fin = H2, np.flatnonzero(r2 <= thresh)
                rf = r2[fin]
        rms = np.sqrt(np.mean(rf * rf)) if len(fin) else np.inf
        if best is None or len(fin) > len(best[2]) or (len(fin) == len(best[2]) and rms < best[3]):
            best = (True, Hf, fin, rms, k)
    return best if best is not None else (False, np.eye(3), np.zeros(0, dtype=np.int64), np.inf, -1)


def symmetric_rms_px(H, view, inliers):
    """intrinsicsdlt.cpp:21-30: sqrt(sum r / 2n) -- the sum of r, not r^2."""
    if len(inliers) == 0:
        return np.inf
    return np.sqrt(residuals(H, view)[inliers].sum() / (2.0 * len(inliers)))


def normalize_hmtx(H):
    H = np.array(H, dtype=np.float64)
    if not np.all(np.isfinite(H)):
        return H
    if H[2, 2] < 0:
        H = -H
    if abs(H[2, 2]) > 1e-12:
        return H / H[2, 2]
    nf = np.linalg.norm(H)
    return H / nf if nf > 1e-12 else H


def _vij(H, i, j):
    return np.array([H[0, i] * H[0, j], H[0, i] * H[1, j] + H[1, i] * H[0, j], H[1, i] * H[1, j],
                     H[0, i] * H[2, j] + H[2, i] * H[0, j], H[1, i] * H[2, j] + H[2, i] * H[1, j], H[2, i] * H[2, j]])


def _try_factor(B):
    if not np.all(np.isfinite(B)):
        return None
    try:
        L = np.linalg.cholesky(B)
    except np.linalg.LinAlgError:
        return None
    K = np.linalg.inv(L.T)
    if not np.all(np.isfinite(K)) or abs(K[2, 2]) < 1e-15:
        return None
    K = K / K[2, 2]
    if K[0, 0] <= 0 or K[1, 1] <= 0:
        K = -K
    return K


def zhang(hs):
    """zhang_intrinsics_from_hs: [fx, fy, cx, cy, skew] or None."""
    if len(hs) < 4:
        return None
    rows = []
    for H in hs:
        Hn = normalize_hmtx(H)
        for r in (_vij(Hn, 0, 1), _vij(Hn, 0, 0) - _vij(Hn, 1, 1)):
            s = np.linalg.norm(r)
            rows.append(r / s if s > 0 else r)
    b = np.linalg.svd(np.array(rows))[2][-1]
    for bb in (b, -b):
        B = np.array([[bb[0], bb[1], bb[3]], [bb[1], bb[2], bb[4]], [bb[3], bb[4], bb[5]]])
        for BB in (B, -B):
            K = _try_factor(BB)
            if K is not None:
                return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]])
    return None


def project_to_so3(M):
    U, _, Vt = np.linalg.svd(M)
    S = np.eye(3)
    if np.linalg.det(U @ Vt) < 0:
        S[2, 2] = -1
    return U @ S @ Vt


def pose_from_homography(k5, H):
    """-> (success, R, t, scale, cond_check)."""
    fx, fy, cx, cy, sk = k5
    if not (np.isfinite(fx) and np.isfinite(fy)) or cx <= 0 or cy <= 0 or not np.isfinite(H[2, 2]):
        return False, None, None, 0.0, 0.0
    K = np.array([[fx, sk, cx], [0, fy, cy], [0, 0, 1.0]])
    Hn = np.linalg.inv(K) @ H
    n1, n2 = np.linalg.norm(Hn[:, 0]), np.linalg.norm(Hn[:, 1])
    if not (n1 > 1e-15 and n2 > 1e-15):
        return False, None, None, 0.0, 0.0
    s = 1.0 / ((n1 + n2) * 0.5)
    R = np.zeros((3, 3))
    R[:, 0], R[:, 1] = s * Hn[:, 0], s * Hn[:, 1]
    R[:, 2] = np.cross(R[:, 0], R[:, 1])
    R = project_to_so3(R)
    t = s * Hn[:, 2]
    if t[2] <= 0:
        R, t = -R, -t
    return True, R, t, s, max(n1, n2) / min(n1, n2)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-15:
        return np.eye(3)
    a = w / th
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * A @ A


def random_pose(rng, dist=1.0):
    R = rodrigues(rng.uniform(-0.35, 0.35, 3))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), dist * rng.uniform(0.8, 1.2)])
    return R, t


def project_view(K5, R, t, XY, noise_px=0.0, rng=None):
    fx, fy, cx, cy, sk = K5
    P = XY[:, 0:1] * R[:, 0] + XY[:, 1:2] * R[:, 1] + t
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    u, v = fx * x + sk * y + cx, fy * y + cy
    if noise_px > 0:
        u = u + rng.normal(0, noise_px, u.shape)
        v = v + rng.normal(0, noise_px, v.shape)
    return np.c_[XY, u, v]


def grid(nx, ny, step):
    X, Y = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step)
    return np.c_[X.ravel(), Y.ravel()] - np.array([(nx - 1) * step / 2, (ny - 1) * step / 2])


def random_view(rng, K5, n, outlier_frac=0.0, noise_px=0.0, half=0.15, dist=1.0):
    """n random target points in [-half, half]^2 seen from a random pose; a fraction replaced by pixels >= 40 px away from their
    true projection.  -> (view [n][4], planted inlier mask)."""
    R, t = random_pose(rng, dist)
    XY = rng.uniform(-half, half, (n, 2))
    view = project_view(K5, R, t, XY, noise_px, rng)
    inl = np.ones(n, dtype=bool)
    m = int(round(outlier_frac * n))
    if m:
        idx = rng.choice(n, m, replace=False)
        ang = rng.uniform(0, 2 * np.pi, m)
        rad = rng.uniform(40.0, 120.0, m)
        view[idx, 2] += rad * np.cos(ang)
        view[idx, 3] += rad * np.sin(ang)
        inl[idx] = False
    return view, inl
