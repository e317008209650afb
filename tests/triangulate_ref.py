"""Independent numpy restatement of cba_triangulate's per-point procedure as calibba.h states it (ray seed, Levenberg-Marquardt,
outlier-camera restarts, final statistics, covariance), on tests/camera_ref.py for the camera models.  Test infrastructure: the host
build of tri_math.hpp (tests/triangulate_cpu) and the device are checked against it.  The Jacobian is derived here on its own, as
K2 . D . G in matrix form, and checked against central differences of camera_ref.project by the CPU tier.  Also the test scene.
"""
import numpy as np

from tests import camera_ref as R
from tests.host_build import ptr

OK, NOT_CONVERGED, BEHIND, DEGENERATE, TOO_FEW = range(5)
LAMBDA0, LAMBDA_MIN, PIVOT_MIN, COST_SLACK_PX = 1e-4, 1e-10, 1e-12, 4e-12


class Options:
    def __init__(self, max_iterations=10, step_tolerance=1e-12, min_cams=2, max_reproj_px=np.inf):
        self.max_iterations, self.step_tolerance, self.min_cams, self.max_reproj_px = max_iterations, step_tolerance, min_cams, max_reproj_px


def quat_to_rotmat(q):  # Eigen's toRotationMatrix, no normalisation
    w, x, y, z = q[:4]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def to_camera(pose7, X):
    """P = R X + t, each row summed left to right, then + t (the order calibba.h states)"""
    Rm, t = quat_to_rotmat(pose7), pose7[4:]
    return np.array([Rm[i, 0] * X[0] + Rm[i, 1] * X[1] + Rm[i, 2] * X[2] + t[i] for i in range(3)])


def denominator(model, intr, P):
    return P[2] if model == R.PINHOLE else P @ R.rot_sensor(intr[10], intr[11])[:, 2]


def project_jacobian(model, intr, P):
    """d(u, v)/dP [2][3] = K2 . D . G: G = d(x, y)/dP of the model's central projection, D = the Brown-Conrady Jacobian,
    K2 = [[fx, skew], [0, fy]]"""
    fx, fy, skew = intr[0], intr[1], intr[4]
    k1, k2, k3, p1, p2 = intr[5:10]
    if model == R.PINHOLE:
        z = P[2]
        x, y = P[0] / z, P[1] / z
        G = np.array([[1.0, 0.0, -x], [0.0, 1.0, -y]]) / z
    else:
        Rs = R.rot_sensor(intr[10], intr[11])
        s = P @ Rs[:, 2]
        mx, my = (P @ Rs[:, 0]) / s, (P @ Rs[:, 1]) / s
        G = np.stack([Rs[:, 0] - mx * Rs[:, 2], Rs[:, 1] - my * Rs[:, 2]]) / s
        x, y = mx - Rs[2, 0] / Rs[2, 2], my - Rs[2, 1] / Rs[2, 2]
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
    off = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
    D = np.array([[rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x, off], [off, rad + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x]])
    return np.array([[fx, skew], [0.0, fy]]) @ D @ G


def _chol3(A):
    """unpivoted Cholesky; None when a pivot is not positive"""
    L = np.zeros((3, 3))
    for j in range(3):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def _chol_solve(L, b):
    y = np.zeros(3)
    for i in range(3):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(3)
    for i in (2, 1, 0):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def seed(model, intrs, invs, poses, uv, cams):
    A, b = np.zeros((3, 3)), np.zeros(3)
    for c in cams:
        Rm, t = quat_to_rotmat(poses[c]), poses[c][4:]
        x, y = R.unproject(model, intrs[c], uv[c][None], None if invs is None else invs[c])[0]
        d = Rm.T @ np.array([x, y, 1.0])
        d = d / np.sqrt(d @ d)
        o = -(Rm.T @ t)
        M = np.eye(3) - np.outer(d, d)
        A += M
        b += o - d * (d @ o)
    L = _chol3(A)
    if L is None or not (np.diag(L) ** 2 > PIVOT_MIN * len(cams)).all():
        return None
    return _chol_solve(L, b)


def linearize(model, intrs, poses, uv, cams, X):
    cost, H, g, front = 0.0, np.zeros((3, 3)), np.zeros(3), True
    for c in cams:
        P = to_camera(poses[c], X)
        with np.errstate(all="ignore"):
            r = R.project(model, intrs[c], P[None])[0] - uv[c]
            J = project_jacobian(model, intrs[c], P) @ quat_to_rotmat(poses[c])
        cost += r @ r
        H += J.T @ J
        g += J.T @ r
        front = front and denominator(model, intrs[c], P) > 0
    return cost, H, g, front


def refine(model, intrs, poses, uv, cams, X, o):
    cost, H, g, _ = linearize(model, intrs, poses, uv, cams, X)
    lam, lin = LAMBDA0, 1
    for _ in range(o.max_iterations):
        L = _chol3(H + lam * np.diag(np.diag(H)))
        if L is None:
            lam *= 10.0
            continue
        d = _chol_solve(L, -g)
        small = np.sqrt(d @ d) <= o.step_tolerance * np.sqrt(X @ X)
        ct, Ht, gt, front = linearize(model, intrs, poses, uv, cams, X + d)
        lin += 1
        slack = COST_SLACK_PX * np.sqrt(len(cams) * cost)  # the rounding floor of the cost
        floor_reached = False
        if front and cost - ct >= -slack:
            floor_reached = cost - ct <= slack
            X, cost, H, g = X + d, ct, Ht, gt
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam *= 10.0
        if small or floor_reached:
            return X, H, OK, lin
    return X, H, NOT_CONVERGED, lin


def triangulate_point(model, intrs, invs, poses, uv, o):
    """uv [n_cams][2] -> dict(xyz, rms, mask, status, cov [3][3], linearisations)"""
    n_cams = len(intrs)
    cams = [c for c in range(n_cams) if np.isfinite(uv[c]).all()]
    min_cams = max(o.min_cams, 2)
    out = dict(xyz=np.full(3, np.nan), rms=np.nan, mask=0, status=TOO_FEW, cov=np.full((3, 3), np.nan), linearisations=0)
    if len(cams) < min_cams:
        return out
    while True:
        out["mask"] = sum(1 << c for c in cams)
        X = seed(model, intrs, invs, poses, uv, cams)
        if X is None:
            out["status"] = DEGENERATE
            return out
        X, H, status, lin = refine(model, intrs, poses, uv, cams, X, o)
        out["linearisations"] += lin
        e2, front = [], True
        for c in cams:
            P = to_camera(poses[c], X)
            with np.errstate(all="ignore"):
                e = R.project(model, intrs[c], P[None])[0] - uv[c]
            e2.append(e[0] * e[0] + e[1] * e[1])
            front = front and denominator(model, intrs[c], P) > 0
        w = int(np.argmax(e2))  # the first among equals
        if e2[w] > o.max_reproj_px ** 2 and len(cams) > min_cams:
            cams = cams[:w] + cams[w + 1:]
            continue
        out["xyz"], out["rms"], out["status"] = X, np.sqrt(sum(e2) / len(cams)), (status if front else BEHIND)
        L = _chol3(H)
        if L is not None:
            out["cov"] = np.stack([_chol_solve(L, e) for e in np.eye(3)], axis=1)
        return out


def triangulate(model, intrs, invs, poses, uv, o=None):
    """uv [n_cams][n][2] -> dict of stacked per-point results"""
    o = o or Options()
    uv = np.asarray(uv, float)
    res = [triangulate_point(model, intrs, invs, poses, uv[:, i], o) for i in range(uv.shape[1])]
    return {k: np.array([r[k] for r in res]) for k in res[0]}


def cost_gradient(model, intrs, poses, uv, mask, X, h=1e-6):
    """(|J^T r|, |J|_F, |r|) of the reprojection cost at X over the cameras of mask, J by central differences of camera_ref.project"""
    rows, res = [], []
    for c in range(len(intrs)):
        if not (int(mask) >> c) & 1:
            continue
        f = lambda Y: R.project(model, intrs[c], to_camera(poses[c], Y)[None])[0]  # noqa: E731
        res.append(f(X) - uv[c])
        rows.append(np.stack([(f(X + h * e) - f(X - h * e)) / (2 * h) for e in np.eye(3)], axis=1))
    J, r = np.concatenate(rows), np.concatenate(res)
    return np.linalg.norm(J.T @ r), np.linalg.norm(J), np.linalg.norm(r)


# ---- the test scene -----------------------------------------------------------------------------------------------------------
def _axis_angle(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _rotmat_to_quat(m):  # trace > 0 only (the scene's rotations are small)
    t = np.sqrt(m[0, 0] + m[1, 1] + m[2, 2] + 1.0)
    return np.array([0.5 * t, (m[2, 1] - m[1, 2]) * 0.5 / t, (m[0, 2] - m[2, 0]) * 0.5 / t, (m[1, 0] - m[0, 1]) * 0.5 / t])


def scene(n_cams, n, model=R.PINHOLE, seed_=0, noise=0.0):
    """Camera c of C sits at x = -0.2 (c - (C-1)/2) m and is yawed 0.15 (c - (C-1)/2) rad about (0.1, 1, 0.05) (its orientation in the
    reference frame: the cameras toe in); for C = 16 both steps are halved.  Own intrinsics around fx 800, k = (-0.25, 0.08, -0.01,
    1e-3, -5e-4).  Points uniform in |x| <= 0.3, |y| <= 0.25, z in [1, 2] m.  Returns intrs [C][10 | 12], poses [C][7], xyz [n][3],
    uv [C][n][2] (noise px Gaussian)."""
    rng = np.random.default_rng(1000 * n_cams + 10 * seed_ + model)
    step = 0.5 if n_cams == 16 else 1.0
    intrs, poses = [], []
    for c in range(n_cams):
        k = c - (n_cams - 1) / 2
        f = 800.0 * (1 + 0.02 * rng.uniform(-1, 1, 2))
        intr = [f[0], f[1], 640.0 + rng.uniform(-5, 5), 480.0 + rng.uniform(-5, 5), 0.0, -0.25, 0.08, -0.01, 1e-3, -5e-4]
        if model == R.SCHEIMPFLUG:
            intr += [0.05 + 0.01 * rng.uniform(-1, 1), -0.04 + 0.01 * rng.uniform(-1, 1)]
        intrs.append(np.array(intr))
        Rc = _axis_angle([0.1, 1.0, 0.05], 0.15 * step * k).T  # reference -> camera
        centre = np.array([-0.2 * step * k, 0.0, 0.0])
        poses.append(np.concatenate([_rotmat_to_quat(Rc), -Rc @ centre]))
    intrs, poses = np.stack(intrs), np.stack(poses)
    xyz = np.column_stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.25, 0.25, n), rng.uniform(1.0, 2.0, n)])
    uv = np.stack([R.project(model, intrs[c], np.stack([to_camera(poses[c], X) for X in xyz])) for c in range(n_cams)])
    if noise:
        uv = uv + noise * rng.standard_normal(uv.shape)
    return intrs, poses, xyz, np.ascontiguousarray(uv)


def dual_inverses(intrs):
    return np.stack([R.dual_inverse(i[5:10]) for i in intrs])


def status_cases():
    """(name, intrs, poses, uv [2][1][2], expected status): two pinhole cameras 0.2 m apart with the same orientation.  The same
    pixel in both gives identical directions from different centres (parallel rays); the pixels of a point behind both cameras give
    rays that meet behind them."""
    intr = np.array([800.0, 800.0, 640.0, 480.0, 0.0, -0.25, 0.08, -0.01, 1e-3, -5e-4])
    intrs = np.stack([intr, intr])
    poses = np.array([[1.0, 0, 0, 0, 0, 0, 0], [1.0, 0, 0, 0, -0.2, 0, 0]])
    same = np.array([[[700.0, 500.0]], [[700.0, 500.0]]])
    Xb = np.array([0.05, 0.02, -1.5])
    behind = np.stack([R.project(R.PINHOLE, intrs[c], to_camera(poses[c], Xb)[None]) for c in range(2)])
    return [("parallel", intrs, poses, same, DEGENERATE), ("behind", intrs, poses, np.ascontiguousarray(behind), BEHIND)]


# ---- the host build of tri_math.hpp (tests/triangulate_cpu) --------------------------------------------------------------------
def host_triangulate(L, model, intrs, invs, poses, uv, o=None):
    """tri_point of the host build over uv [n_cams][n][2] -> the dict triangulate() returns"""
    import ctypes as C

    from calibration_amd.capi import CbaTriangulateOptions

    o = o or Options()
    co = CbaTriangulateOptions(int(o.max_iterations), float(o.step_tolerance), int(o.min_cams), float(o.max_reproj_px))
    intrs, poses, uv = (np.ascontiguousarray(a, float) for a in (intrs, poses, uv))
    invs = None if invs is None else np.ascontiguousarray(invs, float)
    n_cams, n = uv.shape[0], uv.shape[1]
    xyz, rms, cov6 = np.empty((n, 3)), np.empty(n), np.empty((n, 6))
    mask, status, lin = np.empty(n, np.uint32), np.empty(n, np.int32), np.empty(n, np.int32)
    L.tri_points(C.c_int(model), C.c_int(n_cams), ptr(intrs), C.c_int(0 if invs is None else invs.shape[1]), ptr(invs), ptr(poses), C.c_int64(n),
                 ptr(uv), C.byref(co), ptr(xyz), ptr(rms), ptr(mask), ptr(status), ptr(cov6), ptr(lin))
    return dict(xyz=xyz, rms=rms, mask=mask, status=status, cov=cov6[:, [[0, 1, 2], [1, 3, 4], [2, 4, 5]]], linearisations=lin)
