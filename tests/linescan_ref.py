"""numpy restatement of the reference's laser-plane calibration (TEST INFRASTRUCTURE: the checker of cba_calibrate_laser_plane,
cba_fit_plane and cba_invert_brown_conrady), and the synthetic line-scan scenes of the reference's tests:
  unproject                  camera_matrix.h:33-39 normalize, distortion.h:119-134 undistort (5 fixed-point steps),
                             DualBrownConrady::undistort (distortion.h:213-217); Scheimpflug: the inverse of scheimpflug.h:139-181
  points_from_view           linescan.h:63-91 (DLT + pose: tests/planar_seed.py)
  fit_plane_svd, plane_rms   planefit.cpp:68-85 (np.linalg.svd, as the reference's JacobiSVD), linescan.h:93-99
  invert_brown_conrady       distortion.h:165-195 + fit_distortion_full (np.linalg.lstsq)
  scenes                     linescan_test.cpp / linescan_facade_test.cpp: target plane x laser plane, the line clipped to
                             [-0.5, 0.5]^2 on the target, sampled at 400 (or 200) samples per unit, projected.
Planes follow the library's sign convention (d > 0, else the largest normal component positive).
"""
import numpy as np

from tests.planar_seed import homography_dlt, pose_from_homography_normalized


# ---- camera ---------------------------------------------------------------------------------------------------------------
def apply_distortion(x, y, coeffs):
    c = np.asarray(coeffs, dtype=float)
    nr = c.size - 2
    r2 = x * x + y * y
    radial = np.ones_like(x)
    rpow = r2.copy()
    for i in range(nr):
        radial = radial + c[i] * rpow
        rpow = rpow * r2
    p1, p2 = c[nr], c[nr + 1]
    return x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def undistort(xd, yd, intr, inverse=None):
    if inverse is not None:
        return apply_distortion(xd, yd, inverse)
    x, y = xd.copy(), yd.copy()
    for _ in range(5):
        dx, dy = apply_distortion(x, y, intr[5:10])
        x, y = x + xd - dx, y + yd - dy
    return x, y


def normalize(intr, u, v):
    y = (v - intr[3]) / intr[1]
    return (u - intr[2] - intr[4] * y) / intr[0], y


def scheimpflug_basis(intr):
    tx, ty = intr[10], intr[11]
    ctx, stx, cty, sty = np.cos(tx), np.sin(tx), np.cos(ty), np.sin(ty)
    Rs = np.array([[cty, stx * sty, ctx * sty], [0.0, ctx, -stx], [-sty, stx * cty, ctx * cty]])
    m0 = np.array([Rs[2, 0] / Rs[2, 2], Rs[2, 1] / Rs[2, 2]])
    return Rs, m0


def unproject(intr, u, v, inverse=None):
    intr = np.asarray(intr, dtype=float)
    u, v = np.asarray(u, dtype=float), np.asarray(v, dtype=float)
    mx, my = normalize(intr, u, v)
    if intr.size == 10:
        return undistort(mx, my, intr, inverse)
    Rs, m0 = scheimpflug_basis(intr)
    x, y = undistort(mx - m0[0], my - m0[1], intr, inverse)
    P = Rs @ np.stack([x + m0[0], y + m0[1], np.ones_like(x)])
    return P[0] / P[2], P[1] / P[2]


def project(intr, P):
    """Pinhole + Brown-Conrady / Scheimpflug projection of camera-frame points P [n][3] (reproj_math.hpp)."""
    intr = np.asarray(intr, dtype=float)
    P = np.asarray(P, dtype=float).reshape(-1, 3)
    su = sv = 0.0
    if intr.size == 10:
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    else:
        Rs, m0 = scheimpflug_basis(intr)
        q = P @ Rs  # Rs^T P per row
        x, y = q[:, 0] / q[:, 2] - m0[0], q[:, 1] / q[:, 2] - m0[1]
        su, sv = intr[0] * m0[0] + intr[4] * m0[1], intr[1] * m0[1]
    xd, yd = apply_distortion(x, y, intr[5:10])
    return np.stack([intr[0] * xd + intr[4] * yd + intr[2] + su, intr[1] * yd + intr[3] + sv], axis=1)


# ---- the reference's algorithm --------------------------------------------------------------------------------------------
def points_from_view(target_view, laser_uv, intr, inverse=None):
    tv = np.asarray(target_view, dtype=float).reshape(-1, 4)
    lu = np.asarray(laser_uv, dtype=float).reshape(-1, 2)
    xn, yn = unproject(intr, tv[:, 2], tv[:, 3], inverse)
    H = homography_dlt(tv[:, :2], np.stack([xn, yn], axis=1))
    if not np.all(np.isfinite(H)):
        return None
    T = pose_from_homography_normalized(H)
    Hi = np.linalg.inv(H)
    if abs(Hi[2, 2]) > 1e-15:
        Hi = Hi / Hi[2, 2]
    lx, ly = unproject(intr, lu[:, 0], lu[:, 1], inverse)
    hp = Hi @ np.stack([lx, ly, np.ones_like(lx)])
    obj = np.stack([hp[0] / hp[2], hp[1] / hp[2], np.zeros(lx.size)], axis=1)
    return obj @ T[:3, :3].T + T[:3, 3]


def plane_sign(plane, scale):
    p = np.array(plane, dtype=float)
    if abs(p[3]) > 1e-12 * scale:
        return -p if p[3] < 0 else p
    k = int(np.argmax(np.abs(p[:3])))
    return -p if p[k] < 0 else p


def fit_plane_svd(pts):
    pts = np.asarray(pts, dtype=float).reshape(-1, 3)
    c = pts.mean(axis=0)
    _, _, vt = np.linalg.svd(pts - c, full_matrices=False)
    n = vt[2]
    d = -n @ c
    nrm = np.linalg.norm(n)
    return plane_sign(np.r_[n / nrm, d / nrm], np.abs(pts).max())


def plane_rms(pts, plane):
    r = np.asarray(pts).reshape(-1, 3) @ plane[:3] + plane[3]
    return float(np.sqrt(np.mean(r * r)))


def invert_brown_conrady(forward):
    f = np.asarray(forward, dtype=float)
    nr = f.size - 2
    g = -1.0 + 2.0 * np.arange(21) / 20.0
    xu, yu = np.meshgrid(g, g, indexing="ij")
    xu, yu = xu.ravel(), yu.ravel()
    x, y = apply_distortion(xu, yu, f)
    r2 = x * x + y * y
    A = np.zeros((2 * x.size, f.size))
    rpow = r2.copy()
    for k in range(nr):
        A[0::2, k] = x * rpow
        A[1::2, k] = y * rpow
        rpow = rpow * r2
    A[0::2, nr], A[0::2, nr + 1] = 2 * x * y, r2 + 2 * x * x
    A[1::2, nr], A[1::2, nr + 1] = r2 + 2 * y * y, 2 * x * y
    b = np.empty(2 * x.size)
    b[0::2], b[1::2] = xu - x, yu - y
    return np.linalg.lstsq(A, b, rcond=None)[0]


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def laser_line_on_target(c_T_t, n, d, samples_per_unit=400.0, n_samples=None):
    """Target-frame points (z = 0) where the laser plane n.p + d = 0 (camera frame) crosses the [-0.5, 0.5]^2 target."""
    R, t = c_T_t[:3, :3], c_T_t[:3, 3]
    na, da = R[:, 2], -R[:, 2] @ t  # target plane in the camera frame
    nb = np.asarray(n, dtype=float)
    dirc = np.cross(na, nb)
    if dirc @ dirc < 1e-12:
        return np.zeros((0, 3))
    p = np.linalg.solve(np.stack([na, nb, dirc]), np.array([-da, -d, 0.0]))
    dirc = dirc / np.linalg.norm(dirc)
    pt, dt = R.T @ (p - t), R.T @ dirc
    smin, smax = -np.inf, np.inf
    for k in range(2):
        if abs(dt[k]) < 1e-12:
            if not (-0.5 - 1e-14 <= pt[k] <= 0.5 + 1e-14):
                return np.zeros((0, 3))
            continue
        s0, s1 = sorted(((-0.5 - pt[k]) / dt[k], (0.5 - pt[k]) / dt[k]))
        smin, smax = max(smin, s0), min(smax, s1)
    if not smin < smax:
        return np.zeros((0, 3))
    a, b = (pt + smin * dt)[:2], (pt + smax * dt)[:2]
    m = n_samples or max(2, int(np.ceil(np.linalg.norm(b - a) * samples_per_unit)))
    s = smin + np.linspace(0.0, 1.0, m) * (smax - smin)
    pts = pt[None, :] + s[:, None] * dt[None, :]
    pts[:, 2] = 0.0
    return pts


def make_view(c_T_t, n, d, intr, object_xy=None, samples_per_unit=400.0, noise_px=0.0, rng=None, n_samples=None):
    """(target_view [k][4], laser_uv [m][2]) of one view, as the reference's create_view builds them."""
    if object_xy is None:
        object_xy = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
    obj = np.c_[object_xy, np.zeros(len(object_xy))]
    uv = project(intr, obj @ c_T_t[:3, :3].T + c_T_t[:3, 3])
    lt = laser_line_on_target(c_T_t, n, d, samples_per_unit, n_samples)
    luv = project(intr, lt @ c_T_t[:3, :3].T + c_T_t[:3, 3]) if len(lt) else np.zeros((0, 2))
    if noise_px > 0.0:
        uv = uv + rng.normal(scale=noise_px, size=uv.shape)
        luv = luv + rng.normal(scale=noise_px, size=luv.shape)
    return np.c_[object_xy, uv], luv


def grid_xy(k=6):
    g = np.linspace(-0.5, 0.5, k)
    X, Y = np.meshgrid(g, g)
    return np.c_[X.ravel(), Y.ravel()]


def random_scene(rng, n_views, intr, n_true, d_true, noise_px=0.0, samples_per_unit=400.0, grid=6, n_samples=None):
    """Views of a [-0.5, 0.5]^2 target about 1 m in front of the camera at random tilts, all crossed by one laser plane."""
    views = []
    while len(views) < n_views:
        R = rot_x(rng.uniform(-0.35, 0.35))
        ay = rng.uniform(-0.3, 0.3)
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        T = pose(Ry @ R, np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.9, 1.3)]))
        tv, lv = make_view(T, n_true, d_true, intr, grid_xy(grid), samples_per_unit, noise_px, rng, n_samples)
        if len(lv) >= 2:
            views.append((tv, lv))
    return views


def calibrate_laser_plane(views, intr, inverse=None):
    """linear_svd calibrate_laser_plane: (plane, rms, all points)."""
    pts = [points_from_view(tv, lv, intr, inverse) for tv, lv in views]
    allp = np.concatenate([p for p in pts if p is not None], axis=0)
    plane = fit_plane_svd(allp)
    return plane, plane_rms(allp, plane), pts
