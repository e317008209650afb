"""Literal numpy restatement of the reference's camera models (include/calib/models/: camera_matrix.h:33-46, distortion.h:91-160,
208-218, pinhole.h:96-113, scheimpflug.h:139-181), of the documented Scheimpflug inverse and of the undistortion map and apply rules
stated in calibba.h.  Test infrastructure: the host build (tests/camera_cpu) and the device are checked against it.
"""
import numpy as np

PINHOLE, SCHEIMPFLUG = 0, 1


def apply_distortion(x, y, coeffs):  # distortion.h:91-116: [k1 .. k_nr, p1, p2]
    coeffs = np.asarray(coeffs, float)
    nr = coeffs.size - 2
    r2 = x * x + y * y
    radial = np.ones_like(x)
    rpow = r2
    for i in range(nr):
        radial = radial + coeffs[i] * rpow
        rpow = rpow * r2
    p1, p2 = coeffs[nr], coeffs[nr + 1]
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd, yd


def undistort(xd, yd, coeffs, inverse=None):  # distortion.h:119-134 (5 steps) / DualDistortion::undistort (:213-217)
    if inverse is not None:
        return apply_distortion(xd, yd, inverse)
    ux, uy = xd.copy(), yd.copy()
    for _ in range(5):
        dx, dy = apply_distortion(ux, uy, coeffs)
        ux = ux + (xd - dx)
        uy = uy + (yd - dy)
    return ux, uy


def normalize(K, u, v):  # camera_matrix.h:33-39
    y = (v - K[3]) / K[1]
    x = (u - K[2] - K[4] * y) / K[0]
    return x, y


def denormalize(K, x, y):  # camera_matrix.h:41-46
    return K[0] * x + K[4] * y + K[2], K[1] * y + K[3]


def rot_sensor(tau_x, tau_y):  # scheimpflug.h:150-152 (rows)
    ctx, stx, cty, sty = np.cos(tau_x), np.sin(tau_x), np.cos(tau_y), np.sin(tau_y)
    return np.array([[cty, stx * sty, ctx * sty], [0.0, ctx, -stx], [-sty, stx * cty, ctx * cty]])


def project(model, intr, xyz):
    """project(xyz) [n][3] -> [n][2] (pinhole.h:102-107, scheimpflug.h:139-181)."""
    intr = np.asarray(intr, float)
    P = np.asarray(xyz, float).reshape(-1, 3)
    K, dist = intr[:5], intr[5:10]
    if model == PINHOLE:
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        u, v = denormalize(K, *apply_distortion(x, y, dist))
        return np.stack([u, v], axis=1)
    Rs = rot_sensor(intr[10], intr[11])
    axis, base, normal = Rs[:, 0], Rs[:, 1], Rs[:, 2]
    sden = P @ normal
    mx, my = (P @ axis) / sden, (P @ base) / sden
    s0 = normal[2]
    mx0, my0 = axis[2] / s0, base[2] / s0
    u, v = denormalize(K, *apply_distortion(mx - mx0, my - my0, dist))
    su, sv = K[0] * mx0 + K[4] * my0, K[1] * my0  # apply_linear_intrinsics
    return np.stack([u + su, v + sv], axis=1)


def unproject(model, intr, uv, inverse=None):
    """Pixels [n][2] -> normalised (x, y) [n][2]: the pinhole's unproject, the Scheimpflug inverse of calibba.h."""
    intr = np.asarray(intr, float)
    uv = np.asarray(uv, float).reshape(-1, 2)
    K, dist = intr[:5], intr[5:10]
    xd, yd = normalize(K, uv[:, 0], uv[:, 1])
    if model == PINHOLE:
        return np.stack(undistort(xd, yd, dist, inverse), axis=1)
    Rs = rot_sensor(intr[10], intr[11])
    s0 = Rs[2, 2]
    mx0, my0 = Rs[2, 0] / s0, Rs[2, 1] / s0
    dx, dy = undistort(xd - mx0, yd - my0, dist, inverse)
    mx, my = dx + mx0, dy + my0
    P = mx[:, None] * Rs[:, 0] + my[:, None] * Rs[:, 1] + Rs[:, 2]
    return np.stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]], axis=1)


def undistort_map(model, intr, W, H, R=None, new_k5=None):
    """One camera's (map_x, map_y) [H][W] float32: project(R^T K'^-1 (u', v', 1)), NaN where the ray misses the image side."""
    intr = np.asarray(intr, float)
    R = np.eye(3) if R is None else np.asarray(R, float).reshape(3, 3)
    Kp = intr[:5] if new_k5 is None else np.asarray(new_k5, float)
    v, u = np.meshgrid(np.arange(H, dtype=float), np.arange(W, dtype=float), indexing="ij")
    x, y = normalize(Kp, u.ravel(), v.ravel())
    P = np.stack([x, y, np.ones_like(x)], axis=1) @ R  # R^T (x, y, 1) per row
    if model == PINHOLE:
        den = P[:, 2]
    else:
        den = P @ rot_sensor(intr[10], intr[11])[:, 2]
    with np.errstate(all="ignore"):
        uv = project(model, intr, P)
    uv[~(den > 0)] = np.nan
    return uv[:, 0].astype(np.float32).reshape(H, W), uv[:, 1].astype(np.float32).reshape(H, W)


def _taps(src, x, y, border):
    """src [sh][sw][ch] at integer taps x, y (any shape); outside -> border"""
    sh, sw = src.shape[:2]
    inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
    xc, yc = np.clip(x, 0, sw - 1), np.clip(y, 0, sh - 1)
    v = src[yc, xc]
    return np.where(inside[..., None], v, np.asarray(border, src.dtype))


def apply(src, map_x, map_y, border=0.0):
    """One image src [sh][sw] or [sh][sw][ch] (uint8 | float32) through one map [H][W] by calibba.h's rules."""
    mono = src.ndim == 2
    s = src[..., None] if mono else src
    mx, my = np.asarray(map_x, np.float32), np.asarray(map_y, np.float32)
    ok = (np.abs(mx) <= np.float32(2 ** 24)) & (np.abs(my) <= np.float32(2 ** 24))
    mxs, mys = np.where(ok, mx, np.float32(0)), np.where(ok, my, np.float32(0))
    if s.dtype == np.uint8:
        b = 0 if np.isnan(border) else int(np.clip(np.rint(border), 0, 255))
        X = np.rint(mxs * np.float32(32)).astype(np.int64)
        Y = np.rint(mys * np.float32(32)).astype(np.int64)
        x0, y0, a, bb = X >> 5, Y >> 5, (X & 31)[..., None], (Y & 31)[..., None]
        p = [_taps(s, x0 + dx, y0 + dy, b).astype(np.int64) for dy in (0, 1) for dx in (0, 1)]
        w = [(32 - a) * (32 - bb) * 32, a * (32 - bb) * 32, (32 - a) * bb * 32, a * bb * 32]
        r = (w[0] * p[0] + w[1] * p[1] + w[2] * p[2] + w[3] * p[3] + (1 << 14)) >> 15
        out = np.clip(r, 0, 255).astype(np.uint8)
        out[~ok] = b
    else:
        b = np.float32(border)
        fx0, fy0 = np.floor(mxs), np.floor(mys)
        fx, fy = (mxs - fx0)[..., None], (mys - fy0)[..., None]
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        p00, p01, p10, p11 = (_taps(s, x0 + dx, y0 + dy, b) for dy in (0, 1) for dx in (0, 1))
        t = p00 + fx * (p01 - p00)
        bt = p10 + fx * (p11 - p10)
        out = (t + fy * (bt - t)).astype(np.float32)
        out[~ok] = b
    return out[..., 0] if mono else out


def ulp_diff(a, b):
    """|a - b| in float32 ulps (NaN where exactly one is NaN; 0 where both are)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib).astype(float)
    na, nb = np.isnan(a), np.isnan(b)
    d[na & nb] = 0.0
    d[na ^ nb] = np.nan
    return d


def cameras():
    """Test cameras: (name, model, intr): both models, skew on and off, tilts 0 and +-0.2 rad."""
    base = [800.0, 780.0, 640.0, 480.0]
    dist = [-0.21, 0.08, -0.012, 0.0011, -0.0007]
    out = []
    for skew in (0.0, 0.4):
        out.append((f"pinhole_skew{skew}", PINHOLE, np.array(base + [skew] + dist)))
        for tau in ((0.0, 0.0), (0.2, -0.2), (-0.2, 0.2), (0.2, 0.0)):
            out.append((f"scheimpflug_skew{skew}_tau{tau}", SCHEIMPFLUG, np.array(base + [skew] + dist + list(tau))))
    return out


def points(n, seed=0):
    """camera-frame points in front of the camera, inside a ~70 degree cone"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 3.0, n)
    xy = rng.uniform(-0.6, 0.6, (n, 2)) * z[:, None]
    return np.ascontiguousarray(np.column_stack([xy, z]))


def dual_inverse(dist):
    """An inverse fitted by least squares on a grid (the shape of invert_brown_conrady's fit: radial terms as the forward)."""
    g = np.linspace(-0.6, 0.6, 21)
    X, Y = np.meshgrid(g, g)
    x, y = X.ravel(), Y.ravel()
    xd, yd = apply_distortion(x, y, dist)
    r2 = xd * xd + yd * yd
    A = np.zeros((2 * x.size, 5))
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = xd * r2, xd * r2 ** 2, xd * r2 ** 3
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = yd * r2, yd * r2 ** 2, yd * r2 ** 3
    A[0::2, 3], A[0::2, 4] = 2 * xd * yd, r2 + 2 * xd * xd
    A[1::2, 3], A[1::2, 4] = r2 + 2 * yd * yd, 2 * xd * yd
    rhs = np.empty(2 * x.size)
    rhs[0::2], rhs[1::2] = x - xd, y - yd
    return np.linalg.lstsq(A, rhs, rcond=None)[0]
