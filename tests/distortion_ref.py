"""TEST-ONLY numpy restatement of the reference's distortion fits and linear intrinsic estimators, written literally: explicit
design matrices, least squares, corrected observations.

  fit_distortion_full                 include/calib/models/distortion.h:229-363
  fit_distortion_dual                 distortion.h:373-406
  estimate_intrinsics_linear          src/estimation/linear/intrinsicsdlt.cpp:147-312
  estimate_intrinsics_linear_iterative                               :319-368

Observations are an (N, 4) array [x, y, u, v]; K = [fx, fy, cx, cy, skew].  Least squares: numpy's lstsq (an SVD solve, the
minimum-norm solution; ``RCOND`` only decides rank on exactly rank-deficient designs).  The K fit rejects a design whose
smallest singular value is below 1e-12, as the reference does.
"""
import numpy as np

RCOND = 1e-10
DEFAULT_BOUNDS = (np.array([0.0, 0.0, 0.0, 0.0, -0.01]), np.array([2000.0, 2000.0, 1280.0, 720.0, 0.01]))
OK, TOO_FEW, DEGENERATE = 0, 1, 2


def apply_distortion(xy, coeffs):
    """distortion.h:91-116 on an (N, 2) array."""
    coeffs = np.asarray(coeffs, float)
    nr = coeffs.size - 2
    x, y = xy[:, 0], xy[:, 1]
    r2 = x * x + y * y
    radial = np.ones_like(x)
    rpow = r2.copy()
    for i in range(nr):
        radial = radial + coeffs[i] * rpow
        rpow = rpow * r2
    p1, p2 = coeffs[nr], coeffs[nr + 1]
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd, yd], axis=1)


def design(obs, K, nr):
    fx, fy, cx, cy, s = K
    x, y, u, v = obs.T
    n = len(obs)
    r2 = x * x + y * y
    D = np.zeros((2 * n, nr + 2))
    rhs = np.zeros(2 * n)
    rpow = r2.copy()
    for j in range(nr):
        D[0::2, j] = fx * x * rpow + s * y * rpow
        D[1::2, j] = fy * y * rpow
        rpow = rpow * r2
    D[0::2, nr] = fx * (2 * x * y) + s * (r2 + 2 * y * y)
    D[0::2, nr + 1] = fx * (r2 + 2 * x * x) + s * (2 * x * y)
    D[1::2, nr] = fy * (r2 + 2 * y * y)
    D[1::2, nr + 1] = fy * (2 * x * y)
    rhs[0::2] = u - (fx * x + s * y + cx)
    rhs[1::2] = v - (fy * y + cy)
    return D, rhs


def fit_distortion_full(obs, K, nr=2, fixed_idx=(), fixed_val=()):
    """(alpha, residuals) or None.  Duplicate fixed indices: the first in input order wins."""
    obs = np.asarray(obs, float)
    if len(obs) < 8:
        return None
    m = nr + 2
    D, rhs = design(obs, np.asarray(K, float), nr)
    fixed = {}
    for i, idx in enumerate(fixed_idx):
        if int(idx) < 0 or int(idx) >= m:
            raise ValueError("Fixed distortion index out of range")
        fixed.setdefault(int(idx), float(fixed_val[i]) if i < len(fixed_val) else 0.0)
    alpha = np.zeros(m)
    for idx, val in fixed.items():
        alpha[idx] = val
    free = [i for i in range(m) if i not in fixed]
    if free:
        rhs_adj = rhs - D[:, sorted(fixed)] @ alpha[sorted(fixed)] if fixed else rhs
        sol = np.linalg.lstsq(D[:, free], rhs_adj, rcond=RCOND)[0]
        alpha[free] = sol
    return alpha, D @ alpha - rhs


def fit_distortion_dual(obs, K, nr=2, fixed_idx=(), fixed_val=()):
    """(forward, inverse, residuals) or None."""
    obs = np.asarray(obs, float)
    fwd = fit_distortion_full(obs, K, nr, fixed_idx, fixed_val)
    if fwd is None:
        return None
    fx, fy, cx, cy, s = K
    x, y, u, v = obs.T
    yd = (v - cy) / fy
    xd = (u - cx - s * yd) / fx
    inv_obs = np.stack([xd, yd, fx * x + s * y + cx, fy * y + cy], axis=1)
    inv = fit_distortion_full(inv_obs, K, nr, fixed_idx, fixed_val)
    return fwd[0], inv[0], fwd[1]


def _solve(A, b):
    sv = np.linalg.svd(A, compute_uv=False)
    if sv.min() < 1e-12:
        return None
    return np.linalg.lstsq(A, b, rcond=None)[0]


def estimate_intrinsics_linear(obs, bounds=None, use_skew=False):
    """(K, status, fell_back)."""
    obs = np.asarray(obs, float)
    if len(obs) < 2:
        return None, TOO_FEW, 0
    x, y, u, v = obs.T
    one = np.ones_like(x)
    Au = np.stack([x, y, one], 1) if use_skew else np.stack([x, one], 1)
    xu = _solve(Au, u)
    if xu is None:
        return None, DEGENERATE, 0
    xv = _solve(np.stack([y, one], 1), v)
    if xv is None:
        return None, DEGENERATE, 0
    lo, hi = bounds if bounds is not None else DEFAULT_BOUNDS
    fx, fy = xu[0], xv[0]
    cx = xu[2] if use_skew else xu[1]
    cy = xv[1]
    skew = xu[1] if use_skew else 0.0
    out = (fx < lo[0] or fx > hi[0] or fy < lo[1] or fy > hi[1] or cx < lo[2] or cx > hi[2] or cy < lo[3] or cy > hi[3]
           or (use_skew and (skew < lo[4] or skew > hi[4])))
    if out:
        clamp = lambda val, a, b: a if val < a else (b if b < val else val)  # noqa: E731
        K = np.array([clamp(max(500.0, fx), lo[0], hi[0]), clamp(max(500.0, fy), lo[1], hi[1]),
                      clamp(np.mean(u) / 2.0, lo[2], hi[2]), clamp(np.mean(v) / 2.0, lo[3], hi[3]),
                      clamp(skew, lo[4], hi[4]) if use_skew else 0.0])
        return K, OK, 1
    return np.array([fx, fy, cx, cy, skew]), OK, 0


def correct(obs, K, alpha):
    d = apply_distortion(obs[:, :2], alpha) - obs[:, :2]
    return np.stack([obs[:, 0], obs[:, 1], obs[:, 2] - K[0] * d[:, 0] - K[4] * d[:, 1], obs[:, 3] - K[1] * d[:, 1]], 1)


def estimate_intrinsics_linear_iterative(obs, nr, max_iterations=5, use_skew=False):
    """dict(K, alpha, status, iterations, fallbacks, changes): changes = the Σ|ΔK| of every adopted refit."""
    obs = np.asarray(obs, float)
    res = dict(K=None, alpha=None, status=OK, iterations=0, fallbacks=0, changes=[])
    K, st, fb = estimate_intrinsics_linear(obs, None, use_skew)
    if K is None:
        res["status"] = st
        return res
    res["fallbacks"] += fb
    for _ in range(max(max_iterations, 0)):
        d = fit_distortion_full(obs, K, nr)
        if d is None:
            break
        Kn, st, fb = estimate_intrinsics_linear(correct(obs, K, d[0]), None, use_skew)
        if Kn is None:
            break
        res["fallbacks"] += fb
        change = float(np.sum(np.abs(K - Kn)))
        K = Kn
        res["iterations"] += 1
        res["changes"].append(change)
        if change < 1e-6:
            break
    final = fit_distortion_full(obs, K, nr)
    if final is None:
        res["status"] = TOO_FEW
        return res
    res["K"], res["alpha"] = K, final[0]
    return res


def make_scene(n, K=(800.0, 820.0, 400.0, 300.0, 0.0), coeffs=(-0.2, 0.05, 0.001, -0.0005), lim=0.6, noise=0.0, seed=0):
    """n observations: x, y uniform in [-lim, lim], pixels K(distort(x, y)) plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-lim, lim, size=(n, 2))
    d = apply_distortion(xy, coeffs)
    fx, fy, cx, cy, s = K
    u = fx * d[:, 0] + s * d[:, 1] + cx
    v = fy * d[:, 1] + cy
    if noise:
        u = u + rng.normal(0.0, noise, n)
        v = v + rng.normal(0.0, noise, n)
    return np.ascontiguousarray(np.stack([xy[:, 0], xy[:, 1], u, v], 1))
