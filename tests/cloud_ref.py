"""Independent numpy restatement of scan registration as calibba.h states it (cba_point_normals, cba_cloud_index, cba_cloud_nearest,
cba_cloud_register): the normal of a pixel from its 5-point cross, the nearest neighbour by brute force over all valid target points
with the header's distance and tie rule, the rows and sums of a pose's system, the unpivoted 6 x 6 Cholesky, the pose update and the
iteration with its stop rules.  numpy's elementwise operations do not contract, and the operation order is the header's, so normals
and neighbours can be held to the bit; sums are formed in numpy's own order, and every sum comes with the sum of its terms'
magnitudes for the bound on what a different order can change.  Also the scene builders of both tiers and the wrappers of the host
build (tests/cloud_cpu).  Test infrastructure: no product code is imported here.
"""
import math

import numpy as np

from tests.host_build import ptr

OK, NOT_CONVERGED, TOO_FEW, DEGENERATE = 0, 1, 2, 3
SCAN_TILE = 1024  # cells per workgroup of the device's scan (scan_tiles.hpp: SCAN_TILE)


def valid(p):
    return np.isfinite(p).all(axis=-1)


# ---- normals ------------------------------------------------------------------------------------------------------------------------
def _axis_diff(P, A, in_a, B, in_b, mj2):
    """A: the neighbour after P (right / below), B: the one before; in_a, in_b: inside the map -> (difference, has one)"""
    def near(N, inside):
        e = N - P
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            return inside & valid(N) & (d2 <= mj2)
    a, b = near(A, in_a), near(B, in_b)
    hi = np.where(a[..., None], A, P)
    lo = np.where(b[..., None], B, P)
    with np.errstate(invalid="ignore"):
        return hi - lo, a | b


def normals(xyz, viewpoint=None, max_jump=np.inf):
    """xyz [..][H][W][3] -> normals of the same shape, NaN where there is none"""
    P = np.asarray(xyz, dtype=np.float64)
    vp = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, dtype=np.float64)
    mj2 = np.float64(max_jump) * np.float64(max_jump)
    H, W = P.shape[-3], P.shape[-2]

    def shifted(dy, dx):
        out = np.full_like(P, np.nan)
        inside = np.zeros(P.shape[:-1], bool)
        ys, yd = (slice(dy, None), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, None))
        xs, xd = (slice(dx, None), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, None))
        out[..., yd, xd, :] = P[..., ys, xs, :]
        inside[..., yd, xd] = True
        return out, inside

    (R, in_r), (L, in_l), (D, in_d), (U, in_u) = shifted(0, 1), shifted(0, -1), shifted(1, 0), shifted(-1, 0)
    dx, has_x = _axis_diff(P, R, in_r, L, in_l, mj2)
    dy, has_y = _axis_diff(P, D, in_d, U, in_u, mj2)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nx = dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1]
        ny = dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2]
        nz = dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = valid(P) & has_x & has_y & (length > 0.0) & np.isfinite(length)
        nx, ny, nz = nx / length, ny / length, nz / length
        v = vp - P
        s = (nx * v[..., 0] + ny * v[..., 1]) + nz * v[..., 2]
        flip = s < 0.0
    n = np.stack([np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)], axis=-1)
    n[~ok] = np.nan
    return n


# ---- nearest neighbour ---------------------------------------------------------------------------------------------------------------
def nearest(target, query, max_distance, want_gap=False):
    """Brute force over all valid target points: -> index int64 [m], dist2 [m] (and the smallest margin by which any decision of the
    search was taken: best against second best, best against the gate, or the gate against the closest point outside it)"""
    T = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    md2 = np.float64(max_distance) * np.float64(max_distance)
    index = np.full(Q.shape[0], -1, np.int64)
    dist2 = np.full(Q.shape[0], np.nan)
    gap = np.inf
    tv = valid(T)
    for first in range(0, Q.shape[0], 512):
        q = Q[first:first + 512]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = q[:, None, 0] - T[None, :, 0], q[:, None, 1] - T[None, :, 1], q[:, None, 2] - T[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            inside = (d2 <= md2) & tv[None, :] & valid(q)[:, None]
        gated = np.where(inside, d2, np.inf)
        best = gated.argmin(axis=1)  # the first of equal minima: the lowest index
        bd = gated[np.arange(q.shape[0]), best]
        hit = np.isfinite(bd)
        index[first:first + 512] = np.where(hit, best, -1)
        dist2[first:first + 512] = np.where(hit, bd, np.nan)
        if want_gap:
            qv = valid(q)
            allv = np.where(tv[None, :] & qv[:, None], d2, np.inf)
            if hit.any():
                rest = allv[hit].copy()
                rest[np.arange(rest.shape[0]), best[hit]] = np.inf
                gap = min(gap, float((rest.min(axis=1) - bd[hit]).min()), float((md2 - bd[hit]).min()))
            miss = ~hit & qv
            if miss.any():
                gap = min(gap, float((allv[miss].min(axis=1) - md2).min()))
    return (index, dist2, gap) if want_gap else (index, dist2)


# ---- ICP ------------------------------------------------------------------------------------------------------------------------------
def rotation(q):
    w, x, y, z = (np.float64(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.array([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                     [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                     [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]])


def transform(R, t, p):
    """each row summed left to right, then + t"""
    p = np.asarray(p, dtype=np.float64)
    return np.stack([((R[i, 0] * p[..., 0] + R[i, 1] * p[..., 1]) + R[i, 2] * p[..., 2]) + t[i] for i in range(3)], axis=-1)


def normalise(q):
    q = np.asarray(q, dtype=np.float64)
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def system(target, target_normals, source, pose7, metric, max_distance):
    """The system at pose7: dict with H [6][6], g [6], ss, n_pairs, and H_abs, g_abs, ss_abs (the sums of the terms' magnitudes), gap"""
    T = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    p = p[valid(p)]
    R, t = rotation(pose7[:4]), np.asarray(pose7[4:], dtype=np.float64)
    Q = transform(R, t, p) if p.shape[0] else np.zeros((0, 3))
    index, _, gap = nearest(T, Q, max_distance, want_gap=True)
    keep = index >= 0
    if metric == 0:
        N = np.asarray(target_normals, dtype=np.float64).reshape(-1, 3)
        keep &= ~np.isnan(N[np.maximum(index, 0), 0])
    Q, y = Q[keep], T[index[keep]]
    if metric == 0:
        n = N[index[keep]]
        e = Q - y
        r = ((n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2])[:, None]
        J = np.stack([Q[:, 1] * n[:, 2] - Q[:, 2] * n[:, 1], Q[:, 2] * n[:, 0] - Q[:, 0] * n[:, 2], Q[:, 0] * n[:, 1] - Q[:, 1] * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2]], axis=1)[:, None, :]
    else:
        z, o = np.zeros(Q.shape[0]), np.ones(Q.shape[0])
        r = Q - y
        J = np.stack([np.stack([z, Q[:, 2], -Q[:, 1], o, z, z], 1), np.stack([-Q[:, 2], z, Q[:, 0], z, o, z], 1),
                      np.stack([Q[:, 1], -Q[:, 0], z, z, z, o], 1)], axis=1)
    J, r = J.reshape(-1, 6), r.reshape(-1)
    Hterms = J[:, :, None] * J[:, None, :]
    gterms = J * r[:, None]
    return dict(H=Hterms.sum(0), g=gterms.sum(0), ss=float((r * r).sum()), n_pairs=int(keep.sum()), H_abs=np.abs(Hterms).sum(0),
                g_abs=np.abs(gterms).sum(0), ss_abs=float((r * r).sum()), gap=gap)


def cholesky6(H, g):
    """-> xi, or None when a squared diagonal entry of L is <= 1e-12 H_kk"""
    L = np.zeros((6, 6))
    for k in range(6):
        d = H[k, k]
        for j in range(k):
            d = d - L[k, j] * L[k, j]
        if not d > 1e-12 * H[k, k]:
            return None
        L[k, k] = math.sqrt(d)
        for i in range(k + 1, 6):
            s = H[i, k]
            for j in range(k):
                s = s - L[i, j] * L[k, j]
            L[i, k] = s / L[k, k]
    z, xi = np.zeros(6), np.zeros(6)
    for i in range(6):
        s = -g[i]
        for j in range(i):
            s = s - L[i, j] * z[j]
        z[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = z[i]
        for j in range(i + 1, 6):
            s = s - L[j, i] * xi[j]
        xi[i] = s / L[i, i]
    return xi


def update(pose7, xi):
    """-> the new pose7, |omega|, |v|"""
    th = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
    d = np.array([1.0, 0.0, 0.0, 0.0])
    if th != 0.0:
        s = math.sin(0.5 * th) / th
        d = np.array([math.cos(0.5 * th), s * xi[0], s * xi[1], s * xi[2]])
    q = pose7[:4]
    p = np.array([((d[0] * q[0] - d[1] * q[1]) - d[2] * q[2]) - d[3] * q[3],
                  ((d[0] * q[1] + d[1] * q[0]) + d[2] * q[3]) - d[3] * q[2],
                  ((d[0] * q[2] - d[1] * q[3]) + d[2] * q[0]) + d[3] * q[1],
                  ((d[0] * q[3] + d[1] * q[2]) - d[2] * q[1]) + d[3] * q[0]])
    p = normalise(p)
    t = transform(rotation(d), xi[3:], pose7[4:])
    return np.concatenate([p, t]), th, math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])


def extent(target):
    T = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    T = T[valid(T)]
    e = T.max(0) - T.min(0)
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def register(target, target_normals, source, max_distance, metric=0, max_iterations=30, step_tolerance=1e-9, min_pairs=6, init_pose7=None):
    """The iteration of the header.  -> dict: pose7, rms, H, g, n_pairs, iterations, status, gap (the smallest margin of any search
    decision over all evaluations) and the last system's magnitude sums"""
    pose = np.array([1.0, 0, 0, 0, 0, 0, 0]) if init_pose7 is None else np.asarray(init_pose7, dtype=np.float64).copy()
    pose[:4] = normalise(pose[:4])
    bar = max(min_pairs, 6 if metric == 0 else 3)
    ext = extent(target)
    iterations, gap, status = 0, np.inf, None
    while True:
        s = system(target, target_normals, source, pose, metric, max_distance)
        gap = min(gap, s["gap"])
        if status is not None:
            break
        if s["n_pairs"] < bar:
            status = TOO_FEW
            break
        if iterations >= max_iterations:
            status = NOT_CONVERGED
            break
        xi = cholesky6(s["H"], s["g"])
        if xi is None:
            status = DEGENERATE
            break
        pose, w, vn = update(pose, xi)
        iterations += 1
        if w <= step_tolerance and vn <= step_tolerance * ext:
            status = OK
        elif iterations >= max_iterations:
            status = NOT_CONVERGED
    rms = math.sqrt(s["ss"] / s["n_pairs"]) if s["n_pairs"] > 0 else float("nan")
    return dict(s, pose7=pose, rms=rms, iterations=iterations, status=status, gap=gap)


# ---- poses ----------------------------------------------------------------------------------------------------------------------------
def pose_from_rotvec(w, t):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    q = np.array([1.0, 0, 0, 0]) if th == 0 else np.concatenate([[math.cos(th / 2)], math.sin(th / 2) * w / th])
    return np.concatenate([q, np.asarray(t, dtype=np.float64)])


def pose_inverse(pose7):
    q = np.asarray(pose7[:4]) * np.array([1.0, -1, -1, -1])
    return np.concatenate([q, -(rotation(q) @ np.asarray(pose7[4:]))])


def pose_error(pose7, truth7):
    """-> (rotation error in rad, translation error)"""
    Ra, Rb = rotation(normalise(pose7[:4])), rotation(normalise(truth7[:4]))
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    S = Ra @ Rb.T
    ang = math.atan2(0.5 * math.sqrt((S[2, 1] - S[1, 2]) ** 2 + (S[0, 2] - S[2, 0]) ** 2 + (S[1, 0] - S[0, 1]) ** 2), c)
    return ang, float(np.linalg.norm(np.asarray(pose7[4:]) - np.asarray(truth7[4:])))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def surface_map(W, H, seed, focal=60.0, shift=(0.0, 0.0), step=False, holes=0, centre=None):
    """An organised map [H][W][3] of a smooth bumpy surface about 1 away, seen from the origin: pixel (u, v) looks along
    ((u - cx + shift_x) / focal, (v - cy + shift_y) / focal, 1); the depth along the ray is a function of the ray alone, so maps of
    different grids sample one surface.  step: the depth jumps by 0.15 right of the slope 0.12; holes: that many NaN pixels."""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 4)
    cx, cy = ((W - 1) / 2.0, (H - 1) / 2.0) if centre is None else centre
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b = (u - cx + shift[0]) / focal, (v - cy + shift[1]) / focal
    z = 1.0 + 0.05 * np.sin(7.0 * a + ph[0]) * np.cos(6.0 * b + ph[1]) + 0.04 * np.cos(9.0 * a * b + 5.0 * b + ph[2]) + 0.03 * np.sin(11.0 * a + ph[3])
    if step:
        z = z + 0.15 * (a > 0.12)
    xyz = np.stack([a * z, b * z, z], axis=-1)
    if holes:
        hr = np.random.default_rng(seed + 1000)
        xyz[hr.integers(0, H, holes), hr.integers(0, W, holes)] = np.nan
    return xyz


TRUTH = pose_from_rotvec([0.02, -0.03, 0.025], [0.012, -0.009, 0.007])


def scene_pair(seed, partial=False, step=False):
    """target map 48 x 36, its normals, a source 40 x 30 of the same surface on a shifted grid moved by the inverse of TRUTH (so that
    TRUTH maps the source onto the target).  partial: the source's grid starts 14 pixels further right, so a part of it sees surface
    the target does not hold."""
    tgt = surface_map(48, 36, seed, step=step, holes=5 if step else 0)
    src = surface_map(40, 30, seed, shift=(0.37 + (14.0 if partial else 0.0), -0.41), step=step, centre=(23.5 - 4.0, 17.5 - 3.0))
    inv = pose_inverse(TRUTH)
    src = transform(rotation(inv[:4]), inv[4:], src)
    return tgt, normals(tgt, max_jump=0.08 if step else np.inf), src


# ---- the host build (tests/cloud_cpu) ---------------------------------------------------------------------------------------------------
def host_normals(L, xyz, viewpoint=None, max_jump=np.inf):
    import ctypes as C

    p = np.ascontiguousarray(xyz, dtype=np.float64)
    maps = p if p.ndim == 4 else p[None]
    vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64)
    out = np.empty_like(p)
    L.cloud_host_normals(C.c_int(maps.shape[0]), C.c_int(maps.shape[1]), C.c_int(maps.shape[2]), ptr(p), ptr(vp), C.c_double(max_jump), ptr(out))
    return out


def host_nearest(L, target, cell_size, query, max_distance):
    """-> index, dist2 (RuntimeError when the host build refuses the grid)"""
    import ctypes as C

    T = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(-1, 3))
    Q = np.ascontiguousarray(np.asarray(query, dtype=np.float64).reshape(-1, 3))
    index, dist2 = np.empty(Q.shape[0], np.int64), np.empty(Q.shape[0])
    L.cloud_host_nearest.restype = C.c_int
    st = L.cloud_host_nearest(C.c_int64(T.shape[0]), ptr(T), C.c_double(cell_size), C.c_int64(Q.shape[0]), ptr(Q), C.c_double(max_distance),
                              ptr(index), ptr(dist2))
    if st != 0:
        raise RuntimeError(f"host build: grid plan {st}")
    return index, dist2


def host_register(L, target, target_normals, cell_size, sources, max_distance, metric=0, max_iterations=30, step_tolerance=1e-9, min_pairs=6,
                  init_pose7=None):
    """-> one dict per source: pose7, rms, H, g, n_pairs, iterations, status"""
    import ctypes as C

    T = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(-1, 3))
    N = None if target_normals is None else np.ascontiguousarray(np.asarray(target_normals, dtype=np.float64).reshape(-1, 3))
    pts = [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in sources]
    off = np.zeros(len(pts) + 1, np.int64)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    S = np.ascontiguousarray(np.concatenate(pts))
    init = None if init_pose7 is None else np.ascontiguousarray(np.asarray(init_pose7, dtype=np.float64).reshape(len(pts), 7))
    out = np.zeros((len(pts), 53))
    L.cloud_host_register.restype = C.c_int
    st = L.cloud_host_register(C.c_int64(T.shape[0]), ptr(T), ptr(N), C.c_double(cell_size), C.c_int(len(pts)), ptr(off), ptr(S), ptr(init),
                               C.c_int(metric), C.c_double(max_distance), C.c_int(max_iterations), C.c_double(step_tolerance),
                               C.c_int(min_pairs), ptr(out))
    if st != 0:
        raise RuntimeError(f"host build: grid plan {st}")
    return [dict(pose7=o[:7].copy(), rms=o[7], H=o[8:44].reshape(6, 6).copy(), g=o[44:50].copy(), n_pairs=int(o[50]), iterations=int(o[51]),
                 status=int(o[52])) for o in out]


# ---- the index and search cases of both tiers --------------------------------------------------------------------------------------------
QUERY_COUNTS = (1, 63, 64, 65, 256, 257)


def scattered(n, seed, lo=(0.0, 0.0, 0.0), span=(0.9, 0.7, 0.4)):
    return np.asarray(lo) + np.random.default_rng(seed).uniform(0, 1, (n, 3)) * np.asarray(span)


def queries_for(target, m, md, seed):
    """m queries: a third near target points (inside the radius), the rest anywhere in the box grown by two radii"""
    rng = np.random.default_rng(seed)
    T = target[valid(target)]
    lo, hi = T.min(0) - 2 * md, T.max(0) + 2 * md
    q = rng.uniform(lo, hi, (m, 3))
    near = rng.random(m) < 0.34
    q[near] = T[rng.integers(0, T.shape[0], int(near.sum()))] + rng.uniform(-0.5, 0.5, (int(near.sum()), 3)) * md
    return q


def grid_target(cells, cell, n, seed):
    """n >= 2 points whose grid has exactly `cells` = (nx, ny, nz) cells of size `cell`: two opposite corners and points between"""
    c = np.asarray(cells, dtype=np.float64)
    hi = (c - 1) * cell + 0.5 * cell
    pts = np.random.default_rng(seed).uniform(0, 1, (n, 3)) * hi
    pts[0], pts[-1] = 0.0, hi
    return pts


def nearest_cases():
    """dicts: name, target [n][3], cell, md, query [m][3], and for the planted ones want (the index each query must get)"""
    out = []
    for k, n in enumerate((1, 255, 256, 257)):
        t = scattered(n, 10 + k)
        for j, m in enumerate(QUERY_COUNTS):
            out.append(dict(name=f"n{n}_m{m}", target=t, cell=0.1, md=0.0999, query=queries_for(t, m, 0.0999, 100 + 10 * k + j)))
    # all points in one cell: a grid of one cell per axis (also n = 1 above)
    t = scattered(300, 20, span=(0.09, 0.05, 0.02))
    out.append(dict(name="one_cell", target=t, cell=0.1, md=0.05, query=queries_for(t, 257, 0.05, 120)))
    # cell counts at the scan's tile, one below, one above, and one past tile * tile (a third scan level)
    for cells in ((31, 11, 3), (16, 8, 8), (41, 5, 5), (128, 128, 65)):
        t = grid_target(cells, 0.125, 400, 30 + cells[0])
        t[7] = np.nan  # invalid target points keep their indices
        t[200, 1] = np.inf
        out.append(dict(name="cells_%d" % (cells[0] * cells[1] * cells[2]), target=t, cell=0.125, md=0.12, query=queries_for(t, 257, 0.12, 130 + cells[0]),
                        n_cells=cells[0] * cells[1] * cells[2]))
    # points exactly on cell faces: the lattice k / 8 with cell 1 / 8, in shuffled order; queries equidistant from 2 and from 8 points
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) / 8.0
    perm = np.random.default_rng(40).permutation(g.shape[0])
    lattice = g[perm]

    def index_of(p):
        return int(np.flatnonzero((lattice == np.asarray(p)).all(1))[0])

    q, want = [], []
    for base in ((1, 1, 1), (0, 0, 0), (3, 2, 1), (2, 1, 0)):
        b = np.asarray(base) / 8.0
        q.append(b + np.array([1 / 16.0, 0, 0]))  # two
        want.append(min(index_of(b), index_of(b + np.array([1 / 8.0, 0, 0]))))
        q.append(b + 1 / 16.0)                    # eight
        want.append(min(index_of(b + np.array(d) / 8.0) for d in np.ndindex(2, 2, 2)))
    q.append([np.nan, 0.1, 0.1]); want.append(-1)
    q.append([0.1, -np.inf, 0.1]); want.append(-1)
    out.append(dict(name="faces_ties", target=lattice, cell=0.125, md=0.1248, query=np.array(q), want=np.array(want)))
    # the gate: exactly at d2 == md2 (accepted), one ulp beyond (rejected); the box margin: exactly md outside the box (the corner point
    # is at d2 == md2: accepted) and one ulp further (rejected before the grid is touched)
    iso = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [1.5, 1.5, 1.5]])
    md = 7 / 64.0
    q = np.array([[0.5 + md, 0.5, 0.5], [np.nextafter(0.5 + md, 2), 0.5, 0.5], [0.5 - md, 0.5, 0.5], [np.nextafter(0.5 - md, -1), 0.5, 0.5],
                  [1.5, 1.5, 1.5 + md], [1.5, 1.5, np.nextafter(1.5 + md, 3)], [0.5, np.nextafter(0.5 - md, 1), 0.5]])
    out.append(dict(name="gate_margin", target=iso, cell=0.125, md=md, query=q, want=np.array([0, -1, 0, -1, 4, -1, 0])))
    return out
