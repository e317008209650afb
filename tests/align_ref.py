"""Independent numpy restatement of the alignment of many scans as calibba.h states it (cba_cloud_set, cba_cloud_align), over the
restatement of scan registration (tests/cloud_ref.py: the brute-force neighbour, the rotation, the transform, the update): an edge's
relative pose and system, the adjoint, the blocks M = A^T H A and c = A^T g, their assembly in edge order, the unpivoted width-n
Cholesky, the iteration with its stop rules.  Every sum whose order the header fixes is a Python loop in that order; an edge's sums are
formed in numpy's own order and come with the sums of their terms' magnitudes, as cloud_ref.system's do.  Also the scenes of both tiers
and the wrapper of the host build (tests/align_cpu).  Test infrastructure: no product code is imported here.
"""
import math

import numpy as np

from tests import cloud_ref as R
from tests.host_build import ptr

OK, NOT_CONVERGED, TOO_FEW, DEGENERATE = R.OK, R.NOT_CONVERGED, R.TOO_FEW, R.DEGENERATE
IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])


# ---- an edge ----------------------------------------------------------------------------------------------------------------------------
def relative(pose_a, pose_b):
    """T_b^-1 T_a -> (R_ab [3][3], t_ab [3]) by the header's forms"""
    Ra, Rb = R.rotation(pose_a[:4]), R.rotation(pose_b[:4])
    Rab = np.array([[(Rb[0, i] * Ra[0, k] + Rb[1, i] * Ra[1, k]) + Rb[2, i] * Ra[2, k] for k in range(3)] for i in range(3)])
    d = np.asarray(pose_a[4:], dtype=np.float64) - np.asarray(pose_b[4:], dtype=np.float64)
    tab = np.array([(Rb[0, i] * d[0] + Rb[1, i] * d[1]) + Rb[2, i] * d[2] for i in range(3)])
    return Rab, tab


def pairs(target, target_normals, source, Rm, t, metric, max_distance):
    """The pairs of a source at (Rm, t): -> (p [k][3] the paired source points, y [k][3], n [k][3] or None, gap)"""
    T = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    p = p[R.valid(p)]
    Q = R.transform(Rm, t, p) if p.shape[0] else np.zeros((0, 3))
    index, _, gap = R.nearest(T, Q, max_distance, want_gap=True)
    keep = index >= 0
    N = None
    if metric == 0:
        N = np.asarray(target_normals, dtype=np.float64).reshape(-1, 3)
        keep &= ~np.isnan(N[np.maximum(index, 0), 0])
    return p[keep], T[index[keep]], None if N is None else N[index[keep]], gap


def rows(Q, y, n, metric):
    """J [rows][6] and r [rows] of pairs at the transformed points Q"""
    if metric == 0:
        e = Q - y
        r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
        J = np.stack([Q[:, 1] * n[:, 2] - Q[:, 2] * n[:, 1], Q[:, 2] * n[:, 0] - Q[:, 0] * n[:, 2], Q[:, 0] * n[:, 1] - Q[:, 1] * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2]], axis=1)
        return J, r
    z, o = np.zeros(Q.shape[0]), np.ones(Q.shape[0])
    r = Q - y
    J = np.stack([np.stack([z, Q[:, 2], -Q[:, 1], o, z, z], 1), np.stack([-Q[:, 2], z, Q[:, 0], z, o, z], 1),
                  np.stack([Q[:, 1], -Q[:, 0], z, z, z, o], 1)], axis=1)
    return J.reshape(-1, 6), r.reshape(-1)


def edge_system(scans, normals, a, b, poses, metric, max_distance):
    """The system of edge (a, b) at the poses: dict as cloud_ref.system's"""
    Rab, tab = relative(poses[a], poses[b])
    p, y, n, gap = pairs(scans[b], None if normals is None else normals[b], scans[a], Rab, tab, metric, max_distance)
    J, r = rows(R.transform(Rab, tab, p) if p.shape[0] else np.zeros((0, 3)), y, n, metric)
    Hterms = J[:, :, None] * J[:, None, :]
    gterms = J * r[:, None]
    return dict(H=Hterms.sum(0), g=gterms.sum(0), ss=float((r * r).sum()), n_pairs=int(p.shape[0]), H_abs=np.abs(Hterms).sum(0),
                g_abs=np.abs(gterms).sum(0), ss_abs=float((r * r).sum()), gap=gap)


# ---- the system of all scans ---------------------------------------------------------------------------------------------------------------
def adjoint(pose_b):
    """Ad(T_b^-1) on (omega, v) [6][6], each product rounded"""
    Rb, t = R.rotation(pose_b[:4]), np.asarray(pose_b[4:], dtype=np.float64)
    A = np.zeros((6, 6))
    for i in range(3):
        for k in range(3):
            A[i, k] = A[3 + i, 3 + k] = Rb[k, i]
        A[3 + i, 0] = Rb[2, i] * t[1] - Rb[1, i] * t[2]
        A[3 + i, 1] = Rb[0, i] * t[2] - Rb[2, i] * t[0]
        A[3 + i, 2] = Rb[1, i] * t[0] - Rb[0, i] * t[1]
    return A


def blocks(H, g, A):
    """M = A^T (H A) and c = A^T g, every sum left to right over 0..5 from its first product"""
    def chain(terms):
        s = terms[0]
        for v in terms[1:]:
            s = s + v
        return s
    B = np.array([[chain([H[k, l] * A[l, j] for l in range(6)]) for j in range(6)] for k in range(6)])
    M = np.array([[chain([A[k, i] * B[k, j] for k in range(6)]) for j in range(6)] for i in range(6)])
    c = np.array([chain([A[k, i] * g[k] for k in range(6)]) for i in range(6)])
    return M, c


def assemble(n_scans, fixed, edges, used, MC):
    """The reduced system: (H [n][n], g [n]); every entry receives its contributions in edge order"""
    row = [-1 if k == fixed else k if k < fixed else k - 1 for k in range(n_scans)]
    n = 6 * (n_scans - 1)
    H, g = np.zeros((n, n)), np.zeros(n)
    for (a, b), u, (M, c) in zip(edges, used, MC):
        if not u:
            continue
        ra, rb = row[a], row[b]
        if ra >= 0:
            H[6 * ra:6 * ra + 6, 6 * ra:6 * ra + 6] += M
            g[6 * ra:6 * ra + 6] += c
        if rb >= 0:
            H[6 * rb:6 * rb + 6, 6 * rb:6 * rb + 6] += M
            g[6 * rb:6 * rb + 6] -= c
        if ra >= 0 and rb >= 0:
            H[6 * ra:6 * ra + 6, 6 * rb:6 * rb + 6] -= M
            H[6 * rb:6 * rb + 6, 6 * ra:6 * ra + 6] -= M.T
    return H, g


def cholesky(H, g):
    """H xi = -g at the width of H by cloud_ref.cholesky6's sequence -> xi, or None when a squared diagonal entry of L is <= 1e-12 H_kk"""
    n = H.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        d = H[k, k]
        for j in range(k):
            d = d - L[k, j] * L[k, j]
        if not d > 1e-12 * H[k, k]:
            return None
        L[k, k] = math.sqrt(d)
        for i in range(k + 1, n):
            s = H[i, k]
            for j in range(k):
                s = s - L[i, j] * L[k, j]
            L[i, k] = s / L[k, k]
    z, xi = np.zeros(n), np.zeros(n)
    for i in range(n):
        s = -g[i]
        for j in range(i):
            s = s - L[i, j] * z[j]
        z[i] = s / L[i, i]
    for i in range(n - 1, -1, -1):
        s = z[i]
        for j in range(i + 1, n):
            s = s - L[j, i] * xi[j]
        xi[i] = s / L[i, i]
    return xi


def normalised(poses):
    """poses [n][7] with their quaternions normalised once, as the entry does"""
    out = np.asarray(poses, dtype=np.float64).reshape(-1, 7).copy()
    for k in range(out.shape[0]):
        out[k, :4] = R.normalise(out[k, :4])
    return out


def set_extent(scans):
    return max(R.extent(s) for s in scans)


def align(scans, normals, edges, max_distance, metric=0, max_iterations=30, step_tolerance=1e-9, min_pairs=6, init_pose7=None, fixed=0):
    """The iteration of the header.  -> dict: poses [n][7], rms, n_pairs, n_used_edges, iterations, status, edges (one dict per edge:
    the system at the returned poses, and used), gap (the smallest margin of any search decision over all evaluations)"""
    n_scans = len(scans)
    poses = normalised(np.tile(IDENTITY, (n_scans, 1)) if init_pose7 is None else init_pose7)
    bar = max(min_pairs, 6 if metric == 0 else 3)
    ext = set_extent(scans)
    row = [-1 if k == fixed else k if k < fixed else k - 1 for k in range(n_scans)]
    iterations, gap, status = 0, np.inf, None
    while True:
        systems = [edge_system(scans, normals, a, b, poses, metric, max_distance) for a, b in edges]
        for s in systems:
            s["used"] = s["n_pairs"] >= bar
            gap = min(gap, s["gap"])
        used = [s["used"] for s in systems]
        ss = n_pairs = 0
        for s in systems:
            if s["used"]:
                ss = ss + s["ss"]
                n_pairs += s["n_pairs"]
        if status is not None:
            break
        if not any(used):
            status = TOO_FEW
            break
        if iterations >= max_iterations:
            status = NOT_CONVERGED
            break
        MC = [blocks(s["H"], s["g"], adjoint(poses[b])) for s, (a, b) in zip(systems, edges)]
        H, g = assemble(n_scans, fixed, edges, used, MC)
        xi = cholesky(H, g)
        if xi is None:
            status = DEGENERATE
            break
        small = True
        for k in range(n_scans):
            if k == fixed:
                continue
            poses[k], w, vn = R.update(poses[k], xi[6 * row[k]:6 * row[k] + 6])
            small = small and w <= step_tolerance and vn <= step_tolerance * ext
        iterations += 1
        if small:
            status = OK
        elif iterations >= max_iterations:
            status = NOT_CONVERGED
    rms = math.sqrt(ss / n_pairs) if n_pairs > 0 else float("nan")
    return dict(poses=poses, rms=rms, ss=ss, n_pairs=n_pairs, n_used_edges=int(sum(used)), iterations=iterations, status=status, edges=systems,
                gap=gap)


# ---- poses ----------------------------------------------------------------------------------------------------------------------------------
def quat_mul(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]])


def compose(a, b):
    """the pose a after b: x -> a(b(x))"""
    return np.concatenate([R.normalise(quat_mul(a[:4], b[:4])), R.rotation(a[:4]) @ np.asarray(b[4:]) + np.asarray(a[4:])])


def compose_all(a, poses):
    return np.array([compose(a, p) for p in poses])


def apply(pose7, xyz):
    return R.transform(R.rotation(pose7[:4]), np.asarray(pose7[4:], dtype=np.float64), xyz)


def closure_error(poses, truth, first=0, last=-1):
    """the pose of scan `last` relative to scan `first` against the truth's -> (rad, length)"""
    rel = compose(R.pose_inverse(poses[first]), poses[last])
    want = compose(R.pose_inverse(truth[first]), truth[last])
    return R.pose_error(rel, want)


def mean_pose_error(poses, truth):
    e = np.array([R.pose_error(p, t) for p, t in zip(poses, truth)])
    return float(e[:, 0].mean()), float(e[:, 1].mean())


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
MD, CELL = 0.05, 0.0501


def ring_scene(seed, n_scans=6, W=40, H=30, radius=(16.0, 12.0)):
    """n_scans maps W x H of cloud_ref.surface_map's surface, their windows shifted round a circle of `radius` pixels and by a further
    (0.37 k, -0.41 k) pixels for scan k, each moved by the inverse of a random pose of about 0.02 rad and 0.01 (so truth[k] maps scan k
    back onto the surface).  -> scans [n][H][W][3], normals (of each scan in its own frame), truth [n][7]"""
    rng = np.random.default_rng(1000 + seed)
    scans, normals, truth = [], [], []
    for k in range(n_scans):
        ang = 2.0 * np.pi * k / n_scans
        m = R.surface_map(W, H, seed, shift=(radius[0] * math.cos(ang) + 0.37 * k, radius[1] * math.sin(ang) - 0.41 * k))
        T = R.pose_from_rotvec(rng.normal(0, 0.02 / math.sqrt(3), 3), rng.normal(0, 0.01 / math.sqrt(3), 3))
        s = apply(R.pose_inverse(T), m)
        scans.append(s)
        normals.append(R.normals(s))
        truth.append(T)
    return scans, normals, np.array(truth)


def ring_edges(n_scans):
    """both directions of every neighbouring pair round the ring: 2 n_scans directed edges"""
    out = []
    for k in range(n_scans):
        out += [(k, (k + 1) % n_scans), ((k + 1) % n_scans, k)]
    return out


def chain_poses(scans, normals, first_pose, max_distance=MD, metric=0, register=None):
    """Poses by chaining pairwise ICP, scan k onto scan k - 1 from the identity, scan 0 at first_pose.  register: the pairwise solver
    (default: cloud_ref.register) -> poses [n][7], the smallest gap"""
    register = register or (lambda tgt, nrm, src: R.register(tgt, nrm, src, max_distance, metric=metric, max_iterations=60, step_tolerance=1e-12))
    poses, gap = [np.asarray(first_pose, dtype=np.float64)], np.inf
    for k in range(1, len(scans)):
        r = register(scans[k - 1], normals[k - 1], scans[k])
        gap = min(gap, r.get("gap", np.inf))
        poses.append(compose(poses[-1], r["pose7"]))
    return np.array(poses), gap


# ---- the host build (tests/align_cpu) -----------------------------------------------------------------------------------------------------------
def pack(scans, normals=None):
    """-> offset int64 [n + 1], xyz [m][3], normals [m][3] or None"""
    pts = [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in scans]
    off = np.zeros(len(pts) + 1, np.int64)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    nrm = None if normals is None else np.ascontiguousarray(np.concatenate([np.asarray(n, dtype=np.float64).reshape(-1, 3) for n in normals]))
    return off, np.ascontiguousarray(np.concatenate(pts)), nrm


def host_align(L, scans, normals, cell_size, edges, max_distance, metric=0, max_iterations=30, step_tolerance=1e-9, min_pairs=6, init_pose7=None,
               fixed=0, brute=False):
    """-> dict: poses, rms, n_pairs, n_used_edges, iterations, status, edges (dicts H, g, ss, n_pairs, used)"""
    import ctypes as C

    off, xyz, nrm = pack(scans, normals)
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
    init = None if init_pose7 is None else np.ascontiguousarray(np.asarray(init_pose7, dtype=np.float64).reshape(len(scans), 7))
    poses, out, res = np.zeros((len(scans), 7)), np.zeros((e.shape[0], 45)), np.zeros(5)
    L.align_host.restype = C.c_int
    st = L.align_host(C.c_int(len(scans)), ptr(off), ptr(xyz), ptr(nrm), C.c_double(cell_size), C.c_int(e.shape[0]), ptr(e), ptr(init),
                      C.c_int(metric), C.c_double(max_distance), C.c_int(max_iterations), C.c_double(step_tolerance), C.c_int(min_pairs),
                      C.c_int(fixed), C.c_int(1 if brute else 0), ptr(poses), ptr(out), ptr(res))
    if st != 0:
        raise RuntimeError(f"host build: grid plan {st - 10}")
    return dict(poses=poses, rms=res[0], n_pairs=int(res[1]), n_used_edges=int(res[2]), iterations=int(res[3]), status=int(res[4]),
                edges=[dict(H=o[:36].reshape(6, 6).copy(), g=o[36:42].copy(), ss=o[42], n_pairs=int(o[43]), used=bool(o[44])) for o in out])


def host_blocks(L, H, g, pose7_b):
    """-> (A [6][6], M [6][6], c [6]) of the header's align_adjoint and align_edge_blocks"""
    H, g, p = np.ascontiguousarray(H, dtype=np.float64), np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(pose7_b, dtype=np.float64)
    A, out = np.zeros(36), np.zeros(42)
    L.align_host_blocks(ptr(H), ptr(g), ptr(p), ptr(A), ptr(out))
    return A.reshape(6, 6), out[:36].reshape(6, 6), out[36:]
