"""Independent numpy restatement of scan fusion as calibba.h states it (cba_tsdf_integrate, cba_tsdf_extract): the update of every
voxel by one depth map, vectorised per map, and the zero crossings on lattice edges with their points and normals in visiting order.
numpy's elementwise operations do not contract and the operation order is the header's, so D, W, the points and the normals can be
held to the bit.  The projection is written out in cba_camera_project's own expression order (Horner radial polynomial, the
Scheimpflug constants from libm's sine and cosine): tests/camera_ref.py states the same models in the reference's order, which
differs in the last bits, so it serves as the cross-check of this one (test_fusion_cpu) and as the renderer's unprojection.  Also the
scene builder of both tiers (analytic depth maps of a sphere and of a bumpy surface with a depth step and holes) and the wrappers of
the host build (tests/fusion_cpu).  Test infrastructure: no product code is imported here.
"""
import math

import numpy as np

from tests import camera_ref as CR
from tests.host_build import ptr

PINHOLE, SCHEIMPFLUG = CR.PINHOLE, CR.SCHEIMPFLUG
INTEGRATE_BLOCK = 256  # lanes per workgroup of k_tsdf_integrate (tsdf_fusion.hip: TSDF_BLOCK); a lane owns two adjacent x voxels
EXTRACT_TILE = 1024    # voxels per workgroup of the extraction (tsdf_math.hpp: TSDF_EXTRACT_TILE)
SCAN_TILE = 1024       # tile counts per workgroup of the scan (scan_tiles.hpp: SCAN_TILE)


# ---- the camera, in cba_camera_project's order -------------------------------------------------------------------------------------
def rotation(q):
    """R of a pose7's quaternion as cba_triangulate builds it: no normalisation"""
    w, x, y, z = (np.float64(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def sensor_consts(intr):
    """(Rs [9] row-major, m0 [2]) of a Scheimpflug camera"""
    ctx, stx, cty, sty = math.cos(intr[10]), math.sin(intr[10]), math.cos(intr[11]), math.sin(intr[11])
    Rs = [cty, stx * sty, ctx * sty, 0.0, ctx, -stx, -sty, stx * cty, ctx * cty]
    return Rs, (Rs[6] / Rs[8], Rs[7] / Rs[8])


def denominator(model, intr, P0, P1, P2):
    if model == PINHOLE:
        return P2
    Rs, _ = sensor_consts(intr)
    return Rs[2] * P0 + Rs[5] * P1 + Rs[8] * P2


def project(model, intr, P0, P1, P2):
    """(u, v) of camera-frame points (arrays of one shape), unmasked"""
    k = [float(v) for v in intr]
    su = sv = 0.0
    if model == PINHOLE:
        iz = 1.0 / P2
        x, y = P0 * iz, P1 * iz
    else:
        Rs, m0 = sensor_consts(k)
        i_s = 1.0 / (Rs[2] * P0 + Rs[5] * P1 + Rs[8] * P2)
        x = (Rs[0] * P0 + Rs[3] * P1 + Rs[6] * P2) * i_s - m0[0]
        y = (Rs[1] * P0 + Rs[4] * P1 + Rs[7] * P2) * i_s - m0[1]
        su = k[0] * m0[0] + k[4] * m0[1]
        sv = k[1] * m0[1]
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]))
    xy = x * y
    xd = x * rad + 2.0 * k[8] * xy + k[9] * (r2 + 2.0 * x * x)
    yd = y * rad + k[8] * (r2 + 2.0 * y * y) + 2.0 * k[9] * xy
    return k[0] * xd + k[4] * yd + k[2] + su, k[1] * yd + k[3] + sv


# ---- the volume ------------------------------------------------------------------------------------------------------------------------
class Volume:
    """D, W float32 [nz][ny][nx]; lattice point (i, j, k) at origin + (i, j, k) voxel_size (the product rounded, then the sum)"""

    def __init__(self, shape, origin, voxel_size, truncation, max_weight=64.0, max_depth=np.inf):
        self.shape = tuple(int(v) for v in shape)
        nx, ny, nz = self.shape
        self.origin, self.vs = np.asarray(origin, dtype=np.float64), np.float64(voxel_size)
        self.trunc, self.max_weight, self.max_depth = np.float64(truncation), np.float64(max_weight), np.float64(max_depth)
        self.axes = [self.origin[c] + np.arange(n, dtype=np.float64) * self.vs for c, n in enumerate((nx, ny, nz))]
        self.reset()

    def reset(self):
        nx, ny, nz = self.shape
        self.D, self.W = np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)

    def integrate(self, model, intr, depth, poses):
        depth = np.asarray(depth, dtype=np.float64)
        depth = depth[None] if depth.ndim == 2 else depth
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
        H, Wd = depth.shape[1:]
        X0, X1, X2 = self.axes[0][None, None, :], self.axes[1][None, :, None], self.axes[2][:, None, None]
        for m in range(depth.shape[0]):
            R, t = rotation(poses[m, :4]), poses[m, 4:]
            with np.errstate(all="ignore"):
                P = [((R[r, 0] * X0 + R[r, 1] * X1) + R[r, 2] * X2) + t[r] for r in range(3)]
                ok = (P[2] > 0.0) & (denominator(model, intr, *P) > 0.0)
                u, v = project(model, intr, *P)
                px, py = np.floor(u + 0.5), np.floor(v + 0.5)
                ok &= (px >= 0.0) & (px <= Wd - 1.0) & (py >= 0.0) & (py <= H - 1.0)
                d = depth[m][np.where(ok, py, 0.0).astype(np.int64), np.where(ok, px, 0.0).astype(np.int64)]
                ok &= np.isfinite(d) & (d > 0.0) & (d <= self.max_depth)
                s = d - P[2]
                ok &= ~(s < -self.trunc)
                f = s / self.trunc
                f = np.where(f > 1.0, 1.0, f)
                w = self.W.astype(np.float64)
                Dn = ((w * self.D.astype(np.float64) + f) / (w + 1.0)).astype(np.float32)
                Wn = np.minimum(w + 1.0, self.max_weight).astype(np.float32)
            self.D, self.W = np.where(ok, Dn, self.D), np.where(ok, Wn, self.W)
        return self

    def _gradient(self, i, j, k):
        """central differences at voxels (index arrays) -> g [n][3], ok [n]"""
        n = self.shape
        at = [i, j, k]
        g, ok = np.zeros((i.size, 3)), np.ones(i.size, bool)
        for c in range(3):
            inside = (at[c] >= 1) & (at[c] + 1 < n[c])
            hi = [a.copy() for a in at]
            lo = [a.copy() for a in at]
            hi[c], lo[c] = np.minimum(at[c] + 1, n[c] - 1), np.maximum(at[c] - 1, 0)
            ok &= inside & (self.W[hi[2], hi[1], hi[0]] > 0) & (self.W[lo[2], lo[1], lo[0]] > 0)
            g[:, c] = self.D[hi[2], hi[1], hi[0]].astype(np.float64) - self.D[lo[2], lo[1], lo[0]].astype(np.float64)
        return g, ok

    def extract(self, min_weight=1.0):
        """-> xyz [n][3], normals [n][3] (NaN where there is none), in visiting order"""
        nx, ny, nz = self.shape
        D, W = self.D.astype(np.float64), self.W.astype(np.float64)
        heavy, neg = W >= min_weight, D < 0.0
        q = np.zeros((nz, ny, nx, 3), bool)
        q[:, :, :-1, 0] = heavy[:, :, :-1] & heavy[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
        q[:, :-1, :, 1] = heavy[:, :-1, :] & heavy[:, 1:, :] & (neg[:, :-1, :] != neg[:, 1:, :])
        q[:-1, :, :, 2] = heavy[:-1, :, :] & heavy[1:, :, :] & (neg[:-1, :, :] != neg[1:, :, :])
        k, j, i, axis = np.nonzero(q)  # row-major: ascending l, then +x, +y, +z
        bi, bj, bk = i + (axis == 0), j + (axis == 1), k + (axis == 2)
        Da, Db = D[k, j, i], D[bk, bj, bi]
        t = Da / (Da - Db)
        xyz = np.stack([self.axes[0][i], self.axes[1][j], self.axes[2][k]], axis=1)
        along = t * self.vs
        xyz[np.arange(i.size), axis] = xyz[np.arange(i.size), axis] + along
        ga, oka = self._gradient(i, j, k)
        gb, okb = self._gradient(bi, bj, bk)
        with np.errstate(all="ignore"):
            n = ga + t[:, None] * (gb - ga)
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            ok = oka & okb & (length > 0.0) & np.isfinite(length)
            n = n / length[:, None]
        n[~ok] = np.nan
        return xyz, n


def depth_from_xyz(xyz):
    p = np.asarray(xyz, dtype=np.float64)
    return np.where(np.isfinite(p).all(axis=-1), p[..., 2], np.nan)


# ---- poses -----------------------------------------------------------------------------------------------------------------------------
def quaternion_of(R):
    """unit quaternion [w x y z] of a rotation matrix (w > 0 branch or the largest diagonal)"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        c = int(np.argmax(np.diag(R)))
        a, b = (c + 1) % 3, (c + 2) % 3
        s = math.sqrt(1.0 + R[c, c] - R[a, a] - R[b, b]) * 2
        q = [0.0] * 4
        q[0], q[1 + c], q[1 + a], q[1 + b] = (R[b, a] - R[a, b]) / s, 0.25 * s, (R[a, c] + R[c, a]) / s, (R[b, c] + R[c, b]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """pose7 volume frame -> camera of a camera at eye whose optical axis passes through target"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, dtype=np.float64))
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    q = quaternion_of(R)
    return np.concatenate([q, -(rotation(q) @ eye)])


def pose_inverse(pose7):
    q = np.asarray(pose7[:4]) * np.array([1.0, -1, -1, -1])
    return np.concatenate([q, -(rotation(q) @ np.asarray(pose7[4:]))])


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
DIST = [-0.1, 0.02, -0.003, 0.001, -0.0007]
CAMERAS = {PINHOLE: np.array([150.0, 148.0, 39.5, 29.5, 0.0] + DIST),
           SCHEIMPFLUG: np.array([150.0, 148.0, 39.5, 29.5, 0.0] + DIST + [0.03, -0.02])}
MAP_W, MAP_H = 80, 60
SHAPE, ORIGIN, VOXEL = (32, 28, 24), np.array([-1.0, -0.875, -0.75]), 0.0625
TRUNCATION = 4 * VOXEL
SPHERE_C, SPHERE_R = np.array([0.03, -0.02, 0.01]), 0.5
STEP_X = 0.2


def pixel_rays(model, intr, W=MAP_W, H=MAP_H):
    """(x, y) [H][W] with project(x, y, 1) = the pixel centre, to 1e-10 px: the unprojection refined by fixed-point steps"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    xy = CR.unproject(model, intr, np.stack([u.ravel(), v.ravel()], 1))
    x, y = xy[:, 0].reshape(H, W), xy[:, 1].reshape(H, W)
    for _ in range(40):
        pu, pv = project(model, intr, x, y, np.ones_like(x))
        x, y = x + (u - pu) / intr[0], y + (v - pv) / intr[1]
    pu, pv = project(model, intr, x, y, np.ones_like(x))
    assert max(np.abs(pu - u).max(), np.abs(pv - v).max()) < 1e-10
    return x, y


def _world_rays(model, intr, pose7):
    x, y = pixel_rays(model, intr)
    R, t = rotation(pose7[:4]), np.asarray(pose7[4:])
    Ri = np.linalg.inv(R)  # the quaternion is a unit one to rounding: R is a rotation to rounding, and this is its exact inverse
    eye = -(Ri @ t)
    d = np.stack([x, y, np.ones_like(x)], -1) @ Ri.T
    return eye, d


def render_sphere(model, intr, pose7):
    """depth [H][W]: z of the first intersection of each pixel's ray with the sphere, closed form; NaN where it misses"""
    eye, d = _world_rays(model, intr, pose7)
    oc = eye - SPHERE_C
    a, b, c = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        lam = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (lam > 0), lam, np.nan)  # the camera-frame point is lam (x, y, 1): z = lam


def bumpy_height(x, y):
    return 0.08 * np.sin(5.0 * x + 0.3) * np.cos(4.0 * y - 0.2) + 0.05 * np.cos(7.0 * x * y + 3.0 * y) + 0.15 * (x > STEP_X)


def bumpy_slope(x, y):
    hx = 0.4 * np.cos(5.0 * x + 0.3) * np.cos(4.0 * y - 0.2) - 0.35 * y * np.sin(7.0 * x * y + 3.0 * y)
    hy = -0.32 * np.sin(5.0 * x + 0.3) * np.sin(4.0 * y - 0.2) - 0.05 * (7.0 * x + 3.0) * np.sin(7.0 * x * y + 3.0 * y)
    return hx, hy


def render_bumpy(model, intr, pose7, holes=0, seed=0):
    """depth [H][W] of the surface z = bumpy_height(x, y), |x| <= 0.9, |y| <= 0.8, seen from above: the first sign change of
    F(lam) = z - h along the ray on a grid of 600 steps, then bisection to 1e-12; NaN where the ray misses; holes: that many NaN pixels"""
    eye, d = _world_rays(model, intr, pose7)

    def F(lam):
        p = eye + lam[..., None] * d
        inside = (np.abs(p[..., 0]) <= 0.9) & (np.abs(p[..., 1]) <= 0.8)
        return p[..., 2] - bumpy_height(p[..., 0], p[..., 1]), inside

    grid = np.linspace(1.0, 5.0, 601)
    lo, hi = np.full(d.shape[:2], np.nan), np.full(d.shape[:2], np.nan)
    f0, in0 = F(np.full(d.shape[:2], grid[0]))
    for g1 in grid[1:]:
        f1, in1 = F(np.full(d.shape[:2], g1))
        hit = np.isnan(lo) & in0 & in1 & (f0 > 0) & (f1 <= 0)
        lo[hit], hi[hit] = g1 - (grid[1] - grid[0]), g1
        f0, in0 = f1, in1
    ok = ~np.isnan(lo)
    a, b = np.where(ok, lo, 1.0), np.where(ok, hi, 1.0)
    while (b - a).max() > 1e-12:
        mid = 0.5 * (a + b)
        above = F(mid)[0] > 0
        a, b = np.where(above, mid, a), np.where(above, b, mid)
    depth = np.where(ok, 0.5 * (a + b), np.nan)
    if holes:
        rng = np.random.default_rng(seed + 1000)
        depth[rng.integers(0, depth.shape[0], holes), rng.integers(0, depth.shape[1], holes)] = np.nan
    return depth


def sphere_poses():
    """six views around the sphere and a seventh, held out (the chain test registers it onto the fused model)"""
    eyes = [(3.0, 0.2, 0.3), (-2.9, 0.5, -0.4), (0.3, 3.0, 0.5), (-0.4, -3.0, 0.2), (0.8, 0.6, 2.9), (1.8, -1.9, 1.4), (2.4, 1.6, 0.9)]
    return np.array([look_at(e, SPHERE_C) for e in eyes])


def bumpy_poses():
    """five views from above and a sixth, held out"""
    eyes = [(0.0, 0.0, 3.0), (0.9, 0.2, 2.9), (-0.8, 0.4, 2.9), (0.2, -0.9, 2.8), (-0.3, 0.9, 2.8), (0.5, -0.4, 2.9)]
    return np.array([look_at(e, (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)) for e in eyes])


_scenes = {}


def scene(name, model):
    """'sphere' | 'bumpy' -> dict: model, intr, poses [n][7], depth [n][H][W] (computed once per process)"""
    key = (name, model)
    if key not in _scenes:
        intr = CAMERAS[model]
        if name == "sphere":
            poses = sphere_poses()
            depth = np.stack([render_sphere(model, intr, p) for p in poses])
        else:
            poses = bumpy_poses()
            depth = np.stack([render_bumpy(model, intr, p, holes=40, seed=k) for k, p in enumerate(poses)])
        _scenes[key] = dict(model=model, intr=intr, poses=poses, depth=depth)
    return _scenes[key]


def fused(name, model, n_views=None):
    """the restatement's volume of a scene's first n_views views"""
    s = scene(name, model)
    n = len(s["poses"]) if n_views is None else n_views
    return Volume(SHAPE, ORIGIN, VOXEL, TRUNCATION).integrate(model, s["intr"], s["depth"][:n], s["poses"][:n])


def surface_error(name, xyz, normals):
    """-> rms and largest distance of the points from the true surface in voxels, largest angle (rad) between a normal and the true one.
    The bumpy surface's distance is the first-order one, |z - h| / sqrt(1 + |grad h|^2), and points within 2 voxels of the step's
    plane x = STEP_X are left out (the wall is no graph over x, y)."""
    if name == "sphere":
        r = xyz - SPHERE_C
        rn = np.linalg.norm(r, axis=1)
        dist, true_n = np.abs(rn - SPHERE_R), r / rn[:, None]
    else:
        keep = np.abs(xyz[:, 0] - STEP_X) >= 2 * VOXEL
        xyz, normals = xyz[keep], normals[keep]
        hx, hy = bumpy_slope(xyz[:, 0], xyz[:, 1])
        norm = np.sqrt(1.0 + hx * hx + hy * hy)
        dist = np.abs(xyz[:, 2] - bumpy_height(xyz[:, 0], xyz[:, 1])) / norm
        true_n = np.stack([-hx, -hy, np.ones_like(hx)], 1) / norm[:, None]
    has = ~np.isnan(normals[:, 0])
    cosine = np.clip((normals[has] * true_n[has]).sum(1), -1.0, 1.0)
    return float(np.sqrt((dist ** 2).mean())) / VOXEL, float(dist.max()) / VOXEL, float(np.arccos(cosine).max())


def camera_points(model, intr, depth):
    """the organised map [H][W][3] of a depth map, in the camera frame"""
    x, y = pixel_rays(model, intr, depth.shape[1], depth.shape[0])
    return np.stack([x * depth, y * depth, depth], -1)


# ---- cases of both tiers -----------------------------------------------------------------------------------------------------------------
GENERIC_ORIGIN, GENERIC_VOXEL = np.array([-0.05, -0.05, 0.9]), 0.03125
GENERIC_TARGET = GENERIC_ORIGIN + np.array([5, 1, 1]) * GENERIC_VOXEL  # a lattice point: it projects to the principal point of every view


def generic_views(model, n_maps, W=33, H=9, seed=0):
    """n_maps smooth depth maps about 0.93 away with a few invalid pixels (NaN, 0, -1, inf) and poses near the identity that look at GENERIC_TARGET, for a volume
    at GENERIC_ORIGIN: what the size cases integrate"""
    rng = np.random.default_rng(seed)
    intr = np.array([40.0, 38.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.3] + DIST + ([0.04, -0.03] if model == SCHEIMPFLUG else []))
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = np.stack([0.93 + 0.08 * np.sin(0.3 * u + m) * np.cos(0.5 * v - m) + 0.005 * m for m in range(n_maps)]) if n_maps else np.zeros((0, H, W))
    for m in range(n_maps if W * H > 8 else 0):
        for bad in (np.nan, 0.0, -1.0, np.inf):
            depth[m, rng.integers(0, H), rng.integers(0, W)] = bad
    poses = np.array([look_at((0.05 * m - 0.1, 0.02 * m, -0.01 * m), GENERIC_TARGET, up=(0.0, -1.0, 0.0)) for m in range(n_maps)]).reshape(-1, 7)
    return intr, depth, poses


def random_field(shape, seed):
    """D on multiples of 1/8 in [-1, 1] (zeros and -0.0 among them) and W in {0, 1, 2, 3}: planes for upload"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    D = (rng.integers(-8, 9, (nz, ny, nx)) / 8.0).astype(np.float32)
    D[rng.random((nz, ny, nx)) < 0.05] = np.float32(-0.0)
    W = rng.choice(np.array([0, 1, 1, 2, 3], np.float32), (nz, ny, nx))
    return D, W


NX_SIZES = [(nx, 3, 2) for nx in (2, 3, 5, 63, 64, 65, 129)]
# pairs of voxels (one lane each, rows padded to even) just below, at and above a workgroup's 256: 5 x 17 x 3 = 255, 8 x 8 x 4 = 256,
# 3 x 43 x 2 = 258 (257 is prime: no volume has it); and voxel counts around the extract tile: 1023, 1024, 1025
BLOCK_SIZES = [(10, 17, 3), (16, 8, 4), (5, 43, 2), (31, 11, 3), (16, 8, 8), (41, 5, 5)]
FLAT_SHAPE = (1024, 1024, 2)  # 2048 extract tiles: the scan of the tile counts needs a second level


# ---- the host build (tests/fusion_cpu) ---------------------------------------------------------------------------------------------------
def host_integrate(L, vol, model, intr, depth, poses):
    """the host build's update of vol's planes (a Volume; not changed) -> D, W"""
    import ctypes as C

    depth = np.ascontiguousarray(np.asarray(depth, dtype=np.float64))
    depth = depth[None] if depth.ndim == 2 else depth
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
    k = np.ascontiguousarray(np.asarray(intr, dtype=np.float64))
    D, W = np.ascontiguousarray(vol.D.copy()), np.ascontiguousarray(vol.W.copy())
    nx, ny, nz = vol.shape
    o = np.ascontiguousarray(vol.origin)
    L.fusion_host_integrate(C.c_int(nx), C.c_int(ny), C.c_int(nz), ptr(o), C.c_double(vol.vs), C.c_double(vol.trunc), C.c_double(vol.max_weight),
                            C.c_double(vol.max_depth), C.c_int(model), ptr(k), C.c_int(depth.shape[0]), C.c_int(depth.shape[1]),
                            C.c_int(depth.shape[2]), ptr(depth), ptr(poses), ptr(D), ptr(W))
    return D, W


def host_extract(L, vol, min_weight=1.0):
    """the host build's extraction of vol's planes -> xyz, normals"""
    import ctypes as C

    D, W = np.ascontiguousarray(vol.D), np.ascontiguousarray(vol.W)
    nx, ny, nz = vol.shape
    o = np.ascontiguousarray(vol.origin)
    L.fusion_host_extract.restype = C.c_int64
    args = (C.c_int(nx), C.c_int(ny), C.c_int(nz), ptr(o), C.c_double(vol.vs), ptr(D), ptr(W), C.c_double(min_weight))
    n = L.fusion_host_extract(*args, C.c_int64(0), None, None)
    xyz, nrm = np.empty((n, 3)), np.empty((n, 3))
    assert L.fusion_host_extract(*args, C.c_int64(n), ptr(xyz), ptr(nrm)) == n
    return xyz, nrm
