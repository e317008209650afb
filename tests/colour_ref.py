"""Independent numpy restatement of colour in scan fusion as calibba.h states it (cba_tsdf_integrate_colour and rules 6 to 8 of the
scan-fusion section): the {R, G, B, Wc} record of every voxel through one map and its image, vectorised per map; the colour of every
point of the extract; the colour of every hit of a ray cast.  numpy's elementwise operations do not contract and the operation order
is the header's, so the records and the bytes can be held to the bit.  The geometry (projection, poses, edges, the view and the lerp of
the ray cast) is that of tests/fusion_ref.py, tests/mesh_ref.py and tests/raycast_ref.py.  Also the scene builder (the sphere and the
bumpy surface of fusion_ref painted with a smooth function of the surface position, so that the true colour of any point is known)
and the wrappers of the host build (tests/colour_cpu).  Test infrastructure: no product code is imported here.
"""
import ctypes as C

import numpy as np

from tests import fusion_ref as F
from tests import mesh_ref as MR
from tests import raycast_ref as RC
from tests.host_build import ptr


class Volume(F.Volume):
    """fusion_ref's volume with the colour records beside it: C float32 [nz][ny][nx][4], None while the volume has no colour"""

    def __init__(self, *a, **kw):
        self.C = None
        super().__init__(*a, **kw)

    def reset(self):
        super().reset()
        if self.C is not None:
            self.C = np.zeros_like(self.C)

    def integrate_colour(self, model, intr, depth, rgba, poses):
        """rule 6: steps 1 to 6 as rule 2 states them, then step 7; rgba uint8 [n_maps][H][W][4]"""
        depth = np.asarray(depth, dtype=np.float64)
        depth = depth[None] if depth.ndim == 2 else depth
        rgba = np.asarray(rgba, dtype=np.uint8).reshape(depth.shape + (4,))
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
        if depth.shape[0] == 0:
            return self  # no work: nothing is allocated
        nx, ny, nz = self.shape
        if self.C is None:
            self.C = np.zeros((nz, ny, nx, 4), np.float32)
        H, Wd = depth.shape[1:]
        X0, X1, X2 = self.axes[0][None, None, :], self.axes[1][None, :, None], self.axes[2][:, None, None]
        for m in range(depth.shape[0]):
            R, t = F.rotation(poses[m, :4]), poses[m, 4:]
            with np.errstate(all="ignore"):
                P = [((R[r, 0] * X0 + R[r, 1] * X1) + R[r, 2] * X2) + t[r] for r in range(3)]
                ok = (P[2] > 0.0) & (F.denominator(model, intr, *P) > 0.0)
                u, v = F.project(model, intr, *P)
                px, py = np.floor(u + 0.5), np.floor(v + 0.5)
                ok &= (px >= 0.0) & (px <= Wd - 1.0) & (py >= 0.0) & (py <= H - 1.0)
                row, col = np.where(ok, py, 0.0).astype(np.int64), np.where(ok, px, 0.0).astype(np.int64)
                d = depth[m][row, col]
                ok &= np.isfinite(d) & (d > 0.0) & (d <= self.max_depth)
                s = d - P[2]
                ok &= ~(s < -self.trunc)
                f = s / self.trunc
                f = np.where(f > 1.0, 1.0, f)
                w = self.W.astype(np.float64)
                Dn = ((w * self.D.astype(np.float64) + f) / (w + 1.0)).astype(np.float32)
                Wn = np.minimum(w + 1.0, self.max_weight).astype(np.float32)
                # step 7
                pixel = rgba[m][row, col]
                take = ok & (s <= self.trunc) & (pixel[..., 3] != 0)
                wc = self.C[..., 3].astype(np.float64)
                Cn = np.empty_like(self.C)
                for ch in range(3):
                    Cn[..., ch] = ((wc * self.C[..., ch].astype(np.float64) + pixel[..., ch].astype(np.float64)) / (wc + 1.0)).astype(np.float32)
                Cn[..., 3] = np.minimum(wc + 1.0, self.max_weight).astype(np.float32)
            self.D, self.W = np.where(ok, Dn, self.D), np.where(ok, Wn, self.W)
            self.C = np.where(take[..., None], Cn, self.C)
        return self


def to_bytes(Cv):
    """q = floor(C + 0.5), 0 when q < 0 or C is NaN, 255 when q > 255"""
    with np.errstate(invalid="ignore"):
        q = np.floor(np.asarray(Cv, dtype=np.float64) + 0.5)
        return np.where(~(q >= 0.0), 0.0, np.where(q > 255.0, 255.0, q)).astype(np.uint8)


def point_colours(vol, min_weight=1.0):
    """rule 7 -> uint8 [n][4] in the order of vol.extract(min_weight)'s points"""
    q, _, _ = MR.edge_mask(vol, min_weight)
    k, j, i, axis = np.nonzero(q)
    bi, bj, bk = i + (axis == 0), j + (axis == 1), k + (axis == 2)
    D = vol.D.astype(np.float64)
    Da, Db = D[k, j, i], D[bk, bj, bi]
    t = Da / (Da - Db)
    Ca, Cb = vol.C[k, j, i].astype(np.float64), vol.C[bk, bj, bi].astype(np.float64)
    has_a, has_b = Ca[:, 3] > 0.0, Cb[:, 3] > 0.0
    with np.errstate(all="ignore"):
        both = Ca[:, :3] + t[:, None] * (Cb[:, :3] - Ca[:, :3])
    value = np.where((has_a & has_b)[:, None], both, np.where(has_a[:, None], Ca[:, :3], Cb[:, :3]))
    out = np.zeros((i.size, 4), np.uint8)
    out[:, :3], out[:, 3] = to_bytes(value), 255
    out[~(has_a | has_b)] = 0
    return out


def hit_colours(vol, rays, pose7, status, depth):
    """rule 8 for one view: rays [H][W][2], status and depth [H][W] as the ray cast stored them -> uint8 [H][W][4]"""
    rays = np.asarray(rays, dtype=np.float64)
    H, Wd = rays.shape[:2]
    x, y, z = rays[..., 0].ravel(), rays[..., 1].ravel(), np.asarray(depth, dtype=np.float64).ravel()
    hit = np.asarray(status).ravel() == RC.HIT
    R, c = RC.view(np.asarray(pose7, dtype=np.float64))
    n = vol.shape
    with np.errstate(all="ignore"):
        p = [c[r] + z * ((R[0, r] * x + R[1, r] * y) + R[2, r]) for r in range(3)]
        g = [(p[a] - vol.origin[a]) / vol.vs for a in range(3)]
        ok = hit.copy()
        for a in range(3):
            ok &= (g[a] >= 0.0) & (g[a] <= n[a] - 1.0)
        i, f = [], []
        for a in range(3):
            ga = np.where(ok, g[a], 0.0)
            ia = np.minimum(np.floor(ga), n[a] - 2.0)
            i.append(ia.astype(np.int64))
            f.append(ga - ia)
        rows = []
        for dy, dz in ((0, 0), (1, 0), (0, 1), (1, 1)):
            a, b = vol.C[i[2] + dz, i[1] + dy, i[0]].astype(np.float64), vol.C[i[2] + dz, i[1] + dy, i[0] + 1].astype(np.float64)
            ok &= (a[:, 3] > 0.0) & (b[:, 3] > 0.0)
            rows.append(RC._lerp(a[:, :3], b[:, :3], f[0][:, None]))
        value = RC._lerp(RC._lerp(rows[0], rows[1], f[1][:, None]), RC._lerp(rows[2], rows[3], f[1][:, None]), f[2][:, None])
    out = np.zeros((x.size, 4), np.uint8)
    out[:, :3], out[:, 3] = to_bytes(value), 255
    out[~ok] = 0
    return out.reshape(H, Wd, 4)


# ---- painted scenes -------------------------------------------------------------------------------------------------------------------
def paint(p):
    """the true colour [..][3] (float, in [28, 228]) at surface points [..][3]: smooth, so that a voxel-sized error in position moves
    a channel by a few units"""
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([128.0 + 100.0 * np.sin(3.0 * x + 0.5), 128.0 + 100.0 * np.cos(2.5 * y - 0.3), 128.0 + 100.0 * np.sin(2.0 * z + x)], -1)


def painted_image(model, intr, pose7, depth):
    """rgba uint8 [H][W][4] of one rendered depth map: the paint at each pixel's surface point, A = 0 where the ray misses"""
    eye, d = F._world_rays(model, intr, pose7)
    hit = np.isfinite(depth)
    point = eye + np.where(hit, depth, 0.0)[..., None] * d
    out = np.zeros(depth.shape + (4,), np.uint8)
    out[..., :3], out[..., 3] = to_bytes(paint(point)), 255
    out[~hit] = 0
    return out


_painted = {}


def painted_scene(name, model):
    """fusion_ref.scene with rgba [n][H][W][4] beside the depth maps (computed once per process)"""
    key = (name, model)
    if key not in _painted:
        s = dict(F.scene(name, model))
        s["rgba"] = np.stack([painted_image(model, s["intr"], p, d) for p, d in zip(s["poses"], s["depth"])])
        _painted[key] = s
    return _painted[key]


_fused = {}


def fused(name, model, n_views):
    """the restatement's coloured volume of a painted scene's first n_views views (computed once per process; do not change it)"""
    key = (name, model, n_views)
    if key not in _fused:
        s = painted_scene(name, model)
        v = Volume(F.SHAPE, F.ORIGIN, F.VOXEL, F.TRUNCATION)
        _fused[key] = v.integrate_colour(model, s["intr"], s["depth"][:n_views], s["rgba"][:n_views], s["poses"][:n_views])
    return _fused[key]


def colour_error(xyz, rgba):
    """-> (mean, largest) absolute channel difference between the colours of points [n][3] that have one and the paint there, and the
    share of points with A == 0"""
    has = rgba[:, 3] != 0
    diff = np.abs(rgba[has, :3].astype(np.float64) - paint(xyz[has]))
    return float(diff.mean()), float(diff.max()), float(1.0 - has.mean())


def generic_images(n_maps, W=33, H=9, seed=0):
    """rgba [n_maps][H][W][4] for fusion_ref.generic_views: random bytes, about a tenth of the pixels with A == 0"""
    rng = np.random.default_rng(seed + 77)
    rgba = rng.integers(0, 256, (n_maps, H, W, 4), dtype=np.uint8)
    rgba[..., 3] = np.where(rng.random((n_maps, H, W)) < 0.1, 0, np.maximum(rgba[..., 3], 1))
    return rgba


def random_colour(shape, seed):
    """records for upload: channels on multiples of 1/4 in [0, 255] (x.5 among them), Wc in {0, 0, 1, 2}"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed + 900)
    Cv = (rng.integers(0, 1021, (nz, ny, nx, 4)) / 4.0).astype(np.float32)
    Cv[..., 3] = rng.choice(np.array([0, 0, 1, 2], np.float32), (nz, ny, nx))
    return Cv


# ---- the host build (tests/colour_cpu) ---------------------------------------------------------------------------------------------------
def _volume_args(vol):
    nx, ny, nz = vol.shape
    return (C.c_int(nx), C.c_int(ny), C.c_int(nz), ptr(np.ascontiguousarray(vol.origin)), C.c_double(vol.vs))


def host_integrate_colour(L, vol, model, intr, depth, rgba, poses):
    """the host build's update of vol's planes and records (a Volume; not changed) -> D, W, C"""
    depth = np.ascontiguousarray(np.asarray(depth, dtype=np.float64))
    depth = depth[None] if depth.ndim == 2 else depth
    rgba = np.ascontiguousarray(np.asarray(rgba, dtype=np.uint8).reshape(depth.shape + (4,)))
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
    k = np.ascontiguousarray(np.asarray(intr, dtype=np.float64))
    nx, ny, nz = vol.shape
    D, W = np.ascontiguousarray(vol.D.copy()), np.ascontiguousarray(vol.W.copy())
    Cv = np.zeros((nz, ny, nx, 4), np.float32) if vol.C is None else np.ascontiguousarray(vol.C.copy())
    L.colour_host_integrate(*_volume_args(vol), C.c_double(vol.trunc), C.c_double(vol.max_weight), C.c_double(vol.max_depth), C.c_int(model), ptr(k),
                            C.c_int(depth.shape[0]), C.c_int(depth.shape[1]), C.c_int(depth.shape[2]), ptr(depth), ptr(rgba), ptr(poses), ptr(D),
                            ptr(W), ptr(Cv))
    return D, W, Cv


def host_point_colours(L, vol, min_weight=1.0):
    D, W, Cv = np.ascontiguousarray(vol.D), np.ascontiguousarray(vol.W), np.ascontiguousarray(vol.C)
    L.colour_host_points.restype = C.c_int64
    args = (*_volume_args(vol), ptr(D), ptr(W), ptr(Cv), C.c_double(min_weight))
    n = L.colour_host_points(*args, C.c_int64(0), None)
    out = np.zeros((n, 4), np.uint8)
    assert L.colour_host_points(*args, C.c_int64(n), ptr(out)) == n
    return out


def host_hit_colours(L, vol, rays, pose7, status, depth):
    rays = np.ascontiguousarray(np.asarray(rays, dtype=np.float64))
    H, Wd = rays.shape[:2]
    Cv = np.ascontiguousarray(vol.C)
    pose = np.ascontiguousarray(np.asarray(pose7, dtype=np.float64))
    st, z = np.ascontiguousarray(np.asarray(status, dtype=np.uint8)), np.ascontiguousarray(np.asarray(depth, dtype=np.float64))
    out = np.zeros((H, Wd, 4), np.uint8)
    L.colour_host_hits(*_volume_args(vol), ptr(Cv), C.c_int64(H * Wd), ptr(rays), ptr(pose), ptr(st), ptr(z), ptr(out))
    return out
