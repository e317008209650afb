"""Independent numpy restatement of the ray cast as calibba.h states it (cba_tsdf_raycast, rule 5 of the scan-fusion section): the view
of a pose, the range of every ray inside the volume, the trilinear sample, the march and the outputs of a hit, vectorised over the
pixels of one view.  numpy's elementwise operations do not contract and the operation order is the header's, so depth, xyz, normals,
status and the sample counts can be held to the bit.  Everything is a function of a rays table [H][W][2]: the device's fetched one on
the GPU tier, ``pixel_rays`` (tests/camera_ref.py's unprojection) or exact planted values on the CPU tier.  Also the wrapper of the
host build (tests/raycast_cpu).  Test infrastructure: no product code is imported here.
"""
import ctypes as C

import numpy as np

from tests import camera_ref as CR
from tests import fusion_ref as F
from tests.host_build import ptr

MISS, HIT, BEHIND, NO_RAY = 0, 1, 2, 3
MAX_SAMPLES = 65536  # calibba.h: CBA_TSDF_RAY_MAX_SAMPLES
WAVE_W, WAVE_H = 8, 8  # a wavefront's pixel block (tsdf_fusion.hip: TSDF_RAY_WAVE_W)
DEFAULTS = dict(step=0.0, skip=0.5, near_depth=0.0, far_depth=np.inf, min_weight=1.0)


def pixel_rays(model, intr, W, H):
    """rays [H][W][2] by the reference-order unprojection: what the device's table is compared with"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    return CR.unproject(model, intr, np.stack([u.ravel(), v.ravel()], 1)).reshape(H, W, 2)


def view(pose7):
    """R (volume frame -> camera) and the camera's centre in the volume frame"""
    R, t = F.rotation(pose7[:4]), np.asarray(pose7[4:], dtype=np.float64)
    c = np.array([-((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2]) for r in range(3)])
    return R, c


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def _lerp(a, b, t):
    return a + t * (b - a)


def sample(vol, p, min_weight):
    """p: three arrays of one shape -> (valid, F)"""
    n = vol.shape
    g = [(p[a] - vol.origin[a]) / vol.vs for a in range(3)]
    ok = np.ones(np.shape(g[0]), bool)
    for a in range(3):
        ok &= (g[a] >= 0.0) & (g[a] <= n[a] - 1.0)
    i, f = [], []
    for a in range(3):
        ga = np.where(ok, g[a], 0.0)
        ia = np.minimum(np.floor(ga), n[a] - 2.0)
        i.append(ia.astype(np.int64))
        f.append(ga - ia)
    D, W = vol.D, vol.W
    heavy = np.ones_like(ok)
    c = []
    for dy, dz in ((0, 0), (1, 0), (0, 1), (1, 1)):
        j, k = i[1] + dy, i[2] + dz
        heavy &= (W[k, j, i[0]].astype(np.float64) >= min_weight) & (W[k, j, i[0] + 1].astype(np.float64) >= min_weight)
        c.append(_lerp(D[k, j, i[0]].astype(np.float64), D[k, j, i[0] + 1].astype(np.float64), f[0]))
    return ok & heavy, _lerp(_lerp(c[0], c[1], f[1]), _lerp(c[2], c[3], f[1]), f[2])


def cast(vol, rays, pose7, step=0.0, skip=0.5, near_depth=0.0, far_depth=np.inf, min_weight=1.0):
    """one view -> dict: depth [H][W], xyz [H][W][3], normals [H][W][3], status uint8 [H][W], count int32 [H][W]"""
    rays = np.asarray(rays, dtype=np.float64)
    H, Wd = rays.shape[:2]
    x, y = rays[..., 0].ravel(), rays[..., 1].ravel()
    n_px = x.size
    R, c = view(np.asarray(pose7, dtype=np.float64))
    step_eff = np.float64(step) if step > 0 else 0.5 * vol.vs
    skip, min_weight = np.float64(skip), np.float64(min_weight)
    n = vol.shape
    status = np.full(n_px, MISS, np.uint8)
    count = np.zeros(n_px, np.int32)
    z_hit = np.full(n_px, np.nan)
    with np.errstate(all="ignore"):
        has_ray = np.isfinite(x) & np.isfinite(y)
        status[~has_ray] = NO_RAY
        d = [(R[0, r] * x + R[1, r] * y) + R[2, r] for r in range(3)]
        z0, z1 = np.full(n_px, np.float64(near_depth)), np.full(n_px, np.float64(far_depth))
        live = has_ray.copy()
        for a in range(3):
            lo, hi = vol.origin[a], vol.origin[a] + np.float64(n[a] - 1) * vol.vs
            par = d[a] == 0.0
            live &= ~(par & ((c[a] < lo) | (c[a] > hi)))
            ta, tb = (lo - c[a]) / d[a], (hi - c[a]) / d[a]
            z0 = np.where(par, z0, _max(z0, _min(ta, tb)))
            z1 = np.where(par, z1, _min(z1, _max(ta, tb)))
        live &= z0 <= z1
        z, pv, Fp, zp = z0.copy(), np.zeros(n_px, bool), np.zeros(n_px), np.zeros(n_px)
        while live.any():
            at = np.nonzero(live)[0]
            zl = z[at]
            ok, Fv = sample(vol, [c[a] + zl * d[a][at] for a in range(3)], min_weight)
            count[at] += 1
            pvl, Fpl, zpl = pv[at], Fp[at], zp[at]
            neg = ok & (Fv < 0.0)
            hit = neg & pvl & (Fpl >= 0.0)
            behind = (neg & ~pvl) | (ok & (Fv >= 0.0) & pvl & (Fpl < 0.0))
            z_hit[at[hit]] = (zpl + (zl - zpl) * (Fpl / (Fpl - Fv)))[hit]
            status[at[hit]] = HIT
            status[at[behind & ~hit]] = BEHIND
            far = (skip * Fv) * vol.trunc
            adv = np.where(ok & (far > step_eff), far, step_eff)
            zn = zl + adv
            end = hit | behind | ~(zn <= z1[at]) | ~(zn > zl) | (count[at] == MAX_SAMPLES)
            live[at[end]] = False
            go = ~end
            pv[at[go]], Fp[at[go]], zp[at[go]], z[at[go]] = ok[go], Fv[go], zl[go], zn[go]
        hits = status == HIT
        at = np.nonzero(hits)[0]
        zh = z_hit[at]
        p = [c[a] + zh * d[a][at] for a in range(3)]
        grad, all_ok = [], np.ones(at.size, bool)
        for a in range(3):
            up, dn = list(p), list(p)
            up[a], dn[a] = p[a] + vol.vs, p[a] - vol.vs
            oka, Fa = sample(vol, up, min_weight)
            okb, Fb = sample(vol, dn, min_weight)
            all_ok &= oka & okb
            grad.append(Fa - Fb)
        length = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2])
        good = all_ok & (length > 0.0) & np.isfinite(length)
        m = [g / length for g in grad]
        nrm = np.full((n_px, 3), np.nan)
        for r in range(3):
            nrm[at, r] = np.where(good, (R[r, 0] * m[0] + R[r, 1] * m[1]) + R[r, 2] * m[2], np.nan)
        xyz = np.stack([x * z_hit, y * z_hit, z_hit], -1)
    return dict(depth=z_hit.reshape(H, Wd), xyz=xyz.reshape(H, Wd, 3), normals=nrm.reshape(H, Wd, 3), status=status.reshape(H, Wd),
                count=count.reshape(H, Wd))


def cast_views(vol, rays, poses, **opts):
    """several views -> the stacked arrays of cast"""
    out = [cast(vol, rays, p, **opts) for p in np.asarray(poses, dtype=np.float64).reshape(-1, 7)]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def cloud(res, view_index, pose7):
    """the hits of one view of stacked results in the volume frame, row-major: xyz [n][3], normals [n][3] (pose7 rigid)"""
    q = np.asarray(pose7[:4]) / np.linalg.norm(pose7[:4])
    R, t = F.rotation(q), np.asarray(pose7[4:])
    m = res["status"][view_index] == HIT
    return (res["xyz"][view_index][m] - t) @ R, res["normals"][view_index][m] @ R


# ---- the host build (tests/raycast_cpu) ---------------------------------------------------------------------------------------------------
def host_cast(L, vol, rays, pose7, step=0.0, skip=0.5, near_depth=0.0, far_depth=np.inf, min_weight=1.0):
    """the host build of tsdf_ray_math.hpp over one view -> the dict cast returns"""
    rays = np.ascontiguousarray(np.asarray(rays, dtype=np.float64))
    H, Wd = rays.shape[:2]
    n_px = H * Wd
    D, W = np.ascontiguousarray(vol.D), np.ascontiguousarray(vol.W)
    o, pose = np.ascontiguousarray(vol.origin), np.ascontiguousarray(np.asarray(pose7, dtype=np.float64))
    opts = np.array([step, skip, near_depth, far_depth, min_weight], dtype=np.float64)
    depth, xyz, nrm = np.empty(n_px), np.empty((n_px, 3)), np.empty((n_px, 3))
    status, count = np.empty(n_px, np.uint8), np.empty(n_px, np.int32)
    nx, ny, nz = vol.shape
    L.raycast_host_cast(C.c_int(nx), C.c_int(ny), C.c_int(nz), ptr(o), C.c_double(vol.vs), C.c_double(vol.trunc), ptr(D), ptr(W),
                        C.c_int64(n_px), ptr(rays), ptr(pose), ptr(opts), ptr(depth), ptr(xyz), ptr(nrm), ptr(status), ptr(count))
    return dict(depth=depth.reshape(H, Wd), xyz=xyz.reshape(H, Wd, 3), normals=nrm.reshape(H, Wd, 3), status=status.reshape(H, Wd),
                count=count.reshape(H, Wd))
