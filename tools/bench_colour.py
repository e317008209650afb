"""Colour-fusion benchmark: one JSON line with the time of k_tsdf_integrate_colour against k_tsdf_integrate on the same depth maps (1, 4
and 16 maps per call into a 256^3 volume, both camera models), of the same kernel with every colour word loaded up front, of the
extract with and without colour, and of the ray cast's colour pass, next to the bytes each must touch.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_colour.py [--side 256] [--width 640] [--height 480] [--views 4] [--reps 5] [--out profiles/r25_colour.json]
The scene is that of tools/bench_fusion.py (the test scenes' sphere at scan size, 16 cameras on a ring, truncation four voxels) with
the maps painted by tests/colour_ref.py.  The times are device events inside the call, from the _timed entry points that only the
experiment build exports (median over --reps after one warm-up call; the volume is reset before every integrate, so every call
updates the same voxels).  The byte floor of a colour integrate is 8 B read per voxel, 16 B read per voxel that takes colour, what is
stored (8 B per updated voxel, 16 B per voxel that took colour) and the maps once (12 B per pixel).  No ratio is fixed in advance
(DESIGN.md section 7w)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CALIBBA_LIBRARY", os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so"))

from calibration_amd import capi  # noqa: E402
from calibration_amd.fusion import TsdfOptions, TsdfVolume  # noqa: E402
from tests import colour_ref as K  # noqa: E402
from tests import fusion_ref as F  # noqa: E402

COPY_RATE = 6.3e12  # B/s: the achievable copy rate DESIGN.md measures its kernels against


def render(x, y, pose7):
    """-> depth [H][W] of the sphere along the rays (x, y, 1) of a camera at pose7, and the painted image rgba [H][W][4]"""
    R, t = F.rotation(pose7[:4]), np.asarray(pose7[4:])
    Ri = np.linalg.inv(R)
    eye = -(Ri @ t)
    oc = eye - F.SPHERE_C
    dirs = np.stack([x, y, np.ones_like(x)], -1) @ Ri.T
    qa, qb, qc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - F.SPHERE_R ** 2
    disc = qb * qb - 4 * qa * qc
    with np.errstate(invalid="ignore"):
        lam = (-qb - np.sqrt(disc)) / (2 * qa)
    hit = (disc > 0) & (lam > 0)
    rgba = np.zeros(x.shape + (4,), np.uint8)
    rgba[..., :3], rgba[..., 3] = K.to_bytes(K.paint(eye + np.where(hit, lam, 0.0)[..., None] * dirs)), 255
    rgba[~hit] = 0
    return np.where(hit, lam, np.nan), rgba


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    d, u8 = capi.c_double_p, capi.c_uint8_p
    lib.cba_tsdf_integrate_timed.argtypes = [C.c_void_p, C.c_int32, d, C.c_int32, C.c_int32, C.c_int32, d, d, d]
    lib.cba_tsdf_integrate_colour_timed.argtypes = [C.c_void_p, C.c_int32, d, C.c_int32, C.c_int32, C.c_int32, d, u8, d, C.c_int32, d]
    lib.cba_tsdf_extract_timed.argtypes = [C.c_void_p, C.c_double, capi.c_int64_p, d]
    lib.cba_tsdf_raycast_colour_timed.argtypes = [C.c_void_p, C.c_int32, d, C.c_int32, C.c_int32, C.c_int32, d, C.POINTER(capi.CbaTsdfRaycastOptions), d]
    for f in (lib.cba_tsdf_integrate_timed, lib.cba_tsdf_integrate_colour_timed, lib.cba_tsdf_extract_timed, lib.cba_tsdf_raycast_colour_timed):
        f.restype = C.c_int32
    W, H, side = a.width, a.height, a.side
    vs = 2.0 / side
    scale = W / F.MAP_W
    poses = np.array([F.look_at((3.0 * math.cos(t), 3.0 * math.sin(t), 0.6 * math.sin(3 * t)), F.SPHERE_C)
                      for t in np.arange(16) * (2 * math.pi / 16)])
    views = np.ascontiguousarray(np.array([F.look_at((3.0 * math.cos(t), 3.0 * math.sin(t), 0.4 * math.cos(2 * t)), F.SPHERE_C)
                                           for t in (np.arange(a.views) + 0.5) * (2 * math.pi / 16)]))
    res = {"kind": "colour", "side": side, "width": W, "height": H, "views": a.views, "reps": a.reps, "voxels": side ** 3, "copy_rate": COPY_RATE}
    ms, ms3 = np.zeros(2), np.zeros(3)
    n_pts = np.zeros(1, np.int64)

    def median(call):
        call()
        return np.median(np.array([call() for _ in range(a.reps)]), axis=0)

    for model, name in ((F.PINHOLE, "pinhole"), (F.SCHEIMPFLUG, "scheimpflug")):
        intr = F.CAMERAS[model].copy()
        intr[:4] = [150.0 * scale, 148.0 * scale, (W - 1) / 2.0, (H - 1) / 2.0]
        x, y = F.pixel_rays(model, intr, W, H)
        maps = [render(x, y, p) for p in poses]
        depth, rgba = np.ascontiguousarray(np.stack([m[0] for m in maps])), np.ascontiguousarray(np.stack([m[1] for m in maps]))
        k = np.ascontiguousarray(intr)
        opts = TsdfOptions(vs, 4 * vs)
        with TsdfVolume((side, side, side), [-1.0, -1.0, -1.0], opts) as plain, TsdfVolume((side, side, side), [-1.0, -1.0, -1.0], opts) as vol:
            for n_maps in (1, 4, 16):
                def integrate_plain():
                    plain.reset()
                    capi.check(lib, lib.cba_tsdf_integrate_timed(plain._h, model, capi.dptr(k), n_maps, H, W, capi.dptr(depth), capi.dptr(poses),
                                                                 capi.dptr(ms)))
                    return ms.copy()

                def integrate_colour(eager):
                    vol.reset()
                    capi.check(lib, lib.cba_tsdf_integrate_colour_timed(vol._h, model, capi.dptr(k), n_maps, H, W, capi.dptr(depth), capi.u8ptr(rgba),
                                                                        capi.dptr(poses), eager, capi.dptr(ms)))
                    return ms.copy()

                base = median(integrate_plain)
                eager = median(lambda: integrate_colour(1))
                lazy = median(lambda: integrate_colour(0))  # last: the volume keeps the lazy kernel's result
                updated, coloured = int((vol.fetch()[1] > 0).sum()), int((vol.fetch_colour()[..., 3] > 0).sum())
                assert vol.fetch()[0].tobytes() == plain.fetch()[0].tobytes()
                floor = 8 * side ** 3 + 16 * coloured + 8 * updated + 16 * coloured + 12 * n_maps * W * H
                res[f"integrate_{name}_maps{n_maps}"] = dict(
                    plain_kernel_ms=float(base[1]), colour_kernel_ms=float(lazy[1]), eager_kernel_ms=float(eager[1]), ratio=float(lazy[1] / base[1]),
                    eager_ratio=float(eager[1] / base[1]), upload_ms=float(lazy[0]), plain_upload_ms=float(base[0]), updated_voxels=updated,
                    coloured_voxels=coloured, floor_bytes=floor, floor_ms=floor / COPY_RATE * 1e3)
                print(f"{name}, {n_maps} map(s): plain {base[1]:.3f} ms, colour {lazy[1]:.3f} ms ({lazy[1] / base[1]:.3f} x), eager {eager[1]:.3f} ms, "
                      f"floor {floor / COPY_RATE * 1e3:.3f} ms, {updated} voxels updated, {coloured} coloured", file=sys.stderr, flush=True)

            def extract(v):
                capi.check(lib, lib.cba_tsdf_extract_timed(v._h, 1.0, capi.i64ptr(n_pts), capi.dptr(ms)))
                return ms.copy()

            without, with_colour = median(lambda: extract(plain)), median(lambda: extract(vol))
            n = int(n_pts[0])
            res[f"extract_{name}"] = dict(count_scan_ms=float(with_colour[0]), place_ms=float(with_colour[1]), plain_place_ms=float(without[1]),
                                          ratio=float(with_colour[1] / without[1]), points=n, floor_bytes=2 * 8 * side ** 3 + (48 + 32 + 4) * n,
                                          floor_ms=(2 * 8 * side ** 3 + (48 + 32 + 4) * n) / COPY_RATE * 1e3)
            print(f"{name}: extract place {without[1]:.3f} ms without colour, {with_colour[1]:.3f} ms with, {n} points", file=sys.stderr, flush=True)

            def cast():
                o = capi.CbaTsdfRaycastOptions(0.0, 0.5, 0.0, np.inf, 1.0)
                capi.check(lib, lib.cba_tsdf_raycast_colour_timed(vol._h, model, capi.dptr(k), a.views, H, W, capi.dptr(views), C.byref(o),
                                                                  capi.dptr(ms3)))
                return ms3.copy()

            t = median(cast)
            status = np.empty((a.views, H, W), np.uint8)
            capi.check(lib, lib.cba_tsdf_raycast_fetch(vol._h, capi.dptr(None), capi.dptr(None), capi.dptr(None), capi.u8ptr(status), capi.dptr(None)))
            hits = int((status == 1).sum())
            floor = a.views * H * W * (1 + 8 + 4) + 16 * H * W + hits * 8 * 16
            res[f"raycast_{name}"] = dict(cast_ms=float(t[1]), colour_ms=float(t[2]), ratio=float(t[2] / t[1]), hits=hits, floor_bytes=floor,
                                          floor_ms=floor / COPY_RATE * 1e3)
            print(f"{name}: ray cast {t[1]:.3f} ms, colour pass {t[2]:.3f} ms, {hits} hits of {a.views * H * W} pixels", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
