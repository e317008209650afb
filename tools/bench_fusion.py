"""Scan-fusion benchmark: one JSON line with the time of k_tsdf_integrate for 1, 4 and 16 depth maps per call into a 256^3 volume,
for the pinhole model with distortion and for Scheimpflug, and of the extraction of the fused surface, next to the bytes each must
touch.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_fusion.py [--side 256] [--width 640] [--height 480] [--reps 5] [--out profiles/r21_fusion.json]
The scene is the test scenes' sphere (tests/fusion_ref.py) at scan size: a sphere of radius 0.5 in a volume of side 2, seen by 16
cameras on a ring of radius 3, truncation four voxels.  The times are device events inside the call, from cba_tsdf_integrate_timed and
cba_tsdf_extract_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY): upload and
kernel for integrate; count with scan, and place, for extract (median over --reps after one warm-up call; the volume is reset before
every integrate, so every call updates the same voxels).  The byte floor of an integrate is 8 B read per voxel, 8 B written per
updated voxel and the maps once; of an extract two reads of the volume and 48 B per point.  No time is fixed in advance (DESIGN.md
section 7s)."""
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
from tests import fusion_ref as F  # noqa: E402

COPY_RATE = 6.3e12  # B/s: the achievable copy rate DESIGN.md measures its kernels against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    d = capi.c_double_p
    lib.cba_tsdf_integrate_timed.argtypes = [C.c_void_p, C.c_int32, d, C.c_int32, C.c_int32, C.c_int32, d, d, d]
    lib.cba_tsdf_integrate_timed.restype = C.c_int32
    lib.cba_tsdf_extract_timed.argtypes = [C.c_void_p, C.c_double, capi.c_int64_p, d]
    lib.cba_tsdf_extract_timed.restype = C.c_int32
    W, H, side = a.width, a.height, a.side
    vs = 2.0 / side
    scale = W / F.MAP_W
    poses = np.array([F.look_at((3.0 * math.cos(t), 3.0 * math.sin(t), 0.6 * math.sin(3 * t)), F.SPHERE_C)
                      for t in np.arange(16) * (2 * math.pi / 16)])
    res = {"kind": "fusion", "side": side, "width": W, "height": H, "reps": a.reps, "voxels": side ** 3, "copy_rate": COPY_RATE}
    ms = np.zeros(2)
    n_pts = np.zeros(1, np.int64)
    for model, name in ((F.PINHOLE, "pinhole"), (F.SCHEIMPFLUG, "scheimpflug")):
        intr = F.CAMERAS[model].copy()
        intr[:4] = [150.0 * scale, 148.0 * scale, (W - 1) / 2.0, (H - 1) / 2.0]
        x, y = F.pixel_rays(model, intr, W, H)
        depth = np.ascontiguousarray(np.stack([render(x, y, p) for p in poses]))
        k = np.ascontiguousarray(intr)
        with TsdfVolume((side, side, side), [-1.0, -1.0, -1.0], TsdfOptions(vs, 4 * vs)) as vol:
            for n_maps in (1, 4, 16):
                def call():
                    vol.reset()
                    capi.check(lib, lib.cba_tsdf_integrate_timed(vol._h, model, capi.dptr(k), n_maps, H, W, capi.dptr(depth), capi.dptr(poses),
                                                                 capi.dptr(ms)))
                    return ms.copy()
                call()
                med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
                updated = int((vol.fetch()[1] > 0).sum())
                floor = 8 * side ** 3 + 8 * updated + 8 * n_maps * W * H
                res[f"integrate_{name}_maps{n_maps}"] = dict(upload_ms=float(med[0]), kernel_ms=float(med[1]), updated_voxels=updated,
                                                             floor_bytes=floor, floor_ms=floor / COPY_RATE * 1e3)
                print(f"{name}, {n_maps} map(s): kernel {med[1]:.3f} ms, floor {floor / COPY_RATE * 1e3:.3f} ms, {updated} voxels updated",
                      file=sys.stderr, flush=True)

            def extract():
                capi.check(lib, lib.cba_tsdf_extract_timed(vol._h, 1.0, capi.i64ptr(n_pts), capi.dptr(ms)))
                return ms.copy()
            extract()
            med = np.median(np.array([extract() for _ in range(a.reps)]), axis=0)
            floor = 2 * 8 * side ** 3 + 48 * int(n_pts[0])
            res[f"extract_{name}"] = dict(count_scan_ms=float(med[0]), place_ms=float(med[1]), points=int(n_pts[0]), floor_bytes=floor,
                                          floor_ms=floor / COPY_RATE * 1e3)
            print(f"{name}: extract count+scan {med[0]:.3f} ms, place {med[1]:.3f} ms, {int(n_pts[0])} points", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def render(x, y, pose7):
    """the sphere's depth along the rays (x, y, 1) of a camera at pose7 (fusion_ref.render_sphere with the rays given)"""
    R, t = F.rotation(pose7[:4]), np.asarray(pose7[4:])
    Ri = np.linalg.inv(R)
    oc = -(Ri @ t) - F.SPHERE_C
    dirs = np.stack([x, y, np.ones_like(x)], -1) @ Ri.T
    qa, qb, qc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - F.SPHERE_R ** 2
    disc = qb * qb - 4 * qa * qc
    with np.errstate(invalid="ignore"):
        lam = (-qb - np.sqrt(disc)) / (2 * qa)
    return np.where((disc > 0) & (lam > 0), lam, np.nan)


if __name__ == "__main__":
    main()
