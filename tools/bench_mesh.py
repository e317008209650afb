"""Scan-meshing benchmark: one JSON line with the time of cba_tsdf_mesh on the fused sphere of tools/bench_fusion.py (256^3 voxels, a
sphere of radius 0.5, 16 maps), split into the extract's count with scan, its place pass with the edge records, the triangles' count
with scan and their place pass, next to a plain cba_tsdf_extract on the same volume and to the bytes each stage must touch.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_mesh.py [--side 256] [--width 640] [--height 480] [--reps 5] [--out profiles/r22_mesh.json]
The times are device events inside the call, from cba_tsdf_mesh_timed and cba_tsdf_extract_timed, which only the experiment build
exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY): the median over --reps after one warm-up call, with the smallest
and the largest beside it as the spread.  The records cost what the mesh's place pass takes beyond the plain extract's.  Byte floors
at the copy rate DESIGN.md measures its kernels against: a count pass reads the volume once (8 B per voxel); the extract's place pass
reads it again and writes 48 B per point and 32 B per 64 voxels of records; the triangles' place pass reads the volume and the
records and writes 12 B per triangle.  No time is fixed in advance."""
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
from tools.bench_fusion import COPY_RATE, render  # noqa: E402


def spread(rows):
    """rows [reps][stages] -> median, smallest, largest per stage"""
    a = np.array(rows)
    return np.median(a, axis=0), a.min(axis=0), a.max(axis=0)


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
    lib.cba_tsdf_extract_timed.argtypes = [C.c_void_p, C.c_double, capi.c_int64_p, d]
    lib.cba_tsdf_extract_timed.restype = C.c_int32
    lib.cba_tsdf_mesh_timed.argtypes = [C.c_void_p, C.c_double, capi.c_int64_p, capi.c_int64_p, d]
    lib.cba_tsdf_mesh_timed.restype = C.c_int32
    W, H, side = a.width, a.height, a.side
    vs = 2.0 / side
    poses = np.array([F.look_at((3.0 * math.cos(t), 3.0 * math.sin(t), 0.6 * math.sin(3 * t)), F.SPHERE_C)
                      for t in np.arange(16) * (2 * math.pi / 16)])
    intr = F.CAMERAS[F.PINHOLE].copy()
    scale = W / F.MAP_W
    intr[:4] = [150.0 * scale, 148.0 * scale, (W - 1) / 2.0, (H - 1) / 2.0]
    x, y = F.pixel_rays(F.PINHOLE, intr, W, H)
    depth = np.ascontiguousarray(np.stack([render(x, y, p) for p in poses]))
    res = {"kind": "mesh", "side": side, "width": W, "height": H, "reps": a.reps, "voxels": side ** 3, "copy_rate": COPY_RATE}
    ms2, ms4 = np.zeros(2), np.zeros(4)
    n_pts, n_tri = np.zeros(1, np.int64), np.zeros(1, np.int64)
    with TsdfVolume((side, side, side), [-1.0, -1.0, -1.0], TsdfOptions(vs, 4 * vs)) as vol:
        vol.integrate(F.PINHOLE, intr, poses, depth=depth)

        def extract():
            capi.check(lib, lib.cba_tsdf_extract_timed(vol._h, 1.0, capi.i64ptr(n_pts), capi.dptr(ms2)))
            return ms2.copy()

        def mesh():
            capi.check(lib, lib.cba_tsdf_mesh_timed(vol._h, 1.0, capi.i64ptr(n_pts), capi.i64ptr(n_tri), capi.dptr(ms4)))
            return ms4.copy()

        extract()
        e_med, e_min, e_max = spread([extract() for _ in range(a.reps)])
        mesh()
        m_med, m_min, m_max = spread([mesh() for _ in range(a.reps)])
        got = vol.mesh()
    points, tris, vol_bytes, rec_bytes = int(n_pts[0]), int(n_tri[0]), 8 * side ** 3, 32 * ((side ** 3 + 63) // 64)
    floors = {"extract_count_scan": vol_bytes, "extract_place_records": vol_bytes + 48 * points + rec_bytes, "mesh_count_scan": vol_bytes,
              "mesh_place": vol_bytes + rec_bytes + 12 * tris}
    res.update(points=points, triangles=tris, boundary_edges=int(len(got.boundary_edges())), area=got.area(),
               true_area=4.0 * math.pi * F.SPHERE_R ** 2)
    res["extract"] = dict(count_scan_ms=float(e_med[0]), place_ms=float(e_med[1]), min_ms=e_min.tolist(), max_ms=e_max.tolist())
    for k, name in enumerate(floors):
        res[name] = dict(ms=float(m_med[k]), min_ms=float(m_min[k]), max_ms=float(m_max[k]), floor_bytes=floors[name],
                         floor_ms=floors[name] / COPY_RATE * 1e3)
    res["records_ms"] = float(m_med[1] - e_med[1])
    res["mesh_total_ms"] = float(m_med.sum())
    print(f"extract alone: count+scan {e_med[0]:.3f} ms, place {e_med[1]:.3f} ms; in the mesh call: {m_med[0]:.3f} ms, {m_med[1]:.3f} ms; triangles: "
          f"count+scan {m_med[2]:.3f} ms, place {m_med[3]:.3f} ms; {points} points, {tris} triangles", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
