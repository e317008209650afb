"""Ray-cast benchmark: one JSON line with the time of cba_tsdf_raycast per 640 x 480 view on the fused sphere of tools/bench_fusion.py
(256^3 voxels, a sphere of radius 0.5, 16 maps), at skip 0 and 0.5, with a wavefront's pixels as a compact 8 x 8 block and as a 64 x 1
row segment, next to the samples per ray and to the bytes a view must touch.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_raycast.py [--side 256] [--width 640] [--height 480] [--views 4] [--reps 5] [--out profiles/r23_raycast.json]
The times are device events inside the call, from cba_tsdf_raycast_timed, which only the experiment build exports
(calibration_amd/lib_exp, selected through CALIBBA_LIBRARY) and which also takes the width of a wavefront's pixel block: the median
over --reps after one warm-up call, with the smallest and the largest beside it as the spread, divided by the number of views of the
call.  Samples per ray: the device does not report them; they are counted by the host build of the same header
(tests/raycast_cpu) over the device's rays table for the first view, whose depths the host build must reproduce to the bit.  Byte
floor at the copy rate DESIGN.md measures its kernels against: a view writes 65 B per pixel (depth, xyz, normals, status) and reads
its 16 B ray and, once, the 8 B voxels of every cell a sample touched (counted from the same host run).  No time is fixed in
advance."""
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
from tests import host_build  # noqa: E402
from tests import raycast_ref as RC  # noqa: E402
from tools.bench_fusion import COPY_RATE, render  # noqa: E402


def touched_voxels(vol, rays, pose7, step, skip):
    """distinct voxels in the cells the march's samples of one view touch (the restatement's march with the cells recorded)"""
    seen = np.zeros(vol.D.shape, bool)
    inner = RC.sample

    def recording(v, p, min_weight):
        ok, Fv = inner(v, p, min_weight)
        g = [(p[a] - v.origin[a]) / v.vs for a in range(3)]
        box = np.ones(np.shape(g[0]), bool)
        for a in range(3):
            box &= (g[a] >= 0.0) & (g[a] <= v.shape[a] - 1.0)
        i = [np.minimum(np.floor(np.where(box, g[a], 0.0)), v.shape[a] - 2.0).astype(np.int64)[box] for a in range(3)]
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    seen[i[2] + dz, i[1] + dy, i[0] + dx] = True
        return ok, Fv

    RC.sample = recording
    try:
        RC.cast(vol, rays, pose7, step=step, skip=skip)
    finally:
        RC.sample = inner
    return int(seen.sum())


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
    d = capi.c_double_p
    lib.cba_tsdf_raycast_timed.argtypes = [C.c_void_p, C.c_int32, d, C.c_int32, C.c_int32, C.c_int32, d, C.POINTER(capi.CbaTsdfRaycastOptions),
                                           C.c_int32, d]
    lib.cba_tsdf_raycast_timed.restype = C.c_int32
    host = host_build.load("raycast_cpu")
    W, H, side = a.width, a.height, a.side
    vs = 2.0 / side
    poses = np.array([F.look_at((3.0 * math.cos(t), 3.0 * math.sin(t), 0.6 * math.sin(3 * t)), F.SPHERE_C)
                      for t in np.arange(16) * (2 * math.pi / 16)])
    intr = F.CAMERAS[F.PINHOLE].copy()
    scale = W / F.MAP_W
    intr[:4] = [150.0 * scale, 148.0 * scale, (W - 1) / 2.0, (H - 1) / 2.0]
    x, y = F.pixel_rays(F.PINHOLE, intr, W, H)
    depth = np.ascontiguousarray(np.stack([render(x, y, p) for p in poses]))
    # the views that are cast lie between the fused ones
    views = np.ascontiguousarray(np.array([F.look_at((3.0 * math.cos(t), 3.0 * math.sin(t), 0.4 * math.cos(2 * t)), F.SPHERE_C)
                                           for t in (np.arange(a.views) + 0.5) * (2 * math.pi / 16)]))
    res = {"kind": "raycast", "side": side, "width": W, "height": H, "views": a.views, "reps": a.reps, "voxels": side ** 3, "copy_rate": COPY_RATE}
    ms = np.zeros(2)
    k = np.ascontiguousarray(intr)
    with TsdfVolume((side, side, side), [-1.0, -1.0, -1.0], TsdfOptions(vs, 4 * vs)) as vol:
        vol.integrate(F.PINHOLE, intr, poses, depth=depth)

        def cast(skip, wave_w):
            o = capi.CbaTsdfRaycastOptions(0.0, skip, 0.0, np.inf, 1.0)
            capi.check(lib, lib.cba_tsdf_raycast_timed(vol._h, F.PINHOLE, capi.dptr(k), a.views, H, W, capi.dptr(views), C.byref(o), wave_w,
                                                       capi.dptr(ms)))
            return ms.copy()

        def fetch():
            dep, st, rays = np.empty((a.views, H, W)), np.empty((a.views, H, W), np.uint8), np.empty((H, W, 2))
            capi.check(lib, lib.cba_tsdf_raycast_fetch(vol._h, capi.dptr(dep), capi.dptr(None), capi.dptr(None), capi.u8ptr(st), capi.dptr(rays)))
            return dep, st, rays

        Dv, Wv = vol.fetch()
        ref = F.Volume((side, side, side), [-1.0, -1.0, -1.0], vs, 4 * vs)
        ref.D, ref.W = Dv, Wv
        for skip in (0.0, 0.5):
            row = {}
            for wave_w in (8, 64):
                cast(skip, wave_w)
                t = np.array([cast(skip, wave_w) for _ in range(a.reps)]) / a.views
                row["wave_%dx%d" % (wave_w, 64 // wave_w)] = dict(rays_ms=float(np.median(t[:, 0]) * a.views), cast_ms_per_view=float(np.median(t[:, 1])),
                                                                  min_ms=float(t[:, 1].min()), max_ms=float(t[:, 1].max()))
            dep, st, rays = fetch()
            got = RC.host_cast(host, ref, rays, views[0], skip=skip)
            assert got["depth"].tobytes() == dep[0].tobytes() and got["status"].tobytes() == st[0].tobytes(), "the host build disagrees"
            marched = got["count"][got["count"] > 0]
            hit = got["count"][got["status"] == RC.HIT]
            voxels = touched_voxels(ref, rays, views[0], 0.0, skip)
            floor = 65 * H * W + 16 * H * W + 8 * voxels
            row.update(hits=int((st[0] == RC.HIT).sum()), hits_all_views=int((st == RC.HIT).sum()), rays_in_the_box=int(marched.size),
                       samples_per_marched_ray=float(marched.mean()), samples_per_hit_ray=float(hit.mean()), samples_max=int(got["count"].max()),
                       samples_total=int(got["count"].sum()), touched_voxels=voxels, floor_bytes=floor, floor_ms=floor / COPY_RATE * 1e3)
            res["skip_%g" % skip] = row
            print(f"skip {skip}: 8x8 {row['wave_8x8']['cast_ms_per_view']:.3f} ms per view, 64x1 {row['wave_64x1']['cast_ms_per_view']:.3f} ms; "
                  f"{row['hits']} hits, {row['samples_per_marched_ray']:.1f} samples per marched ray; floor {row['floor_ms']:.4f} ms",
                  file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
