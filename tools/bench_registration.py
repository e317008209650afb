"""Scan-registration benchmark: one JSON line with the time of the index build, of cba_cloud_nearest and of one ICP iteration (one
evaluation of the system and one step) for a batch of sources against one target, next to the bytes each kernel must touch.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_registration.py [--width 640] [--height 480] [--target-maps 4] [--sources 8] [--reps 5]
                                          [--out profiles/r20_registration.json]
The scene is the test scenes' surface (tests/cloud_ref.py) at scan size: the target is --target-maps organised maps of one surface
on grids shifted by fractions of a pixel, each source one more such map moved by a small pose; max_distance is three sample
spacings and cell_size max_distance / 0.999.  Index build, normals and nearest are host wall-clock times of the whole call (upload,
kernels, download; median over --reps after one warm-up call): the kernels' own times come from a rocprofv3 --kernel-trace --stats run
of this tool.  The ICP rounds are device events inside the call, from cba_cloud_register_timed, which only the experiment build
exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY): max_iterations = 0 is one evaluation and one step, max_iterations
= 1 two of each.  No time is fixed in advance."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CALIBBA_LIBRARY", os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so"))

from calibration_amd import capi  # noqa: E402
from calibration_amd.registration import CloudIndex, IcpOptions, default_cell_size, point_normals  # noqa: E402
from tests import cloud_ref as R  # noqa: E402


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--target-maps", type=int, default=4)
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    d, p64 = capi.c_double_p, capi.c_int64_p
    lib.cba_cloud_register_timed.argtypes = [C.c_void_p, C.c_int32, p64, d, d, C.POINTER(capi.CbaIcpOptions), C.POINTER(capi.CbaIcpResult), d]
    lib.cba_cloud_register_timed.restype = C.c_int32
    W, H = a.width, a.height
    focal = 1.25 * W
    md = 3.0 / focal
    cell = default_cell_size(md)
    maps = np.stack([R.surface_map(W, H, 1, focal=focal, shift=(0.25 * k, 0.5 * (k % 2))) for k in range(a.target_maps)])
    truth = R.pose_from_rotvec([0.001, -0.0015, 0.001], [0.0008, -0.0006, 0.0005])
    inv = R.pose_inverse(truth)
    sources = [R.transform(R.rotation(inv[:4]), inv[4:], R.surface_map(W, H, 1, focal=focal, shift=(0.1 + 0.11 * k, -0.07 * k))).reshape(-1, 3)
               for k in range(a.sources)]
    n, m = maps.size // 3, sum(s.shape[0] for s in sources)
    res = {"kind": "registration", "width": W, "height": H, "target_maps": a.target_maps, "sources": a.sources, "reps": a.reps,
           "target_points": n, "source_points": m, "max_distance": md, "cell_size": cell}
    res["normals_call_ms"] = median_ms(lambda: point_normals(maps), a.reps)
    normals = point_normals(maps)

    def build():
        CloudIndex(maps, normals, cell).close()
    res["index_create_call_ms"] = median_ms(build, a.reps)
    queries = np.ascontiguousarray(np.concatenate(sources))
    with CloudIndex(maps, normals, cell) as index:
        ext = maps.reshape(-1, 3).max(0) - maps.reshape(-1, 3).min(0)
        n_cells = int(np.prod(np.floor(ext / cell) + 1))
        res["cells"] = n_cells
        res["nearest_call_ms"] = median_ms(lambda: index.nearest(queries, md), a.reps)
        found = index.nearest(queries, md)[0]
        res["nearest_found_share"] = float((found >= 0).mean())
        off = np.zeros(a.sources + 1, np.int64)
        off[1:] = np.cumsum([s.shape[0] for s in sources])
        out = (capi.CbaIcpResult * a.sources)()
        ms = np.zeros(3)
        for metric, name in ((0, "plane"), (1, "point")):
            for iters in (0, 1):
                co = IcpOptions(md, metric=metric, max_iterations=iters, step_tolerance=1e-12)._c()

                def call():
                    capi.check(lib, lib.cba_cloud_register_timed(index._h, a.sources, capi.i64ptr(off), capi.dptr(queries), capi.dptr(None),
                                                                 C.byref(co), out, capi.dptr(ms)))
                    return ms.copy()
                call()
                med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
                res[f"icp_{name}_rounds{iters + 1}"] = dict(upload_ms=float(med[0]), rounds_ms=float(med[1]), download_ms=float(med[2]),
                                                            pairs=int(sum(r.n_pairs for r in out)), rms=float(out[0].rms))
                print(f"{name}, {iters + 1} round(s): {med[1]:.3f} ms for {a.sources} x {W} x {H} points, {sum(r.n_pairs for r in out)} pairs",
                      file=sys.stderr, flush=True)
            res[f"icp_{name}_round_ms"] = res[f"icp_{name}_rounds2"]["rounds_ms"] - res[f"icp_{name}_rounds1"]["rounds_ms"]
    # the bytes each kernel must touch (fp64 coordinates; a record is 32 bytes; counts and starts are int32)
    res["bytes"] = dict(normals=48 * n, count=24 * n + 4 * n + 4 * n, scan=8 * n_cells, scatter=24 * n + 24 * n + 4 * n + 32 * n + 24 * n,
                        nearest_least=24 * m + 16 * m + 32 * m, accumulate_least=24 * m + 32 * m + 24 * m)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
