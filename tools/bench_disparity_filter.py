"""Disparity filter benchmark: one JSON line with the device time of every kernel of cba_disparity_filter_process for a batch of maps,
next to the byte bound of each.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_disparity_filter.py [--width 1280] [--height 720] [--maps 8] [--islands 0.02] [--holes 0.1] [--reps 5]
                                              [--out profiles/r16_disparity_filter.json]
Times are device events around the kernels of one call: median, local labels, merge, flatten, sizes, apply; median over --reps after
one warm-up call, from cba_disparity_filter_process_timed, which only the experiment build exports (calibration_amd/lib_exp, selected
through CALIBBA_LIBRARY).  The input is a slanted plane (one large component per map at speckle_max_diff = 1) with a share --holes of
NaN pixels and a share --islands of pixels in planted 3 x 3 islands 10 px off the plane.  Run for median_half 1 and 2.

The bounds: the bytes a stage must move at the 6.3 TB/s copy rate, per pixel - median 8 (read the map, write
med), local labels 12 (read med, write label and size), merge 8 per pixel on a tile edge (its value and its neighbour's; 39 of 256
pixels), flatten 8 (read and write a label), sizes 4 (read a label), apply 16 (read med, label and size, write the map).  The atomics
and the dependent loads of the union-find are what the ratio to the bound shows.  No time is fixed in advance: the yardstick is the
ratio of measured time to bound, and the share of the SGM kernel time of the same batch (README: 10.2 ms for 8 pairs, 8 paths)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CALIBBA_LIBRARY", os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so"))

from calibration_amd import capi  # noqa: E402

COPY_TBS, SGM_KERNEL_MS = 6.3, 10.2
STAGES = ["median", "local", "merge", "flatten", "sizes", "apply"]
TW, TH = 32, 8
BYTES = {"median": 8.0, "local": 12.0, "merge": 8.0 * (TW + TH - 1) / (TW * TH), "flatten": 8.0, "sizes": 4.0, "apply": 16.0}


def scene(n, H, W, islands, holes, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.indices((H, W))
    a = np.broadcast_to((20 + 0.01 * xx + 0.005 * yy).astype(np.float32), (n, H, W)).copy()
    k = int(islands * n * H * W / 9)
    for i, y, x in zip(rng.integers(0, n, k), rng.integers(0, H - 3, k), rng.integers(0, W - 3, k)):
        a[i, y:y + 3, x:x + 3] += 10.0
    a[rng.random((n, H, W)) < holes] = np.nan
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--islands", type=float, default=0.02)
    ap.add_argument("--holes", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    lib.cba_disparity_filter_process_timed.argtypes = [vp, C.c_int32, fp, fp, capi.c_int64_p, capi.c_double_p]
    lib.cba_disparity_filter_process_timed.restype = C.c_int32
    W, H, n = a.width, a.height, a.maps
    maps = scene(n, H, W, a.islands, a.holes)
    out, stats, ms = np.empty_like(maps), np.zeros((n, 3), np.int64), np.zeros(len(STAGES))
    px = n * W * H
    bound = {s: px * b / (COPY_TBS * 1e12) * 1e3 for s, b in BYTES.items()}
    res = {"kind": "disparity_filter", "width": W, "height": H, "maps": n, "islands": a.islands, "holes": a.holes, "reps": a.reps,
           "speckle_max_size": 100, "speckle_max_diff": 1.0, "stages": STAGES}
    for m in (1, 2):
        o = capi.CbaDisparityFilterOptions(m, 100, 1.0)
        h = vp()
        capi.check(lib, lib.cba_disparity_filter_create(W, H, n, C.byref(o), 0, C.byref(h)))

        def call():
            capi.check(lib, lib.cba_disparity_filter_process_timed(h, n, maps.ctypes.data_as(fp), out.ctypes.data_as(fp), capi.i64ptr(stats),
                                                                   capi.dptr(ms)))
            return ms.copy()
        call()
        med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
        lib.cba_disparity_filter_destroy(h)
        kernel = float(med.sum())
        stages = {s: dict(ms=float(t), bound_ms=bound[s], over_bound=float(t) / bound[s]) for s, t in zip(STAGES, med)}
        print(f"median_half {m}: kernels {kernel:.3f} ms for {n} maps, bounds sum {sum(bound.values()):.3f} ms, "
              f"{kernel / SGM_KERNEL_MS:.3f} of the SGM kernel time", file=sys.stderr, flush=True)
        for s in STAGES:
            print(f"  {s:8s} {stages[s]['ms']:9.3f} ms  bound {bound[s]:7.3f}  x{stages[s]['over_bound']:.1f}", file=sys.stderr)
        res[f"median_half{m}"] = dict(stages=stages, kernel_ms=kernel, bound_ms=sum(bound.values()), kernel_over_bound=kernel / sum(bound.values()),
                                      share_of_sgm_kernel_time=kernel / SGM_KERNEL_MS, maps_per_s=n / (kernel * 1e-3),
                                      valid_in=int(stats[:, 0].sum()), components_removed=int(stats[:, 1].sum()),
                                      pixels_removed=int(stats[:, 2].sum()), valid_out=int(np.isfinite(out).sum()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
