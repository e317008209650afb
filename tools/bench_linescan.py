"""Laser-plane calibration benchmark: one JSON line with the stage times of cba_calibrate_laser_plane at one shape
(default 1000 views x 4096 laser pixels), the scoring kernel's achieved fp64 rate, the point pass's bytes per second, and a
numpy-on-CPU figure of the same work ("kind": "port", described in its "what" field) for scale.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_linescan.py [--views 1000] [--pixels 4096] [--iters 1000] [--reps 5] [--out FILE]
Stage times are device events between the stages of one call, median over --reps after one warm-up call.  They come from
cba_calibrate_laser_plane_timed, which only the experiment build exports (calibration_amd/lib_exp, selected here through
CALIBBA_LIBRARY); it runs the shipped code path with events recorded between the stages.
FLOP of scoring pass 1 per (hypothesis, point): r = n.q + d (3 FMA), the inlier count and the 9 moments
(4 add + 6 FMA) = 22 with FMA = 2.  fp64 vector peak of the MI355X: 78.6 TFLOP/s."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_exp_lib = os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so")
os.environ.setdefault("CALIBBA_LIBRARY", _exp_lib)

from calibration_amd import capi  # noqa: E402
from calibration_amd.capi import CbaLaserPlaneResult, dptr, i64ptr  # noqa: E402
from calibration_amd.linescan import LineScanPlaneFitOptions, LineScanView, RansacOptions, _flatten, _options  # noqa: E402
from tests import linescan_ref as ref  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
FLOP_PASS1, FLOP_PASS2 = 22, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--pixels", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--port-views", type=int, default=100, help="views of the numpy baseline (scaled to --views)")
    a = ap.parse_args()

    intr = np.array([800.0, 790.0, 640.0, 400.0, 0.5, -0.12, 0.03, -0.002, 0.0008, -0.0005])
    n_true = np.array([0.1, 1.0, -0.1]) / np.linalg.norm([0.1, 1.0, -0.1])
    rng = np.random.default_rng(7)
    pairs = ref.random_scene(rng, a.views, intr, n_true, 0.05, noise_px=0.1, n_samples=a.pixels)
    views = [LineScanView(tv, lv) for tv, lv in pairs]
    toff, loff, (X, Y, u, v, lu, lv) = _flatten(views)
    n = int(loff[-1])
    lib = capi.load_library()
    if not hasattr(lib, "cba_calibrate_laser_plane_timed"):
        sys.exit(f"{capi.library_path()} has no stage timing: build the experiment library "
                 "(make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp)")
    lib.cba_calibrate_laser_plane_timed.restype = C.c_int32
    lib.cba_calibrate_laser_plane_timed.argtypes = [
        C.c_int32, capi.c_double_p, C.c_int32, capi.c_double_p, C.c_int32, capi.c_int64_p, capi.c_double_p, capi.c_double_p, capi.c_double_p,
        capi.c_double_p, capi.c_int64_p, capi.c_double_p, capi.c_double_p, C.POINTER(capi.CbaPlaneFitOptions), C.POINTER(CbaLaserPlaneResult),
        capi.c_double_p]

    def run(opts):
        o = _options(opts)
        res = CbaLaserPlaneResult()
        ms = np.zeros(5)
        capi.check(lib, lib.cba_calibrate_laser_plane_timed(0, dptr(intr), 0, dptr(None), len(views), i64ptr(toff), dptr(X), dptr(Y), dptr(u),
                                                            dptr(v), i64ptr(loff), dptr(lu), dptr(lv), C.byref(o), C.byref(res), dptr(ms)))
        return ms, res

    def timed(opts):
        run(opts)
        t, walls = [], []
        for _ in range(a.reps):
            w0 = time.perf_counter()
            ms, res = run(opts)
            walls.append(1e3 * (time.perf_counter() - w0))
            t.append(ms)
        return np.median(np.array(t), axis=0), float(np.median(walls)), res

    svd_ms, svd_wall, svd_res = timed(LineScanPlaneFitOptions(False))
    ropt = LineScanPlaneFitOptions(True, RansacOptions(max_iters=a.iters, thresh=2e-3))
    rs_ms, rs_wall, rs_res = timed(ropt)

    H = a.iters
    s1 = rs_ms[3] * 1e-3
    rate1 = FLOP_PASS1 * H * n / s1 if s1 > 0 else 0.0
    pts_bytes = n * (16 + 24)  # read u, v; write the compact x, y, z
    out = {
        "tool": "bench_linescan", "library": os.path.relpath(capi.library_path(), ROOT),
        "shape": {"views": a.views, "laser_pixels_per_view": a.pixels, "points": n, "ransac_hypotheses": H},
        "svd": {"views_ms": svd_ms[0], "points_ms": svd_ms[1], "fit_ms": svd_ms[2], "call_wall_ms": svd_wall,
                "plane": list(svd_res.plane), "rms": svd_res.rms_error},
        "ransac": {"views_ms": rs_ms[0], "points_ms": rs_ms[1], "fit_ms": rs_ms[2], "score_pass1_ms": rs_ms[3], "score_pass2_ms": rs_ms[4],
                   "call_wall_ms": rs_wall, "inliers": rs_res.inlier_count, "plane": list(rs_res.plane)},
        "score_pass1_fp64_tflops": rate1 * 1e-12,
        "score_pass1_fraction_of_fp64_vector_peak": rate1 / FP64_VECTOR_PEAK,
        "score_pass2_fp64_tflops": FLOP_PASS2 * H * n / (rs_ms[4] * 1e-3) * 1e-12 if rs_ms[4] > 0 else 0.0,
        "points_pass_GBps": pts_bytes / (svd_ms[1] * 1e-3) * 1e-9 if svd_ms[1] > 0 else 0.0,
    }
    # numpy on the host CPU.  svd_ms: tests/linescan_ref.py's points_from_view + fit_plane_svd over --port-views views, scaled
    # to --views.  ransac_score_pass1_ms: an inline numpy loop (residuals, inlier selection, first and second moments of the
    # inliers) for 20 random planes over the --port-views views' points tiled to --views views, scaled to --iters hypotheses.
    k = min(a.port_views, a.views)
    t0 = time.perf_counter()
    pts = [ref.points_from_view(tv, lv, intr) for tv, lv in pairs[:k]]
    allp = np.concatenate(pts)
    ref.fit_plane_svd(allp)
    t_svd = (time.perf_counter() - t0) * a.views / k
    allp_full = np.tile(allp, (a.views // k, 1))
    t0 = time.perf_counter()
    q = allp_full - allp_full.mean(axis=0)
    for h in range(20):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        r = q @ nrm
        m = np.abs(r) <= 2e-3
        qi = q[m]
        qi.sum(axis=0), qi.T @ qi
    t_rs = (time.perf_counter() - t0) * H / 20
    out["port"] = {"kind": "port",
                   "what": (f"numpy on the host CPU. svd_ms: tests/linescan_ref.py points_from_view + fit_plane_svd over {k} views, scaled "
                            f"to {a.views}. ransac_score_pass1_ms: inline numpy scoring loop (residual, inlier select, first and second "
                            f"moments) of 20 random planes over those points tiled to {a.views} views, scaled to {H} hypotheses"),
                   "svd_ms": 1e3 * t_svd, "ransac_score_pass1_ms": 1e3 * t_rs}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
