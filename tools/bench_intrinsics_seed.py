"""Intrinsic-seed benchmark: one JSON line with the stage times of cba_estimate_intrinsics with RANSAC homographies at one shape
(default 1000 views x 10 000 points x 1000 hypotheses, 20 % outliers), the (hypothesis, point) pairs per second and fp64 rate of
the scoring kernel, and a numpy-on-CPU figure of the same work ("kind": "port", described in its "what" field) for scale.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_intrinsics_seed.py [--views 1000] [--points 10000] [--iters 1000] [--reps 3] [--out FILE]
Stage times are device events between the stages of one call, median over --reps after one warm-up call, from
cba_estimate_intrinsics_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through
CALIBBA_LIBRARY).
FLOP per (hypothesis, point) of k_hr_score, counted from hom_ransac_math.hpp with FMA = 2 and divide / sqrt not counted:
the residual and inlier test (hr_resid_parts + hr_is_inlier) 46; pass 1 adds the count and 4 sums (9) = 55; pass 2 (mean
distances) 46 + 10 = 56; pass 3 (normalisation 8, w = u^2 + v^2 3, 24 moments 42) 46 + 53 = 99; pass 4 (r^2 5, 2 sums) 46 + 7 = 53.
A workgroup runs passes 2 and 3 for all its lanes when any of its lanes refits, so at these shapes every pass runs: 263 in all.
That makes "score_fp64_tflops" an upper bound on issued work, not useful work: lanes that do not refit and the per-inlier parts
that run under an exec mask are counted too.  "pairs_per_s" is the useful figure.
fp64 vector peak of the MI355X: 78.6 TFLOP/s."""
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
from calibration_amd.capi import CbaRansacOptions, dptr, i32ptr, i64ptr  # noqa: E402
from calibration_amd.linear import _flatten  # noqa: E402
from tests import hom_ransac_ref as ref  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
FLOP_PASS1, FLOP_ALL = 55, 263


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--port-views", type=int, default=2, help="views of the numpy baseline (scaled to --views)")
    ap.add_argument("--port-iters", type=int, default=20, help="hypotheses per view of the numpy baseline (scaled to --iters)")
    a = ap.parse_args()

    K = np.array([820.0, 790.0, 640.0, 360.0, 0.0])
    rng = np.random.default_rng(7)
    views = [ref.random_view(rng, K, a.points, outlier_frac=0.2, noise_px=0.3)[0] for _ in range(a.views)]
    off, (X, Y, u, v) = _flatten(views)
    lib = capi.load_library()
    if not hasattr(lib, "cba_estimate_intrinsics_timed"):
        sys.exit(f"{capi.library_path()} has no stage timing: build the experiment library "
                 "(make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp)")
    f = lib.cba_estimate_intrinsics_timed
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, capi.c_int64_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, C.c_int32,
                  C.POINTER(CbaRansacOptions), capi.c_int32_p, capi.c_double_p, capi.c_int32_p, capi.c_double_p, capi.c_double_p,
                  capi.c_double_p, capi.c_int32_p, capi.c_double_p]
    o = CbaRansacOptions()
    lib.cba_ransac_options_default(C.byref(o))
    o.max_iters = a.iters
    nv = a.views
    ok, pok = np.zeros(nv, dtype=np.int32), np.zeros(nv, dtype=np.int32)
    H, rms, rt = np.zeros((nv, 9)), np.zeros(nv), np.zeros((nv, 12))
    Kout, st = np.zeros(5), np.zeros(5)
    success = C.c_int32(0)
    rows, walls = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        capi.check(lib, f(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v), 1, C.byref(o), C.byref(success), dptr(Kout), i32ptr(ok),
                          dptr(H), dptr(rms), dptr(rt), i32ptr(pok), dptr(st)))
        if rep:
            walls.append(time.perf_counter() - t0)
            rows.append(st.copy())
    med = np.median(np.array(rows), axis=0)
    pairs = float(a.views) * a.iters * a.points
    score_s = med[0] * 1e-3
    out = {
        "what": "cba_estimate_intrinsics with RANSAC homographies (device stage times, ms, median)",
        "views": a.views, "points_per_view": a.points, "hypotheses": a.iters, "outliers": 0.2, "reps": a.reps,
        "success": bool(success.value), "views_ok": int(ok.sum()), "poses_ok": int(pok.sum()),
        "stage_ms": {"homography_score": med[0], "homography_select_rms": med[1], "zhang_sanitize": med[2], "poses": med[3],
                     "total": med[4]},
        "call_wall_ms": 1e3 * float(np.median(walls)),
        "pairs_per_s": pairs / score_s,
        "score_flop_per_pair": FLOP_ALL,
        "score_fp64_tflops": FLOP_ALL * pairs / score_s * 1e-12,
        "score_fraction_of_fp64_vector_peak": FLOP_ALL * pairs / score_s / FP64_VECTOR_PEAK,
    }
    # numpy on the host CPU: tests/hom_ransac_ref.py's ransac (the reference's work: residuals of every point per hypothesis, a
    # full SVD refit of every hypothesis above min_inliers) over --port-iters hypotheses of --port-views views, scaled.
    kv, ki = min(a.port_views, a.views), min(a.port_iters, a.iters)
    t0 = time.perf_counter()
    for i in range(kv):
        ref.ransac(views[i], max_iters=ki)
    port = time.perf_counter() - t0
    out["port"] = {"kind": "port", "what": f"numpy ransac (hom_ransac_ref.py) over {kv} views x {ki} hypotheses, scaled linearly to "
                                           f"{a.views} views x {a.iters} hypotheses (not measured at that size)",
                   "measured_s": port, "scaled_s": port * (a.views / kv) * (a.iters / ki)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
