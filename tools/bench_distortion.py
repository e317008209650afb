"""Distortion fit / linear intrinsic seed benchmark: one JSON line with the stage times of cba_fit_distortion_batch (forward and
dual) and cba_estimate_intrinsics_linear_iterative_batch (max_iterations 5 and 500) at one problem of 10^7 observations (one camera
of bench.py's 1000 views x 10 000 points) and at 2000 problems of 88 observations.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_distortion.py [--n 10000000] [--reps 5] [--out FILE]
Stage times are device events between the kernels of one call, median over --reps after one warm-up call, from the *_timed
entry points only the experiment build exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY): the moment passes
(k_df_moments), the chunk sums (k_df_chunk_sum), the uploads (host to device, reported separately and excluded from "device_ms"),
the per-problem tail and the residual pass.  Wall times are whole calls from the host, uploads and downloads included."""
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
from calibration_amd.capi import dptr, i32ptr, i64ptr  # noqa: E402
from tests import distortion_ref as R  # noqa: E402

K0 = np.array([800.0, 820.0, 400.0, 300.0, 0.0])


def _bind(lib):
    f = lib.cba_fit_distortion_batch_timed
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, capi.c_int64_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p,
                  C.c_int32, C.c_int32, capi.c_double_p, capi.c_double_p, capi.c_int32_p, capi.c_double_p, capi.c_double_p]
    g = lib.cba_estimate_intrinsics_linear_iterative_batch_timed
    g.restype = C.c_int32
    g.argtypes = [C.c_int32, capi.c_int64_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, C.c_int32, C.c_int32,
                  C.c_int32, capi.c_double_p, capi.c_double_p, capi.c_int32_p, capi.c_int32_p, capi.c_int32_p, capi.c_double_p]
    return f, g


def _measure(call, reps):
    call()
    stages, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ms = call()
        walls.append(time.perf_counter() - t0)
        stages.append(ms.copy())
    med = np.median(np.array(stages), axis=0)
    return dict(moments_ms=float(med[0]), chunk_sum_ms=float(med[1]), upload_ms=float(med[2]), tail_ms=float(med[3]),
                residuals_ms=float(med[4]), device_ms=float(med[5]), wall_ms=1e3 * float(np.median(walls)))


def run(lib, P, n, reps):
    fit, it = _bind(lib)
    obs = np.concatenate([R.make_scene(n, noise=0.5, seed=p) for p in range(P)]) if P > 1 else R.make_scene(n, noise=0.5, seed=1)
    off = np.arange(P + 1, dtype=np.int64) * n
    x, y, u, v = (np.ascontiguousarray(obs[:, k]) for k in range(4))
    K = np.ascontiguousarray(np.tile(K0, (P, 1)))
    m = 4
    co, inv, ok = np.zeros((P, m)), np.zeros((P, m)), np.zeros(P, np.int32)
    res = np.zeros(2 * P * n)
    Ko, st, its, fb = np.zeros((P, 5)), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    ms = np.zeros(6)
    out = {}

    def fit_call(dual):
        def call():
            capi.check(lib, fit(P, i64ptr(off), dptr(x), dptr(y), dptr(u), dptr(v), dptr(K), 2, 1 if dual else 0, dptr(co),
                                dptr(inv) if dual else dptr(None), i32ptr(ok), dptr(res), dptr(ms)))
            return ms
        return call

    def it_call(mi):
        def call():
            capi.check(lib, it(P, i64ptr(off), dptr(x), dptr(y), dptr(u), dptr(v), 2, mi, 0, dptr(Ko), dptr(co), i32ptr(st), i32ptr(its),
                               i32ptr(fb), dptr(ms)))
            return ms
        return call

    out["fit"] = _measure(fit_call(False), reps)
    out["dual"] = _measure(fit_call(True), reps)
    for mi in (5, 500):
        r = _measure(it_call(mi), reps)
        r["iterations_max"] = int(its.max())
        r["tail_us_per_iteration"] = 1e3 * r["tail_ms"] / max(int(its.max()), 1)
        out[f"iterative_{mi}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    res = {"kind": "distortion_fit", "single": dict(P=1, n=a.n, **run(lib, 1, a.n, a.reps)),
           "batch": dict(P=2000, n=88, **run(lib, 2000, 88, a.reps))}
    # bound of the moment pass at n observations: ~32 B read and ~240 FLOP per observation (nr = 2: fewer)
    mom_s = res["single"]["fit"]["moments_ms"] * 1e-3
    res["single"]["moment_pass_TBps"] = 32.0 * a.n / mom_s / 1e12
    res["single"]["moment_pass_share_of_6.3TBps"] = res["single"]["moment_pass_TBps"] / 6.3
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
