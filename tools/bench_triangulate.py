"""Triangulation benchmark: one JSON line with the device time of k_triangulate for 10^7 points seen by 2, 4 and 8 cameras, both
camera models, 0.3 px noise, next to its two bounds and the per-point iteration statistics.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_triangulate.py [--n 10000000] [--reps 5] [--out FILE]
Times are device events around the kernel of one call, median over --reps after one warm-up call, from cba_triangulate_timed, which
only the experiment build exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY); the uploads and downloads of the same
call are reported separately.  The scene is the test scene's 8-camera rig (tests/triangulate_ref.py); 2 and 4 cameras are its
middle cameras.  Bounds: HBM at the 6.3 TB/s copy rate for 16 C bytes read and 40 bytes written per point (xyz, rms_px, used_mask,
status), and fp64 issue at 39.3 T instructions/s for (measured mean linearisations per point) x C x (fp64 instructions of one
camera's share of a linearisation: 135 pinhole, 160 Scheimpflug by a count of tri_math.hpp, not measured; the seed, the final
statistics and the 3 x 3 solves are not in this bound).  idle_lane_share: over wavefronts of 64 consecutive points,
1 - sum(linearisations) / (64 max(linearisations))."""
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
from calibration_amd.capi import dptr, i32ptr  # noqa: E402
from tests import camera_ref as R  # noqa: E402
from tests import triangulate_ref as T  # noqa: E402

HBM_TBPS = 6.3
FP64_INSTR_PER_S = 78.6e12 / 2
LIN_FP64_INSTR_PER_CAMERA = {R.PINHOLE: 135, R.SCHEIMPFLUG: 160}
RIG = 8


def _scene(model, n, noise):
    intrs, poses, _, _ = T.scene(RIG, 1, model)
    rng = np.random.default_rng(7)
    xyz = np.column_stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.25, 0.25, n), rng.uniform(1.0, 2.0, n)])
    uv = np.empty((RIG, n, 2))
    for c in range(RIG):
        uv[c] = R.project(model, intrs[c], xyz @ T.quat_to_rotmat(poses[c]).T + poses[c][4:])
        uv[c] += noise * rng.standard_normal((n, 2))
    return intrs, poses, xyz, uv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    d, i32 = capi.c_double_p, C.c_int32
    lib.cba_triangulate_timed.argtypes = [i32, i32, d, i32, d, d, C.c_int64, d, C.POINTER(capi.CbaTriangulateOptions), d, d, capi.c_uint32_p,
                                          capi.c_int32_p, d, capi.c_int32_p, d]
    lib.cba_triangulate_timed.restype = i32
    o = capi.CbaTriangulateOptions()
    lib.cba_triangulate_options_default(C.byref(o))
    n = a.n
    xyz, rms, ms = np.empty((n, 3)), np.empty(n), np.zeros(3)
    mask, status, lin = np.empty(n, np.uint32), np.empty(n, np.int32), np.empty(n, np.int32)
    res = {"kind": "triangulate", "n_points": n, "reps": a.reps, "noise_px": a.noise}
    for tag, model in (("pinhole", R.PINHOLE), ("scheimpflug", R.SCHEIMPFLUG)):
        intrs, poses, truth, uv_all = _scene(model, n, a.noise)
        for n_cams in (2, 4, 8):
            lo = (RIG - n_cams) // 2
            ci, cp, uv = np.ascontiguousarray(intrs[lo:lo + n_cams]), np.ascontiguousarray(poses[lo:lo + n_cams]), uv_all[lo:lo + n_cams]

            def call():
                capi.check(lib, lib.cba_triangulate_timed(model, n_cams, dptr(ci), 0, dptr(None), dptr(cp), n, dptr(uv), C.byref(o), dptr(xyz),
                                                          dptr(rms), mask.ctypes.data_as(capi.c_uint32_p), i32ptr(status), dptr(None),
                                                          i32ptr(lin), dptr(ms)))
                return ms.copy()
            call()
            med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
            k = float(med[1])
            lin_mean, lin_max = float(lin.mean()), int(lin.max())
            w = lin[: n - n % 64].reshape(-1, 64)
            idle = float(1.0 - w.sum() / (64.0 * w.max(axis=1).sum())) if w.size else 0.0
            hbm_ms = (16 * n_cams + 40) * n / (HBM_TBPS * 1e12) * 1e3
            fp64_ms = lin_mean * n_cams * LIN_FP64_INSTR_PER_CAMERA[model] * n / FP64_INSTR_PER_S * 1e3
            bound = max(hbm_ms, fp64_ms)
            print(f"{tag} C={n_cams}: kernel {k:.3f} ms, {lin_mean:.2f} linearisations per point", file=sys.stderr, flush=True)
            res[f"{tag}_c{n_cams}"] = dict(
                upload_ms=float(med[0]), kernel_ms=k, download_ms=float(med[2]), points_per_s=n / (k * 1e-3), hbm_bound_ms=hbm_ms,
                fp64_issue_bound_ms=fp64_ms, binding="fp64" if fp64_ms >= hbm_ms else "hbm", kernel_over_bound=k / bound,
                linearisations_mean=lin_mean, linearisations_max=lin_max, idle_lane_share=idle,
                status_counts=[int((status == s).sum()) for s in range(5)], rms_px_mean=float(np.nanmean(rms)),
                rel_error_median=float(np.median(np.linalg.norm(xyz - truth, axis=1) / np.linalg.norm(truth, axis=1))))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
