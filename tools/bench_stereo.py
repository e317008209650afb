"""Stereo matching benchmark: one JSON line with the device time of cba_stereo_matcher_process for a batch of rectified pairs, next
to the instruction-count bound of the matching kernel.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_stereo.py [--width 1280] [--height 720] [--disparities 128] [--half-window 4] [--pairs 8] [--reps 5]
                                    [--out profiles/r13_stereo.json]
Times are device events around the kernels of one call (left matching pass, right pass of the left-right check, finish pass), median
over --reps after one warm-up call, from cba_stereo_matcher_process_timed, which only the experiment build exports
(calibration_amd/lib_exp, selected through CALIBBA_LIBRARY); the upload of the images and the download of disparity, cost and xyz are
reported separately.  The scene is a smooth random texture moved by a third of the disparity range.

The bound: one wavefront evaluates one candidate d of one row for 64 - 2r pixels with VALU_PER_STEP vector
instructions, each issued over 2 cycles, on 256 CUs x 4 SIMDs at 2.4 GHz; the left-right check runs the matching pass twice.  No
time is fixed in advance: the yardstick is the ratio of the measured kernel time to this bound."""
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
from tests import stereo_ref as S  # noqa: E402

VALU_PER_STEP = 38  # vector instructions of the d loop's body in k_stereo_match<false> (counted in the gfx950 assembly)
SIMDS, GHZ, ISSUE_CYCLES = 256 * 4, 2.4, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--half-window", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    lib.cba_stereo_matcher_process_timed.argtypes = [vp, C.c_int32, capi.c_uint8_p, capi.c_uint8_p, fp, capi.c_int32_p, fp, capi.c_double_p]
    lib.cba_stereo_matcher_process_timed.restype = C.c_int32
    W, H, D, r, n = a.width, a.height, a.disparities, a.half_window, a.pairs
    rng = np.random.default_rng(0)
    shift = D // 3
    T = S.smooth_noise(rng, H, W + shift)
    q = lambda I: np.ascontiguousarray(np.broadcast_to(np.clip(np.rint(I), 0, 255).astype(np.uint8), (n, H, W)))
    left, right = q(T[:, :W]), q(T[:, shift:shift + W])
    res = {"kind": "stereo", "width": W, "height": H, "num_disparities": D, "half_window": r, "pairs": n, "reps": a.reps,
           "valu_per_step": VALU_PER_STEP}
    geom = capi.CbaStereoGeometry(1000.0, (W - 1) / 2, (H - 1) / 2, 0.1)
    disp, cost, xyz = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.int32), np.empty((n, H, W, 3), np.float32)
    ms = np.zeros(3)
    for tag, lr in (("lr_off", -1), ("lr_on", 1)):
        o = capi.CbaStereoMatchOptions(0, D, r, 10, lr, 1)
        h = vp()
        capi.check(lib, lib.cba_stereo_matcher_create(W, H, n, C.byref(o), C.byref(geom), capi.dptr(None), 0, C.byref(h)))

        def call():
            capi.check(lib, lib.cba_stereo_matcher_process_timed(h, n, capi.u8ptr(left), capi.u8ptr(right), disp.ctypes.data_as(fp),
                                                                 capi.i32ptr(cost), xyz.ctypes.data_as(fp), capi.dptr(ms)))
            return ms.copy()
        call()
        med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
        lib.cba_stereo_matcher_destroy(h)
        k = float(med[1])
        steps = n * (H - 2 * r) * D * -(-W // (64 - 2 * r)) * (2 if lr >= 0 else 1)  # wavefront x row x candidate
        bound_ms = steps * VALU_PER_STEP * ISSUE_CYCLES / (SIMDS * GHZ * 1e9) * 1e3
        inner = disp[:, r:H - r, D + r:W - r]
        print(f"{tag}: kernels {k:.3f} ms for {n} pairs, instruction bound {bound_ms:.3f} ms", file=sys.stderr, flush=True)
        res[tag] = dict(upload_ms=float(med[0]), kernel_ms=k, download_ms=float(med[2]), pairs_per_s=n / (k * 1e-3), bound_ms=bound_ms,
                        kernel_over_bound=k / bound_ms, valid_share=float(np.isfinite(inner).mean()),
                        error_px_max=float(np.nanmax(np.abs(inner - shift))))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
