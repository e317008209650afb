"""Chessboard corner detection benchmark: one JSON line with the device times of the stages of cba_corner_detector_process for a
batch of images, next to the bytes and instruction bounds of the response pass.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_corners.py [--width 1920] [--height 1080] [--images 16] [--square 40] [--reps 5]
                                     [--out profiles/r14_corners.json]
Times are device events around the stages of one call (upload, response, peaks, refine, download), median over --reps after one
warm-up call, from cba_corner_detector_process_timed, which only the experiment build exports (calibration_amd/lib_exp, selected
through CALIBBA_LIBRARY).  The scene is an axis-aligned periodic chessboard with pixel noise, so every image holds
(width / square) x (height / square) corners.

The bounds of the response pass: bytes = 1 read + 2 written per pixel at the 6.3 TB/s copy rate (the halo is
re-read from cache); instructions = VALU_PER_WAVE vector instructions per wavefront of 256 pixels, each issued over 2 cycles, on
256 CUs x 4 SIMDs at 2.4 GHz.  No time is fixed in advance: the yardstick is the ratio of the measured time to the larger bound."""
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
from tests import corner_ref as S  # noqa: E402

VALU_PER_WAVE = 291  # vector instructions of k_corner_response after the staging barrier (counted in the gfx950 assembly)
SIMDS, GHZ, ISSUE_CYCLES, COPY_TBS = 256 * 4, 2.4, 2, 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--square", type=int, default=40)
    ap.add_argument("--max-corners", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    vp = C.c_void_p
    lib.cba_corner_detector_process_timed.argtypes = [vp, C.c_int32, capi.c_uint8_p, capi.c_int32_p, capi.c_int32_p, capi.c_double_p,
                                                      capi.c_double_p, capi.c_int32_p, capi.c_int32_p, capi.c_double_p]
    lib.cba_corner_detector_process_timed.restype = C.c_int32
    W, H, n, m = a.width, a.height, a.images, a.max_corners
    rng = np.random.default_rng(0)
    board = S.checker(H, W, a.square, 3, 5).astype(np.float64)
    images = np.clip(np.rint(board[None] + 2.0 * rng.standard_normal((n, H, W))), 0, 255).astype(np.uint8)
    res = {"kind": "corners", "width": W, "height": H, "images": n, "square": a.square, "max_corners": m, "reps": a.reps,
           "valu_per_wave": VALU_PER_WAVE}
    px = n * W * H
    bytes_ms = 3.0 * px / (COPY_TBS * 1e12) * 1e3
    instr_ms = px / 256.0 * VALU_PER_WAVE * ISSUE_CYCLES / (SIMDS * GHZ * 1e9) * 1e3
    count, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xy, angle = np.empty((n, m, 2)), np.empty((n, m))
    response, flags = np.empty((n, m), np.int32), np.empty((n, m), np.int32)
    ms = np.zeros(5)
    for tag, refine in (("none", 0), ("cog", 1), ("gradient", 2)):
        o = capi.CbaCornerOptions(400, 3, 2, refine, 5, 5)
        h = vp()
        capi.check(lib, lib.cba_corner_detector_create(W, H, n, m, C.byref(o), 0, C.byref(h)))

        def call():
            capi.check(lib, lib.cba_corner_detector_process_timed(h, n, capi.u8ptr(images), capi.i32ptr(count), capi.i32ptr(status),
                                                                  capi.dptr(xy), capi.dptr(angle), capi.i32ptr(response),
                                                                  capi.i32ptr(flags), capi.dptr(ms)))
            return ms.copy()
        call()
        med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
        lib.cba_corner_detector_destroy(h)
        print(f"{tag}: response {med[1]:.3f} ms (bounds: bytes {bytes_ms:.3f}, instructions {instr_ms:.3f}), peaks {med[2]:.3f} ms, "
              f"refine {med[3]:.3f} ms for {n} images, {int(count.mean())} corners each", file=sys.stderr, flush=True)
        res[tag] = dict(upload_ms=float(med[0]), response_ms=float(med[1]), peaks_ms=float(med[2]), refine_ms=float(med[3]),
                        download_ms=float(med[4]), images_per_s=n / (float(med[1] + med[2] + med[3]) * 1e-3),
                        response_bytes_bound_ms=bytes_ms, response_instruction_bound_ms=instr_ms,
                        response_over_bound=float(med[1]) / max(bytes_ms, instr_ms), corners_per_image=float(count.mean()),
                        overflow=int(status.sum()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
