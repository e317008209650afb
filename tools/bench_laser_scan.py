"""Laser profile scanning benchmark: one JSON line with the device time of the scan kernel for batches of 2048 x 1088 frames, both
axes, uint8 and float32, next to its HBM bound.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_laser_scan.py [--width 2048] [--height 1088] [--frames 64] [--reps 5] [--out profiles/r12_laser_scan.json]
Times are device events around the kernel of one call, median over --reps after one warm-up call, from
cba_laser_scanner_process_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through
CALIBBA_LIBRARY); the upload of the frames and the download of the profiles in the same call are reported separately.  The scene is
the test scene (tests/laser_scan_ref.py): a Gaussian line of sigma 2 px on a dark frame, with frame poses.  Bytes counted: W H
sizeof(pixel) read per frame and n_lines 8 (3 + 3) written (xyz, centre, amplitude, width_px); the bound is those bytes at the
6.3 TB/s copy rate.  The window pass re-reads (2 half_window + 1) n_lines samples per frame, which the bound leaves out."""
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
from calibration_amd.capi import dptr  # noqa: E402
from tests import camera_ref as R  # noqa: E402
from tests import laser_scan_ref as S  # noqa: E402

HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    d, i32, vp = capi.c_double_p, C.c_int32, C.c_void_p
    lib.cba_laser_scanner_process_timed.argtypes = [vp, i32, i32, vp, d, d, d, d, d, d]
    lib.cba_laser_scanner_process_timed.restype = i32
    W, H, F = a.width, a.height, a.frames
    res = {"kind": "laser_scan", "width": W, "height": H, "frames": F, "reps": a.reps}
    poses = S.frame_poses(F)
    for axis in (0, 1):
        intr, plane, pos, _, f32, u8 = S.scene(R.PINHOLE, W, H, axis, F)
        n_lines = W if axis == 0 else H
        o = capi.CbaLaserScanOptions()
        lib.cba_laser_scan_options_default(C.byref(o))
        o.axis = axis
        h = vp()
        capi.check(lib, lib.cba_laser_scanner_create(R.PINHOLE, dptr(intr), 0, dptr(None), dptr(np.ascontiguousarray(plane)), W, H, F,
                                                     C.byref(o), 0, C.byref(h)))
        out = [np.empty((F, n_lines)) for _ in range(3)] + [np.empty((F, n_lines, 3))]
        ms = np.zeros(3)
        for tag, img in (("u8", u8), ("f32", f32)):
            dtype = capi.DTYPE_U8 if img.dtype == np.uint8 else capi.DTYPE_F32

            def call():
                capi.check(lib, lib.cba_laser_scanner_process_timed(h, F, dtype, img.ctypes.data_as(vp), dptr(poses), dptr(out[0]), dptr(out[1]),
                                                                    dptr(out[2]), dptr(out[3]), dptr(ms)))
                return ms.copy()
            call()
            med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
            k = float(med[1])
            nbytes = F * (W * H * img.itemsize + n_lines * 8 * 6)
            hbm_ms = nbytes / (HBM_TBPS * 1e12) * 1e3
            print(f"axis {axis} {tag}: kernel {k:.3f} ms for {F} frames, HBM bound {hbm_ms:.3f} ms", file=sys.stderr, flush=True)
            res[f"axis{axis}_{tag}"] = dict(
                upload_ms=float(med[0]), kernel_ms=k, download_ms=float(med[2]), frames_per_s=F / (k * 1e-3), bytes=nbytes,
                hbm_bound_ms=hbm_ms, kernel_over_bound=k / hbm_ms, achieved_tbps=nbytes / (k * 1e-3) / 1e12,
                centre_error_px_max=float(np.nanmax(np.abs(out[0] - pos))), invalid_lines=int(np.isnan(out[0]).sum()))
        lib.cba_laser_scanner_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
