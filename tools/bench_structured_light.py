"""Structured-light decode benchmark: one JSON line with the device time of the decode and points kernels of cba_sl_decoder_process
for a batch of sequences, next to the byte bound of the decode.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_structured_light.py [--width 1920] [--height 1200] [--sequences 2] [--proj-width 1920] [--proj-height 1080]
                                              [--reps 5] [--out profiles/r19_structured_light.json]
Times are device events around the stages of one call: upload, decode, points, download; median over --reps after one warm-up call,
from cba_sl_decoder_process_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through
CALIBBA_LIBRARY).  The input is the test scene's renderer (tests/sl_ref.py) on one image row, repeated down the image: the decode of a
pixel depends on its own samples only.  Run for Gray only (s = 0) and for Gray + phase (s = 3, N = 4, T = 16), each with and without
the modulation output, and with points for the phase case.

The bound: the bytes the decode must move at the 6.3 TB/s copy rate, per pixel - n_images read, 8 n_axes + 1
written, 8 n_axes more with modulation.  No time is fixed in advance: the yardstick is the ratio of measured time to bound."""
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
from tests import camera_ref as R  # noqa: E402
from tests import sl_ref as S  # noqa: E402

COPY_TBS = 6.3
STAGES = ["upload", "decode", "points", "download"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--sequences", type=int, default=2)
    ap.add_argument("--proj-width", type=int, default=1920)
    ap.add_argument("--proj-height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    vp, d = C.c_void_p, capi.c_double_p
    lib.cba_sl_decoder_process_timed.argtypes = [vp, C.c_int32, capi.c_uint8_p, d, d, capi.c_uint8_p, d, d, capi.c_int32_p, d]
    lib.cba_sl_decoder_process_timed.restype = C.c_int32
    W, H, n = a.width, a.height, a.sequences
    px = n * W * H
    res = {"kind": "structured_light", "width": W, "height": H, "sequences": n, "proj_width": a.proj_width, "proj_height": a.proj_height,
           "reps": a.reps, "stages": STAGES, "copy_tbs": COPY_TBS}
    for name, s, N in (("gray", 0, 0), ("gray_phase", 3, 4)):
        o = S.Options(a.proj_width, a.proj_height, 3, s, N, 16)
        row = S.scene(R.PINHOLE, W, 1, o, n_seq=n, seed=0)
        images = np.ascontiguousarray(np.broadcast_to(row["images"], (n, S.image_count(o), H, W)))
        co = capi.CbaSlOptions(o.proj_width, o.proj_height, o.axes, o.s, o.N, o.T, o.min_contrast, o.min_bit_diff, o.min_modulation)
        h = vp()
        capi.check(lib, lib.cba_sl_decoder_create(C.byref(co), W, H, n, 0, C.byref(h)))
        t = capi.CbaTriangulateOptions()
        lib.cba_triangulate_options_default(C.byref(t))
        capi.check(lib, lib.cba_sl_decoder_set_rig(h, R.PINHOLE, capi.dptr(np.ascontiguousarray(row["intr"])), 0, capi.dptr(None),
                                                   capi.dptr(np.ascontiguousarray(row["poses"])), C.byref(t)))
        coord, mod, status = np.empty((n, 2, H, W)), np.empty((n, 2, H, W)), np.empty((n, H, W), np.uint8)
        xyz, rms, ts = np.empty((n, H, W, 3)), np.empty((n, H, W)), np.empty((n, H, W), np.int32)
        ms = np.zeros(len(STAGES))
        forms = [("coord_status", False, False), ("with_modulation", True, False)] + ([("with_points", True, True)] if N else [])
        for form, want_mod, want_points in forms:
            def call():
                capi.check(lib, lib.cba_sl_decoder_process_timed(h, n, capi.u8ptr(images), capi.dptr(coord), capi.dptr(mod if want_mod else None),
                                                                 capi.u8ptr(status), capi.dptr(xyz if want_points else None),
                                                                 capi.dptr(rms if want_points else None), capi.i32ptr(ts if want_points else None),
                                                                 capi.dptr(ms)))
                return ms.copy()
            call()
            med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
            per_px = S.image_count(o) + 8 * 2 + 1 + (8 * 2 if want_mod else 0)
            bound = px * per_px / (COPY_TBS * 1e12) * 1e3
            res[f"{name}_{form}"] = dict(n_images=S.image_count(o), bytes_per_pixel=per_px, decode_ms=float(med[1]), bound_ms=bound,
                                         over_bound=float(med[1]) / bound, points_ms=float(med[2]), upload_ms=float(med[0]),
                                         download_ms=float(med[3]), valid_share=float((status == 0).mean()),
                                         gpixels_per_s=px / (float(med[1]) * 1e-3) / 1e9)
            print(f"{name} {form}: decode {med[1]:.3f} ms for {n} x {W} x {H} x {S.image_count(o)} images, bound {bound:.3f} ms "
                  f"(x{med[1] / bound:.2f}), points {med[2]:.3f} ms", file=sys.stderr, flush=True)
        lib.cba_sl_decoder_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
