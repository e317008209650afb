"""ChArUco detection benchmark: one JSON line with the times of the stages of cba_charuco_detector_process for a batch of images.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_charuco.py [--width 1920] [--height 1080] [--images 16] [--reps 5] [--out profiles/r17_charuco.json]
Method as tools/bench_corners.py: device events round the device stages of one call (upload, response, peaks, refine, arms, read,
download), the steady clock round the two host stages (lattice, match), median over --reps after one warm-up call, from
cba_charuco_detector_process_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through
CALIBBA_LIBRARY).  The arms and read stages include their small upload and download.  The scene is one rendered view of a board
larger than the image (tests/charuco_ref.py, at the size asked for), with fresh pixel noise per image."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CALIBBA_LIBRARY", os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so"))

from calibration_amd import capi, detect  # noqa: E402
from tests import charuco_ref as S  # noqa: E402

STAGES = ["upload", "response", "peaks", "refine", "arms", "host_lattice", "read", "host_match", "download"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--max-corners", type=int, default=4096)
    ap.add_argument("--max-cells", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    vp = C.c_void_p
    lib.cba_charuco_detector_process_timed.argtypes = [vp, C.c_int32, capi.c_uint8_p, capi.c_int32_p, capi.c_int32_p, capi.c_int32_p,
                                                       capi.c_double_p]
    lib.cba_charuco_detector_process_timed.restype = C.c_int32
    W, H, n = a.width, a.height, a.images
    # the camera of the scenes scaled to the size asked for, a 40 x 24 board of 0.01 m squares (about 55 px) hanging over every side
    board = S.make_board(40, 24, bits=5, min_distance=6, square=0.01)
    scale = W / float(S.W_IMG)
    saved = S.CAMERA.copy()
    S.CAMERA[:4] = saved[:4] * scale
    try:
        Rm, t = S.view_pose(board, 1, 1)
        rng = np.random.default_rng(0)
        clean = S.render(board, Rm, t, rng, W, H, ss=2, noise=0.0).astype(np.float64)
    finally:
        S.CAMERA[:] = saved
    images = np.clip(np.rint(clean[None] + 2.0 * rng.standard_normal((n, H, W))), 0, 255).astype(np.uint8)
    b = detect.CharucoBoard(board.squares_x, board.squares_y, board.square, board.codes, board.marker_bits, board.marker_ratio)
    with detect.CharucoDetector(W, H, b, n, a.max_corners, a.max_cells) as d:
        count, nm, cells, ms = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32), np.zeros(9)

        def call():
            capi.check(lib, lib.cba_charuco_detector_process_timed(d._h, n, capi.u8ptr(images), capi.i32ptr(count), capi.i32ptr(nm),
                                                                   capi.i32ptr(cells), capi.dptr(ms)))
            return ms.copy()
        call()
        med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
    res = {"kind": "charuco", "width": W, "height": H, "images": n, "squares": [board.squares_x, board.squares_y], "marker_bits": board.marker_bits,
           "max_corners": a.max_corners, "max_cells": a.max_cells, "reps": a.reps, "corners_per_image": float(count.mean()),
           "markers_per_image": float(nm.mean()), "cells_per_call": int(cells[0])}
    res.update({k + "_ms": float(v) for k, v in zip(STAGES, med)})
    print(", ".join(f"{k} {v:.3f}" for k, v in zip(STAGES, med)), f"ms for {n} images, {count.mean():.0f} corners and {nm.mean():.0f} markers each",
          file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
