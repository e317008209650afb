"""Semi-global matching benchmark: one JSON line with the device time of every stage of cba_sgm_matcher_process for a batch of rectified
pairs, next to the byte bound of each stage and the issue bound of the path kernel.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_sgm.py [--width 1280] [--height 720] [--disparities 128] [--pairs 8] [--reps 5] [--out profiles/r15_sgm.json]
Times are device events around the kernels of one call: census, cost, each path launch in the order of the rule, selection (left
pass, right-map pass, finish kernel), summed over the groups of pairs the workspace budget allows; median over --reps after one
warm-up call, from cba_sgm_matcher_process_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through
CALIBBA_LIBRARY).  The upload of the images and the download of disparity, cost and xyz are reported separately.  The scene is a smooth
random texture moved by a third of the disparity range.  Run for 4 and 8 paths.

The bounds.  Bytes: every stage's volume traffic at the 6.3 TB/s copy rate - the cost kernel writes C (Dp
bytes per pixel), a path launch reads C and reads and writes S (2 Dp bytes per pixel each; the first launch only writes), selection
reads S once per pass.  The census moves few bytes: its bound is the larger of its vector issue and of its 126 byte loads per pixel
at 16 cycles per wavefront load and CU (an estimate: four lanes per cycle).  Issue of a path launch: one wavefront step serves one
pixel of four lines with VALU_PER_STEP vector instructions, each issued over 2 cycles, on 256 CUs x 4 SIMDs at 2.4 GHz.  No time is
fixed in advance: the yardstick is the ratio of measured time to bound."""
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

# vector instructions of one step of k_sgm_path<KP>: a quarter of the block that steps four pixels, counted in the gfx950 assembly
VALU_PER_STEP = {1: 36, 2: 50, 4: 78, 8: 134}
CENSUS_VALU, CENSUS_LOADS, LOAD_CYCLES = 1239, 126, 16  # per pixel, both images; cycles a wavefront's byte load holds the CU's load unit
SIMDS, GHZ, ISSUE_CYCLES, COPY_TBS = 256 * 4, 2.4, 2, 6.3
STAGES = ["upload", "census", "cost"] + [f"path{r}" for r in range(8)] + ["select", "download"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    lib.cba_sgm_matcher_process_timed.argtypes = [vp, C.c_int32, capi.c_uint8_p, capi.c_uint8_p, fp, capi.c_int32_p, fp, capi.c_double_p]
    lib.cba_sgm_matcher_process_timed.restype = C.c_int32
    W, H, D, n = a.width, a.height, a.disparities, a.pairs
    KP = 1 if D <= 32 else 2 if D <= 64 else 4 if D <= 128 else 8
    Dp = 32 * KP
    rng = np.random.default_rng(0)
    shift = D // 3
    T = S.smooth_noise(rng, H, W + shift)
    q = lambda I: np.ascontiguousarray(np.broadcast_to(np.clip(np.rint(I), 0, 255).astype(np.uint8), (n, H, W)))
    left, right = q(T[:, :W]), q(T[:, shift:shift + W])
    res = {"kind": "sgm", "width": W, "height": H, "num_disparities": D, "padded_disparities": Dp, "pairs": n, "reps": a.reps,
           "valu_per_step": VALU_PER_STEP[KP], "stages": STAGES}
    geom = capi.CbaStereoGeometry(1000.0, (W - 1) / 2, (H - 1) / 2, 0.1)
    disp, cost, xyz = np.empty((n, H, W), np.float32), np.empty((n, H, W), np.int32), np.empty((n, H, W, 3), np.float32)
    ms = np.zeros(len(STAGES))
    px = n * W * H
    ms_of = lambda nbytes: nbytes / (COPY_TBS * 1e12) * 1e3
    issue_ms = (px / 4) * VALU_PER_STEP[KP] * ISSUE_CYCLES / (SIMDS * GHZ * 1e9) * 1e3
    for paths in (4, 8):
        o = capi.CbaSgmOptions(0, D, 4, 32, paths, 10, 1, 1, 0)
        h = vp()
        capi.check(lib, lib.cba_sgm_matcher_create(W, H, n, C.byref(o), C.byref(geom), capi.dptr(None), 0, C.byref(h)))

        def call():
            capi.check(lib, lib.cba_sgm_matcher_process_timed(h, n, capi.u8ptr(left), capi.u8ptr(right), disp.ctypes.data_as(fp),
                                                              capi.i32ptr(cost), xyz.ctypes.data_as(fp), capi.dptr(ms)))
            return ms.copy()
        call()
        med = np.median(np.array([call() for _ in range(a.reps)]), axis=0)
        lib.cba_sgm_matcher_destroy(h)
        census_ms = (px / 64) * max(CENSUS_VALU * ISSUE_CYCLES / SIMDS, CENSUS_LOADS * LOAD_CYCLES / 256) / (GHZ * 1e9) * 1e3
        bound = {"census": max(ms_of(px * (2 + 16)), census_ms), "cost": ms_of(px * (16 + Dp)),
                 "select": ms_of(px * (2 * 2 * Dp + 4 + 4 + 2 + 2 + 2 * 4 + 12))}
        for r in range(paths):
            bound[f"path{r}"] = max(ms_of(px * Dp * (3 if r == 0 else 5)), issue_ms)
        kernel = float(med[1:-1].sum())
        stages = {s: dict(ms=float(t), bound_ms=bound.get(s), over_bound=(float(t) / bound[s] if s in bound else None)) for s, t in zip(STAGES, med)}
        inner = disp[:, 4:H - 4, D + 4:W - 4]
        print(f"paths {paths}: kernels {kernel:.3f} ms for {n} pairs, bounds sum {sum(bound.values()):.3f} ms (path issue bound {issue_ms:.3f} ms)",
              file=sys.stderr, flush=True)
        for s in STAGES:
            print(f"  {s:9s} {stages[s]['ms']:9.3f} ms" + (f"  bound {bound[s]:7.3f}  x{stages[s]['over_bound']:.1f}" if s in bound else ""), file=sys.stderr)
        res[f"paths{paths}"] = dict(stages=stages, kernel_ms=kernel, bound_ms=sum(bound.values()), kernel_over_bound=kernel / sum(bound.values()),
                                    path_issue_bound_ms=issue_ms, pairs_per_s=n / (kernel * 1e-3), valid_share=float(np.isfinite(inner).mean()),
                                    error_px_max=float(np.nanmax(np.abs(inner - shift))))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
