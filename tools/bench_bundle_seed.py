"""Hand-eye / bundle seed benchmark: one JSON line with the stage times of cba_estimate_bundle_seed at the C4 shape (2000 robot poses x
4 cameras x 88 points, tests/synth.scene_bundle) and at 2000 x 8, the pair rate of the two Tsai-Lenz passes, the target scan's time
per candidate, and the wall time of the path the call replaces: per camera, cba_estimate_planar_pose_batch over the camera's blocks and
cba_estimate_handeye_dlt over its poses (two passes with a host round trip and a host solve between them).  That path does not
include the initial target, which callers computed in numpy.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_bundle_seed.py [--poses 2000] [--cams 4 8] [--reps 5] [--out FILE]
Stage times are device events between the kernels of one call (uploads excluded), median over --reps after one warm-up call, from
cba_estimate_bundle_seed_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY).
Wall times are whole calls from the host, uploads and host work included, median over --reps after one warm-up."""
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
from calibration_amd.geometry import pose_from_matrix  # noqa: E402
from tests import synth  # noqa: E402


def _median_wall(fn, reps):
    fn()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(walls))


def run_shape(lib, n_poses, n_cams, reps):
    sc = synth.scene_bundle(n_poses, n_cams, noise_px=0.2, seed=2024)
    f = sc.flat
    K = np.ascontiguousarray(sc.gt_intr[:, :5])
    fn = lib.cba_estimate_bundle_seed_timed
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, capi.c_int64_p, capi.c_int32_p, capi.c_double_p, capi.c_double_p, capi.c_double_p,
                   capi.c_double_p, capi.c_double_p, capi.c_double_p, C.c_double, capi.c_double_p, capi.c_int32_p, capi.c_int32_p,
                   capi.c_double_p, capi.c_int32_p, capi.c_double_p]
    g, st, pr = np.zeros((n_cams, 7)), np.zeros(n_cams, np.int32), np.zeros(n_cams, np.int32)
    bt, src, ms = np.zeros(7), np.zeros(1, np.int32), np.zeros(6)
    btg = np.ascontiguousarray(f.blk_b_T_g)

    def batched():
        capi.check(lib, fn(n_cams, f.n_blocks, i64ptr(f.blk_offset), i32ptr(f.blk_cam), dptr(btg), dptr(f.X), dptr(f.Y), dptr(f.u),
                           dptr(f.v), dptr(K), 1.0, dptr(g), i32ptr(st), i32ptr(pr), dptr(bt), i32ptr(src), dptr(ms)))

    batched()
    rows = []
    for _ in range(reps):
        batched()
        rows.append(ms.copy())
    med = np.median(np.array(rows), axis=0)
    wall_batched = _median_wall(batched, reps)
    assert list(st) == [capi.HANDEYE_DLT] * n_cams and src[0] == capi.TARGET_ESTIMATED

    # the path this replaces: per camera, the planar-pose batch over its blocks, then the single-camera Tsai-Lenz seed
    per_cam = []
    for c in range(n_cams):
        idx = np.flatnonzero(f.blk_cam == c)
        arrs = [np.c_[f.X[lo:hi], f.Y[lo:hi], f.u[lo:hi], f.v[lo:hi]] for lo, hi in zip(f.blk_offset[idx], f.blk_offset[idx + 1])]
        off = np.zeros(len(arrs) + 1, dtype=np.int64)
        np.cumsum([a.shape[0] for a in arrs], out=off[1:])
        allp = np.concatenate(arrs)
        cols = [np.ascontiguousarray(allp[:, k]) for k in range(4)]
        bg = np.ascontiguousarray(np.stack([pose_from_matrix(np.r_[np.c_[btg[b, :9].reshape(3, 3), btg[b, 9:]], [[0, 0, 0, 1]]])
                                            for b in idx]))
        per_cam.append((len(arrs), off, cols, bg, np.ascontiguousarray(K[c])))
    g_old = np.zeros((n_cams, 7))

    def per_camera():
        for c, (nv, off, cols, bg, Kc) in enumerate(per_cam):
            P = np.zeros((nv, 7))
            capi.check(lib, lib.cba_estimate_planar_pose_batch(nv, i64ptr(off), *(dptr(a) for a in cols), dptr(Kc), dptr(P)))
            capi.check(lib, lib.cba_estimate_handeye_dlt(nv, dptr(bg), dptr(P), 1.0, dptr(g_old[c])))

    wall_old = _median_wall(per_camera, reps)
    pairs_total = int(sum(pr))
    enumerated = n_cams * n_poses * (n_poses - 1) // 2
    n_cand = f.n_blocks
    return {
        "poses": n_poses, "cams": n_cams, "points_per_block": int(f.blk_offset[-1]) // f.n_blocks, "reps": reps,
        "stage_ms": {"block_poses": med[0], "pass1_rotation": med[1], "pass2_translation": med[2], "target": med[3], "total": med[4],
                     "scan": med[5]},
        "pairs_enumerated_per_pass": enumerated, "pairs_valid": pairs_total,
        "pass1_pairs_per_s": enumerated / (med[1] * 1e-3), "pass2_pairs_per_s": enumerated / (med[2] * 1e-3),
        "scan_candidates": n_cand, "scan_ns_per_candidate": med[5] * 1e6 / n_cand,
        "call_wall_ms": wall_batched,
        "per_camera_path_wall_ms": wall_old,
        "speedup_wall": wall_old / wall_batched,
        "max_g_T_c_diff_vs_per_camera": float(np.abs(g - g_old).max()),
        "seed_max_camera_translation_error_m": float(np.abs(g[:, 4:] - sc.gt_cam_pose[:, 4:]).max()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--cams", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    if not hasattr(lib, "cba_estimate_bundle_seed_timed"):
        sys.exit(f"{capi.library_path()} has no stage timing: build the experiment library "
                 "(make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp)")
    out = {"what": "cba_estimate_bundle_seed (device stage times, ms, median; uploads excluded) vs the per-camera "
                   "cba_estimate_planar_pose_batch + cba_estimate_handeye_dlt path (host wall times)",
           "shapes": [run_shape(lib, a.poses, nc, a.reps) for nc in a.cams]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
