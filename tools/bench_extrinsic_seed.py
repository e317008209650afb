"""Rig-seed benchmark: one JSON line with the stage times of cba_estimate_extrinsic_dlt at the C3 shape (default 4000 views x 8
cameras x 5000 points, tests/synth.scene_extrinsics_shard), points per second, the algorithmic HBM rate of the block-pose stage, and a
numpy-on-CPU figure of the same work ("kind": "port", described in its "what" field) for scale.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_extrinsic_seed.py [--views 4000] [--cams 8] [--reps 5] [--out FILE]
Stage times are device events between the kernels of one call (uploads excluded), median over --reps after one warm-up call, from
cba_estimate_extrinsic_dlt_timed, which only the experiment build exports (calibration_amd/lib_exp, selected through
CALIBBA_LIBRARY).  "call_wall_ms" is the whole call from the host, 5.1 GB of uploads included.
Algorithmic bytes of the block-pose stage: k_ext_block_pose reads X, Y, u, v (32 B per point) in each of its three passes
(centroids, mean distances, Gram); "hbm_bytes_one_pass" counts one pass (what reaches HBM if the second and third passes hit in the
caches), "bytes_three_passes" all three (every pass from HBM).  Both are divided by the stage time and set against the 6.3 TB/s
device-to-device copy rate measured on the MI355X."""
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
from tests import extrinsic_dlt_ref as ref  # noqa: E402
from tests import synth  # noqa: E402

COPY_RATE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4000)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--port-views", type=int, default=4, help="views of the numpy baseline (scaled to --views)")
    a = ap.parse_args()

    t0 = time.perf_counter()
    sc = synth.scene_extrinsics_shard(a.views, 0, a.views, n_cams=a.cams)
    gen_s = time.perf_counter() - t0
    f = sc.flat
    lib = capi.load_library()
    if not hasattr(lib, "cba_estimate_extrinsic_dlt_timed"):
        sys.exit(f"{capi.library_path()} has no stage timing: build the experiment library "
                 "(make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp)")
    fn = lib.cba_estimate_extrinsic_dlt_timed
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, capi.c_int64_p, capi.c_int32_p, capi.c_int32_p, capi.c_double_p, capi.c_double_p,
                   capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p]
    K = np.ascontiguousarray(f.intr[:, :5])
    bv, bc = np.ascontiguousarray(f.blk_view, dtype=np.int32), np.ascontiguousarray(f.blk_cam, dtype=np.int32)
    cr, rt, st = np.zeros((f.n_cams, 7)), np.zeros((f.n_views, 7)), np.zeros(4)
    rows, walls = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        capi.check(lib, fn(f.n_cams, f.n_views, f.n_blocks, i64ptr(f.blk_offset), i32ptr(bv), i32ptr(bc), dptr(f.X), dptr(f.Y),
                           dptr(f.u), dptr(f.v), dptr(K), dptr(cr), dptr(rt), dptr(st)))
        if rep:
            walls.append(time.perf_counter() - t0)
            rows.append(st.copy())
    med = np.median(np.array(rows), axis=0)
    n_obs = int(f.blk_offset[-1])
    s1 = med[0] * 1e-3
    err_c = max(float(np.abs(cr[c, 4:] - sc.gt_cam_pose[c, 4:]).max()) for c in range(f.n_cams))
    out = {
        "what": "cba_estimate_extrinsic_dlt (device stage times, ms, median; uploads excluded)",
        "views": a.views, "cams": a.cams, "points": n_obs, "points_per_block": n_obs // f.n_blocks, "reps": a.reps,
        "stage_ms": {"block_poses": med[0], "camera_averages": med[1], "target_averages": med[2], "total": med[3]},
        "call_wall_ms": 1e3 * float(np.median(walls)),
        "points_per_s": n_obs / (med[3] * 1e-3),
        "block_pose_hbm_bytes_one_pass": 32 * n_obs,
        "block_pose_bytes_per_s_one_pass": 32 * n_obs / s1,
        "block_pose_bytes_per_s_three_passes": 96 * n_obs / s1,
        "copy_rate_bytes_per_s": COPY_RATE,
        "block_pose_fraction_of_copy_rate_one_pass": 32 * n_obs / s1 / COPY_RATE,
        "block_pose_fraction_of_copy_rate_three_passes": 96 * n_obs / s1 / COPY_RATE,
        "seed_max_camera_translation_error_m": err_c,
        "scene_generation_s": gen_s,
    }
    # numpy on the host CPU: tests/extrinsic_dlt_ref.py (planar seed by SVD per block, then the averages) over --port-views views
    kv = min(a.port_views, a.views)
    views = []
    for v in range(kv):
        mv = []
        for c in range(f.n_cams):
            b = v * f.n_cams + c
            lo, hi = f.blk_offset[b], f.blk_offset[b + 1]
            mv.append(np.c_[f.X[lo:hi], f.Y[lo:hi], f.u[lo:hi], f.v[lo:hi]])
        views.append(mv)
    t0 = time.perf_counter()
    ref.estimate_extrinsic_dlt(views, K)
    port = time.perf_counter() - t0
    out["port"] = {"kind": "port", "what": f"numpy estimate_extrinsic_dlt (extrinsic_dlt_ref.py) over {kv} views x {f.n_cams} cameras, "
                                           f"scaled linearly to {a.views} views (not measured at that size)",
                   "measured_s": port, "scaled_s": port * a.views / kv}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
