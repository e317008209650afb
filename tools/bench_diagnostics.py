"""Reprojection-diagnostics benchmark: one JSON line with the device times of the statistics pass (cba_reproj_residual_stats) and of
the fetch form's kernel (cba_reproj_residuals_fetch_blocks over every block) on 1000 views x 10 000 points (10^7 observations,
intrinsic chain, pinhole + Brown-Conrady), each with its fraction of the 6.3 TB/s HBM copy rate.

usage: python tools/bench_diagnostics.py [--views 1000] [--points-side 100] [--reps 5] [--out FILE]
Times are device events around the launches of one pass (block constants, tile kernel, combines), median over --reps after one
warm-up pass (cba_reproj_residual_stats_timed).  Bytes counted: 16 B per observation read (u, v; the target points X, Y are
de-duplicated across views and stay cache resident); the fetch form adds 16 B (r_u, r_v) + 1 B (keep) written per observation.
The host-side compaction of a fetch is not part of the device time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from calibration_amd import capi  # noqa: E402
from calibration_amd.optim import ReprojHandle  # noqa: E402
from tests import synth  # noqa: E402

HBM_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--points-side", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    if lib.cba_device_count() <= 0:
        raise SystemExit("bench_diagnostics: no HIP device visible")
    side = a.points_side
    sc = synth.scene_intrinsics(a.views, rows=side, cols=side, spacing=0.2 / side, noise_px=0.3, seed=1)
    n = sc.flat.n_obs
    out = dict(bench="reprojection diagnostics", views=a.views, observations=n, reps=a.reps)
    with ReprojHandle(sc.flat) as h:
        for name, fetch, per_obs in (("stats", False, 16), ("fetch", True, 33)):
            ms = float(np.median(h.residual_stats_timed(a.reps, fetch)))
            nbytes = per_obs * n
            tbps = nbytes / (ms * 1e-3) / 1e12
            out[name] = dict(kernel_ms=ms, bytes=nbytes, bound_us=nbytes / (HBM_TBPS * 1e12) * 1e6, TBps=tbps,
                             share_of_6_3TBps=tbps / HBM_TBPS)
        st = h.residual_stats(1.0)
        out["global_rms_px"] = st.global_rms
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
