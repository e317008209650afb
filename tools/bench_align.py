"""Multi-scan alignment benchmark: one JSON line with the time of one round of cba_cloud_align (every edge's system, then the step of
all scans) next to the same edge systems formed by single-source cba_cloud_register calls, and the step's share at 12 and 64 scans.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_align.py [--width 640] [--height 480] [--scans 12] [--reps 5] [--out profiles/r24_align.json]
The scene is the test scenes' surface (tests/cloud_ref.py) at scan size: --scans organised maps whose windows are shifted round a
circle of a tenth of the map's sides (so neighbours share most of their surface), each moved by a small pose; the edges are both
directions of every neighbouring pair (24 for 12 scans); max_distance is three sample spacings and cell_size max_distance / 0.999.
Times are device events inside the call (cba_cloud_align_timed and cba_cloud_register_timed, which only the experiment build exports:
calibration_amd/lib_exp, selected through CALIBBA_LIBRARY), the median over --reps after one warm-up call.  max_iterations = 0 is one
evaluation and one step, max_iterations = 1 two of each: one round is their difference.  The comparison forms the same edge systems
with one CloudIndex per scan and one cba_cloud_register call (max_iterations = 0) per edge, the sum of the calls' device times and
the host's clock over all of them.  The step's share comes from a second pair of runs on tiny scans, where the evaluation is small:
the round there is an upper bound of k_align_step's time.  No time is fixed in advance."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CALIBBA_LIBRARY", os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so"))

from calibration_amd import capi  # noqa: E402
from calibration_amd.registration import CloudIndex, CloudSet, IcpOptions, default_cell_size, point_normals  # noqa: E402
from tests import cloud_ref as R  # noqa: E402


def ring(n_scans, W, H, focal):
    rng = np.random.default_rng(7)
    scans, poses = [], []
    for k in range(n_scans):
        ang = 2.0 * math.pi * k / n_scans
        m = R.surface_map(W, H, 1, focal=focal, shift=(0.1 * W * math.cos(ang) + 0.37 * k, 0.1 * H * math.sin(ang) - 0.41 * k))
        T = R.pose_from_rotvec(rng.normal(0, 0.001, 3), rng.normal(0, 0.0005, 3))
        inv = R.pose_inverse(T)
        scans.append(R.transform(R.rotation(inv[:4]), inv[4:], m))
        poses.append(T)
    edges = []
    for k in range(n_scans):
        edges += [(k, (k + 1) % n_scans), ((k + 1) % n_scans, k)]
    return scans, np.array(poses), edges[:2 * n_scans if n_scans > 2 else 2]


def align_rounds(lib, cloud_set, edges, md, init, reps):
    """-> {1: stage medians of max_iterations = 0, 2: of max_iterations = 1}, the result of the last call"""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int32))
    poses, ms = np.empty((cloud_set.n_scans, 7)), np.zeros(3)
    out, res = (capi.CbaAlignEdge * len(edges))(), capi.CbaAlignResult()
    got = {}
    for iters in (0, 1):
        co = capi.CbaAlignOptions(IcpOptions(md, max_iterations=iters, step_tolerance=0.0)._c(), 0)

        def call():
            capi.check(lib, lib.cba_cloud_align_timed(cloud_set._h, len(edges), capi.i32ptr(e), capi.dptr(init), C.byref(co), capi.dptr(poses), out,
                                                      C.byref(res), capi.dptr(ms)))
            return ms.copy()
        call()
        got[iters + 1] = np.median(np.array([call() for _ in range(reps)]), axis=0)
    return got, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    d, p64, p32 = capi.c_double_p, capi.c_int64_p, capi.c_int32_p
    lib.cba_cloud_align_timed.argtypes = [C.c_void_p, C.c_int32, p32, d, C.POINTER(capi.CbaAlignOptions), d, C.POINTER(capi.CbaAlignEdge),
                                          C.POINTER(capi.CbaAlignResult), d]
    lib.cba_cloud_align_timed.restype = C.c_int32
    lib.cba_cloud_register_timed.argtypes = [C.c_void_p, C.c_int32, p64, d, d, C.POINTER(capi.CbaIcpOptions), C.POINTER(capi.CbaIcpResult), d]
    lib.cba_cloud_register_timed.restype = C.c_int32
    W, H, N = a.width, a.height, a.scans
    focal = 1.25 * W
    md = 3.0 / focal
    cell = default_cell_size(md)
    scans, poses, edges = ring(N, W, H, focal)
    normals = [point_normals(s) for s in scans]
    res = {"kind": "align", "width": W, "height": H, "scans": N, "edges": len(edges), "reps": a.reps, "points": N * W * H, "max_distance": md,
           "cell_size": cell}
    t0 = time.perf_counter()
    with CloudSet(scans, normals, cell) as cloud_set:
        res["set_create_call_ms"] = (time.perf_counter() - t0) * 1e3
        got, r = align_rounds(lib, cloud_set, edges, md, poses, a.reps)
        res["align_rounds1"] = dict(upload_ms=float(got[1][0]), rounds_ms=float(got[1][1]), download_ms=float(got[1][2]))
        res["align_rounds2"] = dict(upload_ms=float(got[2][0]), rounds_ms=float(got[2][1]), download_ms=float(got[2][2]))
        res["align_round_ms"] = float(got[2][1] - got[1][1])
        res["pairs"], res["used_edges"], res["rms"] = int(r.n_pairs), int(r.n_used_edges), float(r.rms)
    print(f"align: one round {res['align_round_ms']:.3f} ms for {len(edges)} edges of {W} x {H} points, {res['pairs']} pairs", file=sys.stderr, flush=True)
    # the same edge systems by the single-target API: one index per scan, one call per edge at T_b^-1 T_a
    from tests import align_ref as A  # noqa: E402

    indices = [CloudIndex(s, n, cell) for s, n in zip(scans, normals)]
    try:
        co = IcpOptions(md, max_iterations=0)._c()
        out, ms = (capi.CbaIcpResult * 1)(), np.zeros(3)
        flat = [np.ascontiguousarray(s.reshape(-1, 3)) for s in scans]
        rel = [np.ascontiguousarray(A.compose(R.pose_inverse(poses[b]), poses[a])) for a, b in edges]

        def all_edges():
            dev = 0.0
            for (sa, sb), init in zip(edges, rel):
                off = np.array([0, flat[sa].shape[0]], np.int64)
                capi.check(lib, lib.cba_cloud_register_timed(indices[sb]._h, 1, capi.i64ptr(off), capi.dptr(flat[sa]), capi.dptr(init), C.byref(co), out,
                                                             capi.dptr(ms)))
                dev += ms[1]
            return dev
        all_edges()
        dev, wall = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dev.append(all_edges())
            wall.append((time.perf_counter() - t0) * 1e3)
        res["register_calls_rounds_ms"] = float(np.median(dev))
        res["register_calls_wall_ms"] = float(np.median(wall))
    finally:
        for ix in indices:
            ix.close()
    print(f"register: {len(edges)} calls, rounds {res['register_calls_rounds_ms']:.3f} ms on the device, {res['register_calls_wall_ms']:.1f} ms by the "
          f"host's clock (uploads of the sources included)", file=sys.stderr, flush=True)
    # the step's share: tiny scans (70 points), where a round is little more than k_align_step
    for n_scans in (12, 64):
        small, sp, se = ring(n_scans, 10, 7, 20.0)
        with CloudSet(small, [point_normals(s) for s in small], default_cell_size(0.15)) as cloud_set:
            got, r = align_rounds(lib, cloud_set, se, 0.15, sp, a.reps)
        res[f"tiny_round_ms_{n_scans}_scans"] = float(got[2][1] - got[1][1])
        res[f"tiny_status_{n_scans}_scans"] = int(r.status)
        print(f"tiny scans, {n_scans}: one round {res[f'tiny_round_ms_{n_scans}_scans']:.3f} ms ({len(se)} edges)", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
