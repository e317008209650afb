"""Camera-model benchmark: one JSON line with the device times of cba_camera_project / cba_camera_unproject (10^7 points; the
unprojection in both forms), of the undistortion map (8 cameras x 4096 x 3000) and of apply (8 uint8 RGB images and 8 float32
mono images of that size), each with its fraction of the 6.3 TB/s HBM copy rate.

usage: make -C calibration_amd/csrc EXPERIMENTS=1 LIBDIR=../lib_exp OBJDIR=_build_exp
       python tools/bench_camera.py [--n 10000000] [--reps 5] [--out FILE]
Times are device events around the kernel of one call, median over --reps after one warm-up call, from the *_timed entry points
only the experiment build exports (calibration_amd/lib_exp, selected through CALIBBA_LIBRARY); the uploads and downloads of the
same call are reported separately and are not part of "kernel_ms".  The uint8 RGB apply runs with both load shapes (three aligned
dword loads per tap row, the default, and byte loads: CBA_EXP_CAMERA_U8_LOAD=byte, read only by the experiment build).
Bytes counted per kernel (the minimum traffic): project 40 B per point (24 in, 16 out), unproject 32 B, the map 8 B per pixel
written, apply the map entry (8 B) + the output pixel + the source image once.  The map's fp64 bound is arithmetic only: by a count
of camera_math.hpp (not measured) a pixel costs 3 fp64 divisions and about 60 other fp64 operations, about 90 fp64 instructions."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_exp_lib = os.path.join(ROOT, "calibration_amd", "lib_exp", "libcalibba.so")
os.environ.setdefault("CALIBBA_LIBRARY", _exp_lib)

from calibration_amd import capi  # noqa: E402
from calibration_amd.capi import dptr, i32ptr  # noqa: E402
from tests import camera_ref as R  # noqa: E402

HBM_TBPS = 6.3
# the arithmetic bound of the map: the 78.6 TFLOP/s fp64 vector peak is 39.3 T instructions/s (an FMA counts 2 FLOP); a pixel is
# about 90 fp64 instructions by a count of camera_math.hpp (3 divisions at about 10 instructions each, about 60 others), not measured
FP64_INSTR_PER_S = 78.6e12 / 2
MAP_FP64_INSTR_PER_PIXEL = 90


def _bind(lib):
    d, i32, i64, vp = capi.c_double_p, C.c_int32, C.c_int64, C.c_void_p
    lib.cba_camera_project_timed.argtypes = [i32, d, i64, d, d, d]
    lib.cba_camera_unproject_timed.argtypes = [i32, d, i32, d, i64, d, d, d]
    lib.cba_undistort_map_create_timed.argtypes = [i32, i32, d, d, d, i32, i32, i32, C.POINTER(vp), d]
    lib.cba_undistort_map_apply_timed.argtypes = [vp, i32, capi.c_int32_p, i32, i32, i32, i32, C.c_double, vp, vp, d]
    for f in ("cba_camera_project_timed", "cba_camera_unproject_timed", "cba_undistort_map_create_timed", "cba_undistort_map_apply_timed"):
        getattr(lib, f).restype = C.c_int32


def _measure(call, reps, nbytes):
    call()
    st = np.array([call().copy() for _ in range(reps)])
    med = np.median(st, axis=0)
    k = float(med[1])
    return dict(upload_ms=float(med[0]), kernel_ms=k, download_ms=float(med[2]), bytes=int(nbytes),
                TBps=nbytes / (k * 1e-3) / 1e12, share_of_6_3TBps=nbytes / (k * 1e-3) / 1e12 / HBM_TBPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = capi.load_library()
    _bind(lib)
    ms = np.zeros(3)
    res = {"kind": "camera", "n_points": a.n, "reps": a.reps}
    xyz = R.points(a.n, seed=1)
    uv = np.empty((a.n, 2))
    cams = {name: (model, intr) for name, model, intr in R.cameras()}
    for tag, name in (("pinhole", "pinhole_skew0.0"), ("scheimpflug", "scheimpflug_skew0.0_tau(0.2, -0.2)")):
        model, intr = cams[name]

        def proj():
            capi.check(lib, lib.cba_camera_project_timed(model, dptr(intr), a.n, dptr(xyz), dptr(uv), dptr(ms)))
            return ms
        res[f"project_{tag}"] = _measure(proj, a.reps, 40 * a.n)
        xy = np.empty_like(uv)
        for form, inv in (("iterative", None), ("dual", np.ascontiguousarray(R.dual_inverse(intr[5:10])))):
            def unproj():
                capi.check(lib, lib.cba_camera_unproject_timed(model, dptr(intr), 0 if inv is None else inv.size, dptr(inv), a.n, dptr(uv),
                                                               dptr(xy), dptr(ms)))
                return ms
            res[f"unproject_{tag}_{form}"] = _measure(unproj, a.reps, 32 * a.n)

    W, H, NC = 4096, 3000, 8
    for tag, name in (("pinhole", "pinhole_skew0.4"), ("scheimpflug", "scheimpflug_skew0.0_tau(0.2, -0.2)")):
        model, intr = cams[name]
        intrs = np.ascontiguousarray(np.tile(intr, (NC, 1)))
        intrs[:, 0] = intrs[:, 1] = 3000.0
        intrs[:, 2], intrs[:, 3] = W / 2.0, H / 2.0
        handles = []

        def create():
            h = C.c_void_p()
            capi.check(lib, lib.cba_undistort_map_create_timed(model, NC, dptr(intrs), dptr(None), dptr(None), W, H, 0, C.byref(h), dptr(ms)))
            handles.append(h)
            return ms
        r = _measure(create, a.reps, 8 * W * H * NC)
        px = W * H * NC
        r["fp64_issue_bound_ms_arithmetic"] = px * MAP_FP64_INSTR_PER_PIXEL / FP64_INSTR_PER_S * 1e3
        r["hbm_bound_ms"] = 8.0 * px / (HBM_TBPS * 1e12) * 1e3
        res[f"map_{tag}"] = r
        for h in handles[1:]:
            lib.cba_undistort_map_destroy(h)
        h = handles[0]
        if tag == "pinhole":
            rng = np.random.default_rng(0)
            cam_idx = np.arange(NC, dtype=np.int32)
            for dname, ch, dt, dtype in (("u8_rgb", 3, capi.DTYPE_U8, np.uint8), ("f32_mono", 1, capi.DTYPE_F32, np.float32)):
                shape = (NC, H, W, ch) if ch > 1 else (NC, H, W)
                img = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.random(shape, dtype=np.float32)
                out = np.empty_like(img)

                def apply():
                    capi.check(lib, lib.cba_undistort_map_apply_timed(h, NC, i32ptr(cam_idx), W, H, ch, dt, 0.0, img.ctypes.data_as(C.c_void_p),
                                                                      out.ctypes.data_as(C.c_void_p), dptr(ms)))
                    return ms
                nbytes = 8 * W * H * NC + 2 * img.nbytes
                res[f"apply_{dname}"] = _measure(apply, a.reps, nbytes)
                if dname == "u8_rgb":
                    os.environ["CBA_EXP_CAMERA_U8_LOAD"] = "byte"
                    res["apply_u8_rgb_byte_loads"] = _measure(apply, a.reps, nbytes)
                    del os.environ["CBA_EXP_CAMERA_U8_LOAD"]
                    ref = out.copy()
                    apply()
                    res["apply_u8_rgb_load_shapes_agree"] = bool(np.array_equal(ref, out))
        lib.cba_undistort_map_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
