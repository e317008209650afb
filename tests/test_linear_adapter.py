"""The C++ adapter of the intrinsic seed (include/calibba_linear.hpp).

CPU tier: the header compiles as C++20 with every entry point used, against the TEST-ONLY stand-ins under
tests/linear_adapter_check/ (declarations with the reference's names and members; they pin nothing).
GPU tier: the driver runs the adapter on the RecoversCameraMatrix scene and gives what the Python API gives for it.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import linear
from calibration_amd.linescan import RansacOptions
from calibration_amd.optim import CalibrationBounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "linear_adapter_check")
EXE = os.path.join(DIR, "_build", "lin_adapter_drive")


def test_linear_header_is_valid_cpp20():
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(DIR, "stand_ins"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(DIR, "lin_adapter_drive.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_linear_header_is_not_in_the_optim_adapter():
    assert "calibba_linear" not in open(os.path.join(ROOT, "include", "calibba_adapter.hpp")).read()


@pytest.mark.gpu
def test_linear_adapter_matches_python_api(gpu_lib, tmp_path):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    with open(os.path.join(ROOT, "tests", "golden", "intrinsics_seed_scenes.json")) as f:
        views = [np.asarray(v) for v in json.load(f)["recovers_camera_matrix"]["views"]]
    lines = [str(len(views))]
    for v in views:
        lines.append(str(len(v)))
        lines += [" ".join(repr(float(x)) for x in row) for row in v]
    scene = tmp_path / "scene.txt"
    scene.write_text("\n".join(lines) + "\n")
    p = subprocess.run([EXE, str(scene)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "lin_adapter_drive: all ok" in p.stdout
    rows = [ln.split() for ln in p.stdout.splitlines() if not ln.startswith("lin_")]
    by = {}
    for r in rows:
        by.setdefault(r[0], []).append(r[1:])
    num = lambda xs: np.array([float(x) for x in xs])  # noqa: E731

    lin = linear.estimate_intrinsics(views)
    assert np.array_equal(num(by["K"][0]), np.r_[1.0, lin.kmtx])
    assert len(by["V"]) == len(lin.views)
    for got, ve in zip(by["V"], lin.views):
        g = num(got)
        assert int(g[0]) == ve.view_index and int(g[1]) == len(ve.homography.inliers) and g[2] == ve.forward_rms_px
        assert np.array_equal(g[3:12], ve.homography.hmtx.reshape(9))
        assert np.array_equal(g[12:21], ve.c_se3_t[:3, :3].reshape(9)) and np.array_equal(g[21:24], ve.c_se3_t[:3, 3])

    ro = RansacOptions(max_iters=200)
    linr = linear.estimate_intrinsics(views, linear.IntrinsicsEstimOptions(bounds=CalibrationBounds(), homography_ransac=ro))
    assert np.array_equal(num(by["KR"][0]), np.r_[1.0, linr.kmtx])
    assert by["KR_log"][0][0] == ("sanitized" if linr.log else "-")
    for got, ve in zip(by["VR"], linr.views):
        g = num(got)
        assert int(g[0]) == ve.view_index and int(g[1]) == len(ve.homography.inliers) and g[2] == ve.forward_rms_px

    for tag, opts in (("H0", None), ("H1", ro)):
        h = linear.estimate_homography(views[0], opts)
        g = num(by[tag][0])
        assert g[0] == 1.0 and int(g[1]) == len(h.inliers) and g[2] == h.symmetric_rms_px
        assert np.array_equal(g[3:12], h.hmtx.reshape(9))

    z = linear.zhang_intrinsics_from_hs([ve.homography for ve in lin.views])
    assert np.array_equal(num(by["Z"][0]), np.r_[1.0, z])
    pz = linear.pose_from_homography(lin.kmtx, lin.views[0].homography.hmtx)
    g = num(by["P"][0])
    assert g[0] == 1.0 and g[1] == pz.scale and g[2] == pz.cond_check
    assert np.array_equal(g[3:12], pz.c_se3_t[:3, :3].reshape(9)) and np.array_equal(g[12:15], pz.c_se3_t[:3, 3])
