"""The C++ adapter of the hand-eye / bundle seed (include/calibba_handeye_rig.hpp).

CPU tier: the header compiles as C++20 against the TEST-ONLY stand-ins under tests/handeye_rig_adapter_check/ (declarations with the
reference's names and members; they pin nothing), and calibba_adapter.hpp does not include it.
GPU tier: the driver runs the adapter on the pipeline-stage hand-eye scene and gives bit for bit what the Python API gives.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import capi, handeye_rig, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "handeye_rig_adapter_check")
EXE = os.path.join(DIR, "_build", "he_adapter_drive")


def test_handeye_rig_header_is_valid_cpp20():
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(DIR, "stand_ins"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(DIR, "he_adapter_drive.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_handeye_rig_header_is_not_in_the_optim_adapter():
    assert "calibba_handeye_rig" not in open(os.path.join(ROOT, "include", "calibba_adapter.hpp")).read()


@pytest.mark.gpu
def test_handeye_rig_adapter_matches_python_api(gpu_lib, tmp_path):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    with open(os.path.join(ROOT, "tests", "golden", "kat_scenes.json")) as f:
        sc = json.load(f)["bundle_two_cameras"]
    cams = [np.asarray(c) for c in sc["cams_gt"]]
    obs = [optim.BundleObservation(np.asarray(o["view"]), np.asarray(o["b_T_g"]), o["cam"]) for o in sc["obs"]]
    lines = [str(len(cams))] + [" ".join(repr(float(x)) for x in c[:5]) for c in cams] + [str(len(obs))]
    for o in obs:
        T = o.b_se3_g
        lines.append(f"{o.camera_index} " + " ".join(repr(float(x)) for x in np.r_[T[:3, :3].reshape(9), T[:3, 3]]))
        lines.append(str(len(o.view)))
        lines += [" ".join(repr(float(x)) for x in row) for row in o.view]
    scene = tmp_path / "scene.txt"
    scene.write_text("\n".join(lines) + "\n")
    p = subprocess.run([EXE, str(scene)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "he_adapter_drive: all ok" in p.stdout
    got, status = {}, {}
    for ln in p.stdout.splitlines():
        f = ln.split()
        if f[0] in ("G", "T"):
            got[(f[0], int(f[1]) if f[0] == "G" else 0)] = np.array([float(x) for x in f[(2 if f[0] == "G" else 1):]])
        elif f[0] == "S":
            status[int(f[1])] = (int(f[2]), int(f[3]))
    want = handeye_rig.estimate_bundle_seed(obs, cams)
    for c, T in enumerate(want.g_se3_c):
        assert np.array_equal(got[("G", c)], np.r_[T[:3, :3].reshape(9), T[:3, 3]]), c
        assert status[c] == (int(want.blocks.cam_status[c]), int(want.blocks.cam_pairs[c])) and status[c][0] == capi.HANDEYE_DLT
    assert np.array_equal(got[("T", 0)], np.r_[want.b_se3_t[:3, :3].reshape(9), want.b_se3_t[:3, 3]])
    assert "SRC estimated FAILED 0" in p.stdout
