"""The C++ adapter of the distortion fits and the linear intrinsic estimators (include/calibba_distortion.hpp).

CPU tier: the header compiles as C++20 with every entry point used, against the TEST-ONLY stand-ins under
tests/distortion_adapter_check/ (declarations with the reference's names and members; they pin nothing), and neither existing
adapter header includes it.
GPU tier: the driver runs the adapter on the NoisyFit scene and gives what the Python API gives for it, bit for bit.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import distortion as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "distortion_adapter_check")
EXE = os.path.join(DIR, "_build", "df_adapter_drive")


def test_distortion_header_is_valid_cpp20():
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(DIR, "stand_ins"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(DIR, "df_adapter_drive.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_distortion_header_is_in_no_other_adapter():
    for h in ("calibba_adapter.hpp", "calibba_linear.hpp"):
        assert "calibba_distortion" not in open(os.path.join(ROOT, "include", h)).read()


@pytest.mark.gpu
def test_distortion_adapter_matches_python_api(gpu_lib, tmp_path):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    with open(os.path.join(ROOT, "tests", "golden", "distortion_scenes.json")) as f:
        sc = json.load(f)["noisy_fit"]
    obs, K = np.asarray(sc["obs"]), np.asarray(sc["camera"])
    lines = [" ".join(repr(float(k)) for k in K), str(len(obs))] + [" ".join(repr(float(x)) for x in r) for r in obs]
    scene = tmp_path / "scene.txt"
    scene.write_text("\n".join(lines) + "\n")
    p = subprocess.run([EXE, str(scene)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "df_adapter_drive: all ok" in p.stdout
    by = {r.split()[0]: np.array([float(x) for x in r.split()[1:]]) for r in p.stdout.splitlines() if not r.startswith("df_")}

    f = D.fit_distortion_full(obs, K, 2)
    assert np.array_equal(by["F"], f.distortion) and np.array_equal(by["FR"], f.residuals)
    fx = D.fit_distortion(obs, K, 2, [0, 3], [-0.2])
    assert np.array_equal(by["FX"], fx.distortion) and fx.distortion[3] == 0.0
    d = D.fit_distortion_dual(obs, K, 3)
    assert np.array_equal(by["DF"], d.forward) and np.array_equal(by["DI"], d.inverse)
    assert np.array_equal(by["L"], D.estimate_intrinsics_linear(obs))
    it = D.estimate_intrinsics_linear_iterative(obs, 2, 50, True)
    assert np.array_equal(by["IK"], it.kmtx) and np.array_equal(by["IC"], it.distortion)
