"""The C++ adapter of the rig seed (include/calibba_extrinsics.hpp).

CPU tier: the header compiles as C++20 against the TEST-ONLY stand-ins under tests/extrinsics_adapter_check/ (declarations with the
reference's names and members; they pin nothing), and calibba_adapter.hpp does not include it.
GPU tier: the driver runs the adapter on the Extrinsics.RecoverAllParameters scene and gives bit for bit what the Python API gives.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "extrinsics_adapter_check")
EXE = os.path.join(DIR, "_build", "ext_adapter_drive")


def test_extrinsics_header_is_valid_cpp20():
    cmd = ["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(DIR, "stand_ins"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(DIR, "ext_adapter_drive.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_extrinsics_header_is_not_in_the_optim_adapter():
    assert "calibba_extrinsics" not in open(os.path.join(ROOT, "include", "calibba_adapter.hpp")).read()


@pytest.mark.gpu
def test_extrinsics_adapter_matches_python_api(gpu_lib, tmp_path):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    with open(os.path.join(ROOT, "tests", "golden", "kat_scenes.json")) as f:
        sc = json.load(f)["extrinsics_all_parameters"]
    views = [[np.asarray(pv) for pv in mv] for mv in sc["views"]]
    cams = [np.asarray(c) for c in sc["cams_gt"]]
    lines = [f"{len(views)} {len(cams)}"] + [" ".join(repr(float(x)) for x in c[:5]) for c in cams]
    for mv in views:
        for pv in mv:
            lines.append(str(len(pv)))
            lines += [" ".join(repr(float(x)) for x in row) for row in pv]
    scene = tmp_path / "scene.txt"
    scene.write_text("\n".join(lines) + "\n")
    p = subprocess.run([EXE, str(scene)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ext_adapter_drive: all ok" in p.stdout
    got = {}
    for ln in p.stdout.splitlines():
        f = ln.split()
        if f[0] in ("CR", "RT"):
            got[(f[0], int(f[1]))] = np.array([float(x) for x in f[2:]])
    want = rig.estimate_extrinsic_dlt(views, cams)
    assert len(got) == len(want.c_se3_r) + len(want.r_se3_t)
    for tag, Ts in (("CR", want.c_se3_r), ("RT", want.r_se3_t)):
        for i, T in enumerate(Ts):
            assert np.array_equal(got[(tag, i)], np.r_[T[:3, :3].reshape(9), T[:3, 3]]), (tag, i)
