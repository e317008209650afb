"""CPU tier of the hand-eye / bundle seed: bundle_seed_math.hpp (the per-lane algebra of cba_estimate_bundle_seed) compiled for
the host (tests/bundle_seed_cpu) against the numpy restatement tests/bundle_seed_ref.py, the C ABI's argument errors (all raised
before any device work), the call without blocks, and the reference's BundleStageUtilsTest cases that need no detections."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import capi, handeye_rig
from calibration_amd.capi import dptr, i32ptr, i64ptr
from calibration_amd.geometry import quat_to_rotmat, rotmat_to_quat
from tests import bundle_seed_ref as bref
from tests import extrinsic_dlt_ref as ref
from tests import host_build
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I7 = np.array([1.0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def bs():
    lib = host_build.load("bundle_seed_cpu")
    P, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.bs_pose_row_c.argtypes = [P, P, P]
    lib.bs_target_c.argtypes = [C.c_int, P, I, P, P, P]
    return lib


def _rand_T(rng, rot_deg=180.0, scale=1.0):
    R = synth.make_pose(np.zeros(3), synth.rand_unit_axis(rng), np.deg2rad(rng.uniform(-rot_deg, rot_deg)))[:3, :3]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.normal(0, scale, 3)
    return T


def _p7(T):
    return np.concatenate([rotmat_to_quat(T[:3, :3]), T[:3, 3]])


def _rt12(T):
    return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]])


def _rz(deg):
    T = np.eye(4)
    a = np.deg2rad(deg)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def _target(bs, items, g):
    """items: (b_T_g, cam, c_T_t) in the order to average"""
    B = np.ascontiguousarray(np.stack([_rt12(b) for b, _, _ in items]))
    cam = np.array([c for _, c, _ in items], dtype=np.int32)
    P = np.ascontiguousarray(np.stack([_p7(t) for _, _, t in items]))
    G = np.ascontiguousarray(np.stack([_p7(x) for x in g]))
    out = np.zeros(7)
    bs.bs_target_c(len(items), dptr(B), cam.ctypes.data_as(C.POINTER(C.c_int)), dptr(G), dptr(P), dptr(out))
    return out


@pytest.mark.parametrize("seed", range(4))
def test_pose_row_matches_the_single_camera_table(bs, seed):
    rng = np.random.default_rng(seed)
    T, c = _rand_T(rng), _p7(_rand_T(rng)) * rng.uniform(0.5, 2.0, 1).repeat(7) ** np.r_[1, 1, 1, 1, 0, 0, 0]
    row = np.zeros(24)
    bs.bs_pose_row_c(dptr(np.ascontiguousarray(_rt12(T))), dptr(np.ascontiguousarray(c)), dptr(row))
    assert np.array_equal(row[:12], _rt12(T))
    assert np.abs(row[12:21] - quat_to_rotmat(c[:4] / np.linalg.norm(c[:4])).reshape(-1)).max() <= 1e-15
    assert np.array_equal(row[21:], c[4:])


@pytest.mark.parametrize("seed", range(5))
def test_target_matches_restatement(bs, seed):
    rng = np.random.default_rng(50 + seed)
    n_cams = int(rng.integers(1, 5))
    g = [_rand_T(rng, 30.0, 0.1) for _ in range(n_cams)]
    base = [[_rand_T(rng) for _ in range(int(rng.integers(0, 12)))] for _ in range(n_cams)]
    cam = [[_rand_T(rng, 60.0) for _ in b] for b in base]
    items = [(b, c, t) for c in range(n_cams) for b, t in zip(base[c], cam[c])]
    if not items:
        return
    want, src = bref.initial_target(base, cam, [ref.matrix_of(_p7(x)) for x in g])
    assert src == "estimated"
    assert np.abs(_target(bs, items, g) - want).max() <= 1e-12


def test_target_is_camera_major(bs):
    """Two cameras x two robot poses whose candidates rotate 0, 150 | 250, 40 degrees about z: camera-major and view-major order
    give different sign-rule averages, and the camera-major one (the reference's) is what the device order gives."""
    g = [np.eye(4), np.eye(4)]
    base = [[np.eye(4), np.eye(4)], [np.eye(4), np.eye(4)]]
    cam = [[_rz(0.0), _rz(150.0)], [_rz(250.0), _rz(40.0)]]
    for c in range(2):
        for k in range(2):
            cam[c][k][:3, 3] = [0.1 * c, 0.2 * k, 1.0]
    items_cm = [(base[c][k], c, cam[c][k]) for c in range(2) for k in range(2)]
    items_vm = [(base[c][k], c, cam[c][k]) for k in range(2) for c in range(2)]
    want, _ = bref.initial_target(base, cam, g)
    view_major = ref.average_isometries([cam[c][k] for k in range(2) for c in range(2)])
    assert np.abs(ref.matrix_of(want)[:3, :3] - ref.matrix_of(view_major)[:3, :3]).max() > 0.1
    got = _target(bs, items_cm, g)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(_target(bs, items_vm, g) - view_major).max() <= 1e-12


# ---- the C ABI without a device -----------------------------------------------------------------------------------------
def _call(lib, n_cams, off, bc, min_angle=1.0, given_mask=None, g_given=None, b_given=None, null=None):
    off = np.asarray(off, dtype=np.int64)
    nb = len(off) - 1
    n = max(int(off[-1]) if len(off) and off[-1] > 0 else 0, 1)
    cols = [np.zeros(n) for _ in range(4)]
    K = np.tile([100.0, 100.0, 0.0, 0.0, 0.0], (max(n_cams, 1), 1))
    btg = np.tile(np.r_[np.eye(3).reshape(-1), 0, 0, 0], (max(nb, 1), 1))
    m = max(n_cams, 1)
    args = dict(g=np.zeros((m, 7)), st=np.full(m, -1, dtype=np.int32), pr=np.full(m, -1, dtype=np.int32), bt=np.zeros(7),
                src=np.full(1, -1, dtype=np.int32))
    ptr = {k: (dptr(v) if v.dtype == np.float64 else i32ptr(v)) for k, v in args.items()}
    if null in ptr:
        ptr[null] = dptr(None) if args[null].dtype == np.float64 else i32ptr(None)
    st = lib.cba_estimate_bundle_seed(
        n_cams, nb, i64ptr(off), i32ptr(None if null == "bc" else np.asarray(bc, dtype=np.int32)), dptr(None if null == "btg" else btg),
        *(dptr(a) for a in cols), dptr(None if null == "K" else K), float(min_angle),
        i32ptr(None if given_mask is None else np.asarray(given_mask, dtype=np.int32)),
        dptr(None if g_given is None else np.ascontiguousarray(g_given, dtype=np.float64)),
        dptr(None if b_given is None else np.ascontiguousarray(b_given, dtype=np.float64)),
        ptr["g"], ptr["st"], ptr["pr"], ptr["bt"], ptr["src"], dptr(None), i32ptr(None))
    return st, lib.cba_last_error().decode(), args


def test_argument_errors(lib):
    cases = [
        dict(n_cams=0, off=[0], bc=[]),
        dict(n_cams=-1, off=[0], bc=[]),
        dict(n_cams=1, off=[2, 6], bc=[0]),                 # offsets not starting at 0
        dict(n_cams=1, off=[0, 6, 4], bc=[0, 0]),           # decreasing
        dict(n_cams=2, off=[0, 4, 8], bc=[0, 2]),           # camera out of range
        dict(n_cams=2, off=[0, 4, 8], bc=[-1, 0]),
        dict(n_cams=1, off=[0, 4], bc=[0], min_angle=-1.0),
        dict(n_cams=1, off=[0, 4], bc=[0], min_angle=float("nan")),
        dict(n_cams=1, off=[0, 4], bc=[0], min_angle=float("inf")),
        dict(n_cams=1, off=[0, 4], bc=[0], given_mask=[1]),  # given_mask without g_T_c_given
        dict(n_cams=1, off=[0], bc=[], given_mask=[0]),
    ] + [dict(n_cams=1, off=[0, 4], bc=[0], null=k) for k in ("bc", "btg", "K", "g", "st", "pr", "bt", "src")]
    for kw in cases:
        st, msg, _ = _call(lib, **kw)
        assert st == capi.CBA_ERR_INVALID_ARGUMENT, (kw, st, msg)
    off = np.zeros(1, dtype=np.int64)
    assert lib.cba_estimate_bundle_seed(1, -1, i64ptr(off), i32ptr(None), dptr(None), dptr(None), dptr(None), dptr(None), dptr(None),
                                        dptr(np.ones(5)), 1.0, i32ptr(None), dptr(None), dptr(None), dptr(np.zeros(7)),
                                        i32ptr(np.zeros(1, np.int32)), i32ptr(np.zeros(1, np.int32)), dptr(np.zeros(7)),
                                        i32ptr(np.zeros(1, np.int32)), dptr(None), i32ptr(None)) == capi.CBA_ERR_INVALID_ARGUMENT
    assert lib.cba_estimate_bundle_seed(1, 0, i64ptr(None), i32ptr(None), dptr(None), dptr(None), dptr(None), dptr(None), dptr(None),
                                        dptr(np.ones(5)), 1.0, i32ptr(None), dptr(None), dptr(None), dptr(np.zeros(7)),
                                        i32ptr(np.zeros(1, np.int32)), i32ptr(np.zeros(1, np.int32)), dptr(np.zeros(7)),
                                        i32ptr(np.zeros(1, np.int32)), dptr(None), i32ptr(None)) == capi.CBA_ERR_INVALID_ARGUMENT


def test_no_blocks_gives_identities(lib):
    st, msg, a = _call(lib, 3, [0], [])
    assert st == capi.CBA_OK, msg
    assert np.array_equal(a["g"], np.tile(I7, (3, 1))) and np.array_equal(a["bt"], I7)
    assert list(a["st"]) == [capi.HANDEYE_TOO_FEW_VIEWS] * 3 and list(a["pr"]) == [0, 0, 0]
    assert a["src"][0] == capi.TARGET_IDENTITY


def test_no_blocks_with_given_and_config(lib):
    gg = np.array([[1.0, 0, 0, 0, 0, 0, 0], [0.6, 0.8, 0, 0, 1, 2, 3]])
    bt = np.array([0.0, 1.0, 0, 0, 4, 5, 6])
    st, msg, a = _call(lib, 2, [0], [], given_mask=[0, 1], g_given=gg, b_given=bt)
    assert st == capi.CBA_OK, msg
    assert np.array_equal(a["g"][0], I7) and np.array_equal(a["g"][1], gg[1]) and np.array_equal(a["bt"], bt)
    assert list(a["st"]) == [capi.HANDEYE_TOO_FEW_VIEWS, capi.HANDEYE_GIVEN] and a["src"][0] == capi.TARGET_CONFIG


# ---- BundleStageUtilsTest (bundle_stage_utils_test.cpp) cases without detections, restated on the Python API ----------------
def test_handeye_initialization_prefers_existing_results():
    """HandeyeInitializationPrefersExistingResults (:132-152)"""
    g = np.eye(4)
    g[0, 3] = 1.0
    s = handeye_rig.estimate_bundle_seed([], [np.ones(10)], handeye=[g])
    assert not s.failed
    assert [r["source"] for r in s.report] == ["handeye"] and s.report[0]["success"]
    assert abs(s.g_se3_c[0][0, 3] - 1.0) <= 1e-9
    _, rep, failed, _ = bref.handeye_initialization([[]], [[]], 1.0, [g])
    assert not failed and rep[0]["source"] == "handeye"


def test_choose_initial_target_uses_configuration_when_provided():
    """ChooseInitialTargetUsesConfigurationWhenProvided (:154-165)"""
    t = np.eye(4)
    t[1, 3] = 1.0
    s = handeye_rig.estimate_bundle_seed([], [np.ones(10)], initial_target=t)
    assert s.initial_target_source == "config" and abs(s.b_se3_t[1, 3] - 1.0) <= 1e-9


def test_handeye_initialization_signals_failure_without_data():
    """HandeyeInitializationSignalsFailureWithoutData (:185-198)"""
    s = handeye_rig.estimate_bundle_seed([], [np.ones(10)], min_angle_deg=1.0)
    assert s.failed and len(s.report) == 1 and s.report[0]["success"] is False
    assert s.report[0]["error"] == "insufficient_observations" and s.initial_target_source == "identity"
    _, rep, failed, _ = bref.handeye_initialization([[]], [[]], 1.0)
    assert failed and rep[0] == s.report[0]


def test_bundle_rig_without_usable_views_runs_no_solve():
    r = handeye_rig.calibrate_bundle_rig([[None, np.zeros((3, 4))]], [np.eye(4)], [np.ones(10), np.ones(10)])
    assert r.status == "no_valid_observations" and not r.success and r.used_views == 0
    assert r.view_status == [["missing_image_reference", "insufficient_points"]] and r.view_used == [False]


def test_handeye_stage_fixture_is_what_the_committed_generator_emits(tmp_path):
    """tests/golden/handeye_stage_scenes.json is reproducible from tests/golden/gen_handeye_stage.cpp with the image's g++ /
    libstdc++ (the std::mt19937 stream the reference's make_synthetic_handeye_data draws from)."""
    import json

    gold = os.path.join(ROOT, "tests", "golden")
    exe = str(tmp_path / "gen_handeye_stage")
    subprocess.run(["g++", "-O0", "-std=c++20", "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(gold, "gen_handeye_stage.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(gold, "handeye_stage_scenes.json")) as f:
        assert out == f.read()
    d = json.loads(out)["synthetic_handeye"]
    assert len(d["obs"]) >= 4 and all(len(o["view"]) >= 16 for o in d["obs"])  # ASSERT_GE(observations.size(), 4U)
    assert d["camera"][:4] == [750.0, 760.0, 640.0, 360.0]
