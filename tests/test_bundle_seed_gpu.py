"""GPU tier of the hand-eye / bundle seed (cba_estimate_bundle_seed, calibration_amd.handeye_rig): block poses against
cba_estimate_planar_pose_batch, each camera's g_T_c against cba_estimate_handeye_dlt and the numpy restatement, the status rules,
invariance to block order and to other cameras, the sign rule of the target average, the reference's pipeline-stage KATs, the
golden bundle scenes seeded by the DLT, and a C4-shaped scene."""
import json
import os

import numpy as np
import pytest

from calibration_amd import capi, handeye_rig, optim
from calibration_amd.capi import dptr, i64ptr
from calibration_amd.geometry import inv, make_pose, pose_from_matrix
from tests import bundle_seed_ref as bref
from tests import extrinsic_dlt_ref as ref
from tests import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name, key):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)[key]


def _scene_items(n_cams, n_poses, seed, noise):
    """synth.scene_bundle -> items (cam, b_T_g 4x4, view (N, 4)) in the scene's view-major order, the cameras' K, the scene"""
    sc = synth.scene_bundle(n_poses, n_cams, noise_px=noise, seed=seed)
    f = sc.flat
    items = []
    for b in range(f.n_blocks):
        lo, hi = f.blk_offset[b], f.blk_offset[b + 1]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = f.blk_b_T_g[b, :9].reshape(3, 3), f.blk_b_T_g[b, 9:]
        items.append((int(f.blk_cam[b]), T, np.c_[f.X[lo:hi], f.Y[lo:hi], f.u[lo:hi], f.v[lo:hi]]))
    return items, np.ascontiguousarray(sc.gt_intr[:, :5]), sc


def _seed(items, K, min_angle_deg=1.0, **kw):
    obs = [optim.BundleObservation(a, T, c) for c, T, a in items]
    off, bcam, btg, cols = handeye_rig._flatten(obs)
    return handeye_rig.estimate_bundle_seed_blocks(len(K), off, bcam, btg, *cols, K, min_angle_deg, **kw), obs


def _planar_batch(arrs, K5):
    lib = capi.load_library()
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    np.cumsum([a.shape[0] for a in arrs], out=off[1:])
    allp = np.concatenate(arrs, axis=0)
    cols = [np.ascontiguousarray(allp[:, k]) for k in range(4)]
    P = np.zeros((len(arrs), 7))
    capi.check(lib, lib.cba_estimate_planar_pose_batch(len(arrs), i64ptr(off), *(dptr(c) for c in cols),
                                                       dptr(np.ascontiguousarray(K5, dtype=np.float64)), dptr(P)))
    return P


def _single_dlt(base, blk_pose7, min_angle_deg):
    lib = capi.load_library()
    bg = np.ascontiguousarray(np.stack([pose_from_matrix(T) for T in base]))
    ct = np.ascontiguousarray(np.asarray(blk_pose7, dtype=np.float64))
    x = np.zeros(7)
    capi.check(lib, lib.cba_estimate_handeye_dlt(len(base), dptr(bg), dptr(ct), float(min_angle_deg), dptr(x)))
    return ref.matrix_of(x)


def _check_against_restatement(r, obs, n_cams, min_angle_deg=1.0, handeye=None, config=None):
    base, cam = bref.accumulators(obs, r.blk_pose, n_cams)
    g, rep, failed, pairs = bref.handeye_initialization(base, cam, min_angle_deg, handeye)
    for c in range(n_cams):
        want_status = (capi.HANDEYE_GIVEN if rep[c]["source"] == "handeye" else capi.HANDEYE_TOO_FEW_VIEWS if rep[c]["source"] == "identity"
                       else capi.HANDEYE_DLT if rep[c]["success"] else capi.HANDEYE_NO_PAIRS)
        assert int(r.cam_status[c]) == want_status, (c, int(r.cam_status[c]), rep[c])
        got = ref.matrix_of(r.g_T_c[c])
        assert np.abs(got - g[c]).max() <= 1e-9, (c, np.abs(got - g[c]).max())
        assert int(r.cam_pairs[c]) == pairs[c]
        if int(r.cam_status[c]) == capi.HANDEYE_DLT:
            lst = [k for k, o in enumerate(obs) if o.camera_index == c and len(o.view) >= 4]
            want = _single_dlt([obs[k].b_se3_g for k in lst], r.blk_pose[lst], min_angle_deg)
            assert np.abs(got - want).max() <= 1e-10, (c, np.abs(got - want).max())
    t, src = bref.initial_target(base, cam, [ref.matrix_of(pose_from_matrix(x)) for x in g], config)
    assert handeye_rig._SOURCE[r.target_source] == src
    assert np.abs(r.b_T_t - t).max() <= 1e-9
    return rep, failed


@pytest.mark.parametrize("n_cams,n_poses,noise,seed", [(1, 20, 0.0, 1), (2, 60, 0.2, 2), (4, 120, 0.2, 3), (8, 40, 0.0, 4),
                                                       (3, 300, 0.2, 5)])
def test_block_poses_and_seeds_match(gpu_lib, n_cams, n_poses, noise, seed):
    items, K, _ = _scene_items(n_cams, n_poses, seed, noise)
    r, obs = _seed(items, K)
    for c in range(n_cams):  # block poses: bitwise those of the planar-pose batch with the camera's K
        idx = [k for k, (ci, _, _) in enumerate(items) if ci == c]
        assert np.array_equal(r.blk_pose[idx], _planar_batch([items[k][2] for k in idx], K[c]))
    assert r.blk_ok.all() and r.target_source == capi.TARGET_ESTIMATED
    rep, _ = _check_against_restatement(r, obs, n_cams)
    # scene_bundle's cameras 3 and up have the identity hand-eye rotation (its make_pose gives the identity for an angle <= 0, as
    # the reference's does): without noise every motion pair is then axis-parallel and the reference's filter drops it -> NO_PAIRS
    assert sum(rp["success"] for rp in rep) >= min(n_cams, 3)


def test_too_few_views_and_short_blocks(gpu_lib):
    items, K, _ = _scene_items(2, 12, 7, 0.2)
    cam1 = [k for k, it in enumerate(items) if it[0] == 1]
    for k in cam1[1:]:  # camera 1: one usable block, the rest of 3 points
        items[k] = (1, items[k][1], items[k][2][:3])
    r, obs = _seed(items, K)
    assert int(r.cam_status[0]) == capi.HANDEYE_DLT and int(r.cam_status[1]) == capi.HANDEYE_TOO_FEW_VIEWS
    assert np.array_equal(r.g_T_c[1], ref.IDENTITY7)
    assert not r.blk_ok[cam1[1:]].any() and r.blk_ok[cam1[0]] == 1
    rep, failed = _check_against_restatement(r, obs, 2)
    assert failed and rep[1]["error"] == "insufficient_observations"


def _static_camera_items(K1, g1, b_T_t, n, seed):
    """camera 1 on a robot whose poses turn by at most 0.3 degrees: no motion pair passes a 1-degree filter"""
    rng = np.random.default_rng(seed)
    cam = synth.camera_gt(capi.CAMERA_PINHOLE_BC, False)
    cam[:5] = K1
    grid = synth.make_target_grid(8, 11, 0.02)
    b0 = b_T_t @ inv(make_pose(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.deg2rad(170.0))) @ inv(g1)
    out = []
    for k in range(n):
        T = b0 @ make_pose(rng.uniform(-0.02, 0.02, 3), synth.rand_unit_axis(rng), np.deg2rad(0.3 * rng.uniform()))
        out.append((1, T, synth.render_view(cam, inv(g1) @ inv(T) @ b_T_t, grid, 0.1, rng)))
    return out


def test_no_pairs_camera_keeps_identity_and_enters_the_target(gpu_lib):
    items, K, sc = _scene_items(2, 15, 8, 0.2)
    g1 = ref.matrix_of(sc.gt_cam_pose[1])
    items = [it for it in items if it[0] == 0] + _static_camera_items(K[1], g1, ref.matrix_of(sc.gt_target_pose), 10, 8)
    r, obs = _seed(items, K)
    assert int(r.cam_status[1]) == capi.HANDEYE_NO_PAIRS and int(r.cam_pairs[1]) == 0
    assert np.array_equal(r.g_T_c[1], ref.IDENTITY7)
    rep, failed = _check_against_restatement(r, obs, 2)
    assert failed and rep[1] == {"source": "dlt", "success": False, "error": bref.NO_PAIRS}
    s = handeye_rig.estimate_bundle_seed(obs, K)
    assert s.report[1] == rep[1] and s.failed


def test_given_and_config(gpu_lib):
    items, K, sc = _scene_items(3, 25, 9, 0.2)
    given = [None, ref.matrix_of(sc.gt_cam_pose[1]), None]
    mask, rows = handeye_rig._given(given, 3)
    r, obs = _seed(items, K, given_mask=mask, g_T_c_given=rows)
    assert list(r.cam_status) == [capi.HANDEYE_DLT, capi.HANDEYE_GIVEN, capi.HANDEYE_DLT]
    assert np.array_equal(r.g_T_c[1], rows[1]) and r.cam_pairs[1] == 0
    _check_against_restatement(r, obs, 3, handeye=given)
    bt = pose_from_matrix(make_pose(np.array([0.1, 0.2, 0.3]), np.array([0.0, 0.0, 1.0]), 0.4))
    r2, _ = _seed(items, K, b_T_t_given=bt)
    assert r2.target_source == capi.TARGET_CONFIG and np.array_equal(r2.b_T_t, bt)


def test_order_and_independence(gpu_lib):
    items, K, _ = _scene_items(3, 40, 10, 0.2)
    r, _ = _seed(items, K)
    r_again, _ = _seed(items, K)
    for a, b in ((r.g_T_c, r_again.g_T_c), (r.b_T_t, r_again.b_T_t), (r.blk_pose, r_again.blk_pose), (r.cam_pairs, r_again.cam_pairs)):
        assert np.array_equal(a, b)
    # camera-major listing: every camera keeps its own order
    order = sorted(range(len(items)), key=lambda k: (items[k][0], k))
    r2, _ = _seed([items[k] for k in order], K)
    assert np.array_equal(r.g_T_c, r2.g_T_c) and np.array_equal(r.b_T_t, r2.b_T_t)
    assert np.array_equal(r.blk_pose[order], r2.blk_pose)
    # camera 2's blocks removed: cameras 0 and 1 unchanged
    r3, _ = _seed([it for it in items if it[0] != 2], K)
    assert np.array_equal(r.g_T_c[:2], r3.g_T_c[:2]) and int(r3.cam_status[2]) == capi.HANDEYE_TOO_FEW_VIEWS


def test_target_sign_rule(gpu_lib):
    """A target turned by 120 degrees about -z, where Eigen's matrix -> quaternion conversion switches branch (trace 0): the
    candidates' quaternions come with both signs, so the running-sum rule decides; the device's camera-major scan gives the
    restatement's average."""
    rng = np.random.default_rng(11)
    K = np.array([[900.0, 905.0, 640.0, 360.0, 0.0]] * 2)
    cam = synth.camera_gt(capi.CAMERA_PINHOLE_BC, False)
    cam[:5] = K[0]
    grid = synth.make_target_grid(8, 11, 0.02)
    b_T_t = make_pose(np.array([0.5, -0.1, 0.8]), np.array([0.0, 0.0, -1.0]), np.deg2rad(120.0))
    g = [make_pose(np.array([0.03, 0.0, 0.1]), np.array([0.0, 1.0, 0.0]), 0.1), make_pose(np.array([-0.05, 0.01, 0.1]), np.array([0.0, 1.0, 0.0]), 0.2)]
    items = []
    for _ in range(30):
        c_T_t = synth.random_view_poses(1, rng, dist=1.0, max_tilt_deg=25.0)[0]
        T = b_T_t @ inv(c_T_t) @ inv(g[0])
        for c in range(2):
            items.append((c, T, synth.render_view(cam, inv(g[c]) @ inv(T) @ b_T_t, grid, 0.5, rng)))
    r, obs = _seed(items, K)
    base, camp = bref.accumulators(obs, r.blk_pose, 2)
    gm = [ref.matrix_of(p) for p in r.g_T_c]
    qs = [ref.rotmat_to_quat(T[:3, :3]) for T in bref.candidates(base, camp, gm)]
    assert min(q @ qs[0] for q in qs) < 0.0 < max(q @ qs[0] for q in qs[1:])  # both signs occur
    _check_against_restatement(r, obs, 2)
    plain = np.sum(qs, axis=0)  # without the rule the two sign groups cancel: the rule decides the result
    assert np.linalg.norm(plain) < 0.5 * len(qs)


# ---- the reference's KATs ----------------------------------------------------------------------------------------------------
def _stage_scene():
    sc = _golden("handeye_stage_scenes.json", "synthetic_handeye")
    views = [[np.asarray(o["view"])] for o in sc["obs"]]
    return sc, views, [np.asarray(o["b_T_g"]) for o in sc["obs"]], [np.asarray(sc["camera"])]


def test_handeye_stage_calibrates_synthetic_handeye(gpu_lib):
    """HandEyeCalibrationStageTest.CalibratesSyntheticHandEye (pipeline_stages_test.cpp:265-309)"""
    sc, views, base, cams = _stage_scene()
    res = handeye_rig.calibrate_handeye_rig(views, base, cams, sc["min_angle_deg"],
                                            optim.OptimOptions(max_iterations=sc["handeye_max_iterations"]))
    assert res.status == "ok" and res.sensors[0].status == "ok" and res.sensors[0].used_observations == len(views)
    X, Xgt = res.sensors[0].result.g_se3_c, np.asarray(sc["g_T_c_gt"])
    assert np.linalg.norm(X[:3, 3] - Xgt[:3, 3]) < 5e-3
    assert np.linalg.norm(X[:3, :3] - Xgt[:3, :3]) < 5e-2


def test_bundle_stage_calibrates_synthetic_bundle(gpu_lib):
    """BundleAdjustmentStageTest.CalibratesSyntheticBundle (pipeline_stages_test.cpp:311-372), seeded from the hand-eye stage"""
    sc, views, base, cams = _stage_scene()
    he = handeye_rig.calibrate_handeye_rig(views, base, cams, sc["min_angle_deg"],
                                           optim.OptimOptions(max_iterations=sc["handeye_max_iterations"]))
    assert he.status == "ok"
    opts = optim.BundleOptions(optim.OptimOptions(max_iterations=sc["bundle_max_iterations"]), optimize_intrinsics=False,
                               optimize_skew=False, optimize_target_pose=True, optimize_hand_eye=True)
    res = handeye_rig.calibrate_bundle_rig(views, base, cams, opts, sc["min_angle_deg"], handeye=he)
    assert res.status == "ok" and res.success and res.used_views == len(views)
    assert res.seed.report == [{"source": "handeye", "success": True}] and res.seed.initial_target_source == "estimated"
    assert np.linalg.norm(res.result.b_se3_t[:3, 3] - np.asarray(sc["b_T_t_gt"])[:3, 3]) < 1e-2
    assert np.linalg.norm(res.result.g_se3_c[0][:3, 3] - np.asarray(sc["g_T_c_gt"])[:3, 3]) < 5e-3


def test_choose_initial_target_estimates_from_accumulated_poses(gpu_lib):
    """ChooseInitialTargetEstimatesFromAccumulatedPoses (bundle_stage_utils_test.cpp:167-183): identity base and hand-eye, the board
    rendered at z = 1"""
    cam = synth.camera_gt(capi.CAMERA_PINHOLE_BC, False)
    T = np.eye(4)
    T[2, 3] = 1.0
    view = synth.render_view(cam, T, synth.make_target_grid(6, 8, 0.03))
    s = handeye_rig.estimate_bundle_seed([optim.BundleObservation(view, np.eye(4), 0)], [cam], handeye=[np.eye(4)])
    assert s.initial_target_source == "estimated"
    assert np.abs(s.b_se3_t[:3, 3] - [0.0, 0.0, 1.0]).max() <= 1e-9


@pytest.mark.parametrize("name", ["bundle_single_handeye", "bundle_two_cameras"])
def test_golden_bundle_scenes_from_the_seed(gpu_lib, name):
    """kat_scenes.json's circle-sequence bundles, solved from the DLT seed instead of their near-ground-truth g_T_c_init, with the
    target from the scene's configuration (it is not optimised there) and the scenes' recorded tolerances.  bundle_single_handeye's
    8-pose seed does not reach the basin of the reference's start: that scene keeps the assertions on the seed."""
    from tests import test_oracle_kat as kat
    from tests.test_gpu_parity import _gpu_solver

    sc = dict(_golden("kat_scenes.json", name))
    obs = [optim.BundleObservation(np.asarray(o["view"]), np.asarray(o["b_T_g"]), o["cam"]) for o in sc["obs"]]
    cams = [np.asarray(c) for c in sc["cams_init"]]
    s = handeye_rig.estimate_bundle_seed(obs, cams, initial_target=np.asarray(sc["b_T_t_init"]))
    assert all(rp["source"] == "dlt" and rp["success"] for rp in s.report) and s.initial_target_source == "config"
    _check_against_restatement(s.blocks, obs, len(cams), config=pose_from_matrix(np.asarray(sc["b_T_t_init"])))
    if name == "bundle_single_handeye":
        return
    sc["g_T_c_init"] = [T.tolist() for T in s.g_se3_c]
    kat.solve_kat_bundle(sc, _gpu_solver)


def test_c4_scale_seed_reaches_the_same_cost(gpu_lib):
    """2000 poses x 4 cameras x 88 points at 0.2 px: optimize_bundle from the seed reaches the cost it reaches from the scene's
    perturbed ground truth."""
    items, K, sc = _scene_items(4, 2000, 2024, 0.2)
    r, obs = _seed(items, K)
    assert list(r.cam_status) == [capi.HANDEYE_DLT] * 4 and r.target_source == capi.TARGET_ESTIMATED
    cams = [c.copy() for c in sc.gt_intr]
    opts = optim.BundleOptions(optim.OptimOptions(epsilon=1e-12, compute_covariance=False))
    a = optim.optimize_bundle(obs, cams, [ref.matrix_of(p) for p in r.g_T_c], ref.matrix_of(r.b_T_t), opts)
    b = optim.optimize_bundle(obs, cams, [ref.matrix_of(p) for p in sc.flat.cam_pose], ref.matrix_of(sc.flat.target_pose), opts)
    assert a.core.success and b.core.success
    assert abs(a.core.final_cost - b.core.final_cost) <= 1e-9 * b.core.final_cost
    for Xa, Xb in zip(a.g_se3_c, b.g_se3_c):
        assert np.abs(Xa - Xb).max() <= 2e-5
    assert np.abs(a.b_se3_t - b.b_se3_t).max() <= 2e-5
