"""GPU tier of the rig seed (cba_estimate_extrinsic_dlt, calibration_amd.rig): block poses against cba_estimate_planar_pose_batch,
the averages against the numpy restatement tests/extrinsic_dlt_ref.py, the reference's skip and sign rules, invariance to block
order and to other cameras, the reference's extrinsics KATs seeded by the DLT end to end, and a C3-shaped scene."""
import json
import os

import numpy as np
import pytest

from calibration_amd import capi, optim, rig
from calibration_amd.capi import dptr, i64ptr
from calibration_amd.geometry import make_pose, pose_to_matrix, rotmat_to_quat
from tests import extrinsic_dlt_ref as ref
from tests import helpers, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kat(name):
    with open(os.path.join(ROOT, "tests", "golden", "kat_scenes.json")) as f:
        return json.load(f)[name]


def _scene(n_cams, n_views, seed, noise=0.3, distortion=True):
    rng = np.random.default_rng(seed)
    cams = []
    for _ in range(n_cams):
        cam = synth.camera_gt(capi.CAMERA_PINHOLE_BC, distortion)
        cam[0:2] *= 1 + 0.02 * rng.uniform(-1, 1, 2)
        cams.append(cam)
    grid = synth.make_target_grid(8, 11, 0.02)
    c_T_r = synth.ring_cameras(n_cams)
    r_T_t = synth.random_view_poses(n_views, rng, max_tilt_deg=20.0)
    views = [[synth.render_view(cams[c], c_T_r[c] @ r_T_t[v], grid, noise, rng) for c in range(n_cams)] for v in range(n_views)]
    return np.stack(cams), views


def _blocks(views, order=None):
    """views[v][c] (None / empty: absent) -> (blk_offset, blk_view, blk_cam, X, Y, u, v, arrays in block order)"""
    items = [(v, c, np.asarray(pv, dtype=np.float64).reshape(-1, 4)) for v, mv in enumerate(views) for c, pv in enumerate(mv)
             if pv is not None and len(pv) > 0]
    if order is not None:
        items = [items[i] for i in order]
    off = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([a.shape[0] for _, _, a in items], out=off[1:])
    allp = np.concatenate([a for _, _, a in items], axis=0) if items else np.zeros((0, 4))
    return (off, np.array([v for v, _, _ in items], dtype=np.int32), np.array([c for _, c, _ in items], dtype=np.int32),
            *(allp[:, k] for k in range(4)), [a for _, _, a in items])


def _run(views, K, order=None):
    off, bv, bc, X, Y, u, v, arrs = _blocks(views, order)
    r = rig.estimate_extrinsic_dlt_blocks(len(K), len(views), off, bv, bc, X, Y, u, v, K)
    return r, bv, bc, arrs


def _planar_batch(arrs, K5):
    """raw pose7 of cba_estimate_planar_pose_batch"""
    lib = capi.load_library()
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    np.cumsum([a.shape[0] for a in arrs], out=off[1:])
    allp = np.concatenate(arrs, axis=0)
    cols = [np.ascontiguousarray(allp[:, k]) for k in range(4)]
    P = np.zeros((len(arrs), 7))
    capi.check(lib, lib.cba_estimate_planar_pose_batch(len(arrs), i64ptr(off), *(dptr(c) for c in cols),
                                                       dptr(np.ascontiguousarray(K5, dtype=np.float64)), dptr(P)))
    return P


def _restated_from_blocks(r, bv, bc, arrs, n_views, n_cams):
    T = {(int(v), int(c)): ref.matrix_of(p) for v, c, p in zip(bv, bc, r.blk_pose)}
    npts = {(int(v), int(c)): len(a) for v, c, a in zip(bv, bc, arrs)}
    return ref.steps_2_3(n_views, n_cams, T, npts)


@pytest.mark.parametrize("n_cams,n_views,seed", [(2, 9, 1), (3, 14, 2), (8, 30, 3)])
def test_block_poses_and_averages_match(gpu_lib, n_cams, n_views, seed):
    cams, views = _scene(n_cams, n_views, seed)
    K = cams[:, :5]
    r, bv, bc, arrs = _run(views, K)
    assert r.blk_ok.all()
    for c in range(n_cams):  # bitwise what the planar-pose batch gives for the same blocks and K
        idx = np.flatnonzero(bc == c)
        assert np.array_equal(r.blk_pose[idx], _planar_batch([arrs[i] for i in idx], K[c]))
    cr, rt = _restated_from_blocks(r, bv, bc, arrs, n_views, n_cams)
    assert np.abs(r.c_T_r - cr).max() <= 1e-12
    assert np.abs(r.r_T_t - rt).max() <= 1e-12
    # the whole restatement, block poses from the numpy planar seed (an SVD: agrees with the device's inverse iteration to ~1e-9,
    # the tolerance of the planar-seed parity test)
    cr2, rt2 = ref.estimate_extrinsic_dlt(views, K)
    assert np.abs(r.c_T_r - cr2).max() <= 1e-9
    assert np.abs(r.r_T_t - rt2).max() <= 1e-9
    assert np.array_equal(r.c_T_r[0], ref.IDENTITY7)


def test_skip_rules(gpu_lib):
    cams, views = _scene(4, 7, 11)
    K = cams[:, :5]
    views[1][2] = views[1][2][:3]  # 3 points: skipped in both averages, identity pose, blk_ok = 0
    views[2][0] = None             # camera 0 missing: view 2 is in no camera average, but still gets r_T_t from cameras 1-3
    for v in range(7):             # camera 3 only where camera 0 is missing or short: no valid pair -> identity
        if v not in (2, 4):
            views[v][3] = None
    views[4][0] = views[4][0][:3]
    views[6] = [None, views[6][1][:3], None, None]  # no valid block: identity target pose
    r, bv, bc, arrs = _run(views, K)
    short = [i for i, a in enumerate(arrs) if len(a) < 4]
    assert len(short) == 3 and not r.blk_ok[short].any()
    assert all(np.array_equal(r.blk_pose[i], ref.IDENTITY7) for i in short)
    cr, rt = _restated_from_blocks(r, bv, bc, arrs, 7, 4)
    assert np.abs(r.c_T_r - cr).max() <= 1e-12 and np.abs(r.r_T_t - rt).max() <= 1e-12
    assert np.array_equal(r.c_T_r[3], ref.IDENTITY7) and np.array_equal(r.r_T_t[6], ref.IDENTITY7)
    assert not np.array_equal(r.r_T_t[2], ref.IDENTITY7)
    # view 2 does not enter c_T_r: dropping it entirely leaves every camera pose bitwise unchanged
    r2, _, _, _ = _run([mv for i, mv in enumerate(views) if i != 2], K)
    assert np.array_equal(r2.c_T_r, r.c_T_r)


def test_sequential_sign_rule_on_device(gpu_lib):
    """Camera 1's pose relative to camera 0 turns about the optical axis by 0, 150 and 250 degrees across the views (noise free):
    the average must be the running-sum one of the restatement, not the align-to-first one."""
    cam = synth.camera_gt(capi.CAMERA_PINHOLE_BC, False)
    grid = synth.make_target_grid(8, 11, 0.02)
    rng = np.random.default_rng(5)
    r_T_t = synth.random_view_poses(3, rng, max_tilt_deg=10.0)
    views = []
    for T, deg in zip(r_T_t, (0.0, 150.0, 250.0)):
        C1 = make_pose(np.array([0.01, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.deg2rad(deg))
        views.append([synth.render_view(cam, T, grid), synth.render_view(cam, C1 @ T, grid)])
    K = np.stack([cam[:5], cam[:5]])
    r, bv, bc, arrs = _run(views, K)
    T = {(int(v), int(c)): ref.matrix_of(p) for v, c, p in zip(bv, bc, r.blk_pose)}
    rels = [ref.rel_pose(T[(v, 1)], T[(v, 0)]) for v in range(3)]
    qs = [rotmat_to_quat(M[:3, :3]) for M in rels]
    run = qs[0] + (qs[1] if qs[0] @ qs[1] >= 0 else -qs[1])
    assert min(abs(qs[0] @ qs[1]), abs(run @ qs[2]), abs(qs[0] @ qs[2])) >= 1e-3  # every sign test clear of zero
    assert (run @ qs[2] < 0) != (qs[0] @ qs[2] < 0)
    want, wrong = ref.average_isometries(rels), ref.average_align_to_first(rels)
    assert np.abs(r.c_T_r[1] - want).max() <= 1e-12
    assert np.abs(ref.matrix_of(r.c_T_r[1])[:3, :3] - ref.matrix_of(wrong)[:3, :3]).max() > 0.1


def test_invariance(gpu_lib):
    cams, views = _scene(3, 12, 21)
    K = cams[:, :5]
    r, bv, bc, _ = _run(views, K)
    perm = np.random.default_rng(0).permutation(len(bv))
    rp, bvp, bcp, _ = _run(views, K, order=perm)
    assert np.array_equal(rp.c_T_r, r.c_T_r) and np.array_equal(rp.r_T_t, r.r_T_t)
    assert np.array_equal(rp.blk_pose, r.blk_pose[perm]) and np.array_equal(bvp, bv[perm])
    again, _, _, _ = _run(views, K)
    for a, b in ((again.c_T_r, r.c_T_r), (again.r_T_t, r.r_T_t), (again.blk_pose, r.blk_pose), (again.blk_ok, r.blk_ok)):
        assert np.array_equal(a, b)
    # a fourth camera changes nothing about cameras 1 and 2
    cams4, views4 = _scene(4, 12, 22)
    views_plus = [mv + [mv4[3]] for mv, mv4 in zip(views, views4)]
    r4, _, _, _ = _run(views_plus, np.vstack([K, cams4[3:, :5]]))
    assert np.array_equal(r4.c_T_r[:3], r.c_T_r)


def _views_of(sc):
    return [[np.asarray(pv) for pv in mv] for mv in sc["views"]]


def _approx(a, b, prec):
    """Eigen's isApprox: |a - b| <= prec * min(|a|, |b|)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


def test_kat_recover_all_parameters(gpu_lib):
    """Extrinsics.RecoverAllParameters (extrinsics_test.cpp:75-140): DLT seed with the exact K, target 0 anchored."""
    sc = _kat("extrinsics_all_parameters")
    views = _views_of(sc)
    guess = rig.estimate_extrinsic_dlt(views, [np.asarray(c) for c in sc["cams_gt"]])
    assert _approx(guess.c_se3_r[0], np.eye(4), 1e-12)
    guess.r_se3_t[0] = np.asarray(sc["r_T_t_gt"][0])
    res = optim.optimize_extrinsics(views, [np.asarray(c) for c in sc["cams_init"]], guess.c_se3_r, guess.r_se3_t, optim.ExtrinsicOptions())
    assert res.core.final_cost < 1e-6
    assert len(res.cameras) == 2
    assert abs(res.cameras[0][0] - 100.0) <= 1e-3 and abs(res.cameras[0][1] - 100.0) <= 1e-3
    assert _approx(res.c_se3_r[1][:3, 3], np.asarray(sc["c_T_r_gt"][1])[:3, 3], 1e-3)
    assert _approx(res.r_se3_t[0][:3, 3], np.asarray(sc["r_T_t_gt"][0])[:3, 3], 1e-3)
    assert res.core.covariance is not None and np.trace(res.core.covariance) > 0.0


def test_kat_first_target_pose_fixed(gpu_lib):
    """Extrinsics.FirstTargetPoseFixed (extrinsics_test.cpp:142-199): DLT seed with the perturbed K, a wrong scale on target 0."""
    sc = _kat("extrinsics_first_target_fixed")
    views = _views_of(sc)
    cams0 = [np.asarray(c) for c in sc["cams_init"]]
    guess = rig.estimate_extrinsic_dlt(views, cams0)
    guess.r_se3_t[0][:3, 3] = [0.0, 0.0, 3.0]
    res = optim.optimize_extrinsics(views, cams0, guess.c_se3_r, guess.r_se3_t, optim.ExtrinsicOptions())
    assert _approx(res.r_se3_t[0][:3, 3], [0.0, 0.0, 3.0], 1e-12)
    assert res.core.final_cost > 0.1


def test_kat_stereo_facade(gpu_lib):
    """StereoCalibrationFacadeTest.CalibratesSyntheticData (stereo_calibration_test.cpp:22-124) through calibrate_rig."""
    cam = np.array([400.0, 400.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0])
    cam_poses = [np.eye(4), make_pose(np.array([0.5, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), 0.0)]
    targets = [make_pose(np.array([0.0, 0.0, 4.0]), np.array([0.0, 0.0, 1.0]), 0.0),
               make_pose(np.array([0.2, -0.1, 3.5]), np.array([0.0, 1.0, 0.0]), 0.15),
               make_pose(np.array([-0.1, 0.2, 4.5]), np.array([1.0, 0.0, 0.0]), -0.2)]
    obj = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5], [1.5, 0.5]])

    def render(T):
        P = obj[:, :1] * T[:3, 0] + obj[:, 1:] * T[:3, 1] + T[:3, 3]
        return np.c_[obj, 400.0 * P[:, 0] / P[:, 2], 400.0 * P[:, 1] / P[:, 2]]

    views = [[render(cam_poses[0] @ T), render(cam_poses[1] @ T)] for T in targets]
    res = rig.calibrate_rig(views, [cam, cam], optim.ExtrinsicOptions(optimize_intrinsics=False))
    assert res.success and res.used_views == 3 and res.requested_views == 3 and res.view_status == ["ok"] * 3
    assert len(res.optimization.c_se3_r) == 2 and len(res.optimization.r_se3_t) == 3
    assert _approx(res.optimization.c_se3_r[1][:3, 3], [0.5, 0.0, 0.0], 1e-2)
    for T, Tgt in zip(res.optimization.r_se3_t, targets):
        assert _approx(T[:3, 3], Tgt[:3, 3], 1e-2)


def test_c3_shaped_seed_reaches_the_same_optimum(gpu_lib):
    """500 views x 8 cameras x 5000 points with distortion and noise: optimize_extrinsics from the DLT seed (view 0 anchored to its
    ground truth) reaches the optimum it reaches from the scene's perturbed seed."""
    sc = synth.scene_extrinsics_shard(500, 0, 500)
    fa = sc.flat
    r = rig.estimate_extrinsic_dlt_blocks(fa.n_cams, fa.n_views, fa.blk_offset, fa.blk_view, fa.blk_cam, fa.X, fa.Y, fa.u, fa.v,
                                          fa.intr[:, :5])
    assert r.blk_ok.all()
    fb = helpers.clone(fa)
    fb.cam_pose[:] = r.c_T_r
    fb.view_pose[:] = r.r_T_t
    fb.view_pose[0] = sc.gt_view_pose[0]
    err_c = max(np.abs(pose_to_matrix(p)[:3, 3] - pose_to_matrix(g)[:3, 3]).max() for p, g in zip(r.c_T_r, sc.gt_cam_pose))
    print(f"DLT seed: largest camera translation error {err_c:.3e} m against ground truth")
    # the default tolerance (1e-9) stops both solves in the flat k2 / k3 valley 5e-4 apart at equal cost; at 1e-15 they stop at
    # the same cost with k3 still 7e-6 apart (measured): intrinsics are held to 2e-5, poses to 1e-6, costs to 1e-9
    copts = optim.to_cba_options(optim.OptimOptions(epsilon=1e-15, max_iterations=100, compute_covariance=False))
    sa, _ = optim._solve_flat(fa, copts)
    sb, _ = optim._solve_flat(fb, copts)
    print(sa.report, "|", sb.report)
    assert sa.termination != capi.TERM_FAILURE and sb.termination != capi.TERM_FAILURE, (sa.report, sb.report)
    assert abs(sa.final_cost - sb.final_cost) <= 1e-9 * sa.final_cost
    print("parameter gaps: intr", helpers.rel_diff(fb.intr, fa.intr))
    assert helpers.rel_diff(fb.intr, fa.intr) <= 2e-5
    for pa, pb in ((fa.cam_pose, fb.cam_pose), (fa.view_pose, fb.view_pose)):
        Ma = np.stack([pose_to_matrix(p) for p in pa])
        Mb = np.stack([pose_to_matrix(p) for p in pb])
        print("pose gap", helpers.rel_diff(Mb, Ma))
        assert helpers.rel_diff(Mb, Ma) <= 1e-6
