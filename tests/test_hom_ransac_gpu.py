"""GPU tier of the intrinsic seed (hom_ransac.hip): estimate_homography with and without RANSAC, estimate_intrinsics and
calibrate_planar_intrinsics against the numpy restatement tests/hom_ransac_ref.py and the ground truth of synthetic scenes."""
import json
import os
import time

import numpy as np
import pytest

from calibration_amd import linear, optim
from calibration_amd.linescan import RansacOptions
from tests import hom_ransac_ref as ref

pytestmark = pytest.mark.gpu

K_TRUE = np.array([820.0, 790.0, 640.0, 360.0, 0.0])
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _scene(rng, n_views, nx=6, ny=9, step=0.03, noise=0.0):
    XY = ref.grid(nx, ny, step)
    views, poses = [], []
    for _ in range(n_views):
        R, t = ref.random_pose(rng, 0.5)
        views.append(ref.project_view(K_TRUE, R, t, XY, noise, rng))
        poses.append((R, t))
    return views, poses


def _kat(name):
    with open(os.path.join(GOLD, "intrinsics_seed_scenes.json")) as f:
        return json.load(f)[name]


def _isapprox(a, b, prec):
    """Eigen's isApprox: ||a - b||_F <= prec * min(||a||_F, ||b||_F)."""
    a, b = np.asarray(a), np.asarray(b)
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


def test_recovers_camera_matrix():
    """EstimateIntrinsics.RecoversCameraMatrix (intrinsics_estimate_test.cpp:11-55) on its own scene, at its own tolerances."""
    sc = _kat("recovers_camera_matrix")
    views = [np.asarray(v) for v in sc["views"]]
    res = linear.estimate_intrinsics(views)
    assert res.success and len(res.views) == len(views) == 8
    Kg = np.asarray(sc["cam_gt"][:5])
    assert np.abs(res.kmtx[:4] - Kg[:4]).max() <= 1e-6
    assert abs(res.kmtx[4] - Kg[4]) <= 1e-9
    for ve, T in zip(res.views, sc["c_T_t"]):
        T = np.asarray(T)
        Rg = ve.c_se3_t[:3, :3]
        assert _isapprox(T[:3, :3], Rg, 1e-6) or _isapprox(T[:3, :3], -Rg, 1e-6)
        tg = ve.c_se3_t[:3, 3]
        assert abs(np.dot(tg / np.linalg.norm(tg), T[:3, 3] / np.linalg.norm(T[:3, 3]))) > 0.999


def test_fails_with_too_few_views():
    """EstimateIntrinsics.FailsWithTooFewViews (intrinsics_estimate_test.cpp:57-82)."""
    res = linear.estimate_intrinsics([np.asarray(v) for v in _kat("too_few_views")["views"]])
    assert not res.success and res.views == []


def _ransac_opts(d):
    return RansacOptions(max_iters=d["max_iters"], thresh=d["thresh"], min_inliers=d["min_inliers"], seed=d["seed"],
                         refit_on_inliers=d["refit_on_inliers"])


def test_exact_homography():
    """HomographyTest.ExactHomography (homography_test.cpp:49-71): DLT, then optimize_homography, isApprox(H_true, 1e-6)."""
    sc = _kat("exact_homography")
    view = np.asarray(sc["view"])
    r = linear.estimate_homography(view)
    assert r.success
    o = optim.optimize_homography(view, r.hmtx)
    assert o.core.success and _isapprox(o.homography, sc["H_true"], 1e-6)


def test_noisy_homography():
    """HomographyTest.NoisyHomography (homography_test.cpp:73-93): rms < 0.25, optimised H isApprox(H_true, 1e-2)."""
    sc = _kat("noisy_homography")
    view = np.asarray(sc["view"])
    r = linear.estimate_homography(view)
    assert r.success and r.symmetric_rms_px < 0.25
    Hr = ref.dlt(view[:, :2], view[:, 2:])
    assert _rel(r.hmtx, Hr) <= 1e-9
    assert abs(r.symmetric_rms_px - ref.symmetric_rms_px(Hr, view, np.arange(len(view)))) <= 1e-9
    o = optim.optimize_homography(view, r.hmtx)
    assert o.core.success and _isapprox(o.homography, sc["H_true"], 1e-2)


def test_ransac_recovers_homography_with_outliers():
    """HomographyTest.RansacRecoversHomographyWithOutliers (homography_test.cpp:103-133): 100 exact points + 30 random pairs,
    thresh 1, min_inliers 90, seed 123; then optimize_homography over the WHOLE view, outliers included."""
    sc = _kat("ransac_outliers")
    view = np.asarray(sc["view"])
    r = linear.estimate_homography(view, _ransac_opts(sc["ransac"]))
    assert r.success and len(r.inliers) >= 95 and r.symmetric_rms_px < 1e-3
    o = optim.optimize_homography(view, r.hmtx)
    assert o.core.success and _isapprox(o.homography, sc["H_true"], 1e-2)


def test_ransac_fails_with_too_few_inliers():
    """HomographyTest.RansacFailsWithTooFewInliers (homography_test.cpp:136-160): 4 exact points + 50 random, min_inliers 10."""
    sc = _kat("ransac_too_few_inliers")
    r = linear.estimate_homography(np.asarray(sc["view"]), _ransac_opts(sc["ransac"]))
    assert not r.success and len(r.inliers) == 0
    assert not linear.estimate_homography(np.asarray(sc["view"])[:3], RansacOptions()).success


@pytest.mark.parametrize("refit", [True, False])
def test_ransac_matches_numpy_on_small_views(refit):
    rng = np.random.default_rng(11)
    views = [ref.random_view(rng, K_TRUE, 40 + 7 * i, outlier_frac=0.25, noise_px=0.8)[0] for i in range(6)]
    opts = RansacOptions(max_iters=96, thresh=2.0, min_inliers=12, seed=99, refit_on_inliers=refit)
    got = linear.estimate_homography_batch(views, opts)
    for view, g in zip(views, got):
        ok, H, inl, rms, k = ref.ransac(view, 96, 2.0, 12, 99, refit)
        assert g.success == ok
        assert np.array_equal(g.inliers, inl)
        assert _rel(g.hmtx, H) <= 1e-9
        assert abs(g.symmetric_rms_px - ref.symmetric_rms_px(H, view, inl)) <= 1e-9


def test_planted_outliers_recovered_exactly():
    rng = np.random.default_rng(12)
    data = [ref.random_view(rng, K_TRUE, 400, outlier_frac=0.2) for _ in range(16)]
    got = linear.estimate_homography_batch([d[0] for d in data], RansacOptions(max_iters=256))
    for (view, planted), g in zip(data, got):
        assert g.success and np.array_equal(g.inliers, np.flatnonzero(planted))
        assert _rel(g.hmtx, ref.dlt(view[planted, :2], view[planted, 2:])) <= 1e-9


def test_zhang_on_noisy_views_matches_numpy():
    views, _ = _scene(np.random.default_rng(13), 20, noise=0.2)
    res = linear.estimate_intrinsics(views)
    assert res.success
    hs = [v.homography.hmtx for v in res.views]
    assert _rel(res.kmtx, ref.zhang(hs)) <= 1e-9
    assert np.abs(res.kmtx[:4] - K_TRUE[:4]).max() < 0.05 * K_TRUE.max()
    for ve in res.views:
        ok, R, t, _, _ = ref.pose_from_homography(res.kmtx, ve.homography.hmtx)
        assert ok and np.abs(ve.c_se3_t[:3, :3] - R).max() <= 1e-9 and _rel(ve.c_se3_t[:3, 3], t) <= 1e-9


@pytest.mark.parametrize("use_ransac", [False, True])
def test_failed_views_excluded_and_indexed(use_ransac):
    rng = np.random.default_rng(14)
    views, _ = _scene(rng, 7)
    bad_small = views[1][:3]
    line = views[4].copy()
    line[:, 1] = 0.0  # collinear object points
    # collinear object points fail only under RANSAC (is_degenerate rejects every sample); the reference's all-points DLT has no
    # degeneracy check and returns a finite, meaningless H for them, so the DLT case leaves that view out
    views = [views[0], bad_small, views[2], views[3]] + ([line] if use_ransac else []) + [views[5], views[6]]
    opts = linear.IntrinsicsEstimOptions(homography_ransac=RansacOptions(max_iters=128, min_inliers=8) if use_ransac else None)
    res = linear.estimate_intrinsics(views, opts)
    assert res.success
    assert [v.view_index for v in res.views] == ([0, 2, 3, 5, 6] if use_ransac else [0, 2, 3, 4, 5])
    assert _rel(res.kmtx, ref.zhang([v.homography.hmtx for v in res.views])) <= 1e-9


def test_batch_invariance_and_determinism():
    rng = np.random.default_rng(15)
    big = [ref.random_view(rng, K_TRUE, 120, outlier_frac=0.2, noise_px=0.3)[0] for _ in range(1000)]
    opts = RansacOptions(max_iters=300)
    a = linear.estimate_homography_batch(big, opts)
    b = linear.estimate_homography_batch(big, opts)
    for i in (0, 17, 999):
        alone = linear.estimate_homography(big[i], opts)
        for r in (a[i], b[i]):
            assert np.array_equal(alone.hmtx, r.hmtx) and np.array_equal(alone.inliers, r.inliers)
            assert alone.symmetric_rms_px == r.symmetric_rms_px
    assert all(np.array_equal(x.hmtx, y.hmtx) and x.symmetric_rms_px == y.symmetric_rms_px for x, y in zip(a, b))


def test_calibrate_planar_intrinsics_end_to_end():
    views, _ = _scene(np.random.default_rng(16), 12, 8, 11, 0.025, noise=0.2)
    out = linear.calibrate_planar_intrinsics(views)
    lin = linear.estimate_intrinsics(views)
    assert np.array_equal(out.linear_kmtx, lin.kmtx) and out.linear_view_indices == list(range(12))
    assert out.refine_result.core.success
    cam = out.refine_result.camera
    assert np.abs(cam[:4] - K_TRUE[:4]).max() < 2.0
    seeds = optim.estimate_planar_pose_batch(views, lin.kmtx)
    again = optim.optimize_intrinsics(views, np.r_[lin.kmtx, np.zeros(5)], seeds)
    assert np.array_equal(again.camera, cam)
    with pytest.raises(RuntimeError):
        linear.calibrate_planar_intrinsics(views[:3])


def test_full_size_batch():
    """1000 views x 10 000 points x 1000 hypotheses in one call; planted inlier sets on a sample of views."""
    rng = np.random.default_rng(17)
    n_views, n = 1000, 10000
    sample = [0, 333, 999]
    views, planted = [], {}
    for i in range(n_views):
        v, p = ref.random_view(rng, K_TRUE, n, outlier_frac=0.2)
        views.append(v)
        if i in sample:
            planted[i] = p
    linear.estimate_homography_batch(views[:2], RansacOptions(max_iters=1000))  # warm-up (code objects, buffers)
    t0 = time.perf_counter()
    got = linear.estimate_intrinsics(views, linear.IntrinsicsEstimOptions(homography_ransac=RansacOptions(max_iters=1000)))
    wall = time.perf_counter() - t0
    assert got.success and len(got.views) == n_views
    for i in sample:
        assert np.array_equal(got.views[i].homography.inliers, np.flatnonzero(planted[i]))
    assert np.abs(got.kmtx[:4] - K_TRUE[:4]).max() < 1e-3 * K_TRUE.max()
    assert wall < 30.0, wall
