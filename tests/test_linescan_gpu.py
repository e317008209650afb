"""GPU tier of the laser-plane calibration (cba_calibrate_laser_plane, cba_fit_plane): the reference's KATs at their
tolerances (linescan_test.cpp, linescan_facade_test.cpp, linescan_utils_test.cpp, planefit_test.cpp; scenes restated by
tests/linescan_ref.py), random scenes against the numpy restatement, RANSAC with planted outliers, reproducibility and the
full-size case (1000 views x 4096 laser pixels)."""
import json
import os

import numpy as np
import pytest

from calibration_amd import capi, linescan
from calibration_amd.linescan import LineScanPlaneFitOptions, LineScanView, RansacOptions
from tests import linescan_ref as ref

pytestmark = pytest.mark.gpu

PINHOLE = np.array([800.0, 790.0, 640.0, 400.0, 0.5, -0.12, 0.03, -0.002, 0.0008, -0.0005])
SCHEIM = np.r_[PINHOLE, 0.03, -0.02]
N_TRUE = np.array([0.1, 1.0, -0.1]) / np.linalg.norm([0.1, 1.0, -0.1])


def _views(pairs):
    return [LineScanView(tv, lv) for tv, lv in pairs]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(GOLDEN, "linescan_kats.json")) as f:  # tests/golden/gen_linescan.py
        return json.load(f)


def _jviews(js):
    return [LineScanView(np.array(v["target_view"], dtype=float).reshape(-1, 4), np.array(v["laser_uv"], dtype=float).reshape(-1, 2))
            for v in js]


# ---- reference KATs (scenes: tests/golden/linescan_kats.json, planefit_points.txt) ----------------------------------------
def test_kat_plane_fit_multiple_views(gpu_lib, kats):
    k = kats["plane_fit_multiple_views"]
    # PinholeCamera<DualDistortion>(K, Zero(5))
    res = linescan.calibrate_laser_plane(_jviews(k["views"]), k["intr"], inverse_coeffs=k["inverse_coeffs"])
    assert np.abs(res.plane - k["plane"]).max() <= 1e-6
    assert abs(res.rms_error) <= 1e-9
    assert res.summary == "linear_svd" and res.n_views_used == 2 and res.inlier_count == res.n_points
    assert np.allclose(res.covariance, 0.0)


def test_kat_facade(gpu_lib, kats):
    k = kats["facade"]
    run = linescan.LinescanCalibrationFacade().calibrate(k["intr"], _jviews(k["views"]))
    assert run.success and run.used_views == 2
    assert np.abs(run.result.plane[:3] - k["plane"][:3]).max() <= 1e-3
    assert abs(run.result.plane[3] - k["plane"][3]) <= 1e-2


def test_kat_points_from_view(gpu_lib, kats):
    k = kats["points_from_view"]
    tv, lv = np.array(k["target_view"], dtype=float), np.array(k["laser_uv"], dtype=float)
    pts = linescan.points_from_view(LineScanView(tv, lv), k["intr"], inverse_coeffs=k["inverse_coeffs"])
    assert pts.shape == (3, 3)
    assert np.abs(pts - ref.points_from_view(tv, lv, np.array(k["intr"]), np.array(k["inverse_coeffs"]))).max() <= 1e-12


def test_kat_fit_plane_svd_detects_plane(gpu_lib, kats):
    k = kats["fit_plane_svd_grid"]
    assert np.abs(linescan.fit_plane_svd(k["points"]) - k["plane"]).max() <= 1e-12


def test_kat_plane_rms_zero_for_exact_points(gpu_lib, kats):
    pts = np.array(kats["plane_rms_exact"]["points"])
    plane = linescan.fit_plane_svd(pts)
    assert linescan.plane_rms(pts, plane) <= 1e-12
    _, rms, cnt, _ = linescan._fit(pts, linescan._options(None), False)
    assert rms <= 1e-12 and cnt == 3


def test_kat_svd_matches_ideal_plane(gpu_lib, kats):
    k = kats["svd_ideal_plane"]
    plane = linescan.fit_plane_svd(k["points"])
    assert np.abs(plane - ref.plane_sign(np.array(k["plane"]), 1.0)).max() <= 1e-9


def test_kat_ransac_rejects_outliers(gpu_lib):
    # the reference's own points: std::mt19937(1337) through libstdc++'s uniform_real_distribution (gen_planefit_points.cpp)
    pts = np.loadtxt(os.path.join(GOLDEN, "planefit_points.txt"))
    assert pts.shape == (140, 3)
    n = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    gt = np.r_[n, -n[2]]
    thresh = 0.01
    r = linescan.fit_plane_ransac(pts, RansacOptions(max_iters=2000, thresh=thresh, min_inliers=80, confidence=0.999))
    assert r.success and r.inliers.size >= 100
    est = r.plane if r.plane[:3] @ gt[:3] >= 0 else -r.plane  # align (planefit_test.cpp:18-20)
    assert np.abs(est - gt).max() <= 1e-3
    assert r.inlier_rms < 1e-3
    res = np.abs(pts[r.inliers] @ r.plane[:3] + r.plane[3])
    assert int((res < thresh).sum()) == r.inliers.size  # counted_inliers == inliers.size() (strict <, as the reference counts)


def test_kat_plane_fit_fails_single_view(gpu_lib, kats):
    k = kats["plane_fit_single_view"]
    with pytest.raises(capi.CbaInvalidArgument):
        linescan.calibrate_laser_plane(_jviews(k["views"]), k["intr"], inverse_coeffs=k["inverse_coeffs"])


def test_ransac_without_a_model_is_a_runtime_error(gpu_lib):
    pts = np.random.default_rng(0).normal(size=(50, 3))
    # every point of a view lies exactly on that view's target plane, so only a min_inliers above the point count rules out a model
    opts = LineScanPlaneFitOptions(True, RansacOptions(thresh=1e-9, min_inliers=10 ** 7))
    with pytest.raises(capi.CbaError) as e:
        linescan.calibrate_laser_plane(_views(ref.random_scene(np.random.default_rng(1), 3, PINHOLE, N_TRUE, 0.05, noise_px=0.5)),
                                       PINHOLE, opts)
    assert e.value.status == capi.CBA_ERR_RUNTIME
    assert not linescan.fit_plane_ransac(pts, RansacOptions(thresh=1e-9, min_inliers=10)).success


# ---- random scenes against the numpy restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("intr,dual", [(PINHOLE, False), (PINHOLE, True), (SCHEIM, False)], ids=["pinhole-iterative", "pinhole-dual", "scheimpflug"])
def test_random_scene_matches_numpy(gpu_lib, intr, dual):
    rng = np.random.default_rng(11)
    pairs = ref.random_scene(rng, 12, intr, N_TRUE, 0.05, noise_px=0.1)
    inv = ref.invert_brown_conrady(intr[5:10]) if dual else None
    res = linescan.calibrate_laser_plane(_views(pairs), intr, inverse_coeffs=inv, return_points=True, return_mask=True)
    plane, rms, pts = ref.calibrate_laser_plane(pairs, intr, inv)
    want = np.concatenate(pts, axis=0)
    assert np.abs(res.points - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(res.plane - plane).max() <= 1e-9
    assert abs(res.rms_error - rms) <= 1e-9 * max(rms, 1e-300) + 1e-15
    assert res.n_points == want.shape[0] and res.inlier_count == want.shape[0] and res.inlier_mask.all()
    assert np.abs(res.plane[:3] - N_TRUE).max() < 1e-2  # and it is the laser plane


def test_degenerate_view_is_skipped(gpu_lib):
    rng = np.random.default_rng(12)
    pairs = ref.random_scene(rng, 5, PINHOLE, N_TRUE, 0.05, noise_px=0.1)
    bad_tv = pairs[2][0].copy()
    bad_tv[3, 2] = np.nan  # a lost corner: the homography is not finite
    pairs[2] = (bad_tv, pairs[2][1])
    res = linescan.calibrate_laser_plane(_views(pairs), PINHOLE, return_points=True, return_mask=True)
    assert res.n_views_used == 4
    off = np.cumsum([0] + [lv.shape[0] for _, lv in pairs])
    assert np.isnan(res.points[off[2]:off[3]]).all() and np.isfinite(np.delete(res.points, np.s_[off[2]:off[3]], axis=0)).all()
    assert not res.inlier_mask[off[2]:off[3]].any()
    good = [p for i, p in enumerate(pairs) if i != 2]
    plane, _, _ = ref.calibrate_laser_plane(good, PINHOLE)
    assert np.abs(res.plane - plane).max() <= 1e-9


def _outlier_scene(rng, n_views, n_pix, frac, intr):
    pairs = ref.random_scene(rng, n_views, intr, N_TRUE, 0.05, noise_px=0.1, n_samples=n_pix)
    truth = []
    for k, (tv, lv) in enumerate(pairs):
        out = rng.random(lv.shape[0]) < frac
        lv = lv.copy()
        lv[out] = rng.uniform([200, 100], [1080, 700], size=(int(out.sum()), 2))
        pairs[k] = (tv, lv)
        truth.append(~out)
    return pairs, np.concatenate(truth)


def test_ransac_recovers_plane_with_outliers(gpu_lib):
    rng = np.random.default_rng(13)
    pairs, truth = _outlier_scene(rng, 200, 2048, 0.3, PINHOLE)
    # 3.5 sigma of the points' distance to the plane (0.1 px at ~1 m): a much wider band makes the inlier count flat over a
    # range of planes, and the most inliers need not be the best plane
    thresh = 5e-4
    opts = LineScanPlaneFitOptions(True, RansacOptions(max_iters=500, thresh=thresh, min_inliers=1000))
    res = linescan.calibrate_laser_plane(_views(pairs), PINHOLE, opts, return_points=True, return_mask=True)
    assert res.summary == "ransac"
    # the plane of the true inliers, within the noise
    pts = res.points
    good = ref.fit_plane_svd(pts[truth])
    assert np.abs(res.plane - good).max() <= 2e-4
    assert np.abs(res.plane[:3] - N_TRUE).max() <= 5e-3
    # the mask is the inlier set of the returned plane, and matches the truth away from the threshold band
    r = np.abs(pts @ res.plane[:3] + res.plane[3])
    assert np.array_equal(res.inlier_mask, r <= thresh)
    assert res.inlier_count == int(res.inlier_mask.sum())
    assert abs(res.rms_error - np.sqrt(np.mean(r[res.inlier_mask] ** 2))) <= 1e-12
    # against the truth, away from the threshold band of the TRUE plane (the plane of the true inliers): every true inlier
    # well inside the band is reported, no planted outlier well outside it is, and the planted outliers that fall inside the
    # band are reported (RANSAC cannot tell them apart; the scene is built so that some do)
    rt = np.abs(pts @ good[:3] + good[3])
    assert np.all(res.inlier_mask[truth & (rt < 0.5 * thresh)])
    assert not np.any(res.inlier_mask[~truth & (rt > 2.0 * thresh)])
    in_band = ~truth & (rt < 0.5 * thresh)
    assert in_band.sum() > 0 and np.all(res.inlier_mask[in_band])
    # the exact refit: the plane is the SVD plane of the inlier set of the winner's raw model; it agrees with the SVD plane of
    # the returned inlier set to within the change of that set
    assert np.abs(res.plane - ref.fit_plane_svd(pts[res.inlier_mask])).max() <= 1e-4


def test_ransac_without_refit_returns_a_raw_three_point_model(gpu_lib):
    """refit_on_inliers = 0: the returned plane is the winning hypothesis itself (the plane through three of the points) and
    its inliers are counted against it."""
    rng = np.random.default_rng(16)
    pairs, truth = _outlier_scene(rng, 60, 1024, 0.3, PINHOLE)
    thresh = 5e-4
    opts = LineScanPlaneFitOptions(True, RansacOptions(max_iters=400, thresh=thresh, min_inliers=1000, refit_on_inliers=False))
    res = linescan.calibrate_laser_plane(_views(pairs), PINHOLE, opts, return_points=True, return_mask=True)
    pts = res.points
    r = np.abs(pts @ res.plane[:3] + res.plane[3])
    assert np.sort(r)[2] <= 1e-12 * np.abs(pts).max()  # three points lie on it exactly
    assert np.array_equal(res.inlier_mask, r <= thresh) and res.inlier_count == int(res.inlier_mask.sum())
    assert abs(res.rms_error - np.sqrt(np.mean(r[res.inlier_mask] ** 2))) <= 1e-12
    refit = linescan.calibrate_laser_plane(_views(pairs), PINHOLE, LineScanPlaneFitOptions(True, RansacOptions(
        max_iters=400, thresh=thresh, min_inliers=1000)))
    assert np.sort(np.abs(pts @ refit.plane[:3] + refit.plane[3]))[2] > 1e-11  # the refit is not a three-point plane
    good = ref.fit_plane_svd(pts[truth])
    assert np.abs(res.plane[:3] - good[:3]).max() <= 5e-3


def test_two_calls_are_bitwise_identical(gpu_lib):
    rng = np.random.default_rng(14)
    pairs, _ = _outlier_scene(rng, 40, 1024, 0.2, SCHEIM)
    for opts in (None, LineScanPlaneFitOptions(True, RansacOptions(max_iters=300, thresh=2e-3))):
        a = linescan.calibrate_laser_plane(_views(pairs), SCHEIM, opts, return_points=True, return_mask=True)
        b = linescan.calibrate_laser_plane(_views(pairs), SCHEIM, opts, return_points=True, return_mask=True)
        assert a.plane.tobytes() == b.plane.tobytes() and a.homography.tobytes() == b.homography.tobytes()
        assert a.rms_error == b.rms_error and a.inlier_count == b.inlier_count
        assert a.points.tobytes() == b.points.tobytes() and np.array_equal(a.inlier_mask, b.inlier_mask)


def test_full_size(gpu_lib):
    """1000 views x 4096 laser pixels (4.1e6 points): the SVD form against numpy to 1e-9, RANSAC with max_iters = 1000."""
    rng = np.random.default_rng(15)
    pairs = ref.random_scene(rng, 1000, PINHOLE, N_TRUE, 0.05, noise_px=0.1, n_samples=4096)
    views = _views(pairs)
    res = linescan.calibrate_laser_plane(views, PINHOLE, return_points=True)
    assert res.n_points == 1000 * 4096
    plane = ref.fit_plane_svd(res.points)
    assert np.abs(res.plane - plane).max() <= 1e-9
    assert abs(res.rms_error - ref.plane_rms(res.points, plane)) <= 1e-9 * res.rms_error
    # points_xyz against the restatement on a sample of views
    off = np.cumsum([0] + [lv.shape[0] for _, lv in pairs])
    for k in (0, 499, 999):
        want = ref.points_from_view(pairs[k][0], pairs[k][1], PINHOLE)
        assert np.abs(res.points[off[k]:off[k + 1]] - want).max() <= 1e-10 * np.abs(want).max()
    rr = linescan.calibrate_laser_plane(views, PINHOLE, LineScanPlaneFitOptions(True, RansacOptions(max_iters=1000, thresh=2e-3)))
    assert rr.summary == "ransac" and rr.inlier_count >= 0.99 * res.n_points
    assert np.abs(rr.plane - res.plane).max() <= 1e-5
