"""GPU tier of the distortion fits and the linear intrinsic estimators (cba_fit_distortion_batch,
cba_estimate_intrinsics_linear_batch, cba_estimate_intrinsics_linear_iterative_batch): the reference's DistortionTest KATs at its
own tolerances, parity with the numpy restatement (tests/distortion_ref.py), ground truth, mixed and large batches, and bitwise
batch invariance."""
import json
import os

import numpy as np
import pytest

from calibration_amd import capi, distortion as D
from tests import distortion_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "distortion_scenes.json")) as _f:
    SC = json.load(_f)

K0 = np.array([800.0, 820.0, 400.0, 300.0, 0.0])


def _obs(name):
    return np.asarray(SC[name]["obs"]), np.asarray(SC[name]["camera"])


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _batch(obs_list):
    off = np.zeros(len(obs_list) + 1, np.int64)
    off[1:] = np.cumsum([len(o) for o in obs_list])
    cat = np.concatenate([o for o in obs_list if len(o)] or [np.zeros((0, 4))])
    return off, cat[:, 0], cat[:, 1], cat[:, 2], cat[:, 3]


# ---- the reference's KATs (tests/unit/distortion_test.cpp) ------------------------------------------------------------------
def test_exact_fit(gpu_lib):
    obs, K = _obs("exact_fit")
    r = D.fit_distortion(obs, K, 2)
    assert r is not None
    assert np.all(np.abs(r.distortion - [-0.2, 0.05, 0.001, -0.0005]) < 1e-10)


def test_noisy_fit(gpu_lib):
    obs, K = _obs("noisy_fit")
    r = D.fit_distortion(obs, K, 2)
    assert abs(r.distortion[0] + 0.2) < 0.01 and abs(r.distortion[1] - 0.05) < 0.01
    assert abs(r.distortion[2] - 0.001) < 0.001 and abs(r.distortion[3] + 0.0005) < 0.001


def test_dual_model_round_trip(gpu_lib):
    obs, K = _obs("dual_model")
    r = D.fit_distortion_dual(obs, K, 2)
    assert r is not None
    pt = np.array([[0.1, -0.2]])
    back = R.apply_distortion(R.apply_distortion(pt, r.forward), r.inverse)  # DualBrownConrady: undistort = apply(inverse)
    assert np.all(np.abs(back - pt) < 1e-4)


def test_fixed_coefficients(gpu_lib):
    obs, K = _obs("fixed")
    r = D.fit_distortion_full(obs, K, 2, [0, 3], [-0.2, -0.0005])
    assert r.distortion[0] == -0.2 and r.distortion[3] == -0.0005
    assert abs(r.distortion[1] - 0.05) < 1e-10 and abs(r.distortion[2] - 0.001) < 1e-10


def test_bad_fixed_index_is_an_error(gpu_lib):
    obs, K = _obs("bad_index")
    with pytest.raises(capi.CbaInvalidArgument):
        D.fit_distortion_full(obs, K, 2, [7], [])


# ---- parity with the restatement ------------------------------------------------------------------------------------------
FIT_GRID = [(nr, fixed) for nr in range(4) for fixed in ((), (0,), (nr + 1, 0))]


@pytest.mark.parametrize("nr,fixed", FIT_GRID)
def test_fit_matches_restatement(gpu_lib, nr, fixed):
    obs = R.make_scene(600, noise=0.5, seed=10 + nr)
    K = np.array([790.0, 815.0, 405.0, 296.0, 0.4])
    vals = [0.01 * (i + 1) for i in range(len(fixed))]
    off, x, y, u, v = _batch([obs])
    got = D.fit_distortion_batch(off, x, y, u, v, K, nr, list(fixed), vals, dual=True)
    ref_f, ref_i, ref_r = R.fit_distortion_dual(obs, K, nr, fixed, vals)
    assert got.ok[0] == 1
    assert _rel(got.coeffs[0], ref_f) <= 1e-9 and _rel(got.inverse[0], ref_i) <= 1e-9 and _rel(got.residuals, ref_r) <= 1e-9
    for j, i in enumerate(fixed):
        assert got.coeffs[0][i] == vals[j] and got.inverse[0][i] == vals[j]


ITER_GRID = [(nr, sk, mi) for nr in range(4) for sk in (False, True) for mi in (0, 1, 5, 400)]


@pytest.mark.parametrize("nr,use_skew,max_it", ITER_GRID)
def test_iterative_matches_restatement(gpu_lib, nr, use_skew, max_it):
    obs = R.make_scene(500, noise=0.5, seed=nr)
    ref = R.estimate_intrinsics_linear_iterative(obs, nr, max_it, use_skew)
    assert all(abs(c - 1e-6) / 1e-6 >= 1e-3 for c in ref["changes"])  # the scene stays clear of the stop threshold
    off, x, y, u, v = _batch([obs])
    got = D.estimate_intrinsics_linear_iterative_batch(off, x, y, u, v, nr, max_it, use_skew)
    assert got.status[0] == ref["status"] == capi.LINEAR_OK
    assert got.iterations[0] == ref["iterations"] and got.fallback[0] == ref["fallbacks"]
    assert _rel(got.kmtx[0], ref["K"]) <= 1e-9 and _rel(got.coeffs[0], ref["alpha"]) <= 1e-9


@pytest.mark.parametrize("use_skew", [False, True])
def test_linear_matches_restatement(gpu_lib, use_skew):
    obs = R.make_scene(300, noise=0.5, seed=3)
    off, x, y, u, v = _batch([obs, obs])
    from calibration_amd.optim import CalibrationBounds
    for b in (None, CalibrationBounds(skew_min=-1.0, skew_max=1.0)):
        got = D.estimate_intrinsics_linear_batch(off, x, y, u, v, b, use_skew)
        Kr, st, fb = R.estimate_intrinsics_linear(obs, None if b is None else (
            np.array([b.fx_min, b.fy_min, b.cx_min, b.cy_min, b.skew_min]), np.array([b.fx_max, b.fy_max, b.cx_max, b.cy_max, b.skew_max])),
            use_skew)
        assert list(got.status) == [st, st] and list(got.fallback) == [fb, fb]
        assert _rel(got.kmtx[0], Kr) <= 1e-9 and np.array_equal(got.kmtx[0], got.kmtx[1])


def test_four_k_camera_takes_the_fallback(gpu_lib):
    obs = R.make_scene(400, K=(3000.0, 3000.0, 1920.0, 1080.0, 0.0), seed=5)
    ref = R.estimate_intrinsics_linear_iterative(obs, 2, 5, False)
    cam = D.estimate_intrinsics_linear_iterative(obs, 2, 5, False)
    off, x, y, u, v = _batch([obs])
    got = D.estimate_intrinsics_linear_iterative_batch(off, x, y, u, v, 2, 5, False)
    assert got.fallback[0] == ref["fallbacks"] >= 1 and got.iterations[0] == ref["iterations"]
    assert cam.kmtx[0] == 2000.0 and cam.kmtx[1] == 2000.0
    assert _rel(cam.kmtx, ref["K"]) <= 1e-9


def test_ground_truth_noise_free(gpu_lib):
    obs = R.make_scene(2000, seed=21)
    cam_b = D.estimate_intrinsics_linear_iterative_batch(*_batch([obs]), 2, 1000, False)
    assert cam_b.status[0] == capi.LINEAR_OK and cam_b.iterations[0] < 1000  # stopped by the rule
    assert np.max(np.abs(cam_b.kmtx[0] - K0)) < 1e-4
    assert np.max(np.abs(cam_b.coeffs[0] - [-0.2, 0.05, 0.001, -0.0005])) < 1e-6


# ---- batches -----------------------------------------------------------------------------------------------------------------
def test_mixed_batch(gpu_lib):
    sizes = [0, 1, 7, 8, 88]
    obs = [R.make_scene(n, noise=0.3, seed=40 + n) for n in sizes]
    off, x, y, u, v = _batch(obs)
    K = np.tile(K0, (len(sizes), 1))
    f = D.fit_distortion_batch(off, x, y, u, v, K, 2, dual=True)
    assert list(f.ok) == [0, 0, 0, 1, 1]
    assert np.all(f.coeffs[:3] == 0) and np.all(f.residuals[: 2 * 8] == 0)
    for p in (3, 4):
        ref = R.fit_distortion_dual(obs[p], K0, 2)
        assert _rel(f.coeffs[p], ref[0]) <= 1e-9 and _rel(f.inverse[p], ref[1]) <= 1e-9
        assert _rel(f.residuals[2 * off[p]:2 * off[p + 1]], ref[2]) <= 1e-9
    it = D.estimate_intrinsics_linear_iterative_batch(off, x, y, u, v, 2, 5, False)
    assert list(it.status) == [capi.LINEAR_TOO_FEW, capi.LINEAR_TOO_FEW, capi.LINEAR_TOO_FEW, capi.LINEAR_OK, capi.LINEAR_OK]
    assert list(it.iterations[:3]) == [0, 0, 0] and np.all(it.kmtx[:3] == 0)
    lin = D.estimate_intrinsics_linear_batch(off, x, y, u, v)
    assert list(lin.status) == [capi.LINEAR_TOO_FEW, capi.LINEAR_TOO_FEW, capi.LINEAR_OK, capi.LINEAR_OK, capi.LINEAR_OK]


def test_degenerate_and_no_work(gpu_lib):
    obs = R.make_scene(50, seed=2)
    obs[:, 0] = 0.25
    it = D.estimate_intrinsics_linear_iterative_batch(*_batch([obs]), 2, 5, False)
    assert it.status[0] == capi.LINEAR_DEGENERATE
    z = D.fit_distortion_batch(np.zeros(1, np.int64), [], [], [], [], np.zeros((0, 5)), 2)
    assert z.coeffs.shape == (0, 4)


def test_batch_invariance_bitwise(gpu_lib):
    rng = np.random.default_rng(0)
    obs = [R.make_scene(int(n), noise=0.5, seed=100 + i) for i, n in enumerate(rng.integers(8, 9000, 6))]
    target = obs[2]
    alone_f = D.fit_distortion_batch(*_batch([target]), K0, 3, dual=True)
    alone_i = D.estimate_intrinsics_linear_iterative_batch(*_batch([target]), 3, 50, True)
    for arr in ([*obs], [obs[0][:3], *obs]):  # in a batch; at a shifted offset
        k = next(j for j, o in enumerate(arr) if o is target)
        b = _batch(arr)
        f = D.fit_distortion_batch(*b, np.tile(K0, (len(arr), 1)), 3, dual=True)
        i = D.estimate_intrinsics_linear_iterative_batch(*b, 3, 50, True)
        assert np.array_equal(f.coeffs[k], alone_f.coeffs[0]) and np.array_equal(f.inverse[k], alone_f.inverse[0])
        assert np.array_equal(f.residuals[2 * b[0][k]:2 * b[0][k + 1]], alone_f.residuals)
        assert np.array_equal(i.kmtx[k], alone_i.kmtx[0]) and np.array_equal(i.coeffs[k], alone_i.coeffs[0])
        assert i.iterations[k] == alone_i.iterations[0]
    again = D.fit_distortion_batch(*_batch([target]), K0, 3, dual=True)
    assert np.array_equal(again.coeffs, alone_f.coeffs) and np.array_equal(again.residuals, alone_f.residuals)


def test_many_small_problems(gpu_lib):
    P, n = 2000, 88
    obs = [R.make_scene(n, noise=0.2, seed=1000 + p) for p in range(P)]
    b = _batch(obs)
    it = D.estimate_intrinsics_linear_iterative_batch(*b, 2, 5, False)
    assert np.all(it.status == capi.LINEAR_OK)
    for p in (0, 777, P - 1):
        ref = R.estimate_intrinsics_linear_iterative(obs[p], 2, 5, False)
        assert it.iterations[p] == ref["iterations"] and it.fallback[p] == ref["fallbacks"]
        assert _rel(it.kmtx[p], ref["K"]) <= 1e-9 and _rel(it.coeffs[p], ref["alpha"]) <= 1e-9


def test_large_problem_against_lstsq(gpu_lib):
    obs = R.make_scene(2_000_000, noise=0.5, seed=77)
    K = np.array([801.0, 819.0, 399.0, 301.0, 0.0])
    f = D.fit_distortion_batch(*_batch([obs]), K, 2)
    ref_a, ref_r = R.fit_distortion_full(obs, K, 2)
    assert _rel(f.coeffs[0], ref_a) <= 1e-9 and _rel(f.residuals, ref_r) <= 1e-9


def test_chunk_counts_around_the_chunk_sum_tiling(gpu_lib):
    """Problems of 1, 63, 65 and 130 chunks (4096 observations each, plus a partial chunk): the chunk sum's share of each
    wavefront and its groups of chunks end inside and at their boundaries.  Each agrees with the restatement, and alone with
    itself in the batch, bit for bit."""
    sizes = [17, 63 * 4096, 64 * 4096 + 5, 129 * 4096 + 4095]
    obs = [R.make_scene(n, noise=0.5, seed=300 + i) for i, n in enumerate(sizes)]
    b = _batch(obs)
    f = D.fit_distortion_batch(*b, np.tile(K0, (len(sizes), 1)), 2)
    for p, o in enumerate(obs):
        ref_a, ref_r = R.fit_distortion_full(o, K0, 2)
        assert _rel(f.coeffs[p], ref_a) <= 1e-9 and _rel(f.residuals[2 * b[0][p]:2 * b[0][p + 1]], ref_r) <= 1e-9
        alone = D.fit_distortion_batch(*_batch([o]), K0, 2, want_residuals=False)
        assert np.array_equal(alone.coeffs[0], f.coeffs[p])
