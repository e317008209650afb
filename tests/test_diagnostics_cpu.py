"""CPU tier of the reprojection diagnostics: the C ABI symbols, the Python aggregation of per-block rows, the outlier-rejection
loop's bookkeeping on a stubbed solver, and the report's field names."""
import ctypes as C

import numpy as np
import pytest

import calibration_amd
from calibration_amd import capi, diagnostics as D
from calibration_amd.optim import FlatProblem


def test_symbols_exported_and_no_device(lib):
    for name in ("cba_reproj_residual_stats", "cba_reproj_residuals_fetch_blocks", "cba_reproj_residual_stats_timed"):
        assert hasattr(lib, name)
    if lib.cba_device_count() > 0:
        pytest.skip("a HIP device is visible")
    tot = np.zeros(4)
    assert lib.cba_reproj_residual_stats(None, 1.0, None, capi.dptr(tot)) == capi.CBA_ERR_NO_DEVICE
    assert lib.cba_reproj_residuals_fetch_blocks(None, 0, 1, float("inf"), None, None) == capi.CBA_ERR_NO_DEVICE
    ms = np.zeros(2)
    assert lib.cba_reproj_residual_stats_timed(None, 0, 2, capi.dptr(ms)) == capi.CBA_ERR_NO_DEVICE
    for name in ("ResidualStats", "RobustOptions", "refine_with_outlier_rejection", "build_planar_intrinsics_report", "view_errors"):
        assert hasattr(calibration_amd, name)


def test_compute_global_rms_formula():
    assert D.compute_global_rms([], []) == 0.0
    assert D.compute_global_rms([1.0, 2.0], [0, 0]) == 0.0
    # sqrt((1 * 2*10 + 4 * 2*30) / (2*10 + 2*30))
    assert D.compute_global_rms([1.0, 2.0], [10, 30]) == pytest.approx(np.sqrt((20 + 240) / 80), rel=1e-15)
    # views past the end of the counts weigh nothing (reports/intrinsics.cpp:22-23)
    assert D.compute_global_rms([1.0, 5.0], [10]) == pytest.approx(1.0, rel=1e-15)


def _stats(blk, blk_cam, blk_view, n_views, n_cams, chain=capi.CHAIN_EXTRINSIC):
    blk = np.asarray(blk, float)
    return D.ResidualStats(blk, np.array([blk[:, 0].sum(), blk[:, 1].max(), blk[:, 2].sum(), blk[:, 3].sum()]),
                           np.asarray(blk_cam), None if blk_view is None else np.asarray(blk_view), n_views, n_cams)


def test_aggregation_by_view_camera_and_global():
    # blocks: (view, cam) = (0,0) (0,1) (1,0) (2,1); sums of e2 and counts chosen by hand
    blk = [[8.0, 1.5, 0, 4], [18.0, 2.0, 1, 9], [0.5, 0.3, 0, 1], [0.0, 0.0, 0, 0]]
    st = _stats(blk, [0, 1, 0, 1], [0, 0, 1, 2], 3, 2)
    np.testing.assert_allclose(st.block_rms, [np.sqrt(8 / 8), np.sqrt(18 / 18), np.sqrt(0.5 / 2), 0.0], rtol=1e-15)
    np.testing.assert_allclose(st.view_rms, [np.sqrt(26 / 26), np.sqrt(0.5 / 2), 0.0], rtol=1e-15)
    np.testing.assert_array_equal(st.view_count, [13, 1, 0])
    np.testing.assert_allclose(st.camera_rms, [np.sqrt(8.5 / 10), np.sqrt(18 / 18)], rtol=1e-15)
    assert st.global_rms == pytest.approx(np.sqrt(26.5 / 28), rel=1e-14)
    assert st.global_rms == pytest.approx(st.total_rms, rel=1e-14)
    assert st.n_over == 1 and st.n_obs == 14 and st.max_px == 2.0
    # bundle chain: every block is its own view
    sb = _stats(blk, [0, 0, 0, 0], None, 4, 1, capi.CHAIN_BUNDLE)
    np.testing.assert_allclose(sb.view_rms, sb.block_rms, rtol=0)


def _flat_intrinsic(counts, chain=capi.CHAIN_INTRINSIC, blk_cam=None, blk_view=None, n_cams=1):
    views = []
    k = 0
    for n in counts:
        v = np.zeros((n, 4))
        v[:, 0] = np.arange(k, k + n)  # X = global observation id: lets the stub and the test track observations
        k += n
        views.append(v)
    nb = len(counts)
    blk_cam = np.zeros(nb, np.int32) if blk_cam is None else np.asarray(blk_cam, np.int32)
    blk_view = np.arange(nb, dtype=np.int32) if blk_view is None else np.asarray(blk_view, np.int32)
    n_views = int(blk_view.max()) + 1 if nb else 0
    return FlatProblem(chain, capi.CAMERA_PINHOLE_BC, views, blk_cam, blk_view, np.zeros((n_cams, 10)),
                       None if chain == capi.CHAIN_INTRINSIC else np.tile([1.0, 0, 0, 0, 0, 0, 0], (n_cams, 1)),
                       np.tile([1.0, 0, 0, 0, 0, 0, 0], (n_views, 1)), None)


class _Stub:
    """Drops the observations whose id (X) is listed for each round; records what every round was given."""

    def __init__(self, drops):
        self.drops = [set(d) for d in drops]
        self.seen = []

    def __call__(self, flat, opts, robust, device):
        r = len(self.seen)
        ids = flat.X.astype(int)
        self.seen.append((ids.copy(), flat.blk_view.copy() if flat.blk_view is not None else None, flat.n_views))
        bad = self.drops[r] if r < len(self.drops) else set()
        keep = np.array([i not in bad for i in ids])
        return "summary%d" % r, 1.5, 0.25 + r, keep


def test_robust_loop_bookkeeping():
    # 6 views of 10 observations: ids 0..59
    flat = _flat_intrinsic([10] * 6)
    # round 0: drop 3 in view 1, 7 in view 4 (leaves 3 < min_block_points=4: view 4 removed); round 1: drop one more in view 1
    stub = _Stub([{11, 12, 13, 40, 41, 42, 43, 44, 45, 46}, {15}])
    res = D.refine_with_outlier_rejection(flat, None, D.RobustOptions(threshold_px=1.5, min_block_points=4), round_fn=stub)
    assert res.converged and len(res.rounds) == 3
    assert [r[1] for r in res.rounds] == [10, 1, 0]
    assert res.rounds[0] == (1.5, 10, 0.25)
    assert res.removed_views == [4] and res.removed_blocks == [4]
    np.testing.assert_array_equal(res.block_map, [0, 1, 2, 3, 5])
    # masks over the ORIGINAL observations
    for b in range(6):
        want = np.ones(10, bool)
        if b == 1:
            want[[1, 2, 3, 5]] = False
        if b == 4:
            want[:] = False
        np.testing.assert_array_equal(res.keep[b], want)
    # round 2 solved exactly the kept observations, views renumbered 0..4
    ids, bv, nv = stub.seen[2]
    want_ids = [i for b in range(6) for i in range(10 * b, 10 * b + 10) if res.keep[b][i - 10 * b]]
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(bv, [0, 1, 2, 3, 4])
    assert nv == 5 and res.flat.n_obs == len(want_ids)
    assert res.summary == "summary2"
    assert flat.n_obs == 60  # the input is not modified


def test_robust_loop_stops_at_max_rounds():
    flat = _flat_intrinsic([10] * 5)
    stub = _Stub([{0}, {1}, {2}])
    res = D.refine_with_outlier_rejection(flat, None, D.RobustOptions(threshold_px=1.0, max_rounds=2), round_fn=stub)
    assert not res.converged and len(res.rounds) == 2
    # the last round's drops are reported but not applied: the masks describe the final solve's data
    assert not res.keep[0][0] and res.keep[0][1]
    assert res.flat.n_obs == 49


def test_robust_loop_errors():
    # intrinsic chain below 4 views
    flat = _flat_intrinsic([10] * 4)
    with pytest.raises(ValueError, match="4 required"):
        D.refine_with_outlier_rejection(flat, None, D.RobustOptions(threshold_px=1.0), round_fn=_Stub([set(range(0, 10))]))
    # a camera that loses every block (extrinsic chain, 3 views x 2 cameras)
    flat = _flat_intrinsic([5] * 6, chain=capi.CHAIN_EXTRINSIC, blk_cam=[0, 1, 0, 1, 0, 1], blk_view=[0, 0, 1, 1, 2, 2], n_cams=2)
    drop = set(range(5, 10)) | set(range(15, 20)) | set(range(25, 30))
    with pytest.raises(ValueError, match="camera"):
        D.refine_with_outlier_rejection(flat, None, D.RobustOptions(threshold_px=1.0), round_fn=_Stub([drop]))
    # a view that loses both its blocks is removed (extrinsic chains have no 4-view minimum)
    res = D.refine_with_outlier_rejection(flat, None, D.RobustOptions(threshold_px=1.0), round_fn=_Stub([set(range(10, 20))]))
    assert res.removed_views == [1] and res.removed_blocks == [2, 3]
    np.testing.assert_array_equal(res.flat.blk_view, [0, 0, 1, 1])
    with pytest.raises(ValueError):
        D.refine_with_outlier_rejection(flat, None, D.RobustOptions(max_rounds=0), round_fn=_Stub([]))


def test_report_field_names(monkeypatch):
    from calibration_amd import linear, optim

    views = [np.zeros((n, 4)) for n in (12, 20, 16, 9)]
    res = optim.IntrinsicsOptimizationResult(optim.OptimResult(success=True), np.r_[1000.0, 1001, 640, 360, 0, -0.1, 0.01, 0, 0, 0],
                                             [np.eye(4)] * 4)
    calib = linear.PlanarIntrinsicsCalibration(np.array([990.0, 995, 630, 350, 0]), [0, 2, 3], res, None, 4)
    monkeypatch.setattr(D, "view_errors", lambda v, c, p, device=0: [0.1, 0.2, 0.3, 0.4])
    rep = D.build_planar_intrinsics_report(calib, views, ["a.png", "b.png", "c.png", "d.png"])
    assert set(rep) == {"type", "algorithm", "options", "detector", "cameras"}
    cam = rep["cameras"][0]
    assert set(cam) == {"camera_id", "model", "image_size", "initial_guess", "result"}
    assert set(cam["initial_guess"]) == {"intrinsics", "used_view_indices", "warning_counts"}
    assert set(cam["initial_guess"]["warning_counts"]) == {"invalid_camera_matrix", "homography_decomposition_failures"}
    assert set(cam["result"]) == {"intrinsics", "distortion_model", "distortion_coefficients", "reprojection_rms_px", "per_view"}
    assert set(cam["result"]["intrinsics"]) == {"fx", "fy", "cx", "cy", "skew"}
    pv = cam["result"]["per_view"]
    assert [set(p) for p in pv] == [{"source_image", "corner_count", "rms_px", "used_in_linear_stage"}] * 4
    assert [p["used_in_linear_stage"] for p in pv] == [True, False, True, True]
    assert [p["corner_count"] for p in pv] == [12, 20, 16, 9]
    assert cam["result"]["reprojection_rms_px"] == D.compute_global_rms([0.1, 0.2, 0.3, 0.4], [12, 20, 16, 9])
    assert rep["type"] == "intrinsics" and rep["algorithm"] == "planar"
