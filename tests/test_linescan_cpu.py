"""CPU tier of the laser-plane calibration: linescan_math.hpp (the per-lane device math) compiled for the host with a
SerialCoop driver (tests/linescan_cpu) against the numpy restatement tests/linescan_ref.py, cba_invert_brown_conrady (the
host-only entry point) against np.linalg.lstsq, and the C ABI's defaults and failure modes without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import capi, linescan
from calibration_amd.capi import CbaLaserPlaneResult, CbaPlaneFitOptions, dptr, i64ptr
from tests import host_build
from tests import linescan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PINHOLE = np.array([800.0, 790.0, 640.0, 400.0, 0.5, -0.12, 0.03, -0.002, 0.0008, -0.0005])
SCHEIM = np.r_[PINHOLE, 0.03, -0.02]


@pytest.fixture(scope="module")
def lscpu():
    lib = host_build.load("linescan_cpu")
    P = C.POINTER(C.c_double)
    lib.ls_unproject.argtypes = [C.c_int, P, C.c_int, P, C.c_int, P, P, P, P]
    lib.ls_points_from_view.argtypes = [C.c_int, P, C.c_int, P, C.c_int, P, P, P, P, C.c_int, P, P, P]
    lib.ls_points_from_view.restype = C.c_int
    lib.ls_fit_plane.argtypes = [C.c_int, P, P]
    lib.ls_sign.argtypes = [P, C.c_double]
    lib.ls_homography.argtypes = [P, P]
    lib.ls_hyp.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    return lib


def _model(intr):
    return 1 if len(intr) == 12 else 0


def _unproject(lscpu, intr, u, v, inv=None):
    x, y = np.zeros(u.size), np.zeros(u.size)
    lscpu.ls_unproject(_model(intr), dptr(np.ascontiguousarray(intr)), 0 if inv is None else inv.size, dptr(inv), u.size, dptr(u), dptr(v),
                       dptr(x), dptr(y))
    return x, y


@pytest.mark.parametrize("intr", [PINHOLE, SCHEIM], ids=["pinhole", "scheimpflug"])
@pytest.mark.parametrize("dual", [False, True], ids=["iterative", "dual"])
def test_unproject_matches_numpy(lscpu, intr, dual):
    rng = np.random.default_rng(3)
    u, v = rng.uniform(0, 1280, 500), rng.uniform(0, 800, 500)
    inv = ref.invert_brown_conrady(intr[5:10]) if dual else None
    x, y = _unproject(lscpu, intr, u, v, inv)
    xr, yr = ref.unproject(intr, u, v, inv)
    assert np.abs(x - xr).max() <= 1e-12 and np.abs(y - yr).max() <= 1e-12


def test_scheimpflug_unproject_inverts_projection(lscpu):
    """project(unproject(px)) == px through the projection the library implements (reproj_math.hpp), with a mild distortion
    where 5 fixed-point steps converge to machine precision."""
    intr = np.array([900.0, 905.0, 640.0, 400.0, 0.0, -0.02, 0.001, 0.0, 0.0002, -0.0001, 0.05, -0.04])
    rng = np.random.default_rng(4)
    u, v = rng.uniform(300, 980, 400), rng.uniform(150, 650, 400)
    x, y = _unproject(lscpu, intr, u, v)
    px = ref.project(intr, np.stack([x, y, np.ones_like(x)], axis=1))
    assert np.abs(px - np.stack([u, v], axis=1)).max() <= 1e-9


@pytest.mark.parametrize("intr", [PINHOLE, SCHEIM], ids=["pinhole", "scheimpflug"])
def test_points_from_view_matches_numpy(lscpu, intr):
    rng = np.random.default_rng(5)
    n_true = np.array([0.1, 1.0, -0.1]) / np.linalg.norm([0.1, 1.0, -0.1])
    views = ref.random_scene(rng, 6, intr, n_true, 0.05, noise_px=0.1)
    for tv, lv in views:
        m = lv.shape[0]
        pts = np.zeros((m, 3))
        cols = [np.ascontiguousarray(tv[:, k]) for k in range(4)]
        ok = lscpu.ls_points_from_view(_model(intr), dptr(intr), 0, dptr(None), tv.shape[0], *(dptr(c) for c in cols), m,
                                       dptr(np.ascontiguousarray(lv[:, 0])), dptr(np.ascontiguousarray(lv[:, 1])), dptr(pts))
        want = ref.points_from_view(tv, lv, intr)
        assert ok == 1
        assert np.abs(pts - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def test_degenerate_view_gives_no_points(lscpu):
    intr = PINHOLE
    tv = np.array([[0.0, 0.0, 640.0, 400.0], [1, 0, 700, 400], [1, 1, 700, 460], [0, 1, 640, 460], [0.5, 0.5, np.nan, 430]])
    # a lost corner (NaN pixel): the homography is not finite, the view gives no points (linescan.h:73-75)
    pts = np.zeros((2, 3))
    cols = [np.ascontiguousarray(tv[:, k]) for k in range(4)]
    lu = np.array([600.0, 700.0])
    ok = lscpu.ls_points_from_view(0, dptr(intr), 0, dptr(None), 5, *(dptr(c) for c in cols), 2, dptr(lu), dptr(lu.copy()), dptr(pts))
    assert ok == 0


def test_plane_fit_matches_svd(lscpu):
    rng = np.random.default_rng(6)
    n = np.array([0.3, -0.8, 0.52]) / np.linalg.norm([0.3, -0.8, 0.52])
    base = rng.normal(size=(3000, 3)) * [0.4, 0.1, 0.5] + [0.1, 0.2, 1.0]
    pts = base - np.outer(base @ n + 0.35, n) + rng.normal(scale=1e-4, size=(3000, 1)) * n
    pl = np.zeros(4)
    lscpu.ls_fit_plane(3000, dptr(np.ascontiguousarray(pts)), dptr(pl))
    want = ref.fit_plane_svd(pts)
    assert np.abs(pl - want).max() <= 1e-10
    assert pl[3] > 0


def test_sign_convention(lscpu):
    for p, scale, want in [([0.0, 0.6, -0.8, -0.5], 1.0, [0.0, -0.6, 0.8, 0.5]),  # d < 0: flipped
                           ([0.0, -0.6, 0.8, 0.5], 1.0, [0.0, -0.6, 0.8, 0.5]),  # d > 0: kept
                           ([0.0, 0.6, -0.8, 1e-15], 10.0, [0.0, -0.6, 0.8, -1e-15]),  # |d| tiny: largest |n_k| > 0
                           ([-0.9, 0.1, 0.0, 0.0], 1.0, [0.9, -0.1, 0.0, 0.0])]:
        a = np.array(p, dtype=float)
        lscpu.ls_sign(dptr(a), scale)
        assert np.array_equal(a, np.array(want))
        b = np.array(p, dtype=float)
        assert np.array_equal(ref.plane_sign(b, scale), np.array(want))


def test_plane_homography_is_build_plane_homography(lscpu):
    pl = np.r_[np.array([0.1, 1.0, -0.1]) / np.linalg.norm([0.1, 1.0, -0.1]), 0.5]
    H = np.zeros(9)
    lscpu.ls_homography(dptr(pl), dptr(H))
    n = pl[:3]
    tmp = np.array([0.0, 0.0, 1.0]) if abs(n[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    e1 = np.cross(n, tmp)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    e2 /= np.linalg.norm(e2)
    want = np.linalg.inv(np.stack([e1, e2, -pl[3] * n], axis=1))
    assert np.abs(H.reshape(3, 3) - want).max() <= 1e-12


def test_hypotheses_are_distinct_and_in_range(lscpu):
    idx = (C.c_int64 * 3)()
    for n in (3, 4, 17, 1000003):
        for k in range(200):
            lscpu.ls_hyp(1234567, k, n, idx)
            t = list(idx)
            assert len(set(t)) == 3 and all(0 <= i < n for i in t)


# ---- C ABI, host side -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forward", [[-0.12, 0.03, -0.002, 0.0008, -0.0005], [0.0, 0.0], [-0.3, 0.1, 0.001, -0.002],
                                     [0.05, -0.01, 0.002, 0.0, 0.0, 0.0]])
def test_invert_brown_conrady_matches_lstsq(lib, forward):
    got = linescan.invert_brown_conrady(forward)
    want = ref.invert_brown_conrady(forward)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12


def test_invert_brown_conrady_rejects_short_vector(lib):
    with pytest.raises(capi.CbaError) as e:
        linescan.invert_brown_conrady([0.1])
    assert e.value.status == capi.CBA_ERR_RUNTIME


def test_plane_fit_option_defaults(lib):
    o = CbaPlaneFitOptions()
    lib.cba_plane_fit_options_default(C.byref(o))  # RansacOptions, ransac.h:23-30
    assert (o.use_ransac, o.max_iters, o.thresh, o.min_inliers, o.confidence, o.seed, o.refit_on_inliers) == (0, 1000, 2.0, 12, 0.99, 1234567, 1)


def test_validation_before_device(lib):
    """validate_observations' errors are raised on the host, before any device is needed."""
    v = linescan.LineScanView(np.array([[0, 0, 1, 1], [1, 0, 2, 1], [1, 1, 2, 2], [0, 1, 1, 2.0]]), np.zeros((3, 2)))
    with pytest.raises(capi.CbaInvalidArgument):
        linescan.calibrate_laser_plane([v], PINHOLE)
    short = linescan.LineScanView(v.target_view[:3], v.laser_uv)
    with pytest.raises(capi.CbaInvalidArgument):
        linescan.calibrate_laser_plane([v, short], PINHOLE)
    with pytest.raises(capi.CbaInvalidArgument):
        linescan.fit_plane_svd(np.zeros((2, 3)))


def test_compute_calls_fail_loudly_without_device(lib):
    if lib.cba_device_count() > 0:
        pytest.skip("a GPU is visible: the no-device path is not reachable")
    v = linescan.LineScanView(np.array([[0, 0, 1, 1], [1, 0, 2, 1], [1, 1, 2, 2], [0, 1, 1, 2.0]]), np.ones((3, 2)))
    with pytest.raises(capi.CbaError) as e:
        linescan.calibrate_laser_plane([v, v], PINHOLE)
    assert e.value.status == capi.CBA_ERR_NO_DEVICE
    with pytest.raises(capi.CbaError) as e:
        linescan.fit_plane_svd(np.eye(3))
    assert e.value.status == capi.CBA_ERR_NO_DEVICE


def test_max_iters_is_bounded(lib):
    """max_iters above CBA_PLANE_FIT_MAX_ITERS is an argument error (checked before any device work)."""
    pts = np.eye(3)
    for bad in (0, (1 << 20) + 1, 2**31 - 1):
        with pytest.raises(capi.CbaInvalidArgument):
            linescan._fit(pts, linescan._options(linescan.LineScanPlaneFitOptions(True, linescan.RansacOptions(max_iters=bad))), False)


def test_points_from_view_raises_argument_errors(lib):
    """points_from_view maps only 'no points' to an empty result; a bad argument still raises."""
    v = linescan.LineScanView(np.array([[0, 0, 1, 1], [1, 0, 2, 1], [1, 1, 2, 2], [0, 1, 1, 2.0]]), np.ones((3, 2)))
    for inv in (np.zeros(1), np.zeros(17)):
        with pytest.raises(capi.CbaInvalidArgument):
            linescan.points_from_view(v, PINHOLE, inverse_coeffs=inv)


def test_linescan_kat_fixture_is_current():
    """tests/golden/linescan_kats.json is what tests/golden/gen_linescan.py writes."""
    import json
    from tests.golden import gen_linescan

    with np.errstate(all="ignore"):
        fresh = json.loads(json.dumps(gen_linescan.build()))
    with open(gen_linescan.OUT) as f:
        stored = json.load(f)
    assert stored.keys() == fresh.keys()
    for k in stored:
        a, b = json.dumps(stored[k], sort_keys=True), json.dumps(fresh[k], sort_keys=True)
        assert a == b, k


def test_planefit_fixture_is_libstdcxx_mt19937(tmp_path):
    """tests/golden/planefit_points.txt is what gen_planefit_points.cpp prints (std::mt19937(1337), libstdc++)."""
    src = os.path.join(ROOT, "tests", "golden", "gen_planefit_points.cpp")
    exe = str(tmp_path / "gen")
    subprocess.run(["g++", "-std=c++17", "-O2", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "tests", "golden", "planefit_points.txt")).read()
