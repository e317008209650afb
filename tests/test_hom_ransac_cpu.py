"""CPU tier of the intrinsic seed: hom_ransac_math.hpp (the per-lane device math) compiled for the host (tests/hom_ransac_cpu)
against the numpy restatement tests/hom_ransac_ref.py; the host-only entry points (Zhang, pose_from_homography,
sanitize_intrinsics) and the C ABI's defaults and argument errors without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from calibration_amd import capi, linear
from calibration_amd.capi import CbaRansacOptions, dptr, i32ptr, i64ptr
from calibration_amd.optim import CalibrationBounds
from tests import hom_ransac_ref as ref
from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TRUE = np.array([820.0, 790.0, 640.0, 360.0, 0.0])


@pytest.fixture(scope="module")
def hr():
    lib = host_build.load("hom_ransac_cpu")
    P, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.hr_sample_c.argtypes = [C.c_uint64, C.c_int64, C.c_int64, I]
    lib.hr_degenerate_c.argtypes = [P, P]
    lib.hr_fit4_c.argtypes = [P, P, P, P, P]
    lib.hr_residuals_c.argtypes = [P, C.c_int, P, P, P, P, C.c_double, P, I]
    lib.hr_refit_c.argtypes = [C.c_int, P, P, P, P, I, P]
    lib.hr_zhang_c.argtypes = [C.c_int, P, P]
    lib.hr_pose_c.argtypes = [P, P, P, P, P]
    return lib


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _cols(view):
    return [np.ascontiguousarray(view[:, k]) for k in range(4)]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_minimal_fit_matches_svd_null_vector(hr):
    rng = np.random.default_rng(1)
    for _ in range(200):
        view, _ = ref.random_view(rng, K_TRUE, 4)
        H = np.zeros(9)
        assert hr.hr_fit4_c(*(dptr(c) for c in _cols(view)), dptr(H))
        Hr = ref.dlt(view[:, :2], view[:, 2:])
        assert _rel(H.reshape(3, 3), Hr) <= 1e-9


def test_degeneracy_predicate(hr):
    rng = np.random.default_rng(2)
    for _ in range(300):
        P = rng.uniform(-1, 1, (4, 2))
        if rng.uniform() < 0.5:  # make a triplet (near-)collinear
            P[2] = P[0] + rng.uniform(-2, 2) * (P[1] - P[0]) + rng.normal(0, 1e-8, 2)
        view = np.c_[P, np.zeros((4, 2))]
        X, Y = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1])
        assert bool(hr.hr_degenerate_c(dptr(X), dptr(Y))) == ref.degenerate(view, [0, 1, 2, 3])


def test_residual_and_inlier_test(hr):
    rng = np.random.default_rng(3)
    view, _ = ref.random_view(rng, K_TRUE, 500, outlier_frac=0.2, noise_px=1.5)
    H = ref.dlt(view[:, :2], view[:, 2:])
    r, inl = np.zeros(500), np.zeros(500, dtype=np.int32)
    hr.hr_residuals_c(dptr(np.ascontiguousarray(H.reshape(9))), 500, *(dptr(c) for c in _cols(view)), 2.0, dptr(r), _ip(inl))
    rr = ref.residuals(H, view)
    assert np.abs(r - rr).max() <= 1e-9 * max(1.0, rr.max())
    away = np.abs(rr - 2.0) > 1e-9
    assert np.array_equal(inl[away].astype(bool), (rr <= 2.0)[away])


def test_refit_matches_svd_dlt(hr):
    rng = np.random.default_rng(4)
    for _ in range(20):
        view, planted = ref.random_view(rng, K_TRUE, 300, outlier_frac=0.3, noise_px=0.3)
        H = np.zeros(9)
        assert hr.hr_refit_c(300, *(dptr(c) for c in _cols(view)), _ip(planted.astype(np.int32)), dptr(H))
        Hr = ref.dlt(view[planted, :2], view[planted, 2:])
        assert _rel(H.reshape(3, 3), Hr) <= 1e-9


def _zhang_scene(rng, n_views, noise):
    hs = []
    for _ in range(n_views):
        view, _ = ref.random_view(rng, K_TRUE, 80, noise_px=noise)
        H = ref.dlt(view[:, :2], view[:, 2:])
        hs.append(H / H[2, 2])
    return hs


@pytest.mark.parametrize("noise", [0.0, 0.2])
def test_zhang_matches_svd(hr, lib, noise):
    rng = np.random.default_rng(5)
    hs = _zhang_scene(rng, 20, noise)
    h9 = np.ascontiguousarray(np.stack([h.reshape(9) for h in hs]))
    k5 = np.zeros(5)
    assert hr.hr_zhang_c(20, dptr(h9), dptr(k5))
    kr = ref.zhang(hs)
    assert np.abs(k5 - kr).max() <= 1e-9 * np.abs(kr[:4]).max()
    # the host-only C entry point is the same code
    assert np.array_equal(linear.zhang_intrinsics_from_hs(hs), k5)
    if noise == 0.0:
        assert np.abs(k5 - K_TRUE).max() <= 1e-6 * K_TRUE.max()


def test_zhang_needs_four_views(lib):
    rng = np.random.default_rng(6)
    assert linear.zhang_intrinsics_from_hs(_zhang_scene(rng, 3, 0.0)) is None


def test_pose_from_homography_matches_svd_polar(hr, lib):
    rng = np.random.default_rng(7)
    for _ in range(50):
        view, _ = ref.random_view(rng, K_TRUE, 60, noise_px=0.5)
        H = ref.dlt(view[:, :2], view[:, 2:])
        H = H * rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
        R, t, sc = np.zeros(9), np.zeros(3), np.zeros(2)
        assert hr.hr_pose_c(dptr(K_TRUE), dptr(np.ascontiguousarray(H.reshape(9))), dptr(R), dptr(t), dptr(sc))
        ok, Rr, tr, s, c = ref.pose_from_homography(K_TRUE, H)
        assert ok
        assert np.abs(R.reshape(3, 3) - Rr).max() <= 1e-9
        assert np.abs(t - tr).max() <= 1e-9 * np.abs(tr).max()
        assert abs(sc[0] - s) <= 1e-9 * abs(s) and abs(sc[1] - c) <= 1e-9 * c
        p = linear.pose_from_homography(K_TRUE, H)
        assert p.success and np.abs(p.c_se3_t[:3, :3] - Rr).max() <= 1e-9


def test_pose_from_homography_rejects_bad_k(lib):
    H = np.eye(3)
    assert not linear.pose_from_homography([800.0, 800.0, 0.0, 360.0, 0.0], H).success
    assert not linear.pose_from_homography([np.inf, 800.0, 640.0, 360.0, 0.0], H).success


def test_sanitize_kat_bit_exact(lib):
    """SanitizeIntrinsics.ClampsValuesWithinBounds (intrinsics_estimate_test.cpp:84-107)."""
    b = CalibrationBounds(fx_min=200.0, fy_min=150.0, cx_min=100.0, cx_max=200.0, cy_min=50.0, cy_max=75.0, skew_min=-1.0, skew_max=1.0)
    K, mod = linear.sanitize_intrinsics([-50.0, np.inf, -100.0, 2000.0, np.nan], b)
    assert mod
    assert K.tolist() == [200.0, 150.0, 150.0, 62.5, 0.0]
    K2, mod2 = linear.sanitize_intrinsics([300.0, 300.0, 150.0, 60.0, 0.5], b)
    assert not mod2 and K2.tolist() == [300.0, 300.0, 150.0, 60.0, 0.5]
    assert linear.sanitize_intrinsics([1.0, 2.0, 3.0, 4.0, 5.0], None) == (pytest.approx([1.0, 2.0, 3.0, 4.0, 5.0]), False)


def test_sampler_distinct_in_range_and_position_free(hr):
    idx = (C.c_int * 4)()
    for n in (4, 5, 7, 100, 10000):
        for k in range(300):
            hr.hr_sample_c(1234567, k, n, idx)
            got = list(idx)
            assert len(set(got)) == 4 and min(got) >= 0 and max(got) < n
            assert got == ref.sample(1234567, k, n)  # a function of (seed, k, n) only: no view position enters
    hr.hr_sample_c(1234567, 5, 4, idx)
    assert sorted(idx) == [0, 1, 2, 3]


def test_ransac_options_default(lib):
    o = CbaRansacOptions()
    lib.cba_ransac_options_default(C.byref(o))
    assert (o.max_iters, o.thresh, o.min_inliers, o.confidence, o.seed, o.refit_on_inliers) == (1000, 2.0, 12, 0.99, 1234567, 1)


def test_argument_errors_without_device(lib):
    off = np.array([0, 4], dtype=np.int64)
    z = np.zeros(4)
    H, rms = np.zeros(9), np.zeros(1)
    ok, cnt = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    o = CbaRansacOptions()
    lib.cba_ransac_options_default(C.byref(o))

    def hom(opts, **kw):
        a = dict(X=dptr(z), h9=dptr(H))
        a.update(kw)
        return lib.cba_estimate_homography_ransac_batch(1, i64ptr(off), a["X"], dptr(z), dptr(z), dptr(z), opts, a["h9"], i32ptr(ok),
                                                        i32ptr(cnt), dptr(rms), None)

    assert hom(C.byref(o), X=dptr(None)) == capi.CBA_ERR_INVALID_ARGUMENT
    assert hom(C.byref(o), h9=dptr(None)) == capi.CBA_ERR_INVALID_ARGUMENT
    for field, bad in (("max_iters", -1), ("max_iters", (1 << 16) + 1), ("thresh", -0.5), ("thresh", float("nan"))):
        b = CbaRansacOptions()
        lib.cba_ransac_options_default(C.byref(b))
        setattr(b, field, bad)
        assert hom(C.byref(b)) == capi.CBA_ERR_INVALID_ARGUMENT, field
    bad_off = np.array([0, -1], dtype=np.int64)
    assert lib.cba_estimate_homography_ransac_batch(1, i64ptr(bad_off), dptr(z), dptr(z), dptr(z), dptr(z), None, dptr(H), i32ptr(ok),
                                                    i32ptr(cnt), dptr(rms), None) == capi.CBA_ERR_INVALID_ARGUMENT
    # estimate_intrinsics: no views is an unsuccessful result, not an error; use_ransac without options is an error
    K = np.zeros(5)
    s, san = C.c_int32(7), C.c_int32(7)
    off0 = np.zeros(1, dtype=np.int64)
    assert lib.cba_estimate_intrinsics(0, i64ptr(off0), None, None, None, None, 0, None, None, None, 0, C.byref(s), dptr(K), C.byref(san),
                                       None, None, None, None, None, None) == capi.CBA_OK
    assert s.value == 0
    assert lib.cba_estimate_intrinsics(1, i64ptr(off), dptr(z), dptr(z), dptr(z), dptr(z), 1, None, None, None, 0, C.byref(s), dptr(K),
                                       C.byref(san), i32ptr(ok), dptr(H), dptr(rms), dptr(np.zeros(7)), i32ptr(cnt),
                                       None) == capi.CBA_ERR_INVALID_ARGUMENT
    lo = np.zeros(5)
    assert lib.cba_estimate_intrinsics(1, i64ptr(off), dptr(z), dptr(z), dptr(z), dptr(z), 0, None, dptr(lo), None, 0, C.byref(s), dptr(K),
                                       C.byref(san), i32ptr(ok), dptr(H), dptr(rms), dptr(np.zeros(7)), i32ptr(cnt),
                                       None) == capi.CBA_ERR_INVALID_ARGUMENT
    assert lib.cba_zhang_intrinsics_from_hs(4, None, dptr(K), C.byref(s)) == capi.CBA_ERR_INVALID_ARGUMENT


GOLD = os.path.join(ROOT, "tests", "golden")


def test_seed_fixture_is_what_the_committed_generator_emits(tmp_path):
    """tests/golden/intrinsics_seed_scenes.json is reproducible from tests/golden/gen_intrinsics_seed.cpp with the image's g++ /
    libstdc++ (the std::mt19937 streams and distributions the reference's tests draw from)."""
    import json

    exe = str(tmp_path / "gen_intrinsics_seed")
    subprocess.run(["g++", "-O0", "-std=c++20", "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(GOLD, "gen_intrinsics_seed.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(GOLD, "intrinsics_seed_scenes.json")) as f:
        assert out == f.read()
    d = json.loads(out)
    # sizes of the reference scenes
    assert [len(v) for v in d["recovers_camera_matrix"]["views"]] == [54] * 8
    assert [len(v) for v in d["too_few_views"]["views"]] == [35] * 3
    assert [len(d[k]["view"]) for k in ("exact_homography", "noisy_homography", "ransac_outliers", "ransac_too_few_inliers")] == [4, 50, 130, 54]
    # first draw of std::mt19937(42) through uniform_real_distribution(-100, 100), pinned as a number (libstdc++ takes 53 bits
    # from two 32-bit outputs 1608637542, 3421126067: lo + hi * 2^32); the two Vec2 arguments are evaluated right to left
    u = (1608637542 + 3421126067 * 2.0 ** 32) / 2.0 ** 64
    assert d["ransac_outliers"]["view"][0][1] == pytest.approx(-100.0 + 200.0 * u, abs=1e-12)
    # the exact scenes are what they say: H_true maps the 100 (4) inlier points exactly, the camera renders the views
    for k, n_in in (("ransac_outliers", 100), ("ransac_too_few_inliers", 4), ("exact_homography", 4)):
        v, H = np.asarray(d[k]["view"]), np.asarray(d[k]["H_true"])
        assert ref.residuals(H, v)[:n_in].max() < 1e-9
    sc = d["recovers_camera_matrix"]
    K = np.asarray(sc["cam_gt"][:5])
    for v, T in zip(sc["views"], sc["c_T_t"]):
        v, T = np.asarray(v), np.asarray(T)
        px = ref.project_view(K, T[:3, :3], T[:3, 3], v[:, :2])
        assert np.abs(px[:, 2:] - v[:, 2:]).max() < 1e-9
