"""GPU tier of the camera models (cba_camera_project / _unproject, cba_undistort_map_*): the device against the literal numpy
restatement tests/camera_ref.py, the oracle's projection and the host build of the same math; restated reference KATs; map
consistency; apply of whole image batches; repeatability; NaN and out-of-range map entries."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from calibration_amd import camera as cam
from calibration_amd import distortion as D
from tests import camera_ref as R
from tests import host_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_d = C.POINTER(C.c_double)
CAMS = R.cameras()


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


@pytest.fixture(scope="module")
def camcpu():
    return host_build.load("camera_cpu")


@pytest.mark.parametrize("n", [1, 63, 65, 1_000_000])
def test_project_unproject_against_restatement(gpu_lib, oracle, n):
    xyz = R.points(n, seed=n)
    rng = np.random.default_rng(n)
    for name, model, intr in CAMS:
        uv = cam.project(intr, xyz)
        assert _rel(uv, R.project(model, intr, xyz)) <= 1e-9, name
        idx = rng.choice(n, size=min(n, 10_000), replace=False)
        ref, orc = np.empty(2), np.empty((len(idx), 2))
        for j, i in enumerate(idx):
            oracle.orc_project(model, intr.ctypes.data_as(c_d), np.ascontiguousarray(xyz[i]).ctypes.data_as(c_d), ref.ctypes.data_as(c_d))
            orc[j] = ref
        assert _rel(uv[idx], orc) <= 1e-9, name
        for inv in (None, R.dual_inverse(intr[5:10])):
            xy = cam.unproject(intr, uv, inverse_coeffs=inv)
            assert _rel(xy, R.unproject(model, intr, uv, inv)) <= 1e-12, name


def test_device_matches_host_build(gpu_lib, camcpu):
    from tests.test_camera_cpu import host_project, host_unproject

    xyz = R.points(4097, seed=11)
    for name, model, intr in CAMS:
        uv = cam.project(intr, xyz)
        assert _rel(uv, host_project(camcpu, model, intr, xyz)) <= 1e-12, name
        assert _rel(cam.unproject(intr, uv), host_unproject(camcpu, model, intr, uv)) <= 1e-12, name


def test_distort_undistort_forms(gpu_lib):
    dist = np.array([-0.21, 0.08, -0.012, 0.0011, -0.0007])
    xy = R.points(1000, seed=2)[:, :2] / 3.0
    xd = cam.distort(dist, xy)
    assert _rel(xd, np.column_stack(R.apply_distortion(xy[:, 0], xy[:, 1], dist))) <= 1e-12
    u = cam.undistort(dist, xd)
    assert _rel(u, np.column_stack(R.undistort(xd[:, 0], xd[:, 1], dist))) <= 1e-12
    inv = R.dual_inverse(dist)
    assert _rel(cam.undistort(dist, xd, inverse_coeffs=inv), np.column_stack(R.apply_distortion(xd[:, 0], xd[:, 1], inv))) <= 1e-12


# ---- restated reference KATs (scheimpflug_test.cpp:11-50, distortion_test.cpp:109-126) ------------------------------------------
def test_kat_zero_tilt_matches_pinhole(gpu_lib):
    pin = np.array([800.0, 820.0, 320.0, 240.0, 0.0, 0, 0, 0, 0, 0])
    sch = np.concatenate([pin, [0.0, 0.0]])
    Xc = np.array([[0.2, -0.1, 1.0]])
    assert np.abs(cam.project(sch, Xc) - cam.project(pin, Xc)).max() <= 1e-9


def test_kat_principal_ray(gpu_lib):
    taux, tauy = 0.1, -0.2
    pin = np.array([600.0, 600.0, 400.0, 300.0, 0.0, 0, 0, 0, 0, 0])
    uv = cam.project(np.concatenate([pin, [taux, tauy]]), np.array([[0.0, 0.0, 1.0]]))
    m0 = np.array([[-np.tan(tauy) / np.cos(taux), np.tan(taux)]])
    assert np.abs(uv - cam.project(pin, m0)).max() <= 1e-9


def test_kat_dual_model_round_trip(gpu_lib):
    with open(os.path.join(ROOT, "tests", "golden", "distortion_scenes.json")) as f:
        sc = json.load(f)["dual_model"]
    d = D.fit_distortion_dual(np.asarray(sc["obs"]), np.asarray(sc["camera"]), 2)  # on the device
    fwd, inv = d.forward, d.inverse  # [k1, k2, p1, p2]
    coeffs = np.array([fwd[0], fwd[1], 0.0, fwd[2], fwd[3]])
    pt = np.array([[0.1, -0.2]])
    rec = cam.undistort(coeffs, cam.distort(coeffs, pt), inverse_coeffs=inv)
    assert np.abs(rec - pt).max() <= 1e-4


# ---- maps ----------------------------------------------------------------------------------------------------------------------
def _rig(model, W, H):
    intrs = np.stack([c[2] for c in CAMS if c[1] == model][:2]).copy()
    intrs[:, 0], intrs[:, 1], intrs[:, 2], intrs[:, 3] = 0.8 * W, 0.8 * W, W / 2.0, H / 2.0
    return intrs


def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


@pytest.mark.parametrize("W,H", [(1280, 960), (333, 101)])
@pytest.mark.parametrize("model", [R.PINHOLE, R.SCHEIMPFLUG])
def test_map_against_restatement_and_project(gpu_lib, model, W, H):
    intrs = _rig(model, W, H)
    Rs = np.stack([_rot(0.03, -0.05), _rot(1.3, 0.2)])  # the second turns part of the image behind the camera
    Kp = np.array([[0.7 * W, 0.72 * W, W / 2 + 3.5, H / 2 - 2.0, 0.2], [0.9 * W, 0.9 * W, W / 2, H / 2, 0.0]])
    with cam.UndistortMap(intrs, W, H, R=Rs, new_K=Kp) as m:
        mx, my = m.maps()
        mx2, my2 = m.maps()
    assert np.array_equal(mx, mx2, equal_nan=True) and np.array_equal(my, my2, equal_nan=True)
    for c in range(2):
        rx, ry = R.undistort_map(model, intrs[c], W, H, Rs[c], Kp[c])
        dx, dy = R.ulp_diff(mx[c], rx), R.ulp_diff(my[c], ry)
        assert not np.isnan(dx).any() and not np.isnan(dy).any(), "NaN pattern differs"
        assert dx.max() <= 1 and dy.max() <= 1
    assert not np.isnan(mx[0]).any()
    if H == 960:  # rows below y = cot(1.3) of camera 1 look behind it
        assert np.isnan(mx[1]).any()
    # a fetched entry is project() of the same ray rounded to float32
    rng = np.random.default_rng(W)
    vs, us = rng.integers(0, H, 500), rng.integers(0, W, 500)
    x, y = R.normalize(Kp[0], us.astype(float), vs.astype(float))
    P = np.stack([x, y, np.ones_like(x)], axis=1) @ Rs[0]
    uv = cam.project(intrs[0], P).astype(np.float32)
    assert R.ulp_diff(mx[0][vs, us], uv[:, 0]).max() <= 1 and R.ulp_diff(my[0][vs, us], uv[:, 1]).max() <= 1


def test_identity_map_is_the_pixel_grid(gpu_lib):
    W, H = 1283, 37  # a row tail
    intr = np.array([900.0, 905.0, 640.0, 18.0, 0.0, 0, 0, 0, 0, 0])
    with cam.UndistortMap(intr, W, H) as m:
        mx, my = m.maps()
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    assert np.array_equal(mx[0], u) and np.array_equal(my[0], v)


# ---- apply ---------------------------------------------------------------------------------------------------------------------
def _images(rng, n, h, w, ch, dtype):
    shape = (n, h, w) if ch == 1 else (n, h, w, ch)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(0.0, 1.0, shape).astype(np.float32)


def _check(out, ref, dtype):
    if dtype == np.uint8:
        assert np.array_equal(out, ref)
    else:
        assert np.max(np.abs(out - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-6


@pytest.mark.parametrize("ch,dtype", [(1, np.uint8), (3, np.uint8), (1, np.float32), (3, np.float32), (4, np.uint8), (2, np.float32)])
def test_apply_batch_against_restatement(gpu_lib, ch, dtype):
    W, H = 1280, 960
    intrs = _rig(R.PINHOLE, W, H)
    rng = np.random.default_rng(ch)
    imgs = _images(rng, 3, H, W, ch, dtype)
    cams = np.array([1, 0, 1], np.int32)
    with cam.UndistortMap(intrs, W, H, R=np.stack([_rot(0.02, 0.01), _rot(-0.03, 0.04)])) as m:
        mx, my = m.maps()
        out = m.apply(imgs, cams, border=17)
        again = m.apply(imgs, cams, border=17)
    assert np.array_equal(out, again)  # a repeated call is bitwise identical
    for i in range(3):
        _check(out[i], R.apply(imgs[i], mx[cams[i]], my[cams[i]], 17.0), dtype)


def test_apply_large_sampled(gpu_lib):
    W, H = 4096, 3000
    intr = _rig(R.SCHEIMPFLUG, W, H)[:1]
    rng = np.random.default_rng(4096)
    img = _images(rng, 1, H, W, 3, np.uint8)
    with cam.UndistortMap(intr, W, H) as m:
        mx, my = m.maps()
        out = m.apply(img, 0)
    idx = rng.choice(W * H, 100_000, replace=False)
    vs, us = idx // W, idx % W
    ref = R.apply(img[0], mx[0][vs, us][None], my[0][vs, us][None], 0.0)[0]
    assert np.array_equal(out[0][vs, us], ref)


def test_apply_nan_and_out_of_range_entries_give_border(gpu_lib):
    # a map whose R turns half the rays behind the camera (NaN entries) and whose K' sends others far outside the source
    W, H = 640, 480
    intr = np.array([500.0, 500.0, 320.0, 240.0, 0.0, 0, 0, 0, 0, 0])
    Kp = np.array([[2e-6, 2e-6, 320.0, 240.0, 0.0]])
    with cam.UndistortMap(intr, W, H, R=_rot(1.5707963267948966, 0.0)[None], new_K=Kp) as m:
        mx, my = m.maps()
        for dtype in (np.uint8, np.float32):
            img = _images(np.random.default_rng(1), 1, H, W, 1, dtype)
            out = m.apply(img, [0], border=200)
            bad = ~(np.abs(mx[0]) <= 2 ** 24) | ~(np.abs(my[0]) <= 2 ** 24)
            assert np.isnan(mx[0]).any() and (np.abs(mx[0]) > 2 ** 24).any()
            assert np.all(out[0][bad] == 200)
            _check(out[0], R.apply(img[0], mx[0], my[0], 200.0), dtype)
