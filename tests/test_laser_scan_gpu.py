"""GPU tier of laser profile scanning (cba_laser_points, cba_laser_scanner): the kernels against the numpy restatement
(tests/laser_scan_ref.py) and against the host build of the same header, at the sizes where the kernels change path - a width that
is or is not a multiple of the load width, frame bases that are unaligned, one and several workgroups - with the edge cases of the
peak rule planted, and the independence, determinism and handle checks."""
import functools
import json
import os

import numpy as np
import pytest

from calibration_amd import capi, linescan
from calibration_amd.linescan import LaserScanner, LaserScanOptions, LineScanView, laser_points
from tests import camera_ref as R
from tests import host_build
from tests import laser_scan_ref as S

pytestmark = pytest.mark.gpu

MODELS = [R.PINHOLE, R.SCHEIMPFLUG]
SIZES = [(1, 1), (3, 2), (67, 37), (64, 64), (130, 33), (257, 5)]


@pytest.fixture(scope="module")
def host():
    return host_build.load("laser_scan_cpu")


@functools.lru_cache(maxsize=None)
def _scene(model, W, H, axis, n_frames):
    out = S.scene(model, W, H, axis, n_frames)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def _opts(o):
    return LaserScanOptions(o.axis, o.roi_begin, o.roi_end, o.half_window, o.floor_level, o.min_peak)


def _gpu(intr, plane, images, o, poses=None, inv=None, max_frames=None):
    n, H, W = images.shape
    with LaserScanner(intr, plane, W, H, max_frames or n, _opts(o), inverse_coeffs=inv) as sc:
        r = sc.process(images, poses)
    return dict(centre=r.centre, amplitude=r.amplitude, width_px=r.width_px, xyz=r.xyz)


def _check(got, ref, u8):
    for k in ("centre", "amplitude", "width_px"):
        assert S.same_nan(got[k], ref[k]), k
        if u8:
            assert S.bitwise(got[k], ref[k]), k
        else:
            assert S.rel(got[k], ref[k]) <= 1e-12, k
    assert S.same_nan(got["xyz"], ref["xyz"]) and S.rel(got["xyz"], ref["xyz"]) <= 1e-12


def _both(host, model, intr, plane, images, o, poses=None, inv=None):
    got = _gpu(intr, plane, images, o, poses, inv)
    u8 = images.dtype == np.uint8
    _check(got, S.scan(model, intr, inv, plane, images, o, poses), u8)
    _check(got, S.host_scan(host, model, intr, inv, plane, images, o, poses), u8)
    return got


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("model", MODELS)
def test_sizes(gpu_lib, host, model, size, axis, n_frames):
    """both dtypes; three frames of 67 x 37 uint8 put the second frame's base on an odd address"""
    W, H = size
    intr, plane, _, _, f32, u8 = _scene(model, W, H, axis, n_frames)
    inv = R.dual_inverse(intr[5:10]) if W == 64 else None
    for img in (u8, f32):
        _both(host, model, intr, plane, img, S.Options(axis), S.frame_poses(n_frames) if n_frames == 3 else None, inv)


def _plants(axis, dtype):
    """the 67 x 37 scene, 3 frames, with one edge case per line of frame 0 (lines 0..11) inside the ROI [pb, pe)"""
    _, _, _, _, f32, u8 = _scene(R.PINHOLE, 67, 37, axis, 3)
    img = (u8 if dtype == np.uint8 else f32).copy()
    side = 37 if axis == 0 else 67
    pb, pe = 3, side - 4
    for l in range(12):
        S.line_view(img, axis, 0, l)[:] = 0
    L = [S.line_view(img, axis, 0, l) for l in range(12)]
    L[0][pb] = 250              # peak at the first ROI position
    L[0][pb - 1] = 255          # ... brighter samples outside the ROI do not count
    L[1][pe - 1] = 250          # peak at the last ROI position
    L[1][pe] = 255
    L[2][10] = 255              # plateaus of 1, 2 and 9 samples
    L[3][10:12] = 255
    L[4][10:19] = 255
    L[5][[8, 20]] = 240         # two equal separate maxima
    L[5][[7, 9, 19, 21]] = 100
    L[7][12] = 20               # below min_peak
    L[8][:] = 40                # equal to floor_level
    if dtype != np.uint8:
        g = S.line_view(f32, axis, 1, 9).copy()
        k = int(np.argmax(g))
        L[9][:] = g
        L[9][[k - 2, k + 1]] = np.nan
        L[10][:] = np.nan       # no sample
        L[11][10:19] = 255
        L[11][13] = np.nan      # NaN inside a plateau
        S.line_view(img, axis, 2, 3)[::3] = np.nan
    return img, pb, pe


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("axis", [0, 1])
def test_planted_edge_cases(gpu_lib, host, axis, dtype):
    img, pb, pe = _plants(axis, dtype)
    intr = S.camera(R.PINHOLE, 67, 37)
    for hw in (0, 5, 1000):
        for roi in ((0, 0), (pb, pe)):
            o = S.Options(axis, roi[0], roi[1], hw, floor_level=40.0, min_peak=30.0)
            got = _both(host, R.PINHOLE, intr, S.PLANE, img, o)
            if roi != (0, 0):
                c = got["centre"][0]
                assert np.isnan(c[[6, 7, 8]]).all() and np.isnan(got["xyz"][0, [6, 7, 8]]).all()
                if hw == 5:
                    assert c[0] == pb and c[1] == pe - 1 and c[2] == 10.0 and c[3] == 10.5 and c[4] == 14.0 and abs(c[5] - 8.0) < 1e-12


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("run", [2, 9])
def test_plateau_across_every_cut(gpu_lib, host, axis, dtype, run):
    """line i (counted over the frames) has a plateau of `run` samples that starts at position i, for every i up to side - 2: whatever
    cuts the kernel makes along the search direction, one of the plateaus straddles each"""
    _, _, _, _, f32, u8 = _scene(R.PINHOLE, 67, 37, axis, 3)
    img = (u8 if dtype == np.uint8 else f32).copy()
    side, n_lines = (37, 67) if axis == 0 else (67, 37)
    for i in range(side - 1):
        line = S.line_view(img, axis, i // n_lines, i % n_lines)
        line[:] = 7
        line[i:i + run] = 230
    got = _both(host, R.PINHOLE, S.camera(R.PINHOLE, 67, 37), S.PLANE, img, S.Options(axis, half_window=0))
    for i in range(side - 1):
        assert got["centre"][i // n_lines, i % n_lines] == (i + min(i + run, side) - 1) / 2


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_points_of_process_and_laser_points_agree_bitwise(gpu_lib, model, axis):
    intr, plane, _, _, f32, u8 = _scene(model, 67, 37, axis, 3)
    poses = S.frame_poses(3)
    assert abs(np.linalg.norm(poses[1, :4]) - 1.0) > 0.01
    n_lines = 67 if axis == 0 else 37
    off = np.arange(4) * n_lines
    for p in (None, poses):
        r = _gpu(intr, plane, u8, S.Options(axis), p)
        idx = np.broadcast_to(np.arange(n_lines, dtype=float), r["centre"].shape)
        uv = np.stack([idx, r["centre"]] if axis == 0 else [r["centre"], idx], axis=-1).reshape(-1, 2)
        xyz = laser_points(uv, intr, plane, frame_offset=None if p is None else off, frame_poses=p)
        assert S.bitwise(xyz, r["xyz"].reshape(-1, 3))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("axis", [0, 1])
def test_independence_and_determinism(gpu_lib, axis, dtype):
    intr, plane, _, _, f32, u8 = _scene(R.PINHOLE, 130, 33, axis, 3)
    img = u8 if dtype == np.uint8 else f32
    o = S.Options(axis)
    a, b = _gpu(intr, plane, img, o), _gpu(intr, plane, img, o)
    for k in a:
        assert S.bitwise(a[k], b[k]), k
    for f in range(3):
        one = _gpu(intr, plane, img[f:f + 1], o, max_frames=2)
        for k in a:
            assert S.bitwise(one[k][0], a[k][f]), (k, f)
    # every other line replaced by noise: the lines that stay keep their bits
    rng = np.random.default_rng(5)
    noisy = img.copy()
    noise = rng.integers(0, 256, img.shape).astype(img.dtype)
    if axis == 0:
        noisy[:, :, 1::2] = noise[:, :, 1::2]
    else:
        noisy[:, 1::2, :] = noise[:, 1::2, :]
    c = _gpu(intr, plane, noisy, o)
    for k in a:
        assert S.bitwise(c[k][:, 0::2], a[k][:, 0::2]), k


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("model", MODELS)
def test_laser_points(gpu_lib, host, model, n):
    intr = S.camera(model, 640, 480)
    rng = np.random.default_rng(n)
    uv = np.ascontiguousarray(rng.uniform([0, 0], [640, 480], (n, 2)))
    inv = R.dual_inverse(intr[5:10])
    for iv in (None, inv):
        xyz, pxy = laser_points(uv, intr, S.PLANE, inverse_coeffs=iv, want_plane_xy=True)
        rx, rp = S.points(model, intr, iv, S.PLANE, uv, want_plane_xy=True)
        assert xyz.shape == (n, 3) and pxy.shape == (n, 2)
        assert S.rel(xyz, rx) <= 1e-12 and S.rel(pxy, rp) <= 1e-12
        if n:
            hx, hp = S.host_points(host, model, intr, iv, S.PLANE, uv, want_plane_xy=True)
            assert S.rel(xyz, hx) <= 1e-12 and S.rel(pxy, hp) <= 1e-12
    # frames with empty ones among them
    poses = S.frame_poses(5)
    cuts = np.sort(rng.integers(0, n + 1, 2))
    off = np.array([0, cuts[0], cuts[0], cuts[1], n, n])
    frame = np.searchsorted(off, np.arange(n), side="right") - 1
    got = laser_points(uv, intr, S.PLANE, frame_offset=off, frame_poses=poses)
    assert S.rel(got, S.points(model, intr, None, S.PLANE, uv, frame, poses)) <= 1e-12
    one = laser_points(uv, intr, S.PLANE, frame_poses=poses[1])
    assert S.rel(one, S.points(model, intr, None, S.PLANE, uv, None, poses[1:2])) <= 1e-12


@pytest.mark.parametrize("model", MODELS)
def test_laser_points_nan_cases(gpu_lib, model):
    intr = S.camera(model, 640, 480)
    n = S.PLANE[:3]
    uv = np.ascontiguousarray(np.random.default_rng(2).uniform([0, 0], [640, 480], (65, 2)))
    behind = np.r_[-n, S.PLANE[3]]  # every ray of the image meets it at s < 0
    xyz, pxy = laser_points(uv, intr, behind, want_plane_xy=True)
    assert np.isnan(xyz).all() and np.isnan(pxy).all()
    # a ray parallel to the plane: the plane through the ray of a pixel.  n' = r x e is orthogonal to r up to rounding, so choose the
    # pixel's ray first and build the normal from the device's own unprojection of it
    lib = capi.load_library()
    px = np.array([[321.0, 200.0]])
    xy = np.empty((1, 2))
    capi.check(lib, lib.cba_camera_unproject(model, capi.dptr(intr), 0, capi.dptr(None), 1, capi.dptr(px), capi.dptr(xy)))
    par = np.array([1.0, 0.0, -xy[0, 0], 0.5])  # n.r = x - x = 0 exactly
    assert np.isnan(laser_points(px, intr, par)).all()
    assert np.isnan(laser_points(np.array([[np.nan, 1.0], [1.0, np.inf]]), intr, S.PLANE)).all()


def test_calibrate_then_scan(gpu_lib):
    """The calibration's own points and laser_points of its pixels on its plane agree to 3 rms_error: each differs from the plane by at
    most the residual.  The KAT scene is noise-free, so rms_error is 1.0e-16, below the rounding of the points themselves
    (|P| 2^-52 = 2.7e-16 per operation; the restatement's two point sets differ by 9.6e-16): the bound carries the 1e-12 |P| that every
    other xyz comparison of this file allows for rounding, and would be 3 rms_error alone on a scene with a residual above it."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linescan_kats.json")) as f:
        k = json.load(f)["plane_fit_multiple_views"]
    views = [LineScanView(np.array(v["target_view"], dtype=float).reshape(-1, 4), np.array(v["laser_uv"], dtype=float).reshape(-1, 2))
             for v in k["views"]]
    res = linescan.calibrate_laser_plane(views, k["intr"], inverse_coeffs=k["inverse_coeffs"], return_points=True)
    uv = np.concatenate([v.laser_uv for v in views])
    xyz, pxy = laser_points(uv, k["intr"], res, inverse_coeffs=k["inverse_coeffs"], want_plane_xy=True)
    ok = np.isfinite(res.points).all(axis=1)
    assert ok.any() and np.isfinite(xyz[ok]).all()
    # both sets lie on the plane to the calibration's own residual: each differs from the plane by at most rms_error (plus rounding)
    bound = 3.0 * res.rms_error + 1e-12 * np.linalg.norm(xyz[ok], axis=1).max()
    assert np.linalg.norm(xyz[ok] - res.points[ok], axis=1).max() <= bound
    back = np.c_[pxy[ok], np.ones(ok.sum())] @ np.linalg.inv(res.homography).T
    ray = back / back[:, 2:3]
    assert np.abs(ray[:, :2] * xyz[ok, 2:3] - xyz[ok, :2]).max() <= 1e-9 * np.abs(xyz[ok]).max()


def test_handle(gpu_lib):
    intr, plane, _, _, f32, u8 = _scene(R.PINHOLE, 64, 64, 0, 3)
    for _ in range(2):  # create, process, destroy: twice
        with LaserScanner(intr, plane, 64, 64, max_frames=2) as sc:
            with pytest.raises(capi.CbaInvalidArgument):
                sc.process(u8)  # 3 frames > max_frames
            a = sc.process(u8[:2])
            b = sc.process(f32[:1])  # the dtype is chosen per call
            assert a.centre.shape == (2, 64) and b.xyz.shape == (1, 64, 3) and np.isfinite(a.xyz).all()
            with pytest.raises(ValueError):
                sc.process(u8[:, :32])
            with pytest.raises(ValueError):
                sc.process(u8.astype(np.float64))
        with pytest.raises(ValueError):
            sc.process(u8[:1])
