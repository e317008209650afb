"""CPU tier of laser profile scanning: the host build of calibration_amd/csrc/laser_scan_math.hpp (tests/laser_scan_cpu, compiled
here) against the independent numpy restatement tests/laser_scan_ref.py, the geometry of the points, the centre of gravity against
the rendered ground truth, and the argument errors of the C ABI and of the Python layer (raised before any device work)."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi, linescan
from calibration_amd.linescan import LaserScanner, LaserScanOptions, laser_points
from tests import camera_ref as R
from tests import host_build
from tests import laser_scan_ref as S

MODELS = [R.PINHOLE, R.SCHEIMPFLUG]
SIZES = [(1, 1), (3, 2), (67, 37), (64, 64), (130, 33), (257, 5)]

# Ground truth: the error of the centre of gravity over p0 +- 5 samples on a sampled (and, for uint8, quantised) Gaussian of sigma 2 px
# against the true line position.  It belongs to the rule, not to an implementation: measured on the restatement, on the 67 x 37
# scene with 3 frames, its maximum is 0.0294 px (uint8, axis 1; 0.0262 axis 0; float32 0.0249) - the window cuts the Gaussian's tails
# at 2.5 sigma.  The bar is twice that maximum.
CENTRE_BAR_PX = 2 * 0.0294


@pytest.fixture(scope="module")
def host():
    return host_build.load("laser_scan_cpu")


def _check(got, ref, u8):
    for k in ("centre", "amplitude", "width_px"):
        assert S.same_nan(got[k], ref[k]), k
        if u8:
            assert S.bitwise(got[k], ref[k]), k
        else:
            assert S.rel(got[k], ref[k]) <= 1e-12, k
    assert S.same_nan(got["xyz"], ref["xyz"]) and S.rel(got["xyz"], ref["xyz"]) <= 1e-12


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("model", MODELS)
def test_host_build_matches_restatement(host, model, size, axis):
    W, H = size
    intr, plane, _, _, f32, u8 = S.scene(model, W, H, axis, 3)
    inv = R.dual_inverse(intr[5:10]) if W == 64 else None
    poses = S.frame_poses(3)
    side = H if axis == 0 else W
    for o in (S.Options(axis), S.Options(axis, half_window=0, floor_level=12.5, min_peak=30.0),
              S.Options(axis, 1, side - 1, half_window=1000) if side > 2 else S.Options(axis, half_window=1000)):
        for img in (u8, f32):
            for p in (None, poses):
                _check(S.host_scan(host, model, intr, inv, plane, img, o, p), S.scan(model, intr, inv, plane, img, o, p), img.dtype == np.uint8)


def test_host_build_edge_lines(host):
    """plateaus, ties, invalid lines and NaN, one line each"""
    side = 40
    lines = np.zeros((12, side), np.float32)
    lines[0, 0] = 250           # peak at the first position: the window clips
    lines[1, side - 1] = 250    # ... at the last
    lines[2, 10] = 255          # plateaus of 1, 2 and 9 samples
    lines[3, 10:12] = 255
    lines[4, 10:19] = 255
    lines[5, [8, 20]] = 240     # two equal separate maxima: the lower position wins
    lines[5, [7, 9, 19, 21]] = 100
    lines[7, 5] = 20            # below min_peak
    lines[8, :] = 40            # equal to floor_level: sum g == 0
    lines[9] = 200 * np.exp(-((np.arange(side) - 17.3) ** 2) / 8)
    lines[10] = lines[9]
    lines[11] = lines[4]
    o = S.Options(1, half_window=5, floor_level=40.0, min_peak=30.0)
    intr = S.camera(R.PINHOLE, side, 12)
    u8 = np.rint(lines).astype(np.uint8)[None]
    f32 = lines.copy()
    f32[9, [15, 18]] = np.nan   # NaN next to the peak
    f32[10, :] = np.nan         # no sample at all
    f32[11, 13] = np.nan        # NaN inside the plateau ends it
    for img in (u8, f32[None]):
        ref = S.scan(R.PINHOLE, intr, None, S.PLANE, img, o)
        _check(S.host_scan(host, R.PINHOLE, intr, None, S.PLANE, img, o), ref, img.dtype == np.uint8)
        c = ref["centre"][0]
        assert c[0] == 0.0 and c[1] == side - 1 and c[2] == 10.0 and c[3] == 10.5 and c[4] == 14.0
        assert abs(c[5] - 8.0) < 1e-12 and np.isnan(c[[6, 7, 8]]).all()
        assert np.isnan(ref["xyz"][0, [6, 7, 8]]).all() and np.isfinite(ref["xyz"][0, :6]).all()
        assert ref["amplitude"][0, 7] == 20.0 and ref["amplitude"][0, 8] == 40.0 and ref["amplitude"][0, 6] == 0.0
    ref = S.scan(R.PINHOLE, intr, None, S.PLANE, f32[None], o)
    assert np.isnan(ref["amplitude"][0, 10]) and np.isnan(ref["centre"][0, 10]) and abs(ref["centre"][0, 11] - 95.0 / 7.0) < 1e-12  # plateau 10..12, window 5..17


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_geometry_of_the_points(host, model, axis):
    intr, plane, _, _, f32, u8 = S.scene(model, 67, 37, axis, 3)
    o = S.Options(axis)
    r = S.host_scan(host, model, intr, None, plane, u8, o)
    P = r["xyz"].reshape(-1, 3)
    assert np.isfinite(P).all()
    assert np.max(np.abs(P @ plane[:3] + plane[3]) / np.linalg.norm(P, axis=1)) <= 1e-12
    idx = np.broadcast_to(np.arange(r["centre"].shape[1], dtype=float), r["centre"].shape)
    uv = np.stack([idx, r["centre"]] if axis == 0 else [r["centre"], idx], axis=-1).reshape(-1, 2)
    assert np.abs(R.project(model, intr, P) - uv).max() <= 1e-9
    xyz, pxy = S.host_points(host, model, intr, None, plane, uv, want_plane_xy=True)
    assert S.bitwise(xyz, P)
    ref_xyz, ref_pxy = S.points(model, intr, None, plane, uv, want_plane_xy=True)
    assert S.rel(xyz, ref_xyz) <= 1e-12 and S.rel(pxy, ref_pxy) <= 1e-12
    back = np.c_[pxy, np.ones(len(pxy))] @ np.linalg.inv(S.plane_homography(plane)).T  # Hp^-1 (a, b, 1) = s' (x, y, 1)
    ray = back / back[:, 2:3]
    s = -plane[3] / (ray @ plane[:3])
    assert np.max(np.linalg.norm(s[:, None] * ray - P, axis=1) / np.linalg.norm(P, axis=1)) <= 1e-12
    # frames and poses: a non-unit quaternion, an empty frame in the table
    poses = S.frame_poses(3)
    off = np.array([0, 5, 5, len(uv)])
    frame = np.r_[np.zeros(5, int), np.full(len(uv) - 5, 2)]
    assert S.rel(S.host_points(host, model, intr, None, plane, uv, off, poses), S.points(model, intr, None, plane, uv, frame, poses)) <= 1e-12
    # a ray parallel to the plane and a plane behind the camera
    n = plane[:3]
    x = 0.05
    par = R.project(model, intr, np.array([[x, -(n[0] * x + n[2]) / n[1], 1.0]]))
    xy = R.unproject(model, intr, par)[0]
    if n[0] * xy[0] + n[1] * xy[1] + n[2] == 0.0:  # the round trip kept den at exactly 0
        assert np.isnan(S.host_points(host, model, intr, None, plane, par)).all()
    behind = np.r_[-n, plane[3]]  # n.r > 0 for every ray of the image: s < 0
    assert np.isnan(S.host_points(host, model, intr, None, behind, uv)).all() and np.isnan(S.points(model, intr, None, behind, uv)).all()


@pytest.mark.parametrize("axis", [0, 1])
def test_centre_against_ground_truth(host, axis):
    intr, plane, pos, _, f32, u8 = S.scene(R.PINHOLE, 67, 37, axis, 3)
    o = S.Options(axis)
    for img in (u8, f32):
        ref = S.scan(R.PINHOLE, intr, None, plane, img, o)
        got = S.host_scan(host, R.PINHOLE, intr, None, plane, img, o)
        assert np.abs(ref["centre"] - pos).max() <= CENTRE_BAR_PX / 2
        assert np.abs(got["centre"] - pos).max() <= CENTRE_BAR_PX


# ---- argument errors, all before any device work ------------------------------------------------------------------------------------
def _d(a):
    return capi.dptr(None if a is None else np.ascontiguousarray(a, float))


def test_laser_abi_defaults_and_argument_errors(lib):
    o = capi.CbaLaserScanOptions()
    lib.cba_laser_scan_options_default(C.byref(o))
    assert (o.axis, o.roi_begin, o.roi_end, o.half_window, o.floor_level, o.min_peak) == (0, 0, 0, 5, 0.0, 1.0)
    I = capi.CBA_ERR_INVALID_ARGUMENT
    intr = S.camera(R.PINHOLE, 64, 48)
    uv, xyz = np.zeros((4, 2)), np.empty((4, 3))
    ok = dict(model=0, intr=intr, n_inv=0, inv=None, plane=S.PLANE, n=4, uv=uv, n_frames=0, off=None, poses=None, xyz=xyz)

    def points(**kw):
        a = dict(ok, **kw)
        off = None if a["off"] is None else np.ascontiguousarray(a["off"], np.int64)
        return lib.cba_laser_points(a["model"], _d(a["intr"]), a["n_inv"], _d(a["inv"]), _d(a["plane"]), a["n"], _d(a["uv"]), a["n_frames"],
                                    capi.i64ptr(off), _d(a["poses"]), capi.dptr(a["xyz"]), capi.dptr(None))

    assert points(model=2) == I and points(n=-1) == I and points(n_frames=-1) == I
    assert points(n_inv=1, inv=np.zeros(1)) == I and points(n_inv=17, inv=np.zeros(17)) == I
    for name in ("intr", "plane", "uv", "xyz"):
        assert points(**{name: None}) == I, name
    assert points(plane=[0.0, 0.0, 0.0, 1.0]) == I and points(plane=[np.nan, 0.0, 1.0, 1.0]) == I and points(plane=[0.0, np.inf, 1.0, 1.0]) == I
    pose = np.array([[1.0, 0, 0, 0, 0, 0, 0]])
    assert points(poses=np.tile(pose, (2, 1)), n_frames=2) == I and points(poses=pose, n_frames=0) == I
    for off in ([1, 4], [0, 3], [0, 5]):
        assert points(off=off, n_frames=1) == I, off
    assert points(off=[0, 3, 2, 4], n_frames=3) == I
    assert points(n=0, uv=None, xyz=None) == capi.CBA_OK  # no work, no device needed
    assert points(n=0, uv=None, xyz=None, off=[0, 0, 0], n_frames=2, poses=np.tile(pose, (2, 1))) == capi.CBA_OK

    def create(model=0, intr_=intr, n_inv=0, inv=None, plane=S.PLANE, W=64, H=48, max_frames=2, opts=o, out=True, **fields):
        co = None
        if opts is not None:
            co = capi.CbaLaserScanOptions()
            lib.cba_laser_scan_options_default(C.byref(co))
            for k, v in fields.items():
                setattr(co, k, v)
        h = C.c_void_p()
        st = lib.cba_laser_scanner_create(model, _d(intr_), n_inv, _d(inv), _d(plane), W, H, max_frames, None if co is None else C.byref(co), 0,
                                          C.byref(h) if out else None)
        assert st != capi.CBA_OK or h.value
        if h.value:
            lib.cba_laser_scanner_destroy(h)
        return st

    assert create(model=3) == I and create(intr_=None) == I and create(plane=None) == I and create(opts=None) == I and create(out=False) == I
    assert create(n_inv=1, inv=np.zeros(1)) == I and create(plane=[0.0, 0.0, 0.0, 0.5]) == I
    assert create(W=0) == I and create(H=0) == I and create(W=capi.IMAGE_MAX_SIDE + 1) == I and create(max_frames=0) == I
    assert create(axis=2) == I and create(half_window=-1) == I
    assert create(roi_begin=5, roi_end=5) == I and create(roi_begin=-1, roi_end=4) == I and create(roi_begin=0, roi_end=49) == I
    assert create(axis=1, roi_begin=0, roi_end=65) == I and create(roi_begin=7, roi_end=3) == I
    assert create(floor_level=np.nan) == I and create(min_peak=np.inf) == I
    assert lib.cba_laser_scanner_process(None, 1, 0, None, capi.dptr(None), capi.dptr(None), capi.dptr(None), capi.dptr(None), capi.dptr(None)) == I
    lib.cba_laser_scanner_destroy(None)
    if lib.cba_device_count() <= 0:
        assert create() == capi.CBA_ERR_NO_DEVICE and create(roi_begin=0, roi_end=48) == capi.CBA_ERR_NO_DEVICE
        assert points() == capi.CBA_ERR_NO_DEVICE


def test_python_layer_validates(lib):
    intr = S.camera(R.PINHOLE, 64, 48)
    with pytest.raises(ValueError):
        laser_points(np.zeros((4, 3)), intr, S.PLANE)
    with pytest.raises(ValueError):
        laser_points(np.zeros((4, 2)), intr, S.PLANE[:3])
    with pytest.raises(ValueError):
        laser_points(np.zeros((4, 2)), np.zeros(11), S.PLANE)
    with pytest.raises(ValueError):
        laser_points(np.zeros((4, 2)), intr, S.PLANE, frame_offset=[0, 2, 4], frame_poses=np.zeros((3, 7)))
    with pytest.raises(capi.CbaInvalidArgument):
        laser_points(np.zeros((4, 2)), intr, S.PLANE, frame_offset=[0, 2, 3])
    with pytest.raises(capi.CbaInvalidArgument):
        LaserScanner(intr, S.PLANE, 64, 48, opts=LaserScanOptions(half_window=-1))
    with pytest.raises(capi.CbaInvalidArgument):
        LaserScanner(intr, S.PLANE, 64, 48, opts=LaserScanOptions(axis=1, roi_begin=10, roi_end=100))
    res = linescan.LineScanCalibrationResult(plane=S.PLANE, homography=np.eye(3), rms_error=0.0, inlier_count=0, summary="", n_points=0,
                                             n_views_used=0)
    assert laser_points(np.zeros((0, 2)), intr, res).shape == (0, 3)
    xyz, pxy = laser_points(np.zeros((0, 2)), intr, res, want_plane_xy=True)
    assert xyz.shape == (0, 3) and pxy.shape == (0, 2)
