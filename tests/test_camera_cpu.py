"""CPU tier of the camera models: the host build of calibration_amd/csrc/camera_math.hpp (tests/camera_cpu, compiled here) against
the literal numpy restatement tests/camera_ref.py and the oracle's projection, its unprojection against tests/linescan_cpu's
ls_unproject bit for bit, and the C ABI's argument errors (raised before any device work)."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import camera as cam
from calibration_amd import capi
from tests import camera_ref as R
from tests import host_build
from tests.host_build import ptr

c_f = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def camcpu():
    return host_build.load("camera_cpu")


@pytest.fixture(scope="module")
def lscpu():
    return host_build.load("linescan_cpu")


def host_project(L, model, intr, xyz):
    xyz = np.ascontiguousarray(xyz, float)
    uv = np.empty((xyz.shape[0], 2))
    L.cam_project(model, ptr(np.asarray(intr, float)), C.c_int64(xyz.shape[0]), ptr(xyz), ptr(uv))
    return uv


def host_unproject(L, model, intr, uv, inv=None):
    uv = np.ascontiguousarray(uv, float)
    xy = np.empty_like(uv)
    L.cam_unproject(model, ptr(np.asarray(intr, float)), 0 if inv is None else len(inv), None if inv is None else ptr(np.asarray(inv, float)),
                    C.c_int64(uv.shape[0]), ptr(uv), ptr(xy))
    return xy


def host_map(L, model, intrs, W, H, Rs=None, Kp=None):
    intrs = np.ascontiguousarray(intrs, float)
    n = intrs.shape[0]
    mx = np.empty((n, H, W), np.float32)
    my = np.empty_like(mx)
    Rp = None if Rs is None else ptr(np.ascontiguousarray(Rs, float))
    Kpp = None if Kp is None else ptr(np.ascontiguousarray(Kp, float))
    L.cam_map(model, n, ptr(intrs), Rp, Kpp, W, H, mx.ctypes.data_as(c_f), my.ctypes.data_as(c_f))
    return mx, my


def host_apply(L, src, mx, my, border=0.0):
    s = np.ascontiguousarray(src)
    ch = 1 if s.ndim == 2 else s.shape[2]
    H, W = mx.shape
    out = np.empty((H, W) + (() if s.ndim == 2 else (ch,)), s.dtype)
    L.cam_apply(0 if s.dtype == np.uint8 else 1, s.ctypes.data_as(C.c_void_p), s.shape[1], s.shape[0], ch,
                np.ascontiguousarray(mx).ctypes.data_as(c_f), np.ascontiguousarray(my).ctypes.data_as(c_f), W, H, C.c_double(border),
                out.ctypes.data_as(C.c_void_p))
    return out


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


CAMS = R.cameras()


@pytest.mark.parametrize("name,model,intr", CAMS, ids=[c[0] for c in CAMS])
def test_project_matches_restatement_and_oracle(camcpu, oracle, name, model, intr):
    xyz = R.points(4000, seed=3)
    uv = host_project(camcpu, model, intr, xyz)
    assert _rel(uv, R.project(model, intr, xyz)) <= 1e-9
    ref = np.empty(2)
    orc = np.empty_like(uv)
    for i in range(0, xyz.shape[0], 7):
        oracle.orc_project(model, capi.dptr(intr), capi.dptr(np.ascontiguousarray(xyz[i])), capi.dptr(ref))
        orc[i] = ref
    assert _rel(uv[::7], orc[::7]) <= 1e-9


@pytest.mark.parametrize("name,model,intr", CAMS, ids=[c[0] for c in CAMS])
@pytest.mark.parametrize("dual", [False, True])
def test_unproject_matches_restatement_and_linescan_bitwise(camcpu, lscpu, name, model, intr, dual):
    inv = R.dual_inverse(intr[5:10]) if dual else None
    uv = R.project(model, intr, R.points(3000, seed=5))
    xy = host_unproject(camcpu, model, intr, uv, inv)
    assert _rel(xy, R.unproject(model, intr, uv, inv)) <= 1e-12
    # tests/linescan_cpu's ls_unproject: the same code, so the same bits
    u, v = np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1])
    x, y = np.empty(len(u)), np.empty(len(u))
    lscpu.ls_unproject(model, ptr(intr), 0 if inv is None else len(inv), None if inv is None else ptr(np.ascontiguousarray(inv)), len(u),
                       ptr(u), ptr(v), ptr(x), ptr(y))
    assert np.array_equal(xy[:, 0], x) and np.array_equal(xy[:, 1], y)
    if not dual:  # the 5-step fixed point undoes project to well below a pixel's worth
        xyz = R.points(3000, seed=5)
        if model == R.PINHOLE:
            assert np.abs(xy - xyz[:, :2] / xyz[:, 2:]).max() < 1e-3


@pytest.mark.parametrize("name,model,intr", CAMS, ids=[c[0] for c in CAMS])
@pytest.mark.parametrize("inverse", ["none", "four", "four_null"])
def test_fill_camera_pads_with_zeros_and_builds_the_constants(camcpu, name, model, intr, inverse):
    """ls_fill_camera (linescan_math.hpp), the one camera fill of every pipeline: the intrinsics padded to 12, the inverse
    coefficients given (none when the pointer is null, whatever the count says) padded to 16, the Scheimpflug constants."""
    intr = np.asarray(intr, float)
    ni = 12 if model == R.SCHEIMPFLUG else 10
    assert len(intr) == ni
    inv = np.array([0.3, -0.07, 1e-3, -2e-4]) if inverse == "four" else None
    n_inv = 0 if inverse == "none" else 4
    m, k = C.c_int(-1), C.c_int(-1)
    intr12, inv16, sd, sd_ref = np.empty(12), np.empty(16), np.empty(36), np.empty(36)
    camcpu.cam_fill_camera(model, ptr(intr), n_inv, None if inv is None else ptr(inv), C.byref(m), C.byref(k), ptr(intr12), ptr(inv16),
                           ptr(sd), ptr(sd_ref))
    assert m.value == model
    assert k.value == (4 if inv is not None else 0)
    assert np.array_equal(intr12[:ni], intr)
    assert intr12[ni:].tobytes() == bytes(8 * (12 - ni))
    if inv is not None:
        assert np.array_equal(inv16[:4], inv)
    assert inv16[k.value:].tobytes() == bytes(8 * (16 - k.value))
    if model == R.SCHEIMPFLUG:
        assert sd.tobytes() == sd_ref.tobytes()
    else:
        assert sd.tobytes() == bytes(8 * 36)


def test_distort_is_project_with_identity_k(camcpu):
    dist = np.array([-0.21, 0.08, -0.012, 0.0011, -0.0007])
    xy = R.points(500, seed=9)[:, :2] / 3.0
    one = np.column_stack([xy, np.ones(len(xy))])
    uv = host_project(camcpu, R.PINHOLE, np.concatenate([[1.0, 1.0, 0.0, 0.0, 0.0], dist]), one)
    xd, yd = R.apply_distortion(xy[:, 0], xy[:, 1], dist)
    assert _rel(uv, np.column_stack([xd, yd])) <= 1e-12


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@pytest.mark.parametrize("W,H", [(37, 23), (64, 48)])
@pytest.mark.parametrize("model", [R.PINHOLE, R.SCHEIMPFLUG])
def test_map_matches_restatement(camcpu, W, H, model):
    intrs = np.stack([c[2] for c in CAMS if c[1] == model][:2])
    intrs[:, 2] = W / 2.0
    intrs[:, 3] = H / 2.0
    intrs[:, 0] = intrs[:, 1] = 0.6 * W
    Rs = np.stack([_rot(0.05, -0.1, 0.02), _rot(1.4, 0.3, 0.0)]).reshape(2, 9)  # the second turns part of the grid behind
    Kp = np.array([[0.5 * W, 0.52 * W, W / 2 + 1.5, H / 2 - 0.5, 0.3], [0.7 * W, 0.7 * W, W / 2, H / 2, 0.0]])
    for rs, kp in ((None, None), (Rs, None), (Rs, Kp)):
        mx, my = host_map(camcpu, model, intrs, W, H, rs, kp)
        for c in range(2):
            rx, ry = R.undistort_map(model, intrs[c], W, H, None if rs is None else rs[c], None if kp is None else kp[c])
            dx, dy = R.ulp_diff(mx[c], rx), R.ulp_diff(my[c], ry)
            assert not np.isnan(dx).any() and not np.isnan(dy).any(), "NaN pattern differs"
            assert dx.max() <= 1 and dy.max() <= 1
    assert np.isnan(host_map(camcpu, model, intrs, W, H, Rs, Kp)[0][1]).any()


def test_identity_map_is_the_pixel_grid(camcpu):
    W, H = 37, 23
    intr = np.array([30.0, 31.0, 18.0, 11.5, 0.0, 0, 0, 0, 0, 0])
    mx, my = host_map(camcpu, R.PINHOLE, intr[None], W, H)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    assert np.array_equal(mx[0], u) and np.array_equal(my[0], v)


def _images(rng, sh, sw, ch, dtype):
    shape = (sh, sw) if ch == 1 else (sh, sw, ch)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def _special_maps(rng, H, W, sw, sh):
    mx = rng.uniform(-3.0, sw + 2.0, (H, W)).astype(np.float32)
    my = rng.uniform(-3.0, sh + 2.0, (H, W)).astype(np.float32)
    mx[0, :5] = [np.nan, 2 ** 24 + 4, -(2 ** 24) - 4, 2.5, 3.015625]  # NaN, out of range, half-way ties of 32 m
    my[0, :5] = [1.0, 1.0, 1.0, np.nan, 1.03125]
    mx[1, :3] = [sw - 1 + 0.5, -0.5, 0.0]
    return mx, my


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_apply_matches_restatement(camcpu, ch, dtype):
    rng = np.random.default_rng(ch)
    sh, sw, H, W = 29, 41, 17, 33
    src = _images(rng, sh, sw, ch, dtype)
    mx, my = _special_maps(rng, H, W, sw, sh)
    for border in (0.0, 77.6, -3.0):
        got = host_apply(camcpu, src, mx, my, border)
        ref = R.apply(src, mx, my, border)
        if dtype == np.uint8:
            assert np.array_equal(got, ref)
        else:
            assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-6
        b = np.asarray(R.apply(src[:1, :1], np.full((1, 1), np.nan, np.float32), np.zeros((1, 1), np.float32), border))
        assert np.array_equal(got[0, 0], b.reshape(got[0, 0].shape))  # the NaN entry gives the border


# ---- the C ABI's argument errors, all before any device work -----------------------------------------------------------------
def _d(a):
    return capi.dptr(None if a is None else np.ascontiguousarray(a, float))


def test_camera_abi_argument_errors(lib):
    I = capi.CBA_ERR_INVALID_ARGUMENT
    intr = np.array(CAMS[0][2])
    xyz, uv = np.ones((4, 3)), np.zeros((4, 2))
    assert lib.cba_camera_project(7, _d(intr), 4, _d(xyz), capi.dptr(uv)) == I
    assert lib.cba_camera_project(0, _d(None), 4, _d(xyz), capi.dptr(uv)) == I
    assert lib.cba_camera_project(0, _d(intr), -1, _d(xyz), capi.dptr(uv)) == I
    assert lib.cba_camera_project(0, _d(intr), 4, _d(None), capi.dptr(uv)) == I
    assert lib.cba_camera_project(0, _d(intr), 4, _d(xyz), capi.dptr(None)) == I
    assert lib.cba_camera_project(0, _d(intr), 0, _d(None), capi.dptr(None)) == capi.CBA_OK  # n == 0: no work
    inv = np.zeros(17)
    for n_inv in (1, 17):
        assert lib.cba_camera_unproject(0, _d(intr), n_inv, _d(inv), 4, _d(uv), capi.dptr(uv.copy())) == I
    assert lib.cba_camera_unproject(2, _d(intr), 0, _d(None), 4, _d(uv), capi.dptr(uv.copy())) == I
    assert lib.cba_camera_unproject(0, _d(intr), 0, _d(None), -5, _d(uv), capi.dptr(uv.copy())) == I
    assert lib.cba_camera_unproject(0, _d(intr), 0, _d(None), 4, _d(None), capi.dptr(uv.copy())) == I
    assert lib.cba_camera_unproject(0, _d(intr), 0, _d(None), 0, _d(None), capi.dptr(None)) == capi.CBA_OK

    h = C.c_void_p()
    two = np.stack([intr, intr])
    ok_args = dict(model=0, n=2, intr=two, R=None, K=None, w=64, h=48)

    def create(**kw):
        a = dict(ok_args, **kw)
        return lib.cba_undistort_map_create(a["model"], a["n"], _d(a["intr"]), _d(a["R"]), _d(a["K"]), a["w"], a["h"], 0, C.byref(h))

    assert create(model=5) == I
    assert create(n=0) == I
    assert create(intr=None) == I
    for side in (0, 32769, -1):
        assert create(w=side) == I
        assert create(h=side) == I
    assert create(K=np.array([[0.0, 1, 0, 0, 0], [1, 1, 0, 0, 0]])) == I
    assert create(K=np.array([[1.0, 1, 0, 0, 0], [1, 0, 0, 0, 0]])) == I
    bad = two.copy()
    bad[1, 1] = 0.0
    assert create(intr=bad) == I  # fy of the camera's own K
    assert lib.cba_undistort_map_create(0, 1, _d(intr), _d(None), _d(None), 8, 8, 0, None) == I
    assert lib.cba_undistort_map_fetch(None, None, None) == I
    assert lib.cba_undistort_map_apply(None, 1, capi.i32ptr(np.zeros(1, np.int32)), 8, 8, 1, 0, 0.0, None, None) == I
    lib.cba_undistort_map_destroy(None)  # a no-op


def test_python_layer_validates(lib):
    with pytest.raises(ValueError):
        cam.project(np.zeros(9), np.ones((2, 3)))  # neither 10 nor 12 entries (linescan._camera)
    with pytest.raises(ValueError):
        cam.distort(np.zeros(4), np.zeros((2, 2)))
    with pytest.raises(capi.CbaInvalidArgument):
        cam.unproject(CAMS[0][2], np.zeros((2, 2)), inverse_coeffs=np.zeros(1))
    with pytest.raises(capi.CbaInvalidArgument):
        cam.UndistortMap(CAMS[0][2], 0, 10)
    assert cam.project(CAMS[0][2], np.zeros((0, 3))).shape == (0, 2)
