"""GPU tier of the triangulation (cba_triangulate, calibration_amd.triangulate): the device against ground truth, against the host
build of the same header (tests/triangulate_cpu) and the independent numpy restatement (tests/triangulate_ref.py), the gradient of the
reprojection cost at the returned points, the round trip through cba_camera_project, missing observations and outlier cameras to
the bit, the status cases, the covariance, the arguments, and a calibrated rig end to end.  Sizes 1, 63, 64, 65 and 257 cover the
wavefront tail and the block tail."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import camera, capi, optim, rig
from calibration_amd.geometry import make_pose
from calibration_amd.triangulate import TriangulateOptions, triangulate
from tests import camera_ref as R
from tests import host_build
from tests import triangulate_ref as T

pytestmark = pytest.mark.gpu

MODELS = [R.PINHOLE, R.SCHEIMPFLUG]
SHAPES = [(1, 2), (63, 3), (64, 5), (65, 16), (257, 3)]  # (points, cameras)


@pytest.fixture(scope="module")
def tricpu():
    return host_build.load("triangulate_cpu")


def _dev(intrs, invs, poses, uv, o=None):
    o = o or T.Options()
    r = triangulate(intrs, poses, uv, invs, TriangulateOptions(o.max_iterations, o.step_tolerance, o.min_cams, o.max_reproj_px), covariance=True)
    mask = (r.used * (1 << np.arange(r.used.shape[1]))[None, :]).sum(axis=1).astype(np.uint32)
    return dict(xyz=r.xyz, rms=r.rms_px, mask=mask, status=r.status, cov=r.cov)


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1e-300, np.abs(b)))


def _relnorm(a, b):
    return np.max(np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1))


def _all_seen(n_cams):
    return (1 << n_cams) - 1


def _same_bits(a, b, keys=("xyz", "rms", "mask", "status", "cov")):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n,n_cams", SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_ground_truth_noise_free(gpu_lib, model, n, n_cams, dual):
    intrs, poses, xyz, uv = T.scene(n_cams, n, model)
    r = _dev(intrs, T.dual_inverses(intrs) if dual else None, poses, uv)
    assert _relnorm(r["xyz"], xyz) <= 1e-9
    assert (r["status"] == T.OK).all() and (r["mask"] == _all_seen(n_cams)).all()
    assert r["rms"].max() <= 1e-9


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n,n_cams", [(65, 2), (63, 3), (64, 5), (65, 16), (257, 3)])
@pytest.mark.parametrize("model", MODELS)
def test_minimiser_noisy(gpu_lib, tricpu, model, n, n_cams, dual):
    """0.3 px noise: the device agrees with the host build of the same header and with the numpy restatement, the cost's gradient
    (central differences of camera_ref's projection) vanishes at the returned points, and does not at the seeds."""
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    invs = T.dual_inverses(intrs) if dual else None
    r = _dev(intrs, invs, poses, uv)
    host = T.host_triangulate(tricpu, model, intrs, invs, poses, uv)
    assert (r["status"] == T.OK).all() and np.array_equal(r["mask"], host["mask"])
    print(f"device vs host: xyz {_relnorm(r['xyz'], host['xyz']):.2e} rms {_rel(r['rms'], host['rms']):.2e}")
    assert _relnorm(r["xyz"], host["xyz"]) <= 1e-9 and _rel(r["rms"], host["rms"]) <= 1e-9
    k = 12 if n_cams < 16 else 5  # the restatement and the gradients are Python loops: the first points
    ref = T.triangulate(model, intrs, invs, poses, uv[:, :k])
    print(f"device vs restatement: xyz {_relnorm(r['xyz'][:k], ref['xyz']):.2e} rms {_rel(r['rms'][:k], ref['rms']):.2e}")
    assert _relnorm(r["xyz"][:k], ref["xyz"]) <= 1e-9 and _rel(r["rms"][:k], ref["rms"]) <= 1e-9
    assert np.array_equal(r["status"][:k], ref["status"]) and np.array_equal(r["mask"][:k], ref["mask"])
    seed = _dev(intrs, invs, poses, uv, T.Options(max_iterations=0))
    assert (seed["status"] == T.NOT_CONVERGED).all()
    for i in range(k):
        g, jn, rn = T.cost_gradient(model, intrs, poses, uv[:, i], r["mask"][i], r["xyz"][i])
        assert g <= 1e-6 * jn * rn
        g, jn, rn = T.cost_gradient(model, intrs, poses, uv[:, i], seed["mask"][i], seed["xyz"][i])
        assert g > 1e-6 * jn * rn  # the refinement is doing the work


@pytest.mark.parametrize("model", MODELS)
def test_round_trip_through_camera_project(gpu_lib, model):
    n_cams, n = 3, 257
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    r = _dev(intrs, None, poses, uv)
    s = np.zeros(n)
    for c in range(n_cams):
        P = np.stack([T.to_camera(poses[c], X) for X in r["xyz"]])
        e = camera.project(intrs[c], P) - uv[c]
        s += e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    assert _rel(r["rms"], np.sqrt(s / n_cams)) <= 1e-12


@pytest.mark.parametrize("model", MODELS)
def test_missing_observations_bitwise(gpu_lib, tricpu, model):
    n_cams, n = 5, 257
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    rng = np.random.default_rng(4)
    for i in range(n):
        drop = rng.permutation(n_cams)[: rng.integers(0, n_cams - 1)]  # at least two cameras stay
        uv[drop, i, rng.integers(0, 2)] = np.nan if i % 2 else np.inf
    uv[1:, 200] = np.nan  # one camera left
    r = _dev(intrs, None, poses, uv)
    seen = np.isfinite(uv).all(axis=2)
    expect = (seen * (1 << np.arange(n_cams))[:, None]).sum(axis=0)
    expect[200] = 0
    assert np.array_equal(r["mask"], expect)
    assert r["status"][200] == T.TOO_FEW and np.isnan(r["xyz"][200]).all() and np.isnan(r["rms"][200]) and np.isnan(r["cov"][200]).all()
    ok = np.arange(n) != 200
    assert (r["status"][ok] == T.OK).all()
    host = T.host_triangulate(tricpu, model, intrs, None, poses, uv)
    assert np.array_equal(r["status"], host["status"]) and _relnorm(r["xyz"][ok], host["xyz"][ok]) <= 1e-9
    for i in range(n):  # the same point alone: the same bits
        one = _dev(intrs, None, poses, np.ascontiguousarray(uv[:, i:i + 1]))
        assert _same_bits(one, {k: v[i:i + 1] for k, v in r.items()}), i


@pytest.mark.parametrize("model", MODELS)
def test_outlier_camera_bitwise(gpu_lib, model):
    n_cams, n = 5, 65
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    bad = np.arange(n) % 3 == 0
    cam = np.arange(n) % n_cams
    uv[cam[bad], np.flatnonzero(bad), 1] += 50.0  # across the epipolar lines (along them a displacement is largely a change of depth)
    o = T.Options(max_reproj_px=2.0)
    r = _dev(intrs, None, poses, uv, o)
    expect = np.full(n, _all_seen(n_cams))
    expect[bad] &= ~(1 << cam[bad])
    assert np.array_equal(r["mask"], expect) and (r["status"] == T.OK).all()
    gone = uv.copy()
    gone[cam[bad], np.flatnonzero(bad)] = np.nan
    assert _same_bits(r, _dev(intrs, None, poses, gone, o))
    off = _dev(intrs, None, poses, uv)
    assert (off["rms"][bad] > 2.0).all() and (off["mask"] == _all_seen(n_cams)).all()
    assert (r["rms"] < 2.0).all()


def test_status_cases(gpu_lib):
    for name, intrs, poses, uv, expect in T.status_cases():
        r = _dev(intrs, None, poses, uv)
        assert r["status"][0] == expect, name
        if expect == T.DEGENERATE:
            assert np.isnan(r["xyz"]).all() and np.isnan(r["rms"]).all() and np.isnan(r["cov"]).all()
        else:
            assert np.isfinite(r["xyz"]).all() and r["xyz"][0, 2] < 0
    intrs, poses, _, uv = T.scene(3, 65, R.PINHOLE, noise=0.3)
    r = _dev(intrs, None, poses, uv, T.Options(max_iterations=1))
    assert (r["status"] == T.NOT_CONVERGED).all() and np.isfinite(r["xyz"]).all() and np.isfinite(r["rms"]).all()


@pytest.mark.parametrize("n_cams", [2, 5])
@pytest.mark.parametrize("model", MODELS)
def test_covariance(gpu_lib, model, n_cams):
    intrs, poses, _, uv = T.scene(n_cams, 65, model, noise=0.3)
    r = _dev(intrs, None, poses, uv)
    assert np.array_equal(r["cov"], np.swapaxes(r["cov"], 1, 2)) and (np.linalg.eigvalsh(r["cov"]) > 0).all()
    for i in range(0, 65, 4):
        _, H, _, _ = T.linearize(model, intrs, poses, uv[:, i], list(range(n_cams)), r["xyz"][i])
        assert np.linalg.cond(H) <= 5e2
        ref = np.linalg.inv(H)
        assert np.abs(r["cov"][i] - ref).max() <= 1e-6 * np.abs(ref).max()


def _d(a):
    return capi.dptr(None if a is None else np.ascontiguousarray(a, float))


def test_repeatability_and_arguments(gpu_lib):
    lib = gpu_lib
    intrs, poses, _, uv = T.scene(5, 257, R.SCHEIMPFLUG, noise=0.3)
    assert _same_bits(_dev(intrs, None, poses, uv), _dev(intrs, None, poses, uv))
    o = capi.CbaTriangulateOptions()
    lib.cba_triangulate_options_default(C.byref(o))
    xyz, st = np.empty((257, 3)), np.empty(257, np.int32)

    def call(model=1, n_cams=5, intr=intrs, n_inv=0, inv=None, pose=poses, n=257, px=uv, opts=o, out=xyz, status=st):
        return lib.cba_triangulate(model, n_cams, _d(intr), n_inv, _d(inv), _d(pose), n, _d(px), None if opts is None else C.byref(opts),
                                   capi.dptr(out), capi.dptr(None), None, capi.i32ptr(status), capi.dptr(None))

    assert call() == capi.CBA_OK  # rms_px, used_mask and cov6 may be NULL
    assert np.array_equal(xyz, _dev(intrs, None, poses, uv)["xyz"]) and (st == T.OK).all()
    assert call(n=0) == capi.CBA_OK and call(n=0, px=None, out=None, status=None) == capi.CBA_OK
    I = capi.CBA_ERR_INVALID_ARGUMENT
    assert call(n_cams=1) == I
    assert call(n_cams=17, intr=np.tile(intrs[:1], (17, 1)), pose=np.tile(poses[:1], (17, 1))) == I
    for name in ("intr", "pose", "px", "opts", "out", "status"):
        assert call(**{name: None}) == I, name
    assert call(model=2) == I
    assert call(n_inv=1, inv=np.zeros((5, 1))) == I
    assert b"n_inverse_coeffs" in lib.cba_last_error()


def test_calibrated_rig_end_to_end(gpu_lib):
    """The stereo scene of the rig facade's test (two cameras 0.5 m apart, three target poses, six corners), calibrated by
    calibrate_rig; the corners triangulated from the calibrated cameras and c_se3_r are r_se3_t . (X, Y, 0)."""
    cam = np.array([400.0, 400.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0])
    cam_poses = [np.eye(4), make_pose(np.array([0.5, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), 0.0)]
    targets = [make_pose(np.array([0.0, 0.0, 4.0]), np.array([0.0, 0.0, 1.0]), 0.0),
               make_pose(np.array([0.2, -0.1, 3.5]), np.array([0.0, 1.0, 0.0]), 0.15),
               make_pose(np.array([-0.1, 0.2, 4.5]), np.array([1.0, 0.0, 0.0]), -0.2)]
    obj = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5], [1.5, 0.5]])

    def render(Tm):
        P = obj[:, :1] * Tm[:3, 0] + obj[:, 1:] * Tm[:3, 1] + Tm[:3, 3]
        return np.c_[obj, 400.0 * P[:, 0] / P[:, 2], 400.0 * P[:, 1] / P[:, 2]]

    views = [[render(cam_poses[0] @ Tm), render(cam_poses[1] @ Tm)] for Tm in targets]
    res = rig.calibrate_rig(views, [cam, cam], optim.ExtrinsicOptions(optimize_intrinsics=False))
    assert res.success
    uv = np.stack([np.concatenate([v[c][:, 2:] for v in views]) for c in range(2)])
    tri = triangulate(res.optimization.cameras, res.optimization.c_se3_r, uv, covariance=True)
    assert (tri.status == capi.TRI_OK).all() and tri.used.all() and tri.cov.shape == (18, 3, 3)
    want = np.concatenate([obj[:, :1] * Tm[:3, 0] + obj[:, 1:] * Tm[:3, 1] + Tm[:3, 3] for Tm in res.optimization.r_se3_t])
    assert np.abs(tri.xyz - want).max() <= 1e-6
