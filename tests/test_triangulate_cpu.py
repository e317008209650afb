"""CPU tier of the triangulation: the host build of calibration_amd/csrc/tri_math.hpp (tests/triangulate_cpu, compiled here) against
the independent numpy restatement tests/triangulate_ref.py on the scenes the GPU tier uses, the restatement's own Jacobian against
central differences, and the argument errors of the C ABI and of the Python layer (raised before any device work)."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.triangulate import TriangulateOptions, triangulate
from tests import camera_ref as R
from tests import host_build
from tests import triangulate_ref as T

MODELS = [R.PINHOLE, R.SCHEIMPFLUG]


@pytest.fixture(scope="module")
def tricpu():
    return host_build.load("triangulate_cpu")


def _rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def _relnorm(a, b):
    return np.max(np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1))


def _all_seen(n_cams):
    return (1 << n_cams) - 1


@pytest.mark.parametrize("model", MODELS)
def test_restatement_jacobian_matches_central_differences(model):
    intrs, poses, xyz, _ = T.scene(3, 20, model)
    for X in xyz:
        for c in range(3):
            P = T.to_camera(poses[c], X)
            J = T.project_jacobian(model, intrs[c], P)
            h = 1e-6
            num = np.stack([(R.project(model, intrs[c], (P + h * e)[None])[0] - R.project(model, intrs[c], (P - h * e)[None])[0]) / (2 * h)
                            for e in np.eye(3)], axis=1)
            assert np.abs(J - num).max() <= 1e-6 * np.abs(num).max()


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n_cams", [2, 3, 5, 16])
@pytest.mark.parametrize("model", MODELS)
def test_ground_truth_noise_free(tricpu, model, n_cams, dual):
    """Noise-free pixels give the true point to the parity bar, from a seed the undistortion leaves 1e-9 .. 1e-6 away (the 5-step
    fixed point) or ~1e-4 away (the fitted dual inverse), in a handful of linearisations and with cond(J^T J) of a few hundred."""
    intrs, poses, xyz, uv = T.scene(n_cams, 65, model)
    invs = T.dual_inverses(intrs) if dual else None
    r = T.host_triangulate(tricpu, model, intrs, invs, poses, uv)
    assert _relnorm(r["xyz"], xyz) <= 1e-9
    assert (r["status"] == T.OK).all() and (r["mask"] == _all_seen(n_cams)).all()
    assert r["rms"].max() <= 1e-9
    s = T.host_triangulate(tricpu, model, intrs, invs, poses, uv, T.Options(max_iterations=0))
    assert (s["status"] == T.NOT_CONVERGED).all()
    assert _relnorm(s["xyz"], xyz) <= (2e-3 if dual else 1e-5)
    assert r["linearisations"].max() <= (6 if dual else 4)
    H = np.linalg.inv(r["cov"])
    assert np.linalg.cond(H).max() <= 5e2


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("n_cams", [2, 3, 5, 16])
@pytest.mark.parametrize("model", MODELS)
def test_minimiser_matches_restatement(tricpu, model, n_cams, dual):
    n = 33 if n_cams < 16 else 9
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    invs = T.dual_inverses(intrs) if dual else None
    r = T.host_triangulate(tricpu, model, intrs, invs, poses, uv)
    ref = T.triangulate(model, intrs, invs, poses, uv)
    assert (r["status"] == T.OK).all() and np.array_equal(r["status"], ref["status"]) and np.array_equal(r["mask"], ref["mask"])
    assert _relnorm(r["xyz"], ref["xyz"]) <= 1e-9
    assert _rel(r["rms"], ref["rms"]) <= 1e-9
    assert np.max(np.abs(r["cov"] - ref["cov"]) / np.abs(ref["cov"]).max(axis=(1, 2), keepdims=True)) <= 1e-6
    assert (np.linalg.eigvalsh(r["cov"]) > 0).all()
    seed = T.host_triangulate(tricpu, model, intrs, invs, poses, uv, T.Options(max_iterations=0))
    for i in range(n):
        g, jn, rn = T.cost_gradient(model, intrs, poses, uv[:, i], r["mask"][i], r["xyz"][i])
        assert g <= 1e-6 * jn * rn
        g, jn, rn = T.cost_gradient(model, intrs, poses, uv[:, i], seed["mask"][i], seed["xyz"][i])
        assert g > 1e-6 * jn * rn  # the seed alone is not the minimiser


@pytest.mark.parametrize("model", MODELS)
def test_missing_observations(tricpu, model):
    n_cams, n = 5, 40
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    rng = np.random.default_rng(4)
    for i in range(n):
        drop = rng.permutation(n_cams)[: rng.integers(0, n_cams - 1)]
        uv[drop, i, rng.integers(0, 2)] = np.nan if i % 2 else np.inf
    uv[1:, 0] = np.nan  # one camera left
    r = T.host_triangulate(tricpu, model, intrs, None, poses, uv)
    ref = T.triangulate(model, intrs, None, poses, uv)
    assert np.array_equal(r["status"], ref["status"]) and np.array_equal(r["mask"], ref["mask"])
    seen = np.isfinite(uv).all(axis=2)
    assert np.array_equal(r["mask"][1:], (seen[:, 1:] * (1 << np.arange(n_cams))[:, None]).sum(axis=0))
    assert r["status"][0] == T.TOO_FEW and r["mask"][0] == 0 and np.isnan(r["xyz"][0]).all() and np.isnan(r["rms"][0])
    assert (r["status"][1:] == T.OK).all()
    assert _relnorm(r["xyz"][1:], ref["xyz"][1:]) <= 1e-9
    three = T.host_triangulate(tricpu, model, intrs, None, poses, uv, T.Options(min_cams=3))
    assert np.array_equal(three["status"] == T.TOO_FEW, seen.sum(axis=0) < 3)
    for i in range(n):  # a point alone gives the same bits
        one = T.host_triangulate(tricpu, model, intrs, None, poses, uv[:, i:i + 1])
        assert one["xyz"].tobytes() == r["xyz"][i].tobytes() and one["rms"].tobytes() == r["rms"][i].tobytes()


@pytest.mark.parametrize("model", MODELS)
def test_outlier_camera_is_dropped(tricpu, model):
    n_cams, n = 5, 24
    intrs, poses, _, uv = T.scene(n_cams, n, model, noise=0.3)
    bad = np.arange(n) % 3 == 0
    cam = np.arange(n) % n_cams
    uv[cam[bad], np.flatnonzero(bad), 1] += 50.0  # across the epipolar lines (along them a displacement is largely a change of depth)
    o = T.Options(max_reproj_px=2.0)
    r = T.host_triangulate(tricpu, model, intrs, None, poses, uv, o)
    expect = np.full(n, _all_seen(n_cams))
    expect[bad] &= ~(1 << cam[bad])
    assert np.array_equal(r["mask"], expect) and (r["status"] == T.OK).all()
    ref = T.triangulate(model, intrs, None, poses, uv, o)
    assert np.array_equal(r["mask"], ref["mask"]) and _relnorm(r["xyz"], ref["xyz"]) <= 1e-9
    gone = uv.copy()
    gone[cam[bad], np.flatnonzero(bad)] = np.nan
    g = T.host_triangulate(tricpu, model, intrs, None, poses, gone, o)
    for k in ("xyz", "rms", "mask", "status", "cov"):
        assert r[k].tobytes() == g[k].tobytes()
    off = T.host_triangulate(tricpu, model, intrs, None, poses, uv)
    assert (off["rms"][bad] > 2.0).all() and (off["mask"] == _all_seen(n_cams)).all()
    two = T.host_triangulate(tricpu, model, intrs[:2], None, poses[:2], uv[:2], o)  # never below two cameras
    assert (two["mask"] == 3).all()


def test_status_cases(tricpu):
    for name, intrs, poses, uv, expect in T.status_cases():
        r = T.host_triangulate(tricpu, R.PINHOLE, intrs, None, poses, uv)
        assert r["status"][0] == expect, name
        assert T.triangulate(R.PINHOLE, intrs, None, poses, uv)["status"][0] == expect, name
        if expect == T.DEGENERATE:
            assert np.isnan(r["xyz"]).all() and np.isnan(r["rms"]).all() and r["mask"][0] == 3
        else:
            assert np.isfinite(r["xyz"]).all() and r["xyz"][0, 2] < 0
    intrs, poses, _, uv = T.scene(3, 17, R.PINHOLE, noise=0.3)
    r = T.host_triangulate(tricpu, R.PINHOLE, intrs, None, poses, uv, T.Options(max_iterations=1))
    assert (r["status"] == T.NOT_CONVERGED).all() and np.isfinite(r["xyz"]).all() and np.isfinite(r["rms"]).all()
    assert (r["linearisations"] == 2).all()


# ---- the C ABI's argument errors, all before any device work -------------------------------------------------------------------
def _d(a):
    return capi.dptr(None if a is None else np.ascontiguousarray(a, float))


def test_triangulate_abi_defaults_and_argument_errors(lib):
    o = capi.CbaTriangulateOptions()
    lib.cba_triangulate_options_default(C.byref(o))
    assert (o.max_iterations, o.step_tolerance, o.min_cams, o.max_reproj_px) == (10, 1e-12, 2, np.inf)
    assert capi.TRI_MAX_CAMS == 16
    intrs, poses, _, uv = T.scene(2, 4)
    xyz, st = np.empty((4, 3)), np.empty(4, np.int32)
    I = capi.CBA_ERR_INVALID_ARGUMENT
    ok = dict(model=0, n_cams=2, intr=intrs, n_inv=0, inv=None, poses=poses, n=4, uv=uv, opts=o, xyz=xyz, st=st)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cba_triangulate(a["model"], a["n_cams"], _d(a["intr"]), a["n_inv"], _d(a["inv"]), _d(a["poses"]), a["n"], _d(a["uv"]),
                                   None if a["opts"] is None else C.byref(a["opts"]), capi.dptr(a["xyz"]), capi.dptr(None), None,
                                   capi.i32ptr(a["st"]), capi.dptr(None))

    wide = np.tile(intrs[:1], (17, 1))
    assert call(n_cams=1) == I and call(n_cams=17, intr=wide, poses=np.tile(poses[:1], (17, 1))) == I
    assert call(model=2) == I
    assert call(n_inv=1, inv=np.zeros((2, 1))) == I and call(n_inv=17, inv=np.zeros((2, 17))) == I
    for name in ("intr", "poses", "uv", "opts", "xyz", "st"):
        assert call(**{name: None}) == I, name
    assert call(n=-1) == I
    zero_f = intrs.copy()
    zero_f[1, 0] = 0.0
    assert call(intr=zero_f) == I
    for field, value in (("max_iterations", -1), ("step_tolerance", -1.0), ("step_tolerance", np.nan), ("max_reproj_px", 0.0),
                         ("max_reproj_px", np.nan)):
        bad = capi.CbaTriangulateOptions()
        lib.cba_triangulate_options_default(C.byref(bad))
        setattr(bad, field, value)
        assert call(opts=bad) == I, field
    assert call(n=0, uv=None, xyz=None, st=None) == capi.CBA_OK  # n == 0: no work, no device needed


def test_python_layer_validates(lib):
    intrs, poses, _, uv = T.scene(2, 4)
    with pytest.raises(ValueError):
        triangulate([intrs[0], np.zeros(12)], poses, uv)  # two models
    with pytest.raises(ValueError):
        triangulate(intrs, poses[:1], uv)
    with pytest.raises(ValueError):
        triangulate(intrs, poses, uv[0])
    with pytest.raises(capi.CbaInvalidArgument):
        triangulate(intrs, poses, uv, opts=TriangulateOptions(max_iterations=-1))
    r = triangulate(intrs, np.stack([np.eye(4)] * 2), np.zeros((2, 0, 2)), covariance=True)
    assert r.xyz.shape == (0, 3) and r.used.shape == (0, 2) and r.cov.shape == (0, 3, 3)
