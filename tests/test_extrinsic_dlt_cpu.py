"""CPU tier of the rig seed: extrinsic_dlt_math.hpp (the per-lane algebra of cba_estimate_extrinsic_dlt) compiled for the host
(tests/extrinsic_dlt_cpu) against the numpy restatement tests/extrinsic_dlt_ref.py, and the C ABI's argument errors, which are all
raised before any device work."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi, rig
from calibration_amd.capi import dptr, i32ptr, i64ptr
from calibration_amd.geometry import rotmat_to_quat
from tests import extrinsic_dlt_ref as ref
from tests import host_build
from tests import synth


@pytest.fixture(scope="module")
def ext():
    lib = host_build.load("extrinsic_dlt_cpu")
    P, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.ext_average_c.argtypes = [C.c_int, P, P]
    lib.ext_steps_c.argtypes = [C.c_int, C.c_int, P, I, P, P]
    return lib


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _pose7(R, t):
    return np.concatenate([rotmat_to_quat(R), t])


def _rz(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _average(ext, poses7):
    P = np.ascontiguousarray(np.asarray(poses7, dtype=np.float64).reshape(-1, 7))
    out = np.zeros(7)
    ext.ext_average_c(len(P), dptr(P), dptr(out))
    return out


def _random_pose7(rng, rot_deg=180.0):
    axis = synth.rand_unit_axis(rng)
    R = synth.make_pose(np.zeros(3), axis, np.deg2rad(rng.uniform(-rot_deg, rot_deg)))[:3, :3]
    return _pose7(R, rng.normal(0, 1, 3))


def test_average_affines_computes_mean(ext):
    """Se3Utils.AverageAffinesComputesMean (se3_utils_test.cpp:30-40)."""
    poses = [np.r_[1.0, 0, 0, 0, float(i), 0, 0] for i in range(5)]
    avg = _average(ext, poses)
    assert abs(avg[4] - 2.0) <= 1e-12
    assert np.allclose(ref.matrix_of(avg)[:3, :3], np.eye(3), atol=1e-12)


def test_average_follows_the_running_sum_not_the_first_quaternion(ext):
    """0, 150 and 250 degrees about z: the 250-degree quaternion keeps its sign against the first one but is negated against the
    running sum, and the two rules give different rotations."""
    poses = [_pose7(_rz(a), np.array([0.1 * i, 0.0, 0.0])) for i, a in enumerate((0.0, 150.0, 250.0))]
    Ts = [ref.matrix_of(p) for p in poses]
    qs = [rotmat_to_quat(T[:3, :3]) for T in Ts]
    run = qs[0] + (qs[1] if qs[0] @ qs[1] >= 0 else -qs[1])
    assert abs(qs[0] @ qs[1]) > 1e-3 and abs(run @ qs[2]) > 1e-3 and abs(qs[0] @ qs[2]) > 1e-3  # no sign test near a tie
    assert (run @ qs[2] < 0) != (qs[0] @ qs[2] < 0)
    want, wrong = ref.average_isometries(Ts), ref.average_align_to_first(Ts)
    assert np.abs(ref.matrix_of(want)[:3, :3] - ref.matrix_of(wrong)[:3, :3]).max() > 0.1
    got = _average(ext, poses)
    assert np.abs(got - want).max() <= 1e-13
    # the order matters: the same poses fed in another order give another rotation
    got_rev = _average(ext, poses[::-1])
    assert np.abs(ref.matrix_of(got_rev)[:3, :3] - ref.matrix_of(got)[:3, :3]).max() > 1e-3
    assert np.abs(got_rev - ref.average_isometries(Ts[::-1])).max() <= 1e-13


@pytest.mark.parametrize("seed", range(6))
def test_average_matches_restatement_on_random_sets(ext, seed):
    rng = np.random.default_rng(100 + seed)
    poses = [_random_pose7(rng) for _ in range(int(rng.integers(1, 40)))]
    got = _average(ext, poses)
    want = ref.average_isometries([ref.matrix_of(p) for p in poses])
    assert np.abs(got - want).max() <= 1e-13


@pytest.mark.parametrize("n_views,n_cams,drop", [(5, 2, 0.0), (12, 3, 0.2), (40, 8, 0.3), (7, 1, 0.0)])
def test_steps_2_3_match_restatement(ext, n_views, n_cams, drop):
    """Random block poses (rotations up to 180 degrees, so the sign rule is exercised) with absent blocks and blocks of 3 points."""
    rng = np.random.default_rng(n_views * 10 + n_cams)
    P = np.zeros((n_views, n_cams, 7))
    N = np.zeros((n_views, n_cams), dtype=np.int32)
    T, npts = {}, {}
    for v in range(n_views):
        for c in range(n_cams):
            P[v, c] = _random_pose7(rng)
            N[v, c] = 0 if rng.uniform() < drop else int(rng.choice([3, 4, 50]))
            if N[v, c] > 0:
                T[(v, c)] = ref.matrix_of(P[v, c])
                npts[(v, c)] = int(N[v, c])
    cr, rt = np.zeros((n_cams, 7)), np.zeros((n_views, 7))
    ext.ext_steps_c(n_views, n_cams, dptr(np.ascontiguousarray(P.reshape(-1))), N.ctypes.data_as(C.POINTER(C.c_int)), dptr(cr), dptr(rt))
    cr_ref, rt_ref = ref.steps_2_3(n_views, n_cams, T, npts)
    assert np.abs(cr - cr_ref).max() <= 1e-13
    assert np.abs(rt - rt_ref).max() <= 1e-13


# ---- argument errors through the shipped library (no device needed: validation comes first) --------------------------------
def _call(lib, n_cams, n_views, off, bv, bc, n_pts=None):
    off = np.asarray(off, dtype=np.int64)
    n = max(int(off[-1]) if len(off) else 0, 1) if n_pts is None else n_pts
    cols = [np.zeros(n) for _ in range(4)]
    K = np.tile([100.0, 100.0, 0.0, 0.0, 0.0], (max(n_cams, 1), 1))
    cr, rt = np.zeros((max(n_cams, 1), 7)), np.zeros((max(n_views, 1), 7))
    st = lib.cba_estimate_extrinsic_dlt(n_cams, n_views, len(off) - 1, i64ptr(off), i32ptr(np.asarray(bv, dtype=np.int32)),
                                        i32ptr(np.asarray(bc, dtype=np.int32)), *(dptr(a) for a in cols), dptr(K), dptr(cr), dptr(rt),
                                        dptr(None), i32ptr(None))
    return st, lib.cba_last_error().decode(), cr, rt


def test_empty_rig_is_the_references_runtime_error(lib):
    for nc, nv in ((0, 3), (2, 0), (-1, 1)):
        st, msg, _, _ = _call(lib, nc, nv, [0], [], [])
        assert st == capi.CBA_ERR_RUNTIME and msg == "Empty views or cameras provided"


def test_block_errors_are_invalid_arguments(lib):
    cases = [
        ([0, 4, 8], [0, 0], [1, 1], "share view 0 and camera 1"),   # duplicate (view, camera)
        ([0, 4, 8], [0, 2], [0, 1], "view index out of range"),
        ([0, 4, 8], [0, 1], [0, 2], "camera index out of range"),
        ([0, 4, 8], [-1, 1], [0, 0], "view index out of range"),
        ([0, 6, 4], [0, 1], [0, 0], "bad block offsets"),           # decreasing
        ([0, -4, 4], [0, 1], [0, 0], "bad block offsets"),          # negative
        ([2, 6, 8], [0, 1], [0, 0], "block offsets must start at 0"),
    ]
    for off, bv, bc, what in cases:
        st, msg, _, _ = _call(lib, 2, 2, off, bv, bc, n_pts=8)
        assert st == capi.CBA_ERR_INVALID_ARGUMENT, (off, bv, bc, st, msg)
        assert what in msg, msg


def test_no_blocks_gives_identities(lib):
    st, msg, cr, rt = _call(lib, 3, 4, [0], [], [])
    assert st == capi.CBA_OK, msg
    assert np.array_equal(cr, np.tile(ref.IDENTITY7, (3, 1))) and np.array_equal(rt, np.tile(ref.IDENTITY7, (4, 1)))


def test_null_arguments(lib):
    off = np.array([0, 4], dtype=np.int64)
    st = lib.cba_estimate_extrinsic_dlt(1, 1, 1, i64ptr(off), i32ptr(np.zeros(1, np.int32)), i32ptr(None), dptr(np.zeros(4)),
                                        dptr(np.zeros(4)), dptr(np.zeros(4)), dptr(np.zeros(4)), dptr(np.ones(5)), dptr(np.zeros(7)),
                                        dptr(np.zeros(7)), dptr(None), i32ptr(None))
    assert st == capi.CBA_ERR_INVALID_ARGUMENT


def test_python_api_raises_the_references_errors():
    v = np.zeros((4, 4))
    with pytest.raises(capi.CbaError) as e:
        rig.estimate_extrinsic_dlt([], [np.ones(5)])
    assert e.value.status == capi.CBA_ERR_RUNTIME and e.value.message == "Empty views or cameras provided"
    with pytest.raises(capi.CbaError) as e:
        rig.estimate_extrinsic_dlt([[v, v]], [])
    assert e.value.status == capi.CBA_ERR_RUNTIME and e.value.message == "Empty views or cameras provided"
    with pytest.raises(capi.CbaError) as e:
        rig.estimate_extrinsic_dlt([[v, v], [v]], [np.ones(10), np.ones(10)])
    assert e.value.status == capi.CBA_ERR_RUNTIME
    assert e.value.message == "View 1 has wrong number of cameras: expected 2, got 1"


def test_calibrate_rig_without_usable_views_runs_no_solve():
    few = np.zeros((3, 4))
    r = rig.calibrate_rig([[None, np.zeros((5, 4))], [few, np.zeros((5, 4))]], [np.ones(10), np.ones(10)])
    assert not r.success and r.used_views == 0 and r.requested_views == 2
    assert r.view_status == ["missing_image", "insufficient_points"]
    assert r.optimization is None and r.initial_guess is None
