"""The C ABI's checks of the observation arrays and their offset tables, entry point by entry point.  Every check comes before
any device work, so the shipped library answers without a GPU: a bad table is CBA_ERR_INVALID_ARGUMENT with the message
recorded below, and a well-formed call ends at CBA_ERR_NO_DEVICE.  The entry points differ on purpose or by history in whether
a table must start at 0 and whether a group may hold more than 2^31 - 1 observations; EXPECTED records what each one answers
(taken from the library before the checks were merged into one helper) and pins it.

The whole file skips itself where a device is visible: some entry points set no limit on a group's size, so the 2^31 table
passes their check and only the missing device stops the call - with a device it would read far past these small buffers."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.capi import dptr, i32ptr, i64ptr, u8ptr

G, PER = 4, 4            # groups (views / blocks / problems) and observations in each
N = G * PER
INVALID, NO_DEVICE = capi.CBA_ERR_INVALID_ARGUMENT, capi.CBA_ERR_NO_DEVICE
NODEV_MSG = "no HIP device visible: libcalibba has no CPU fallback"

GOOD = [0, 4, 8, 12, 16]
TABLES = {
    "good": GOOD,
    "start_not_0": [2, 6, 10, 14, 18],
    "decreasing": [0, 8, 4, 12, 16],
    "negative": [0, -4, 4, 8, 12],
    "span_2_31": [0, 2 ** 31, 2 ** 31 + 4, 2 ** 31 + 8, 2 ** 31 + 12],
    "null_table": None,
}
CASES = list(TABLES) + ["null_data"]


@pytest.fixture(scope="module")
def lib():
    lib = capi.load_library()
    if lib.cba_device_count() > 0:
        pytest.skip("argument checks that end at CBA_ERR_NO_DEVICE: not to be run where a device is visible")
    return lib


def _d(*shape):
    return np.zeros(shape if shape else (N,))


def _i(n):
    return np.zeros(n, dtype=np.int32)


def _semidlt(lib, off, X, Y, u, v):
    o, s = capi.default_options(lib), capi.CbaSummary()
    return lib.cba_optimize_intrinsics_semidlt(G, off, X, Y, u, v, dptr(_d(5)), dptr(_d(G, 7)), 2, dptr(None), dptr(None), i32ptr(None),
                                               dptr(None), 0, C.byref(o), C.byref(s), dptr(None), dptr(None), dptr(None))


@capi.ALLREDUCE_FN
def _dummy_allreduce(buf, count, user):
    return 0


def _semidlt_sharded(lib, off, X, Y, u, v):
    o, s = capi.default_options(lib), capi.CbaSummary()
    return lib.cba_optimize_intrinsics_semidlt_sharded(G, off, X, Y, u, v, G, 0, dptr(_d(5)), dptr(_d(G, 7)), 2, dptr(None), dptr(None),
                                                       i32ptr(None), dptr(None), 0, C.byref(o), C.byref(s), dptr(None), dptr(None),
                                                       dptr(None), _dummy_allreduce, None, 1, 0, 0)


def _homography(lib, off, X, Y, u, v):
    return lib.cba_estimate_homography_batch(G, off, X, Y, u, v, dptr(_d(G, 9)), i32ptr(_i(G)))


def _planar_pose(lib, off, X, Y, u, v):
    return lib.cba_estimate_planar_pose_batch(G, off, X, Y, u, v, dptr(np.array([100.0, 100.0, 0.0, 0.0, 0.0])), dptr(_d(G, 7)))


def _laser(lib, toff, X, Y, u, v, loff=None):
    o, r = capi.CbaPlaneFitOptions(), capi.CbaLaserPlaneResult()
    lib.cba_plane_fit_options_default(C.byref(o))
    intr = np.array([100.0, 100.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    good = np.asarray(GOOD, dtype=np.int64)
    return lib.cba_calibrate_laser_plane(0, dptr(intr), 0, dptr(None), G, toff, X, Y, u, v, i64ptr(good) if loff is None else loff,
                                         dptr(_d()), dptr(_d()), C.byref(o), C.byref(r), dptr(None), u8ptr(None))


def _laser_laser_table(lib, off, X, Y, u, v):
    """cba_calibrate_laser_plane with the table under test as laser_offset (the laser pixels' table has a policy of its own)."""
    return _laser(lib, i64ptr(np.asarray(GOOD, dtype=np.int64)), X, Y, u, v, loff=off)


def _homography_ransac(lib, off, X, Y, u, v):
    o = capi.CbaRansacOptions()
    lib.cba_ransac_options_default(C.byref(o))
    return lib.cba_estimate_homography_ransac_batch(G, off, X, Y, u, v, C.byref(o), dptr(_d(G, 9)), i32ptr(_i(G)), i32ptr(_i(G)),
                                                    dptr(_d(G)), u8ptr(None))


def _intrinsics(lib, off, X, Y, u, v):
    return lib.cba_estimate_intrinsics(G, off, X, Y, u, v, 0, None, dptr(None), dptr(None), 0, i32ptr(_i(1)), dptr(_d(5)), i32ptr(_i(1)),
                                       i32ptr(_i(G)), dptr(_d(G, 9)), dptr(_d(G)), dptr(_d(G, 12)), i32ptr(_i(G)), u8ptr(None))


def _extrinsic_dlt(lib, off, X, Y, u, v):
    bv, bc = np.array([0, 0, 1, 1], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32)
    K = np.tile([100.0, 100.0, 0.0, 0.0, 0.0], (2, 1))
    return lib.cba_estimate_extrinsic_dlt(2, 2, G, off, i32ptr(bv), i32ptr(bc), X, Y, u, v, dptr(K), dptr(_d(2, 7)), dptr(_d(2, 7)),
                                          dptr(None), i32ptr(None))


def _bundle_seed(lib, off, X, Y, u, v):
    bTg = np.tile([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], (G, 1))
    K = np.tile([100.0, 100.0, 0.0, 0.0, 0.0], (2, 1))
    return lib.cba_estimate_bundle_seed(2, G, off, i32ptr(np.array([0, 1, 0, 1], dtype=np.int32)), dptr(bTg), X, Y, u, v, dptr(K), 1.0,
                                        i32ptr(None), dptr(None), dptr(None), dptr(_d(2, 7)), i32ptr(_i(2)), i32ptr(_i(2)), dptr(_d(7)),
                                        i32ptr(_i(1)), dptr(None), i32ptr(None))


def _fit_distortion(lib, off, X, Y, u, v):
    K = np.tile([100.0, 100.0, 0.0, 0.0, 0.0], (G, 1))
    return lib.cba_fit_distortion_batch(G, off, X, Y, u, v, dptr(K), 2, 0, i32ptr(None), dptr(None), 0, dptr(_d(G, 5)), dptr(None),
                                        i32ptr(_i(G)), dptr(None))


def _linear(lib, off, X, Y, u, v):
    return lib.cba_estimate_intrinsics_linear_batch(G, off, X, Y, u, v, dptr(None), dptr(None), 0, dptr(_d(G, 5)), i32ptr(_i(G)),
                                                    i32ptr(_i(G)))


def _linear_iterative(lib, off, X, Y, u, v):
    return lib.cba_estimate_intrinsics_linear_iterative_batch(G, off, X, Y, u, v, 2, 3, 0, dptr(_d(G, 5)), dptr(_d(G, 5)), i32ptr(_i(G)),
                                                              i32ptr(_i(G)), i32ptr(_i(G)))


ENTRY_POINTS = {
    "cba_optimize_intrinsics_semidlt": _semidlt,
    "cba_optimize_intrinsics_semidlt_sharded": _semidlt_sharded,
    "cba_estimate_homography_batch": _homography,
    "cba_estimate_planar_pose_batch": _planar_pose,
    "cba_calibrate_laser_plane": _laser,
    "cba_calibrate_laser_plane[laser_offset]": _laser_laser_table,
    "cba_estimate_homography_ransac_batch": _homography_ransac,
    "cba_estimate_intrinsics": _intrinsics,
    "cba_estimate_extrinsic_dlt": _extrinsic_dlt,
    "cba_estimate_bundle_seed": _bundle_seed,
    "cba_fit_distortion_batch": _fit_distortion,
    "cba_estimate_intrinsics_linear_batch": _linear,
    "cba_estimate_intrinsics_linear_iterative_batch": _linear_iterative,
}

# What the library answered before the checks were merged (status, cba_last_error()), per entry point and case.  Not to be edited
# to follow the code: a difference here is a change of the C ABI's behaviour.
_NODEV = (NO_DEVICE, NODEV_MSG)


def _row(start_not_0, order, span_2_31):
    """One entry point's answers: the message for a table not starting at 0 and for a 2^31 group (None: accepted, the call goes
    on to the missing device), and the message for a decreasing step."""
    bad = lambda msg: _NODEV if msg is None else (INVALID, msg)
    return {"good": _NODEV, "start_not_0": bad(start_not_0), "decreasing": bad(order), "negative": bad(order),
            "span_2_31": bad(span_2_31), "null_table": (INVALID, "null argument"), "null_data": (INVALID, "null argument")}


_VIEWS_ANY_START = _row(None, "bad view offsets", "bad view offsets")
_VIEWS = _row("view offsets must start at 0", "bad view offsets", "bad view offsets")
_BLOCKS = _row("block offsets must start at 0", "bad block offsets", "bad block offsets")
_PROBLEMS = _row("offsets must start at 0", "offsets must not decrease", None)
EXPECTED = {
    "cba_optimize_intrinsics_semidlt": _VIEWS_ANY_START,
    "cba_optimize_intrinsics_semidlt_sharded": _VIEWS_ANY_START,
    "cba_estimate_homography_batch": _VIEWS_ANY_START,
    "cba_estimate_planar_pose_batch": _VIEWS_ANY_START,
    "cba_calibrate_laser_plane": _row("offsets must start at 0", "bad view offsets", "bad view offsets"),
    "cba_calibrate_laser_plane[laser_offset]": _row("offsets must start at 0", "bad view offsets", None),
    "cba_estimate_homography_ransac_batch": _VIEWS,
    "cba_estimate_intrinsics": _VIEWS,
    "cba_estimate_extrinsic_dlt": _BLOCKS,
    "cba_estimate_bundle_seed": _BLOCKS,
    "cba_fit_distortion_batch": _PROBLEMS,
    "cba_estimate_intrinsics_linear_batch": _PROBLEMS,
    "cba_estimate_intrinsics_linear_iterative_batch": _PROBLEMS,
}


def observe(lib, entry, case):
    """(status, message) of one entry point on one case.  The data arrays hold N entries; no call here reaches a device."""
    table = TABLES.get(case, GOOD)
    off = None if table is None else np.asarray(table, dtype=np.int64)
    cols = [_d() for _ in range(4)]
    ptrs = [dptr(c) for c in cols]
    if case == "null_data":
        ptrs[0] = dptr(None)
    st = ENTRY_POINTS[entry](lib, i64ptr(off), *ptrs)
    return st, lib.cba_last_error().decode()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_offset_table_checks(lib, entry, case):
    assert observe(lib, entry, case) == EXPECTED[entry][case]


def test_every_case_is_pinned():
    assert set(EXPECTED) == set(ENTRY_POINTS)
    for entry, row in EXPECTED.items():
        assert set(row) == set(CASES), entry
        assert row["good"] == _NODEV, entry
