"""GPU tier of scan registration (cba_point_normals, cba_cloud_index, cba_cloud_nearest, cba_cloud_register) through the Python layer:
the device against the numpy restatement (tests/cloud_ref.py) and the host build of cloud_math.hpp - normals and neighbours to the bit
at the sizes where a kernel changes path (target and query counts around a wavefront and a workgroup, one cell, cell counts around the
scan's tile of 1024 cells and past 1024 x 1024, points on cell faces, planted ties, the gate and the box margin to the ulp), the sums
of a system inside the bound of a different order, full solves after the restatement's own condition, batch independence,
repeatability, the planted statuses, ground truth, and the argument errors that need a live handle."""
import ctypes as C

import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.registration import CloudIndex, IcpOptions, default_cell_size, point_normals, register
from tests import cloud_ref as R
from tests import host_build
from tests import test_cloud_cpu as cpu
from tests.test_cloud_cpu import CELL, INIT, MD, TRUTH_ERROR, check_sums, normal_map, planar_scene, ragged_sources, solved

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024  # the scan kernel's block of cells (scan_tiles.hpp: SCAN_TILE); cloud_ref.nearest_cases builds around it


@pytest.fixture(scope="module")
def host():
    return host_build.load("cloud_cpu")


def as_dict(r):
    return dict(pose7=r.pose7, rms=r.rms, H=r.H, g=r.g, n_pairs=r.n_pairs, iterations=r.iterations, status=r.status)


def same_bits(a, b):
    return all(np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes() for k in ("pose7", "rms", "H", "g")) and \
        (a.n_pairs, a.iterations, a.status) == (b.n_pairs, b.iterations, b.status)


# ---- 1. index and nearest ------------------------------------------------------------------------------------------------------------
def test_nearest_equals_brute_force_to_the_bit(gpu_lib, host):
    assert R.SCAN_TILE == SCAN_TILE
    for c in R.nearest_cases():
        ref_index, ref_dist2 = R.nearest(c["target"], c["query"], c["md"])
        with CloudIndex(c["target"], None, c["cell"]) as index:
            got_index, got_dist2 = index.nearest(c["query"], c["md"])
            again = index.nearest(c["query"], c["md"])
        assert np.array_equal(got_index, ref_index), c["name"]
        assert np.array_equal(got_dist2, ref_dist2, equal_nan=True), c["name"]
        assert np.array_equal(again[0], got_index) and np.array_equal(again[1], got_dist2, equal_nan=True)
        h_index, h_dist2 = R.host_nearest(host, c["target"], c["cell"], c["query"], c["md"])
        assert np.array_equal(got_index, h_index) and np.array_equal(got_dist2, h_dist2, equal_nan=True), c["name"]
        if "want" in c:
            assert np.array_equal(got_index, c["want"]), c["name"]


def test_nearest_on_a_scan_sized_neighbourhood(gpu_lib):
    # the scene's map as a target: every query that is a target point finds itself at distance 0; dist2 may be left out
    tgt, _, src, _ = solved("partial", 0)
    with CloudIndex(tgt, None, CELL) as index:
        i, d = index.nearest(tgt, MD)
        ok = R.valid(tgt.reshape(-1, 3))
        assert np.array_equal(i[ok], np.flatnonzero(ok)) and (d[ok] == 0).all() and (i[~ok] == -1).all()
        out = np.empty(3, np.int64)
        q = np.ascontiguousarray(tgt.reshape(-1, 3)[:3])
        capi.check(gpu_lib, gpu_lib.cba_cloud_nearest(index._h, 3, capi.dptr(q), MD, capi.i64ptr(out), capi.dptr(None)))
        assert np.array_equal(out, i[:3])


def test_index_and_register_argument_errors(gpu_lib):
    tgt, nrm, src, _ = solved("plain", 0)
    with pytest.raises(capi.CbaInvalidArgument, match="2\\^24"):
        CloudIndex(tgt, None, 1e-4)
    with pytest.raises(capi.CbaInvalidArgument, match="cell_size"):
        CloudIndex(tgt, None, 0.0)
    with pytest.raises(capi.CbaInvalidArgument):
        CloudIndex(tgt, None, CELL, device=99)
    with pytest.raises(ValueError):
        CloudIndex(tgt, nrm[:5], CELL)
    with CloudIndex(tgt, None, CELL) as index:
        for md in (0.999 * CELL * (1 + 1e-12), CELL, 0.0, -1.0, np.nan, np.inf):
            with pytest.raises(capi.CbaInvalidArgument, match="max_distance"):
                index.nearest(src, md)
            with pytest.raises(capi.CbaInvalidArgument, match="max_distance"):
                index.register([src], IcpOptions(md, metric=1))
        assert index.nearest(src, 0.999 * CELL)[0].shape == (1200,)
        with pytest.raises(capi.CbaInvalidArgument, match="normals"):
            index.register([src], IcpOptions(MD, metric=0))
        for bad in (IcpOptions(MD, metric=2), IcpOptions(MD, metric=1, max_iterations=-1), IcpOptions(MD, metric=1, step_tolerance=-1.0),
                    IcpOptions(MD, metric=1, step_tolerance=np.nan)):
            with pytest.raises(capi.CbaInvalidArgument):
                index.register([src], bad)
        for q in ([0.0, 0, 0, 0], [np.nan, 0, 0, 0]):
            with pytest.raises(capi.CbaInvalidArgument, match="quaternion"):
                index.register([src], IcpOptions(MD, metric=1), init_pose7=[q + [0.0, 0, 0]])
        assert index.register([], IcpOptions(MD, metric=1)) == []
        assert index.nearest(np.zeros((0, 3)), MD)[0].shape == (0,)
        # NULLs at the C boundary
        h, o = index._h, IcpOptions(MD, metric=1)._c()
        off = np.array([0, 2], np.int64)
        res = (capi.CbaIcpResult * 1)()
        q = np.zeros((2, 3))
        bad = capi.CBA_ERR_INVALID_ARGUMENT
        assert gpu_lib.cba_cloud_nearest(h, 2, capi.dptr(None), MD, capi.i64ptr(np.zeros(2, np.int64)), capi.dptr(None)) == bad
        assert gpu_lib.cba_cloud_nearest(h, 2, capi.dptr(q), MD, capi.i64ptr(None), capi.dptr(None)) == bad
        assert gpu_lib.cba_cloud_register(h, 1, capi.i64ptr(None), capi.dptr(q), capi.dptr(None), C.byref(o), res) == bad
        assert gpu_lib.cba_cloud_register(h, 1, capi.i64ptr(off), capi.dptr(None), capi.dptr(None), C.byref(o), res) == bad
        assert gpu_lib.cba_cloud_register(h, 1, capi.i64ptr(off), capi.dptr(q), capi.dptr(None), None, res) == bad
        assert gpu_lib.cba_cloud_register(h, 1, capi.i64ptr(off), capi.dptr(q), capi.dptr(None), C.byref(o), None) == bad
        assert gpu_lib.cba_cloud_register(h, 1, capi.i64ptr(np.array([1, 2], np.int64)), capi.dptr(q), capi.dptr(None), C.byref(o), res) == bad
        assert gpu_lib.cba_cloud_register(h, 1, capi.i64ptr(np.array([0, -1], np.int64)), capi.dptr(q), capi.dptr(None), C.byref(o), res) == bad
    with pytest.raises(ValueError, match="closed"):
        index.nearest(src, MD)


# ---- 2. normals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cpu.NORMAL_SIZES)
def test_normals_equal_restatement_and_host_build_to_the_bit(gpu_lib, host, size):
    W, H = size
    xyz, max_jump, vp = normal_map(W, H)
    batch = np.stack([xyz, xyz[::-1, ::-1] * 1.5, np.full_like(xyz, np.nan)])  # a pixel's result does not depend on the other maps
    for maps in (xyz, batch):
        for jump, view in ((max_jump, vp), (np.inf, None)):
            ref = R.normals(maps, view, jump)
            got = point_normals(maps, view, jump)
            assert got.shape == maps.shape
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert np.array_equal(got, ref, equal_nan=True)
            assert np.array_equal(got, R.host_normals(host, maps, view, jump), equal_nan=True)
    with pytest.raises(capi.CbaInvalidArgument, match="max_jump"):
        point_normals(xyz, None, 0.0)
    with pytest.raises(capi.CbaInvalidArgument, match="max_jump"):
        point_normals(xyz, None, np.nan)


# ---- 3. register -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_statistics_at_the_initial_pose_within_the_order_bound(gpu_lib, metric):
    tgt, nrm, src, _ = solved("partial", metric)
    sources = ragged_sources(src)
    assert [len(s) for s in sources] == [0, 1, 5, 64, 257, 1200]
    pose = np.concatenate([R.normalise(INIT[:4]), INIT[4:]])
    with CloudIndex(tgt, nrm, CELL) as index:
        got = index.register(sources, IcpOptions(MD, metric=metric, max_iterations=0), init_pose7=np.tile(INIT, (len(sources), 1)))
    for s, g in zip(sources, got):
        ref = R.system(tgt, nrm, s, pose, metric, MD)
        print(f"metric {metric}, {len(s)} points: pairs {g.n_pairs}, largest |H - H_ref| / bound "
              f"{(np.abs(g.H - ref['H']) / np.maximum(2 * max(len(s), 1) * 2.0 ** -53 * ref['H_abs'], 1e-300)).max():.3g}")
        check_sums(as_dict(g), ref, max(len(s), 1))
        assert np.array_equal(g.pose7, pose) and g.iterations == 0
        assert g.status == (R.TOO_FEW if ref["n_pairs"] < 6 else R.NOT_CONVERGED)


@pytest.mark.parametrize("metric", [0, 1])
def test_batch_independence_and_repeatability(gpu_lib, metric):
    tgt, nrm, src, _ = solved("partial", metric)
    sources = ragged_sources(src)
    opts = IcpOptions(MD, metric=metric, max_iterations=8, step_tolerance=1e-12)
    with CloudIndex(tgt, nrm, CELL) as index:
        batch = index.register(sources, opts)
        again = index.register(sources, opts)
        alone = [index.register([s], opts)[0] for s in sources]
        mixed = index.register(sources[::-1], opts)[::-1]
    with CloudIndex(tgt, nrm, CELL) as other:  # another build of the index: the order inside a cell may differ, no result does
        rebuilt = other.register(sources, opts)
    for b, a, o, m, r in zip(batch, again, alone, mixed, rebuilt):
        assert same_bits(b, a) and same_bits(b, o) and same_bits(b, m) and same_bits(b, r)
    assert batch[0].status == R.TOO_FEW and batch[0].n_pairs == 0 and batch[-1].iterations > 0


@pytest.mark.parametrize("metric", [0, 1])
def test_source_on_the_target_stays_at_the_identity(gpu_lib, metric):
    tgt, nrm, _, _ = solved("plain", metric)
    src = tgt.reshape(-1, 3)[::3]
    with CloudIndex(tgt, nrm, CELL) as index:
        r = index.register([src], IcpOptions(MD, metric=metric, step_tolerance=1e-12))[0]
    assert (r.g == 0).all() and r.rms == 0
    assert (r.status, r.iterations, r.n_pairs) == (R.OK, 1, len(src))
    assert r.pose7.tobytes() == np.array([1.0, 0, 0, 0, 0, 0, 0]).tobytes()


@pytest.mark.parametrize("scene", sorted(cpu.SCENES))
@pytest.mark.parametrize("metric", [0, 1])
def test_full_solve_against_restatement_and_ground_truth(gpu_lib, scene, metric):
    tgt, nrm, src, ref = solved(scene, metric)
    assert ref["gap"] >= 1e-9 * MD ** 2  # the condition: no search decision of the restatement was closer than this
    with CloudIndex(tgt, nrm, CELL) as index:
        got = index.register([src], IcpOptions(MD, metric=metric, max_iterations=60, step_tolerance=1e-12))[0]
    drot, dtr = R.pose_error(got.pose7, ref["pose7"])
    print(f"{scene} metric {metric}: status {got.status}, iterations {got.iterations}, pairs {got.n_pairs}; against the restatement "
          f"{drot:.3g} rad, {dtr:.3g}, rms {abs(got.rms - ref['rms']) / ref['rms']:.3g} relative")
    assert (got.status, got.iterations, got.n_pairs) == (ref["status"], ref["iterations"], ref["n_pairs"])
    assert drot <= 1e-9 and dtr <= 1e-9 * R.extent(tgt)
    assert abs(got.rms - ref["rms"]) <= 1e-9 * ref["rms"]
    rot, tr = R.pose_error(got.pose7, R.TRUTH)
    assert rot <= 2 * TRUTH_ERROR[(scene, metric)][0] and tr <= 2 * TRUTH_ERROR[(scene, metric)][1]
    # the facade: builds the index itself (cell_size from max_distance, normals from the organised target), same rule
    if scene == "plain":
        one = register(src, tgt, IcpOptions(MD, metric=metric, max_iterations=60, step_tolerance=1e-12))
        assert one.status == R.OK and R.pose_error(one.pose7, R.TRUTH)[0] <= 2 * TRUTH_ERROR[(scene, metric)][0]
        assert 0.999 * default_cell_size(MD) >= MD and one.matrix.shape == (4, 4)


def test_planted_statuses(gpu_lib):
    tgt, nrm, src = planar_scene()
    with CloudIndex(tgt, nrm, CELL) as index:
        r = index.register([src], IcpOptions(MD, metric=0))[0]
    assert (r.status, r.iterations, r.n_pairs) == (R.DEGENERATE, 0, len(src))
    tgt, nrm, src, ref = solved("plain", 1)
    far = src.reshape(-1, 3) + np.array([0.0, 0.0, 3.0])
    with CloudIndex(tgt, nrm, CELL) as index:
        got = index.register([src.reshape(-1, 3)[:0], far, src], IcpOptions(MD, metric=1, max_iterations=2, step_tolerance=1e-12))
    assert [(g.status, g.n_pairs, g.iterations) for g in got[:2]] == [(R.TOO_FEW, 0, 0)] * 2 and np.isnan(got[0].rms) and np.isnan(got[1].rms)
    capped = R.register(tgt, nrm, src, MD, metric=1, max_iterations=2, step_tolerance=1e-12)
    assert (got[2].status, got[2].iterations, got[2].n_pairs) == (R.NOT_CONVERGED, 2, capped["n_pairs"])
    assert R.pose_error(got[2].pose7, capped["pose7"])[0] <= 1e-9


def test_package_exports():
    for name in ("CloudIndex", "IcpOptions", "IcpResult", "point_normals", "register"):
        assert hasattr(cal, name)
