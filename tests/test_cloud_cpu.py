"""CPU tier of scan registration (cba_point_normals, cba_cloud_index, cba_cloud_nearest, cba_cloud_register): the numpy restatement
(tests/cloud_ref.py) against the host build of cloud_math.hpp (tests/cloud_cpu) - normals and neighbours to the bit, the iteration to
the bars of the GPU tier - and against ground truth on rendered scenes; the conditions under which the GPU tier compares full solves;
the stand-alone driver under the sanitizers; and what the library checks before it asks for a device."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.capi import dptr, i64ptr
from tests import cloud_ref as R
from tests import host_build

MD, CELL = 0.05, 0.0501
# The scenes of the full solves (cloud_ref.scene_pair): (seed, partial, step).  "plain": the whole source lies on the target's surface;
# "partial": the source starts 14 pixels further right and the surface has a depth step and holes, so the gate rejects a fifth of it.
SCENES = {"plain": (1, False, False), "partial": (1, True, True)}
# Ground truth, measured on the restatement with max_distance 0.05, step_tolerance 1e-12, max_iterations 60: the rotation error in rad
# and the translation error of the returned pose against cloud_ref.TRUTH, (scene, metric).  Point to point slides along a sampled
# surface towards the closest samples, which is what the figures of metric 1 show; point to plane is held by the surface itself.  The
# figures are the measured values rounded up in their fourth digit.  The host build is held to these plus 1e-9, the device (GPU tier)
# to twice these.
TRUTH_ERROR = {("plain", 0): (3.443e-4, 5.774e-5), ("plain", 1): (3.720e-2, 8.263e-3),
               ("partial", 0): (2.207e-3, 4.838e-4), ("partial", 1): (8.172e-3, 1.905e-2)}
NORMAL_SIZES = [(1, 1), (3, 2), (64, 4), (65, 3), (130, 33)]


@pytest.fixture(scope="module")
def host():
    return host_build.load("cloud_cpu")


_solved = {}


def solved(scene, metric):
    """the scene and the restatement's full solve of it, computed once for the module (and for the GPU tier, which imports this)"""
    key = (scene, metric)
    if key not in _solved:
        seed, partial, step = SCENES[scene]
        tgt, nrm, src = R.scene_pair(seed, partial=partial, step=step)
        ref = R.register(tgt, nrm, src, MD, metric=metric, max_iterations=60, step_tolerance=1e-12)
        _solved[key] = (tgt, nrm, src, ref)
    return _solved[key]


def normal_map(W, H):
    """a map with a depth step, holes and (for more than one row) a NaN row end, and its max_jump and viewpoint"""
    xyz = R.surface_map(W, H, seed=W + H, focal=max(W, H) * 1.3, step=True, holes=max(1, W * H // 40) if W * H > 2 else 0)
    return xyz, 0.1, np.array([0.05, -0.02, 0.1])


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------
def test_driver_runs_clean_under_sanitizers():
    p = host_build.run_sanitized("cloud_cpu")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "cloud_driver: 0 mismatches" in p.stdout and not p.stderr.strip(), p.stdout + p.stderr


# ---- nearest neighbour -------------------------------------------------------------------------------------------------------------------
def test_nearest_restatement_equals_host_build_to_the_bit(host):
    for c in R.nearest_cases():
        index, dist2 = R.nearest(c["target"], c["query"], c["md"])
        h_index, h_dist2 = R.host_nearest(host, c["target"], c["cell"], c["query"], c["md"])
        assert np.array_equal(index, h_index), c["name"]
        assert np.array_equal(dist2, h_dist2, equal_nan=True), c["name"]
        assert np.array_equal(np.isnan(dist2), index < 0)
        if "want" in c:
            assert np.array_equal(index, c["want"]), c["name"]


def test_nearest_cases_cover_what_they_claim():
    cases = {c["name"]: c for c in R.nearest_cases()}
    assert {c["n_cells"] for c in cases.values() if "n_cells" in c} >= {R.SCAN_TILE - 1, R.SCAN_TILE, R.SCAN_TILE + 1}
    assert max(c.get("n_cells", 0) for c in cases.values()) > R.SCAN_TILE * R.SCAN_TILE
    for c in cases.values():
        if "n_cells" in c:
            t = c["target"][R.valid(c["target"])]
            assert int(np.prod(np.floor((t.max(0) - t.min(0)) / c["cell"]) + 1)) == c["n_cells"]
    t = cases["one_cell"]["target"]
    assert (np.floor((t.max(0) - t.min(0)) / cases["one_cell"]["cell"]) == 0).all()
    # the planted ties are real ties and the gate cases sit exactly on and one ulp off the bar
    c = cases["faces_ties"]
    d2 = ((c["query"][:8, None, :] - c["target"][None]) ** 2).sum(-1)
    assert [int((row == row.min()).sum()) for row in d2] == [2, 8] * 4
    c = cases["gate_margin"]
    assert (c["query"][0, 0] - 0.5) ** 2 == c["md"] ** 2 and (c["query"][1, 0] - 0.5) ** 2 > c["md"] ** 2


def test_host_build_refuses_too_many_cells(host):
    t = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    with pytest.raises(RuntimeError, match="grid plan 2"):
        R.host_nearest(host, t, 1.0 / 300.0, t, 0.001)  # 301^3 > 2^24
    R.host_nearest(host, t, 1.0 / 255.0, t, 0.001)      # 256^3 == 2^24


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", NORMAL_SIZES)
def test_normals_restatement_equals_host_build_to_the_bit(host, size):
    W, H = size
    xyz, max_jump, vp = normal_map(W, H)
    for jump, view in ((max_jump, vp), (np.inf, None)):
        ref = R.normals(xyz, view, jump)
        got = R.host_normals(host, xyz, view, jump)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got, ref, equal_nan=True)
        ok = ~np.isnan(ref[..., 0])
        if W * H == 1:
            assert not ok.any()
        else:
            assert ok.any() or W * H <= 6
        assert np.allclose(np.linalg.norm(ref[ok], axis=-1), 1.0, atol=1e-15)
        towards = ((np.zeros(3) if view is None else view) - xyz[ok]) * ref[ok]
        assert (towards.sum(-1) >= 0).all()


def test_normals_rule_on_planted_maps():
    # a plane z = 1 + x / 4 seen from the origin: every pixel, also beside a hole and at the border, has the plane's normal
    v, u = np.mgrid[0:5, 0:6].astype(float)
    xyz = np.stack([u / 8, v / 8, 1 + u / 32], -1)
    xyz[2, 3] = np.nan
    n = R.normals(xyz)
    want = np.array([0.25, 0.0, -1.0]) / np.sqrt(1.0625)
    ok = ~np.isnan(xyz[..., 0])
    assert np.allclose(n[ok], want, atol=1e-15) and np.isnan(n[2, 3]).all()
    # max_jump: a pixel whose right neighbour is across a step uses the one-sided difference to the left; one cut off on both sides of
    # an axis has no normal
    xyz = np.stack([u / 8, v / 8, np.ones_like(u)], -1)
    xyz[:, 3:, 2] += 1.0
    n = R.normals(xyz, max_jump=0.5)
    assert np.allclose(n[:, :, 2], -1.0) and not np.isnan(n).any()
    xyz[:, 4:, 2] += 1.0  # column 3 is now alone in its row
    n = R.normals(xyz, max_jump=0.5)
    assert np.isnan(n[:, 3]).all() and not np.isnan(n[:, :3]).any()
    # a viewpoint behind the surface turns the normals round
    assert np.array_equal(R.normals(xyz[:, :3], viewpoint=[0, 0, 5.0]), -R.normals(xyz[:, :3]))


# ---- the iteration -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("metric", [0, 1])
def test_full_solve_restatement_host_build_and_ground_truth(host, scene, metric):
    tgt, nrm, src, ref = solved(scene, metric)
    # the condition under which another implementation must take the same decisions: no search decision closer than 1e-9 md^2
    print(f"{scene} metric {metric}: gap {ref['gap']:.3g} ({ref['gap'] / MD ** 2:.3g} md^2), status {ref['status']}, iterations "
          f"{ref['iterations']}, pairs {ref['n_pairs']}, rms {ref['rms']:.6g}")
    assert ref["gap"] >= 1e-9 * MD ** 2
    assert ref["status"] == R.OK and ref["iterations"] < 60
    rot, tr = R.pose_error(ref["pose7"], R.TRUTH)
    print(f"  restatement against truth: {rot:.4g} rad, {tr:.4g}")
    bar = TRUTH_ERROR[(scene, metric)]
    assert 0.99 * bar[0] <= rot <= bar[0] and 0.99 * bar[1] <= tr <= bar[1]  # the constants are the measured values
    if scene == "partial":
        assert ref["n_pairs"] < 0.85 * R.valid(src).sum()  # the gate rejects
    got = R.host_register(host, tgt, nrm, CELL, [src], MD, metric=metric, max_iterations=60, step_tolerance=1e-12)[0]
    assert (got["status"], got["iterations"], got["n_pairs"]) == (ref["status"], ref["iterations"], ref["n_pairs"])
    drot, dtr = R.pose_error(got["pose7"], ref["pose7"])
    assert drot <= 1e-9 and dtr <= 1e-9 * R.extent(tgt)
    assert abs(got["rms"] - ref["rms"]) <= 1e-9 * ref["rms"]
    hrot, htr = R.pose_error(got["pose7"], R.TRUTH)
    assert hrot <= bar[0] + 1e-9 and htr <= bar[1] + 1e-9


def ragged_sources(src):
    flat = src.reshape(-1, 3)
    return [flat[:0], flat[7:8], flat[100:105], flat[200:264], flat[300:557], flat]


INIT = 1.7 * R.pose_from_rotvec([0.01, 0.0, -0.01], [0.002, 0.0, -0.001])  # not normalised: the entry normalises it


def check_sums(got, ref, m):
    """max_iterations = 0: the terms are the restatement's to the bit, so only the order of the sums differs: 2 m 2^-53 sum |terms|.  ss
    is recovered from rms = sqrt(ss / n): a division, a root (which halves a relative error), a square and a product, each within
    2^-53 relative: 8 2^-53 ss covers them."""
    u = 2.0 ** -53
    assert got["n_pairs"] == ref["n_pairs"]
    assert (np.abs(got["H"] - ref["H"]) <= 2 * m * u * ref["H_abs"]).all()
    assert (np.abs(got["g"] - ref["g"]) <= 2 * m * u * ref["g_abs"]).all()
    assert np.array_equal(got["H"], got["H"].T)
    if ref["n_pairs"] == 0:
        assert np.isnan(got["rms"])
    else:
        assert abs(got["rms"] ** 2 * got["n_pairs"] - ref["ss"]) <= 2 * m * u * ref["ss_abs"] + 8 * u * ref["ss"]


@pytest.mark.parametrize("metric", [0, 1])
def test_statistics_at_the_initial_pose(host, metric):
    tgt, nrm, src, _ = solved("partial", metric)
    sources = ragged_sources(src)
    got = R.host_register(host, tgt, nrm, CELL, sources, MD, metric=metric, max_iterations=0, init_pose7=np.tile(INIT, (len(sources), 1)))
    pose = np.concatenate([R.normalise(INIT[:4]), INIT[4:]])
    for s, g in zip(sources, got):
        ref = R.system(tgt, nrm, s, pose, metric, MD)
        check_sums(g, ref, max(len(s), 1))
        assert np.array_equal(g["pose7"], pose) and g["iterations"] == 0
        assert g["status"] == (R.TOO_FEW if ref["n_pairs"] < 6 else R.NOT_CONVERGED)  # min_pairs is 6 here, for both metrics


@pytest.mark.parametrize("metric", [0, 1])
def test_source_on_the_target_stays_at_the_identity(host, metric):
    tgt, nrm, _, _ = solved("plain", metric)
    src = tgt.reshape(-1, 3)[::3]
    for r in (R.register(tgt, nrm, src, MD, metric=metric, step_tolerance=1e-12),
              R.host_register(host, tgt, nrm, CELL, [src], MD, metric=metric, step_tolerance=1e-12)[0]):
        assert (r["g"] == 0).all() and r["rms"] == 0
        assert (r["status"], r["iterations"], r["n_pairs"]) == (R.OK, 1, len(src))
        assert r["pose7"].tobytes() == np.array([1.0, 0, 0, 0, 0, 0, 0]).tobytes()


def planar_scene():
    """the plane z = 1 with its exact normals, and a source on it"""
    v, u = np.mgrid[0:20, 0:24].astype(float)
    tgt = np.stack([(u - 11.5) / 60, (v - 9.5) / 60, np.ones_like(u)], -1)
    return tgt, R.normals(tgt), tgt.reshape(-1, 3)[5:300:2] + np.array([0.004, -0.003, 0.002])


def test_planted_statuses(host):
    tgt, nrm, src = planar_scene()
    assert np.array_equal(nrm[5, 5], [0.0, 0.0, -1.0])
    for r in (R.register(tgt, nrm, src, MD, metric=0), R.host_register(host, tgt, nrm, CELL, [src], MD, metric=0)[0]):
        assert (r["status"], r["iterations"]) == (R.DEGENERATE, 0) and r["n_pairs"] == len(src)
    tgt, nrm, src, ref = solved("plain", 1)
    far = src.reshape(-1, 3) + np.array([0.0, 0.0, 3.0])
    got = R.host_register(host, tgt, nrm, CELL, [src.reshape(-1, 3)[:0], far, src], MD, metric=1, max_iterations=2, step_tolerance=1e-12)
    assert [(g["status"], g["n_pairs"], g["iterations"]) for g in got[:2]] == [(R.TOO_FEW, 0, 0)] * 2 and np.isnan(got[0]["rms"])
    capped = R.register(tgt, nrm, src, MD, metric=1, max_iterations=2, step_tolerance=1e-12)
    assert (got[2]["status"], got[2]["iterations"]) == (R.NOT_CONVERGED, 2) == (capped["status"], capped["iterations"])
    assert got[2]["n_pairs"] == capped["n_pairs"] and ref["iterations"] > 2


# ---- the library without a device: every argument error comes first ----------------------------------------------------------------------
def test_argument_errors_come_before_the_device(lib):
    t = np.ascontiguousarray(R.scattered(50, 1))
    h = C.c_void_p()
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    assert lib.cba_cloud_index_create(50, dptr(t), dptr(None), 0.0, 0, C.byref(h)) == bad and b"cell_size" in lib.cba_last_error()
    assert lib.cba_cloud_index_create(50, dptr(t), dptr(None), -1.0, 0, C.byref(h)) == bad
    assert lib.cba_cloud_index_create(50, dptr(t), dptr(None), float("nan"), 0, C.byref(h)) == bad
    assert lib.cba_cloud_index_create(50, dptr(None), dptr(None), 0.1, 0, C.byref(h)) == bad
    assert lib.cba_cloud_index_create(50, dptr(t), dptr(None), 0.1, 0, None) == bad
    assert lib.cba_cloud_index_create(0, dptr(t), dptr(None), 0.1, 0, C.byref(h)) == bad
    assert lib.cba_cloud_index_create(50, dptr(t), dptr(None), 1e-4, 0, C.byref(h)) == bad
    message = lib.cba_last_error().decode()
    assert "2^24" in message and "fits" in message
    fit = float(message.split("cell_size of ")[1].split()[0])
    assert 0 < fit < 0.01 and np.prod(np.floor((t.max(0) - t.min(0)) / fit) + 1) <= capi.CLOUD_MAX_CELLS
    assert lib.cba_cloud_index_create(2, dptr(np.full((2, 3), np.nan)), dptr(None), 0.1, 0, C.byref(h)) == bad and b"valid" in lib.cba_last_error()
    assert not h.value
    xyz = np.zeros((1, 2, 2, 3))
    out = np.zeros_like(xyz)
    assert lib.cba_point_normals(1, 2, 2, dptr(None), dptr(None), 1.0, dptr(out)) == bad
    assert lib.cba_point_normals(1, 2, 2, dptr(xyz), dptr(None), 0.0, dptr(out)) == bad and b"max_jump" in lib.cba_last_error()
    assert lib.cba_point_normals(1, 0, 2, dptr(xyz), dptr(None), 1.0, dptr(out)) == bad
    assert lib.cba_point_normals(-1, 2, 2, dptr(xyz), dptr(None), 1.0, dptr(out)) == bad
    assert lib.cba_point_normals(0, 2, 2, dptr(None), dptr(None), 1.0, dptr(None)) == capi.CBA_OK  # no work
    assert lib.cba_cloud_nearest(None, 1, dptr(t), 0.05, i64ptr(np.zeros(1, np.int64)), dptr(None)) == bad
    o = capi.CbaIcpOptions()
    lib.cba_icp_options_default(C.byref(o))
    assert (o.metric, o.max_distance, o.max_iterations, o.step_tolerance, o.min_pairs) == (0, 0.0, 30, 1e-9, 6)
    assert lib.cba_cloud_register(None, 0, i64ptr(None), dptr(None), dptr(None), C.byref(o), None) == bad
    assert C.sizeof(capi.CbaIcpResult) == 8 * 50 + 16 and C.sizeof(capi.CbaIcpOptions) == 40
    # with everything in order the answer is the device's: a handle, or CBA_ERR_NO_DEVICE where there is none
    st = lib.cba_cloud_index_create(50, dptr(t), dptr(None), 0.1, 0, C.byref(h))
    if lib.cba_device_count() > 0:
        assert st == capi.CBA_OK and h.value
        lib.cba_cloud_index_destroy(h)
    else:
        assert st == capi.CBA_ERR_NO_DEVICE and not h.value
        assert lib.cba_point_normals(1, 2, 2, dptr(xyz), dptr(None), 1.0, dptr(out)) == capi.CBA_ERR_NO_DEVICE
