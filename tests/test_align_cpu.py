"""CPU tier of the alignment of many scans (cba_cloud_set, cba_cloud_align): the blocks and their signs against finite differences of
the energy (independent of the restatement's own algebra), the numpy restatement (tests/align_ref.py) against the host build of
cloud_math.hpp (tests/align_cpu) - pair counts equal, sums inside the bound of a different order, full solves to the project's bar -
loop closure on a ring of six scans against ground truth, the planted statuses, the stand-alone driver under the sanitizers, and what
the library checks before it asks for a device."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.capi import dptr, i32ptr, i64ptr
from tests import align_ref as A
from tests import cloud_ref as R
from tests import host_build

MD, CELL = A.MD, A.CELL
RING_SEEDS = (3, 4)
RING_ROUNDS = 12
# Ground truth on the ring of six scans (align_ref.ring_scene), measured on the restatement with max_distance 0.05, point to plane,
# twelve rounds from the chain of pairwise solves, scan 0 held at its true pose: per seed the closure error (the pose of scan 5
# relative to scan 0 against the truth's: rad, length) and the mean pose error, after the chain and after align.  The figures are the
# measured values rounded up in their fourth digit.  The host build and the device are held to these times 1.25 (DESIGN.md 7u's
# convention, for last-bit differences in sine and cosine).  Seed 3 ends at the cap (the iteration does not settle below 1e-9 there),
# seed 4 converges in eight rounds.
RING_TRUTH = {
    3: dict(chain_closure=(5.327e-3, 6.534e-3), chain_mean=(4.224e-3, 3.228e-3), closure=(2.481e-3, 1.614e-3), mean=(2.744e-3, 2.958e-3),
            status=A.NOT_CONVERGED, iterations=12),
    4: dict(chain_closure=(8.123e-3, 5.401e-3), chain_mean=(5.219e-3, 3.327e-3), closure=(4.654e-4, 1.841e-3), mean=(1.827e-3, 1.339e-3),
            status=A.OK, iterations=8),
}
FOUR_SEED, FOUR_FIXED = 11, 2


@pytest.fixture(scope="module")
def host():
    return host_build.load("align_cpu")


_solved = {}


def ring(seed):
    """the ring scene, the chain of pairwise solves (by the host build of registration: it is only the start) and the restatement's
    twelve rounds from it, computed once for both tiers"""
    key = ("ring", seed)
    if key not in _solved:
        scans, normals, truth = A.ring_scene(seed)
        pairwise = host_build.load("cloud_cpu")
        chain, _ = A.chain_poses(scans, normals, truth[0], register=lambda tgt, nrm, src: R.host_register(
            pairwise, tgt, nrm, CELL, [src], MD, metric=0, max_iterations=60, step_tolerance=1e-12)[0])
        ref = A.align(scans, normals, A.ring_edges(6), MD, max_iterations=RING_ROUNDS, step_tolerance=1e-9, init_pose7=chain, fixed=0)
        _solved[key] = (scans, normals, truth, chain, ref)
    return _solved[key]


def four(metric):
    """four scans round the ring, scan 2 held at its true (non-identity) pose, every scan started there: point to plane to the end,
    point to point (which slides along a sampled surface) for three rounds"""
    key = ("four", metric)
    if key not in _solved:
        scans, normals, truth = A.ring_scene(FOUR_SEED, n_scans=4)
        init = np.tile(truth[FOUR_FIXED], (4, 1))
        opts = dict(metric=metric, max_iterations=30 if metric == 0 else 3, step_tolerance=1e-9, init_pose7=init, fixed=FOUR_FIXED)
        ref = A.align(scans, normals, A.ring_edges(4), MD, **opts)
        _solved[key] = (scans, normals, truth, opts, ref)
    return _solved[key]


def check_edge(got, ref, m):
    """an edge's sums against the restatement's: the terms are equal to the bit where every search decision is, so only the order of
    the sums differs: 2 m 2^-53 sum |terms| (tests/test_cloud_cpu.py: check_sums)"""
    u = 2.0 ** -53
    assert got["n_pairs"] == ref["n_pairs"] and got["used"] == ref["used"]
    assert (np.abs(got["H"] - ref["H"]) <= 2 * m * u * ref["H_abs"]).all()
    assert (np.abs(got["g"] - ref["g"]) <= 2 * m * u * ref["g_abs"]).all()
    assert np.array_equal(got["H"], got["H"].T)
    assert abs(got["ss"] - ref["ss"]) <= 2 * m * u * ref["ss_abs"]


def check_solve(got, ref, scans):
    """a full solve against the restatement's: the project's bar for full solves"""
    assert (got["status"], got["iterations"], got["n_used_edges"], got["n_pairs"]) == \
        (ref["status"], ref["iterations"], ref["n_used_edges"], ref["n_pairs"])
    ext = A.set_extent(scans)
    for k in range(len(scans)):
        drot, dtr = R.pose_error(got["poses"][k], ref["poses"][k])
        assert drot <= 1e-9 and dtr <= 1e-9 * ext, k
    assert abs(got["rms"] - ref["rms"]) <= 1e-9 * ref["rms"]
    assert [e["n_pairs"] for e in got["edges"]] == [e["n_pairs"] for e in ref["edges"]]


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------
def test_driver_runs_clean_under_sanitizers():
    p = host_build.run_sanitized("align_cpu")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "align_driver: 0 mismatches" in p.stdout and not p.stderr.strip(), p.stdout + p.stderr


# ---- the blocks and their signs: finite differences of the energy -----------------------------------------------------------------------
def _energy(p, y, n, Ta, Tb, metric):
    Rab, tab = A.relative(Ta, Tb)
    J, r = A.rows(R.transform(Rab, tab, p), y, n, metric)
    return 0.5 * float((r * r).sum()), J, r


def _difference_errors(metric, h, blocks_of):
    """Frozen pairs between two scans at general poses; central differences of E = 0.5 sum r^2 under the left updates of the rule
    (cloud_ref.update) of T_a (directions 0..5) and T_b (6..11).  -> the largest error of the gradient against [c, -c] and of the
    Hessian against [[M, -M], [-M^T, M]], each relative to the largest entry.  The gradient is taken with residuals of about 0.01; the
    Hessian with targets on the transformed points, where every residual is zero and the Gauss-Newton M is the Hessian."""
    rng = np.random.default_rng(5)
    Ta = R.pose_from_rotvec([0.3, -0.2, 0.25], [0.4, -0.3, 0.2])
    Tb = R.pose_from_rotvec([-0.2, 0.35, 0.1], [-0.25, 0.5, 0.3])
    p = rng.uniform(-0.5, 0.5, (40, 3))
    n = rng.normal(size=(40, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    Rab, tab = A.relative(Ta, Tb)
    Q = R.transform(Rab, tab, p)
    off = Q + 0.01 * np.sin(np.arange(120.0).reshape(40, 3))
    eye = np.eye(12)

    def E(y, d):
        return _energy(p, y, n, R.update(Ta, d[:6])[0], R.update(Tb, d[6:])[0], metric)[0]

    _, J, r = _energy(p, off, n, Ta, Tb, metric)
    _, c = blocks_of(J.T @ J, J.T @ r, Tb)
    grad = np.array([(E(off, h * eye[k]) - E(off, -h * eye[k])) / (2 * h) for k in range(12)])
    want = np.concatenate([c, -c])
    _, J, r = _energy(p, Q, n, Ta, Tb, metric)
    assert (r == 0).all()
    M, _ = blocks_of(J.T @ J, J.T @ r, Tb)
    hess = np.array([[(E(Q, h * (eye[k] + eye[l])) - E(Q, h * (eye[k] - eye[l])) - E(Q, h * (eye[l] - eye[k])) + E(Q, -h * (eye[k] + eye[l])))
                      / (4 * h * h) for l in range(12)] for k in range(12)])
    full = np.block([[M, -M], [-M.T, M]])
    return np.abs(grad - want).max() / np.abs(want).max(), np.abs(hess - full).max() / np.abs(full).max()


# The step and the bars: central differences are off by their truncation error, which falls by four when the step is halved.
# Measured on the restatement at h = 1e-4: gradient 5.3e-7 (metric 0) and 1.7e-9 (metric 1), Hessian 2.6e-9 and 1.5e-9, relative to the
# largest entry; at 2e-4 four times these.  The bars are 2e-6 and 1e-8; a wrong sign or a transposed block is an error of order 1.
FD_STEP, FD_GRADIENT_BAR, FD_HESSIAN_BAR = 1e-4, 2e-6, 1e-8


@pytest.mark.parametrize("metric", [0, 1])
def test_blocks_agree_with_finite_differences(host, metric):
    def restated(H, g, Tb):
        return A.blocks(H, g, A.adjoint(Tb))

    def built(H, g, Tb):
        return A.host_blocks(host, H, g, Tb)[1:]

    eg, eh = _difference_errors(metric, FD_STEP, restated)
    eg2, eh2 = _difference_errors(metric, 2 * FD_STEP, restated)
    print(f"metric {metric}: gradient {eg:.3g} (at twice the step {eg2:.3g}), Hessian {eh:.3g} ({eh2:.3g})")
    assert eg <= FD_GRADIENT_BAR and eh <= FD_HESSIAN_BAR
    assert 3.0 <= eg2 / eg <= 5.0 and 3.0 <= eh2 / eh <= 5.0  # it is the truncation error that is measured
    hg, hh = _difference_errors(metric, FD_STEP, built)
    assert hg <= FD_GRADIENT_BAR and hh <= FD_HESSIAN_BAR
    # the adjoint itself, and A = I: the identity pose gives H and g back to the bit
    Tb = R.pose_from_rotvec([-0.2, 0.35, 0.1], [-0.25, 0.5, 0.3])
    Tb[:4] = R.normalise(Tb[:4])  # as the entry does
    assert np.array_equal(A.host_blocks(host, np.eye(6), np.zeros(6), Tb)[0], A.adjoint(Tb))
    rng = np.random.default_rng(6)
    J = rng.normal(size=(9, 6))
    H, g = J.T @ J, rng.normal(size=6)
    for M, c in (A.blocks(H, g, A.adjoint(A.IDENTITY)), A.host_blocks(host, H, g, A.IDENTITY)[1:]):
        assert np.array_equal(M, H) and np.array_equal(c, g)


# ---- the host build against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_edge_statistics_at_the_start(host, metric):
    scans, normals, truth, chain, _ = ring(4)
    edges = A.ring_edges(6) + [(0, 3), (2, 0), (2, 0)]  # an opposite pair and a duplicate beside the ring's twelve
    ref = A.align(scans, normals, edges, MD, metric=metric, max_iterations=0, init_pose7=chain, fixed=0)
    assert ref["gap"] >= 1e-9 * MD ** 2
    for brute in (False, True):
        got = A.host_align(host, scans, normals, CELL, edges, MD, metric=metric, max_iterations=0, init_pose7=chain, fixed=0, brute=brute)
        assert (got["status"], got["iterations"], got["n_used_edges"]) == (A.NOT_CONVERGED, 0, len(edges)) == \
            (ref["status"], ref["iterations"], ref["n_used_edges"])
        assert np.array_equal(got["poses"], A.normalised(chain)) and got["n_pairs"] == ref["n_pairs"]
        for g, r in zip(got["edges"], ref["edges"]):
            check_edge(g, r, 1200)
        assert abs(got["rms"] - ref["rms"]) <= 1e-9 * ref["rms"]
    assert np.array_equal(got["edges"][-1]["H"], got["edges"][-2]["H"])  # a duplicate counts separately and is the same system


@pytest.mark.parametrize("metric", [0, 1])
def test_full_solve_of_four_scans(host, metric):
    scans, normals, truth, opts, ref = four(metric)
    print(f"metric {metric}: gap {ref['gap'] / MD ** 2:.3g} md^2, status {ref['status']}, iterations {ref['iterations']}, rms {ref['rms']:.6g}, "
          f"mean error {A.mean_pose_error(ref['poses'], truth)}")
    assert ref["gap"] >= 1e-9 * MD ** 2
    assert (ref["status"], ref["iterations"]) == ((A.OK, 9) if metric == 0 else (A.NOT_CONVERGED, 3))
    held = A.normalised(truth[FOUR_FIXED])[0]
    assert ref["poses"][FOUR_FIXED].tobytes() == held.tobytes()  # the held pose is not touched
    got = A.host_align(host, scans, normals, CELL, A.ring_edges(4), MD, **opts)
    check_solve(got, ref, scans)
    assert got["poses"][FOUR_FIXED].tobytes() == held.tobytes()
    if metric == 0:  # as accurate as the pairwise solves are (tests/test_cloud_cpu.py: TRUTH_ERROR of the plain scene, metric 0)
        rot, tr = A.mean_pose_error(ref["poses"], truth)
        assert rot <= 3e-3 and tr <= 3e-3


@pytest.mark.parametrize("seed", RING_SEEDS)
def test_loop_closure_on_the_ring(host, seed):
    scans, normals, truth, chain, ref = ring(seed)
    want = RING_TRUTH[seed]
    print(f"seed {seed}: gap {ref['gap'] / MD ** 2:.3g} md^2, status {ref['status']}, iterations {ref['iterations']}, rms {ref['rms']:.6g}")
    assert ref["gap"] >= 1e-9 * MD ** 2
    assert (ref["status"], ref["iterations"]) == (want["status"], want["iterations"])
    got = A.host_align(host, scans, normals, CELL, A.ring_edges(6), MD, max_iterations=RING_ROUNDS, step_tolerance=1e-9, init_pose7=chain, fixed=0)
    check_solve(got, ref, scans)
    figures = {"chain_closure": A.closure_error(chain, truth), "chain_mean": A.mean_pose_error(chain, truth),
               "closure": A.closure_error(ref["poses"], truth), "mean": A.mean_pose_error(ref["poses"], truth)}
    print(f"  restatement: {figures}")
    for name, (rot, tr) in figures.items():  # the constants are the measured values
        assert 0.99 * want[name][0] <= rot <= want[name][0] and 0.99 * want[name][1] <= tr <= want[name][1], name
    for name, (rot, tr) in (("closure", A.closure_error(got["poses"], truth)), ("mean", A.mean_pose_error(got["poses"], truth))):
        assert rot <= 1.25 * want[name][0] and tr <= 1.25 * want[name][1], name
    # what the feature is for: the last scan meets the first better than after the chain
    assert A.closure_error(got["poses"], truth)[0] < A.closure_error(chain, truth)[0]
    assert A.closure_error(ref["poses"], truth)[0] < A.closure_error(chain, truth)[0]


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_planted_statuses(host):
    scans, normals, truth, opts, _ = four(0)
    init = A.normalised(opts["init_pose7"])  # normalised again it stays: what comes back can be compared to the bit

    def both(edges, **kw):
        kw = dict(dict(max_iterations=30, step_tolerance=1e-9, init_pose7=init, fixed=FOUR_FIXED), **kw)
        return A.align(scans, normals, edges, MD, **kw), A.host_align(host, scans, normals, CELL, edges, MD, **kw)

    # scan 3 is connected by no edge: the solve fails, no pose is touched
    for r in both([(0, 1), (1, 2), (2, 1), (1, 0)]):
        assert (r["status"], r["iterations"], r["n_used_edges"]) == (A.DEGENERATE, 0, 4) and np.array_equal(r["poses"], init)
    # a min_pairs that no edge reaches: every edge is reported, none is used
    ref, got = both([(0, 1), (1, 2), (3, 2)], min_pairs=100000)
    assert ref["status"] == got["status"] == A.TOO_FEW and got["n_used_edges"] == 0
    assert [e["n_pairs"] for e in got["edges"]] == [e["n_pairs"] for e in ref["edges"]] and min(e["n_pairs"] for e in got["edges"]) > 0
    # every scan far from every other: no edge is used
    far = init.copy()
    far[:, 6] += 3.0 * np.arange(4)
    for r in both(A.ring_edges(4), init_pose7=far):
        assert (r["status"], r["iterations"], r["n_used_edges"], r["n_pairs"]) == (A.TOO_FEW, 0, 0, 0) and np.isnan(r["rms"])
        assert all(e["n_pairs"] == 0 and not e["used"] for e in r["edges"])
    # max_iterations = 0: the statistics at the start
    ref, got = both(A.ring_edges(4), max_iterations=0)
    assert ref["status"] == got["status"] == A.NOT_CONVERGED and got["iterations"] == 0 and np.array_equal(got["poses"], init)
    assert got["n_pairs"] == ref["n_pairs"] > 0 and abs(got["rms"] - ref["rms"]) <= 1e-9 * ref["rms"]
    # every source a subset of its target, so each scan lies exactly on its neighbours; a generous tolerance: one round, which moves nothing
    tgt, nrm = R.surface_map(48, 36, 1), R.normals(R.surface_map(48, 36, 1))
    on = [tgt, tgt.reshape(-1, 3)[::3], tgt.reshape(-1, 3)[::6]]
    on_normals = [nrm, nrm.reshape(-1, 3)[::3], nrm.reshape(-1, 3)[::6]]
    edges = [(1, 0), (2, 0), (2, 1)]
    for r in (A.align(on, on_normals, edges, MD, step_tolerance=1e-6), A.host_align(host, on, on_normals, CELL, edges, MD, step_tolerance=1e-6)):
        assert (r["status"], r["iterations"], r["rms"]) == (A.OK, 1, 0.0)
        assert np.array_equal(r["poses"], np.tile(A.IDENTITY, (3, 1)))


def test_the_two_cycle_ends_at_the_cap(host):
    # seed 3 of the ring: the iteration does not settle; at the cap the statistics are those of the returned poses
    scans, normals, truth, chain, ref = ring(3)
    assert ref["status"] == A.NOT_CONVERGED and ref["iterations"] == RING_ROUNDS
    got = A.host_align(host, scans, normals, CELL, A.ring_edges(6), MD, max_iterations=RING_ROUNDS, step_tolerance=1e-9, init_pose7=chain, fixed=0)
    assert got["status"] == A.NOT_CONVERGED and abs(got["rms"] - ref["rms"]) <= 1e-9 * ref["rms"]
    # further on one pair flips between two neighbours for ever: the poses of round k + 2 are those of round k, not those of k + 1
    runs = [A.host_align(host, scans, normals, CELL, A.ring_edges(6), MD, max_iterations=k, step_tolerance=1e-9, init_pose7=chain, fixed=0)
            for k in (40, 41, 42)]
    assert [r["status"] for r in runs] == [A.NOT_CONVERGED] * 3
    step = max(R.pose_error(a, b)[0] for a, b in zip(runs[0]["poses"], runs[1]["poses"]))
    back = max(R.pose_error(a, b)[0] for a, b in zip(runs[0]["poses"], runs[2]["poses"]))
    print(f"two-cycle: step {step:.3g} rad, after two rounds {back:.3g} rad")
    assert step > 1e-9 and back <= 1e-3 * step


# ---- the library without a device: every argument error comes first ----------------------------------------------------------------------
def test_argument_errors_come_before_the_device(lib):
    scans = [R.scattered(50, 1), R.scattered(40, 2), R.scattered(30, 3)]
    off, xyz, _ = A.pack(scans)
    h = C.c_void_p()
    bad = capi.CBA_ERR_INVALID_ARGUMENT

    def create(n=3, offset=off, points=xyz, cell=0.1, out=C.byref(h)):
        return lib.cba_cloud_set_create(n, i64ptr(offset), dptr(points), dptr(None), cell, 0, out)

    assert create(out=None) == bad
    assert create(n=1) == bad and b"n_scans" in lib.cba_last_error()
    assert create(n=65) == bad
    assert create(offset=None) == bad and create(points=None) == bad
    assert create(offset=np.array([1, 50, 90, 120], np.int64)) == bad and b"offsets" in lib.cba_last_error()
    assert create(offset=np.array([0, 90, 50, 120], np.int64)) == bad
    for cell in (0.0, -1.0, float("nan")):
        assert create(cell=cell) == bad and b"cell_size" in lib.cba_last_error()
    assert create(offset=np.array([0, 50, 50, 120], np.int64)) == bad and b"scan 1 has no valid point" in lib.cba_last_error()
    holed = xyz.copy()
    holed[90:] = np.nan
    assert create(points=holed) == bad and b"scan 2 has no valid point" in lib.cba_last_error()
    assert create(cell=1e-4) == bad
    message = lib.cba_last_error().decode()
    assert "2^24" in message and "fits" in message and "scan 0" in message
    fit = float(message.split("cell_size of ")[1].split()[0])
    assert 0 < fit < 0.01 and np.prod(np.floor((scans[0].max(0) - scans[0].min(0)) / fit) + 1) <= capi.CLOUD_MAX_CELLS
    assert not h.value
    o = capi.CbaAlignOptions()
    lib.cba_align_options_default(C.byref(o))
    assert (o.icp.metric, o.icp.max_distance, o.icp.max_iterations, o.icp.step_tolerance, o.icp.min_pairs, o.fixed) == (0, 0.0, 30, 1e-9, 6, 0)
    assert C.sizeof(capi.CbaAlignEdge) == 8 * 45 and C.sizeof(capi.CbaAlignResult) == 32 and C.sizeof(capi.CbaAlignOptions) == 48
    poses, res = np.zeros((3, 7)), capi.CbaAlignResult()
    assert lib.cba_cloud_align(None, 0, i32ptr(None), dptr(None), C.byref(o), dptr(poses), None, C.byref(res)) == bad
    # with everything in order the answer is the device's: a handle, or CBA_ERR_NO_DEVICE where there is none
    st = create()
    if lib.cba_device_count() > 0:
        assert st == capi.CBA_OK and h.value
        lib.cba_cloud_set_destroy(h)
    else:
        assert st == capi.CBA_ERR_NO_DEVICE and not h.value
