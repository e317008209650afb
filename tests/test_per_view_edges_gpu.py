"""GPU tier of the per-view wave solvers' edge tests: k_planar_pose, k_homography, k_sd_pass1 / k_sd_pass2 / k_sd_resid with
k_sd_alpha, k_planar_seed and k_dlt_homography through the C ABI and the Python facade, on the scenes of tests/per_view_scenes.py.

Each of these kernels gives one wavefront a whole view (lanes stride over the view's points, sums cross the wave in DPP) and packs
four waves into a block.  The scenes put the point counts at the ends of the lane-stride loop's trips (n_min, n_min + 1, 63 / 64 / 65,
127 / 128 / 129, 257) and the view counts at the ends of the blocks (1, 3, 4, 5, 8, 9 and the batch reversed), the smallest and the
largest view in one block.  Checked: every view against the oracle at the project's strict bars, capped at 1 and 2 iterations and
converged; a view alone equal to the same view inside a batch BIT FOR BIT, whatever shares its block and wherever it stands; a
degenerate or non-finite view ends as the oracle ends it and leaves its neighbours' bits alone.

There is no looser bar for any view here: tests/test_per_view_edges_cpu.py shows on the host build of the same headers that
every view of these scenes meets the strict one (bars and their sources: its module docstring).
"""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi, optim
from calibration_amd.capi import CbaSummary, dptr, i32ptr, i64ptr
from calibration_amd.geometry import pose_from_matrix, pose_to_matrix, poses_from_matrices
from tests import helpers
from tests import per_view_scenes as pv
from tests.helpers import options
from tests.per_view_scenes import assert_hom_parity, assert_planar_parity, assert_semidlt_parity, mode_options

pytestmark = pytest.mark.gpu

SUMMARY_FIELDS = ("termination", "success", "iterations", "successful_steps", "initial_cost", "final_cost")


def _flatten(views):
    off = np.zeros(len(views) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in views], out=off[1:])
    allv = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 4) for v in views])
    return (off,) + tuple(np.ascontiguousarray(allv[:, k]) for k in range(4))


def _summaries(summ, nv):
    return {f: np.array([getattr(summ[i], f) for i in range(nv)]) for f in SUMMARY_FIELDS}


def gpu_planar(lib, views, inits, nr, o):
    """cba_optimize_planar_pose_batch, raw outputs: every array has one row per view"""
    nv = len(views)
    off, X, Y, u, v = _flatten(views)
    pose7 = np.ascontiguousarray(poses_from_matrices(np.asarray(inits, dtype=np.float64)))
    summ = (CbaSummary * nv)()
    dist, rms, cov = np.zeros((nv, nr + 2)), np.zeros(nv), np.zeros((nv, 36))
    capi.check(lib, lib.cba_optimize_planar_pose_batch(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v), dptr(pv.PLANAR_K), nr, dptr(pose7),
                                                       C.byref(o), summ, dptr(dist), dptr(rms), dptr(cov)))
    return dict(pose7=pose7, dist=dist, rms=rms, cov=cov, summ=summ, **_summaries(summ, nv))


def gpu_hom(lib, views, inits, o):
    nv = len(views)
    off, X, Y, u, v = _flatten(views)
    h = np.ascontiguousarray(np.stack([np.asarray(H, dtype=np.float64).reshape(9) for H in inits]))
    summ = (CbaSummary * nv)()
    cov = np.zeros((nv, 64))
    capi.check(lib, lib.cba_optimize_homography_batch(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v), dptr(h), C.byref(o), summ, dptr(cov)))
    return dict(h=h, cov=cov, summ=summ, **_summaries(summ, nv))


def gpu_seed(lib, views):
    nv = len(views)
    off, X, Y, u, v = _flatten(views)
    pose7 = np.zeros((nv, 7))
    capi.check(lib, lib.cba_estimate_planar_pose_batch(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v), dptr(pv.SEED_K), dptr(pose7)))
    return dict(pose7=pose7)


def gpu_dlt(lib, views):
    nv = len(views)
    off, X, Y, u, v = _flatten(views)
    H, ok = np.zeros((nv, 9)), np.zeros(nv, dtype=np.int32)
    capi.check(lib, lib.cba_estimate_homography_batch(nv, i64ptr(off), dptr(X), dptr(Y), dptr(u), dptr(v), dptr(H), i32ptr(ok)))
    return dict(H=H, ok=ok)


def rows_equal(a, i, b, j):
    """every output of view i of run a equals that of view j of run b, bit for bit -> the names that differ"""
    return [k for k in a if k != "summ" and not np.array_equal(a[k][i], b[k][j])]


def planar_row(r, i):
    """view i of a gpu_planar run in the layout of pv.planar_solve"""
    return dict(st=0, pose6=helpers.pose6_of(pose_to_matrix(r["pose7"][i])), s=r["summ"][i], dist=r["dist"][i], rms=float(r["rms"][i]),
                cov=r["cov"][i].reshape(6, 6))


def hom_row(r, i):
    return dict(st=0, h=r["h"][i], s=r["summ"][i], cov=r["cov"][i].reshape(8, 8))


def batches(items):
    """The prefixes of the batch and the batch reversed -> [(tag, indices into items)]"""
    n = len(items)
    return [(f"first {c}", list(range(c))) for c in pv.VIEW_COUNTS if c <= n] + [("reversed", list(range(n))[::-1])]


# ---- 1. planar pose, ragged, all four num_radial ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(pv.MODES))
@pytest.mark.parametrize("nr", [0, 1, 2, 3])
def test_planar_pose_ragged_batches_match_oracle(gpu_lib, oracle, nr, mode):
    """Every view of every batch against orc_planar_pose_solve: 8 .. 257 points, so up to five trips of the lane-stride loop in
    each of the three passes of an evaluation; all four template instances of the kernel."""
    o = mode_options(mode)
    views, inits = pv.planar_batch()
    ref = [pv.planar_solve(oracle.orc_planar_pose_solve, vw, T0, nr, o) for vw, T0 in zip(views, inits)]
    for tag, idx in batches(views):
        r = gpu_planar(gpu_lib, [views[k] for k in idx], [inits[k] for k in idx], nr, o)
        for row, k in enumerate(idx):
            assert_planar_parity(ref[k], planar_row(r, row), mode, ("planar", nr, mode, tag, len(views[k])))


# ---- 2. semi-DLT, ragged ------------------------------------------------------------------------------------------------------------------
def _gpu_semidlt(gpu_lib):
    gpu_lib.cba_optimize_intrinsics_semidlt.argtypes = helpers.SEMIDLT_SOLVE_ARGS
    return gpu_lib.cba_optimize_intrinsics_semidlt


@pytest.mark.parametrize("mode", list(pv.MODES))
@pytest.mark.parametrize("nr", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(pv.SEMIDLT_SIZES))
def test_semidlt_ragged_problems_match_oracle(gpu_lib, oracle, name, nr, mode):
    """Views of different lengths: the off[i] addressing of every wave, the out1 / out2 row of every view (view_errors and the
    poses are compared PER VIEW) and, with 9 views, a last block of one live wave."""
    d = pv.semidlt_problem(name, nr)
    o = mode_options(mode)
    want_cov = mode == "converged"
    ra = helpers.semidlt_solve(oracle.orc_semidlt_solve, d, nr, o, want_cov=want_cov)
    rb = helpers.semidlt_solve(_gpu_semidlt(gpu_lib), d, nr, o, want_cov=want_cov)
    assert_semidlt_parity(ra, rb, mode, ("semidlt", name, nr, mode))


@pytest.mark.parametrize("name", list(pv.SEMIDLT_SIZES))
def test_semidlt_permuted_views(gpu_lib, name):
    """Reversing the views reverses view_errors and the poses.  K and alpha agree to 1e-9 and not to the bit: the pass-1 sum over
    the views runs in view order."""
    nr = 2
    d = pv.semidlt_problem(name, nr)
    perm = list(range(d["n_views"]))[::-1]
    o = mode_options("converged")
    st0, k0, p0, s0, d0, v0, _ = helpers.semidlt_solve(_gpu_semidlt(gpu_lib), d, nr, o, want_cov=False)
    st1, k1, p1, s1, d1, v1, _ = helpers.semidlt_solve(_gpu_semidlt(gpu_lib), pv.semidlt_permuted(d, perm), nr, o, want_cov=False)
    assert st0 == 0 and st1 == 0 and s0.termination == s1.termination == capi.TERM_CONVERGENCE
    print("permuted", name, np.abs(k0 - k1).max() / np.abs(k0).max(), np.abs(d0 - d1).max(), np.abs(p0[perm] - p1).max(), np.abs(v0[perm] - v1).max())
    assert np.abs(k0 - k1).max() <= 1e-9 * np.abs(k0).max() and np.abs(d0 - d1).max() <= 1e-9
    assert np.abs(p0[perm] - p1).max() <= 1e-9 and np.abs(v0[perm] - v1).max() <= 1e-9


def test_semidlt_one_rank_sharded_equals_plain_on_the_ragged_problem(gpu_lib):
    """The sharded evaluator (split pass-1 sum, row gather of the per-view table) with one rank, over RCCL and over the host
    callback, on views of different lengths: equal to the plain entry point to the last bit
    (test_semidlt_rccl_transport_one_rank_equals_the_plain_entry_point asserts the same on views of one size)."""
    nr = 3
    d = pv.semidlt_problem("wave-edges", nr)
    V = d["n_views"]
    seeds = [pose_to_matrix(p) for p in d["poses0"]]
    opt = optim.IntrinsicsOptimOptions(core=optim.OptimOptions(epsilon=1e-12, compute_covariance=True), num_radial=nr)
    ref = optim.optimize_intrinsics_semidlt(d["views"], d["kappa0"], seeds, opt)
    assert ref.core.success
    runs = [optim.optimize_intrinsics_semidlt_sharded(d["views"], 0, V, d["kappa0"], seeds, 1, 0, rccl_id=optim.rccl_unique_id(), opts=opt, device=0),
            optim.optimize_intrinsics_semidlt_sharded(d["views"], 0, V, d["kappa0"], seeds, 1, 0, allreduce=lambda arr: None, opts=opt, device=0)]
    for res in runs:
        assert res.core.success == ref.core.success and res.core.iterations == ref.core.iterations and res.core.final_cost == ref.core.final_cost
        assert np.array_equal(res.camera, ref.camera) and np.array_equal(res.distortion, ref.distortion)
        assert np.array_equal(np.stack([pose_from_matrix(T) for T in res.c_se3_t]), np.stack([pose_from_matrix(T) for T in ref.c_se3_t]))
        assert np.array_equal(res.core.covariance, ref.core.covariance) and res.view_errors == ref.view_errors


# ---- 3. planar seed and DLT homography over the ladder --------------------------------------------------------------------------------------
def test_planar_seed_and_dlt_homography_over_the_ladder(gpu_lib):
    from tests.planar_seed import estimate_planar_pose, homography_dlt

    views = pv.seed_batch()
    ref_T = [estimate_planar_pose(vw, pv.SEED_K) for vw in views]
    ref_H = [homography_dlt(vw[:, :2], vw[:, 2:]) for vw in views]
    for tag, idx in batches(views):
        sub = [views[k] for k in idx]
        s, h = gpu_seed(gpu_lib, sub), gpu_dlt(gpu_lib, sub)
        for row, k in enumerate(idx):
            n = len(views[k])
            gap = np.abs(pose_to_matrix(s["pose7"][row]) - ref_T[k]).max()
            hgap = np.abs(h["H"][row].reshape(3, 3) - ref_H[k]).max() / np.abs(ref_H[k]).max()
            print("seed", tag, n, gap, "dlt", hgap)
            assert gap <= (1e-9 if n > 4 else 1e-7), (tag, n)
            assert h["ok"][row] == 1 and hgap <= 1e-8, (tag, n)
    # a view of fewer than 4 points inside a block: identity / ok = 0, its three neighbours unchanged
    keep = [0, 1, 3]  # 4, 257 and 5 points
    short = views[2][:3]
    with_short = [views[0], views[1], short, views[3]]
    s0, h0 = gpu_seed(gpu_lib, [views[k] for k in keep]), gpu_dlt(gpu_lib, [views[k] for k in keep])
    s1, h1 = gpu_seed(gpu_lib, with_short), gpu_dlt(gpu_lib, with_short)
    assert np.array_equal(s1["pose7"][2], [1, 0, 0, 0, 0, 0, 0])
    assert h1["ok"][2] == 0 and np.array_equal(h1["H"][2].reshape(3, 3), np.eye(3))
    for row0, row1 in zip(range(3), (0, 1, 3)):
        assert rows_equal(s0, row0, s1, row1) == [] and rows_equal(h0, row0, h1, row1) == [], (row0, row1)


# ---- 4. bitwise batch invariance ------------------------------------------------------------------------------------------------------------
def assert_batch_invariant(run, n, what):
    """run(indices) -> raw outputs of the batch of those views.  A view alone, in the whole batch and in the reversed batch: the
    same bits in every output; the same batch twice: the same bits."""
    full, again, rev = run(list(range(n))), run(list(range(n))), run(list(range(n))[::-1])
    for k in range(n):
        alone = run([k])
        assert rows_equal(alone, 0, full, k) == [], (what, "alone vs batch", k, rows_equal(alone, 0, full, k))
        assert rows_equal(alone, 0, rev, n - 1 - k) == [], (what, "alone vs reversed batch", k, rows_equal(alone, 0, rev, n - 1 - k))
        assert rows_equal(full, k, again, k) == [], (what, "two calls", k)


@pytest.mark.parametrize("nr", [0, 1, 2, 3])
def test_planar_pose_view_does_not_depend_on_its_batch(gpu_lib, nr):
    views, inits = pv.planar_batch()
    o = mode_options("converged")
    assert_batch_invariant(lambda idx: gpu_planar(gpu_lib, [views[k] for k in idx], [inits[k] for k in idx], nr, o), len(views), ("planar", nr))


def test_homography_view_does_not_depend_on_its_batch(gpu_lib, oracle):
    views, inits = pv.hom_batch()
    o = mode_options("converged")
    assert_batch_invariant(lambda idx: gpu_hom(gpu_lib, [views[k] for k in idx], [inits[k] for k in idx], o), len(views), "homography")
    # (the same scenes against the oracle: the CPU tier's homography scenes, so that the isolation test's healthy views are known good)
    r = gpu_hom(gpu_lib, views, inits, o)
    for k, (vw, H0) in enumerate(zip(views, inits)):
        assert_hom_parity(pv.hom_solve(oracle.orc_homography_solve, vw, H0, o), hom_row(r, k), "converged", ("homography", len(vw)))


def test_planar_seed_and_dlt_view_does_not_depend_on_its_batch(gpu_lib):
    views = pv.seed_batch()
    assert_batch_invariant(lambda idx: gpu_seed(gpu_lib, [views[k] for k in idx]), len(views), "planar seed")
    assert_batch_invariant(lambda idx: gpu_dlt(gpu_lib, [views[k] for k in idx]), len(views), "dlt homography")


# ---- 5. isolation: one bad view inside a block of healthy ones --------------------------------------------------------------------------------
def assert_bad_view_is_isolated(run, ref_bad, healthy_n, what):
    """run(with_bad) -> raw outputs of [h0, BAD, h1, h2, h3] (with_bad) or [h0, h1, h2, h3]: the call returns, the bad view ends as
    the oracle ends it with a zeroed covariance, the healthy views keep their bits."""
    clean, dirty = run(False), run(True)
    bad = 1
    print(what, "bad view: termination", dirty["termination"][bad], "iterations", dirty["iterations"][bad], "oracle", ref_bad["s"].termination,
          ref_bad["s"].iterations)
    assert ref_bad["st"] == 0
    assert dirty["termination"][bad] == ref_bad["s"].termination and bool(dirty["success"][bad]) == bool(ref_bad["s"].success), what
    assert not np.any(ref_bad["cov"]) and not np.any(dirty["cov"][bad]), what
    for k in range(healthy_n):
        row = k if k < bad else k + 1
        assert dirty["success"][row] == 1 or dirty["termination"][row] == capi.TERM_NO_CONVERGENCE, (what, k)
        assert rows_equal(clean, k, dirty, row) == [], (what, "healthy view", k, rows_equal(clean, k, dirty, row))


@pytest.mark.parametrize("kind", ["collinear", "nan"])
@pytest.mark.parametrize("nr", [0, 2])
def test_bad_planar_view_leaves_its_block_alone(gpu_lib, oracle, nr, kind):
    o = options(epsilon=1e-12, max_iterations=10)  # every wave leaves within 10 iterations
    views, inits = pv.planar_batch()
    views, inits = views[:4], inits[:4]  # 8, 257, 64 and 9 points: with the bad view, one full block and one wave of the next
    if kind == "collinear":
        bad, _T, bad0 = pv.collinear_planar_view()
    else:
        bad, bad0 = pv.with_nan(views[2]), inits[2]

    def run(with_bad):
        vs, ts = list(views), list(inits)
        if with_bad:
            vs.insert(1, bad)
            ts.insert(1, bad0)
        return gpu_planar(gpu_lib, vs, ts, nr, o)

    assert_bad_view_is_isolated(run, pv.planar_solve(oracle.orc_planar_pose_solve, bad, bad0, nr, o), 4, ("planar", nr, kind))


@pytest.mark.parametrize("kind", ["collinear", "nan"])
def test_bad_homography_view_leaves_its_block_alone(gpu_lib, oracle, kind):
    o = options(epsilon=1e-12, max_iterations=10)
    views, inits = pv.hom_batch()
    views, inits = views[:4], inits[:4]
    if kind == "collinear":
        bad, bad0 = pv.collinear_hom_view()
    else:
        bad, bad0 = pv.with_nan(views[2]), inits[2]

    def run(with_bad):
        vs, hs = list(views), list(inits)
        if with_bad:
            vs.insert(1, bad)
            hs.insert(1, bad0)
        return gpu_hom(gpu_lib, vs, hs, o)

    assert_bad_view_is_isolated(run, pv.hom_solve(oracle.orc_homography_solve, bad, bad0, o), 4, ("homography", kind))
