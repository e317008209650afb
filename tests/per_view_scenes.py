"""Scenes of the per-view wave solvers' edge tests (tests/test_per_view_edges_cpu.py and tests/test_per_view_edges_gpu.py share
them: the CPU tier proves on the host build of the same headers that every view here meets the strict bars, the GPU tier then
runs the kernels on exactly these inputs).  Plain numpy, fixed seeds, nothing cached on disk.

The four kernels (k_planar_pose, k_sd_pass1/pass2/resid, k_planar_seed, k_dlt_homography) and k_homography give ONE 64-lane
wavefront a whole view and pack FOUR waves into a block, so the sizes that matter are

  point counts   n_min, n_min + 1 (a wave with 4 .. 9 live lanes), 63 / 64 / 65 (the end of the first trip of the lane-stride
                 loop), 127 / 128 / 129 (the end of the second) and 257 (a fifth trip with one live lane);
  view counts    1, 3, 4, 5, 8, 9 (a lone wave, a block short of one wave, one full block, one wave into the next, ...).

n_min: the smallest count the reference accepts and at which the problem is determined.
  planar pose    8 for every num_radial: fit_distortion_full refuses fewer than 8 observations (include/calib/models/distortion.h
                 k_min_observations, restated in oracle/residuals.hpp PlanarPoseVPBlock and in vp_math.hpp), and 8 points already
                 give 2 n = 16 > 6 + num_radial + 2 equations for num_radial <= 3 (determinacy alone would allow 5 / 5 / 6 / 6);
  homography     4 (optimize_homography and the DLT, src/estimation/optim/homography.cpp "At least 4 correspondences");
  planar seed    4 (src/estimation/linear/planarpose_linear.cpp: fewer give the identity).

Points are scattered uniformly over the board extent (a grid cannot have 127 or 257 corners), observation noise is 0.2 px.
Every view has a seed of its own, so that one badly conditioned view can be replaced without touching the others.
"""
import ctypes as C

import numpy as np

from calibration_amd import capi
from calibration_amd.capi import CbaSummary, dptr
from tests import helpers, synth
from tests.helpers import options

PLANAR_N_MIN = 8
HOM_N_MIN = 4
SEED_N_MIN = 4
VIEW_COUNTS = (1, 3, 4, 5, 8, 9)
NOISE_PX = 0.2
BOARD = np.array([0.9, 0.7])  # metres: the extent the points are scattered over


def batch_order(n_min):
    """The ladder [n_min, n_min + 1, 63, 64, 65, 127, 128, 129, 257] in batch order: the smallest and the largest view share
    block 0, [n_min, 257, 64, n_min + 1 | 65, 63, 128, 127 | 129]; the prefixes of VIEW_COUNTS end inside and at the end of a
    block, and 9 views leave ONE live wave in the last block.  Reversed, the smallest view is that lone wave."""
    a, b = n_min, n_min + 1
    return [a, 257, 64, b, 65, 63, 128, 127, 129]


def scatter(rng, n):
    return rng.uniform(-0.5, 0.5, (n, 2)) * BOARD


# ---- planar pose ------------------------------------------------------------------------------------------------------------------
PLANAR_CAM = synth.camera_gt(0)
PLANAR_K = np.ascontiguousarray(PLANAR_CAM[:5])
# size -> seed of that view (rejected seeds: module docstring of tests/test_per_view_edges_cpu.py)
PLANAR_SEEDS = {8: 1180, 9: 1009, 63: 1063, 64: 1064, 65: 1065, 127: 1127, 128: 1128, 129: 1129, 257: 1257}


def planar_view(n, seed):
    """-> (view (n, 4) [X Y u v], true pose 4x4, initial pose 4x4): the target 1.5 m in front of the full Brown-Conrady camera,
    tilted up to 25 degrees; the start 1.5 degrees and up to 2 cm off."""
    rng = np.random.default_rng(seed)
    T = synth.random_view_poses(1, rng, dist=1.5)[0]
    view = synth.render_view(PLANAR_CAM, T, scatter(rng, n), NOISE_PX, rng, cull=False)
    return np.ascontiguousarray(view), T, synth.perturb_pose(T, rng, 1.5, 0.02)


def planar_batch():
    """-> (views, inits) in batch order"""
    vs = [planar_view(n, PLANAR_SEEDS[n]) for n in batch_order(PLANAR_N_MIN)]
    return [v[0] for v in vs], [v[2] for v in vs]


def collinear_planar_view(n=40, seed=77):
    """All target points on one line of the board: rotating the target about that line moves no point, so the 2n x 6 Jacobian
    has an exact null direction whatever the observations are."""
    rng = np.random.default_rng(seed)
    T = synth.random_view_poses(1, rng, dist=1.5)[0]
    s = rng.uniform(-0.5, 0.5, n)
    pts = np.stack([s * BOARD[0], 0.4 * s * BOARD[1]], axis=1)
    view = synth.render_view(PLANAR_CAM, T, pts, NOISE_PX, rng, cull=False)
    return np.ascontiguousarray(view), T, synth.perturb_pose(T, rng, 1.5, 0.02)


def with_nan(view, row=5, col=2):
    out = np.array(view, dtype=np.float64, copy=True)
    out[row % len(out), col] = np.nan
    return out


# ---- homography refinement ----------------------------------------------------------------------------------------------------------
HOM_SEEDS = {4: 2004, 5: 2005, 63: 2063, 64: 2064, 65: 2065, 127: 2127, 128: 2128, 129: 2129, 257: 2257}


def hom_view(n, seed):
    """-> (view, initial H): helpers.homography_scene at 0.2 px noise; the start is the float64 DLT 0.1 % off, H22 = 1."""
    view, _ = helpers.homography_scene(n, NOISE_PX, seed=seed)
    H0 = helpers.dlt_homography(view) * (1 + 1e-3)
    H0[2, 2] = 1.0
    return view, H0


def hom_batch():
    vs = [hom_view(n, HOM_SEEDS[n]) for n in batch_order(HOM_N_MIN)]
    return [v[0] for v in vs], [v[1] for v in vs]


def collinear_hom_view(n=40, seed=78):
    """Source points on one line: the homography is determined on that line only."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-100, 100, n)
    xy = np.stack([s, 0.3 * s + 10.0], axis=1)
    uv = helpers.apply_homography(helpers.homography_true(), xy) + rng.normal(0, NOISE_PX, (n, 2))
    H0 = helpers.homography_true() * (1 + 1e-3)
    H0[2, 2] = 1.0
    return np.ascontiguousarray(np.c_[xy, uv]), H0


# ---- planar seed and DLT homography -------------------------------------------------------------------------------------------------
SEED_CAM = synth.camera_gt(0, distortion=False)
SEED_K = np.ascontiguousarray(SEED_CAM[:5])
SEED_SEEDS = {4: 3004, 5: 3005, 63: 3063, 64: 3064, 65: 3065, 127: 3127, 128: 3128, 129: 3129, 257: 3257}


def seed_view(n, seed):
    """-> (view, true pose): the target 1.2 m in front of a distortion-free camera, tilted up to 35 degrees."""
    rng = np.random.default_rng(seed)
    T = synth.random_view_poses(1, rng, dist=1.2, max_tilt_deg=35.0, jitter=0.15)[0]
    return np.ascontiguousarray(synth.render_view(SEED_CAM, T, scatter(rng, n), NOISE_PX, rng, cull=False)), T


def seed_batch():
    return [seed_view(n, SEED_SEEDS[n])[0] for n in batch_order(SEED_N_MIN)]


# ---- semi-DLT intrinsics --------------------------------------------------------------------------------------------------------------
SEMIDLT_SIZES = {"wave-edges": (63, 64, 65, 127, 129), "ragged-9": (12, 257, 64, 30, 65, 6, 128, 100, 129)}
SEMIDLT_SEEDS = {"wave-edges": 4001, "ragged-9": 4002}


def semidlt_problem(name, nr):
    """A ragged semi-DLT problem in the layout of helpers.semidlt_scene (helpers.semidlt_solve takes it): views of
    SEMIDLT_SIZES[name] points through a camera whose radial coefficients beyond num_radial are zero (the variable-projection
    model is then exact up to the noise), start = the reference tests' camera_init and poses 2 degrees / 1 cm off."""
    from calibration_amd.geometry import pose_from_matrix

    sizes = SEMIDLT_SIZES[name]
    rng = np.random.default_rng(SEMIDLT_SEEDS[name])
    cam = synth.camera_gt(0).copy()
    cam[5 + nr:8] = 0.0
    poses = synth.random_view_poses(len(sizes), rng, dist=1.5, max_tilt_deg=35.0, jitter=0.15)
    views = [np.ascontiguousarray(synth.render_view(cam, T, scatter(rng, n), NOISE_PX, rng, cull=False)) for T, n in zip(poses, sizes)]
    poses0 = np.ascontiguousarray(np.stack([pose_from_matrix(synth.perturb_pose(T, rng)) for T in poses]))
    return semidlt_pack(views, np.ascontiguousarray(synth.camera_init(cam)[:5]), poses0)


def semidlt_pack(views, kappa0, poses0):
    off = np.zeros(len(views) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in views], out=off[1:])
    allv = np.concatenate(views)
    return dict(off=off, X=np.ascontiguousarray(allv[:, 0]), Y=np.ascontiguousarray(allv[:, 1]), u=np.ascontiguousarray(allv[:, 2]),
                v=np.ascontiguousarray(allv[:, 3]), kappa0=np.ascontiguousarray(kappa0, dtype=np.float64).copy(),
                poses0=np.ascontiguousarray(poses0, dtype=np.float64).copy(), n_views=len(views), views=list(views))


def semidlt_permuted(d, perm):
    """The same problem with its views in the order `perm` (new view i = old view perm[i])."""
    return semidlt_pack([d["views"][k] for k in perm], d["kappa0"], d["poses0"][list(perm)])


def columns(view):
    return tuple(np.ascontiguousarray(view[:, k]) for k in range(4))


# ---- one view through an entry point with the oracle's argument list (orc_* / hm_*) --------------------------------------------------
def planar_solve(fn, view, init, nr, o):
    """-> dict(st, pose6, s (CbaSummary), dist, rms, cov (6, 6))"""
    X, Y, u, v = columns(view)
    p, s, d, rms, cov = helpers.pose6_of(init), CbaSummary(), np.zeros(nr + 2), C.c_double(), np.zeros((6, 6))
    st = fn(len(view), dptr(X), dptr(Y), dptr(u), dptr(v), dptr(PLANAR_K), nr, dptr(p), C.byref(o), C.byref(s), dptr(d), C.byref(rms), dptr(cov))
    return dict(st=st, pose6=p, s=s, dist=d, rms=rms.value, cov=cov)


def hom_solve(fn, view, H0, o):
    """-> dict(st, h (9), s, cov (8, 8))"""
    X, Y, u, v = columns(view)
    h, s, cov = np.ascontiguousarray(H0, dtype=np.float64).reshape(9).copy(), CbaSummary(), np.zeros((8, 8))
    st = fn(len(view), dptr(X), dptr(Y), dptr(u), dptr(v), dptr(h), C.byref(o), C.byref(s), dptr(cov))
    return dict(st=st, h=h, s=s, cov=cov)


# ---- the bars, shared by both tiers (module docstring of tests/test_per_view_edges_cpu.py) ----------------------------------------------
# epsilon 1e-12 everywhere: capped at 1 and 2 iterations no stopping rule is involved; converged, the bars measure arithmetic
# parity and not where each solver happened to stop
MODES = {"cap1": dict(max_iterations=1), "cap2": dict(max_iterations=2), "converged": {}}


def mode_options(mode, **kw):
    return options(epsilon=1e-12, **MODES[mode], **kw)


def assert_planar_parity(a, b, mode, tag):
    """a: the oracle's solve of one view, b: the solve under test (pv.planar_solve dictionaries)"""
    sa, sb = a["s"], b["s"]
    print(tag, "iters", sa.iterations, sb.iterations, "pose", np.abs(a["pose6"] - b["pose6"]).max(), "rms", abs(a["rms"] - b["rms"]),
          "dist", np.abs(a["dist"] - b["dist"]).max(), "cov", np.abs(a["cov"] - b["cov"]).max() / max(np.abs(a["cov"]).max(), 1e-300))
    assert a["st"] == 0 and b["st"] == 0, tag
    assert sa.termination == sb.termination and bool(sa.success) == bool(sb.success), (tag, sa.report, sb.termination)
    if mode == "converged":
        assert sa.termination == capi.TERM_CONVERGENCE and abs(sa.iterations - sb.iterations) <= 1, (tag, sa.iterations, sb.iterations)
    else:
        assert sa.iterations == sb.iterations == MODES[mode]["max_iterations"] and sa.successful_steps == sb.successful_steps, tag
    assert np.abs(a["pose6"] - b["pose6"]).max() <= 1e-9, tag
    assert abs(a["rms"] - b["rms"]) <= 1e-9 * max(1.0, a["rms"]), tag
    assert np.abs(a["dist"] - b["dist"]).max() <= 1e-8, tag
    assert np.any(a["cov"]) and np.abs(a["cov"] - b["cov"]).max() <= 1e-6 * np.abs(a["cov"]).max(), tag


def assert_hom_parity(a, b, mode, tag):
    sa, sb = a["s"], b["s"]
    print(tag, "iters", sa.iterations, sb.iterations, "h", np.abs(a["h"] - b["h"]).max(), "cost", abs(sa.final_cost - sb.final_cost))
    assert a["st"] == 0 and b["st"] == 0, tag
    assert sa.termination == sb.termination and bool(sa.success) == bool(sb.success), (tag, sa.report, sb.termination)
    if mode == "converged":
        assert sa.termination == capi.TERM_CONVERGENCE and abs(sa.iterations - sb.iterations) <= 1, (tag, sa.iterations, sb.iterations)
    else:
        assert sa.iterations == sb.iterations == MODES[mode]["max_iterations"] and sa.successful_steps == sb.successful_steps, tag
    assert np.abs(a["h"] - b["h"]).max() <= 1e-9 * max(1.0, np.abs(a["h"]).max()), tag
    assert abs(sa.final_cost - sb.final_cost) <= 1e-9 * max(1.0, sa.final_cost), tag
    if sa.final_cost > 1e-12:  # (an exact fit - 4 correspondences - has ssr = rounding, and so has its ssr-scaled covariance)
        assert np.any(a["cov"]) and np.abs(a["cov"] - b["cov"]).max() <= 1e-6 * np.abs(a["cov"]).max(), tag
    else:
        assert np.any(a["cov"]) == np.any(b["cov"]), tag


def assert_semidlt_parity(ra, rb, mode, tag):
    """ra, rb: helpers.semidlt_solve tuples of the oracle and of the solve under test"""
    (sta, ka, pa, sa, da, va, ca), (stb, kb, pb, sb, db, vb, cb) = ra, rb
    print(tag, "iters", sa.iterations, sb.iterations, "K", np.abs(ka - kb).max() / np.abs(ka).max(), "poses", np.abs(pa - pb).max(),
          "dist", np.abs(da - db).max(), "view errors", np.abs(va - vb).max(), "cost", abs(sa.final_cost - sb.final_cost))
    assert sta == 0 and stb == 0, tag
    if mode == "converged":
        assert sa.termination == sb.termination == capi.TERM_CONVERGENCE and abs(sa.iterations - sb.iterations) <= 2, (tag, sa.report, sb.report)
    else:
        assert sa.termination == sb.termination == capi.TERM_NO_CONVERGENCE, (tag, sa.report, sb.report)
        assert sa.iterations == sb.iterations == MODES[mode]["max_iterations"] and sa.successful_steps == sb.successful_steps, tag
    assert abs(sa.final_cost - sb.final_cost) <= 1e-9 * max(1.0, sa.final_cost), tag
    assert np.abs(ka - kb).max() <= 1e-9 * np.abs(ka).max(), tag
    assert np.abs(pa - pb).max(axis=1).max() <= 1e-9, (tag, np.abs(pa - pb).max(axis=1))  # every view's pose
    assert np.abs(da - db).max() <= 1e-9 * max(1.0, np.abs(da).max()), tag
    assert np.abs(va - vb).max() <= 1e-9, (tag, np.abs(va - vb))  # per view: a table row in another view's place shows here first
    if mode == "converged":
        dg = np.sqrt(np.abs(np.diag(ca)))
        nz = dg > 0
        assert np.any(nz) and (np.abs(ca - cb)[np.ix_(nz, nz)] / np.outer(dg[nz], dg[nz])).max() <= 1e-5, tag
