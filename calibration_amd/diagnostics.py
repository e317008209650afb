"""Reprojection diagnostics: per-block / per-view / per-camera RMS, the planar intrinsics report and outlier rejection.

Everything numerical comes from one residual-only GPU pass (``cba_reproj_residual_stats`` /
``cba_reproj_residuals_fetch_blocks``); this module only aggregates the per-block rows and keeps the books of the
cull-and-re-solve loop.  Residuals are raw: r = projection - observation, no loss and no weights.

* ``ResidualStats``                  per-block rows {sum e2, max |r| (px), #not kept, #obs} and their aggregates
* ``view_errors``                    the reference's per-view RMS (intrinsicssemidlt.cpp:137-151) of a solved intrinsics result;
  ``extrinsic_view_errors`` / ``bundle_view_errors`` the same per (view, camera) block of the other two chains
* ``compute_global_rms``             reports/intrinsics.cpp:12-31
* ``build_planar_intrinsics_report`` the reference's report dict (include/calib/pipeline/reports/intrinsics.h)
* ``refine_with_outlier_rejection``  solve, cull observations over a threshold, re-solve from the solved parameters
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import capi
from .optim import (FlatProblem, ReprojHandle, flatten_bundle, flatten_extrinsics, flatten_intrinsics)


def compute_global_rms(view_rms: Sequence[float], corner_counts: Sequence[int]) -> float:
    """compute_global_rms (reports/intrinsics.cpp:12-31): sqrt(sum rms_i^2 * 2 n_i / sum 2 n_i); views past the end of
    ``corner_counts`` count with 0 points; 0 when there is nothing to average."""
    if len(view_rms) == 0:
        return 0.0
    sum_sq, total = 0.0, 0
    for i, rms in enumerate(view_rms):
        m = 2 * (int(corner_counts[i]) if i < len(corner_counts) else 0)
        sum_sq += float(rms) * float(rms) * m
        total += m
    return float(np.sqrt(sum_sq / total)) if total else 0.0


def _rms(s: np.ndarray, n: np.ndarray) -> np.ndarray:
    s, n = np.asarray(s, float), np.asarray(n, float)
    out = np.zeros(s.shape)
    nz = n > 0
    out[nz] = np.sqrt(s[nz] / (2.0 * n[nz]))
    return out


@dataclass
class ResidualStats:
    """Per-block rows ``blk`` [n_blocks][4] = {sum e2, max sqrt(e2) (px), #not kept, #observations} and ``total`` [4], with
    e2 = r_u^2 + r_v^2.  ``blk_view`` (None for the bundle chain: there every block is its own view) and ``blk_cam`` map the
    blocks to views and cameras."""
    blk: np.ndarray
    total: np.ndarray
    blk_cam: np.ndarray
    blk_view: Optional[np.ndarray] = None
    n_views: int = 0
    n_cams: int = 0
    threshold_px: float = float("inf")

    @classmethod
    def from_flat(cls, flat: FlatProblem, blk, total, threshold_px=float("inf")) -> "ResidualStats":
        bv = None if flat.chain == capi.CHAIN_BUNDLE or flat.blk_view is None else np.asarray(flat.blk_view, np.int64)
        nv = flat.n_views if bv is not None else flat.n_blocks
        return cls(np.asarray(blk, float).reshape(-1, 4), np.asarray(total, float).reshape(4), np.asarray(flat.blk_cam, np.int64), bv,
                   int(nv), int(flat.n_cams), float(threshold_px))

    # ---- per block --------------------------------------------------------------------------------
    @property
    def block_sum_sq(self) -> np.ndarray:
        return self.blk[:, 0]

    @property
    def block_max_px(self) -> np.ndarray:
        return self.blk[:, 1]

    @property
    def block_over(self) -> np.ndarray:
        return self.blk[:, 2].astype(np.int64)

    @property
    def block_count(self) -> np.ndarray:
        return self.blk[:, 3].astype(np.int64)

    @property
    def block_rms(self) -> np.ndarray:
        """sqrt(s / (2 n)) per block (0 for an empty block)."""
        return _rms(self.blk[:, 0], self.blk[:, 3])

    # ---- aggregates -------------------------------------------------------------------------------
    def _view_key(self) -> np.ndarray:
        return self.blk_view if self.blk_view is not None else np.arange(self.blk.shape[0])

    @property
    def view_count(self) -> np.ndarray:
        return np.bincount(self._view_key(), weights=self.blk[:, 3], minlength=self.n_views).astype(np.int64)

    @property
    def view_rms(self) -> np.ndarray:
        """sqrt(sum s / sum 2 n) over each view's blocks (the bundle chain: per block)."""
        k = self._view_key()
        return _rms(np.bincount(k, weights=self.blk[:, 0], minlength=self.n_views), np.bincount(k, weights=self.blk[:, 3], minlength=self.n_views))

    @property
    def camera_rms(self) -> np.ndarray:
        k = self.blk_cam
        return _rms(np.bincount(k, weights=self.blk[:, 0], minlength=self.n_cams), np.bincount(k, weights=self.blk[:, 3], minlength=self.n_cams))

    @property
    def global_rms(self) -> float:
        """compute_global_rms of the per-view RMS and point counts (equal to sqrt(total s / total 2 n) up to rounding)."""
        return compute_global_rms(list(self.view_rms), list(self.view_count))

    @property
    def total_rms(self) -> float:
        return float(_rms(self.total[0:1], self.total[3:4])[0])

    @property
    def max_px(self) -> float:
        return float(self.total[1])

    @property
    def n_over(self) -> int:
        return int(self.total[2])

    @property
    def n_obs(self) -> int:
        return int(self.total[3])


def _stats_of(flat: FlatProblem, device: int = 0, threshold_px: float = float("inf")) -> ResidualStats:
    with ReprojHandle(flat, device) as h:
        return h.residual_stats(threshold_px)


def view_errors(views, camera, c_se3_t, device: int = 0) -> List[float]:
    """Per-view RMS (px) of an intrinsics result, the reference's definition (intrinsicssemidlt.cpp:137-151:
    sqrt(sum over the view's 2 n residual components of r^2 / (2 n))), from the GPU pass.  ``optimize_intrinsics`` leaves
    ``view_errors`` empty, as the reference does: ``view_errors(views, res.camera, res.c_se3_t)`` fills it."""
    return [float(x) for x in _stats_of(flatten_intrinsics(views, camera, c_se3_t), device).view_rms]


def extrinsic_view_errors(views, cameras, c_se3_r, r_se3_t, device: int = 0) -> np.ndarray:
    """RMS (px) of every (view, camera) block of an extrinsic rig result: [n_views][n_cams], NaN where the camera has no
    observations of the view."""
    flat = flatten_extrinsics(views, cameras, c_se3_r, r_se3_t)
    st = _stats_of(flat, device)
    out = np.full((len(views), len(cameras)), np.nan)
    out[flat.blk_view, flat.blk_cam] = st.block_rms
    return out


def bundle_view_errors(observations, cameras, g_se3_c, b_se3_t, device: int = 0) -> List[float]:
    """RMS (px) of every BundleObservation (one (pose, camera) block each) of a hand-eye bundle result."""
    return [float(x) for x in _stats_of(flatten_bundle(observations, cameras, g_se3_c, b_se3_t), device).block_rms]


def _kmtx(k) -> dict:
    k = np.asarray(k, float).reshape(-1)
    return {"fx": float(k[0]), "fy": float(k[1]), "cx": float(k[2]), "cy": float(k[3]), "skew": float(k[4])}


def build_planar_intrinsics_report(calib, views, source_names: Optional[Sequence[str]] = None, camera_id: str = "cam0",
                                   model: str = "pinhole_brown_conrady", image_size=None, algorithm: str = "planar",
                                   options: Optional[dict] = None, detector: Optional[dict] = None, device: int = 0) -> dict:
    """build_planar_intrinsics_report (src/pipeline/reports/intrinsics.cpp:33-88) for a ``linear.PlanarIntrinsicsCalibration``
    and the views it was computed from, as a dict with the reference's field names (include/calib/pipeline/reports/intrinsics.h).

    The per-view ``rms_px`` and ``reprojection_rms_px`` come from the GPU diagnostics pass at the refined camera and poses.  The
    reference fills them from ``refine_result.view_errors``, which its optimize_intrinsics never sets, so its report carries
    zeros there.  Without refined poses (refine=False) the values stay 0, as in the reference."""
    res = calib.refine_result
    n = len(views)
    counts = [int(np.asarray(v).reshape(-1, 4).shape[0]) for v in views]
    if len(res.c_se3_t) == n and n > 0:
        rms = view_errors(views, res.camera, res.c_se3_t, device)
    else:
        rms = [0.0] * n
    names = list(source_names) if source_names is not None else [f"view_{i}" for i in range(n)]
    linear_idx = [int(i) for i in calib.linear_view_indices]
    cam = np.asarray(res.camera, float).reshape(-1)
    per_view = [{"source_image": names[i], "corner_count": counts[i], "rms_px": float(rms[i]), "used_in_linear_stage": i in linear_idx}
                for i in range(n)]
    warnings = {"invalid_camera_matrix": 0, "homography_decomposition_failures": 0}
    camera = {
        "camera_id": camera_id,
        "model": model,
        "image_size": None if image_size is None else [int(image_size[0]), int(image_size[1])],
        "initial_guess": {"intrinsics": _kmtx(calib.linear_kmtx), "used_view_indices": linear_idx, "warning_counts": warnings},
        "result": {
            "intrinsics": _kmtx(cam[:5]),
            "distortion_model": model,
            "distortion_coefficients": [float(x) for x in cam[5:]],
            "reprojection_rms_px": compute_global_rms(rms, counts),
            "per_view": per_view,
        },
    }
    return {"type": "intrinsics", "algorithm": algorithm, "options": dict(options or {}), "detector": dict(detector or {}),
            "cameras": [camera]}


# ---- outlier rejection ---------------------------------------------------------------------------------------------------
@dataclass
class RobustOptions:
    """threshold_px: fixed cull threshold (px); None = k_sigma x the round's global RMS.  A residual block left with fewer than
    min_block_points observations is removed; at most max_rounds solves."""
    threshold_px: Optional[float] = None
    k_sigma: float = 3.0
    min_block_points: int = 4
    max_rounds: int = 5


@dataclass
class RobustResult:
    """flat: the final problem (kept observations, solved parameters); summary: its solve.  keep: one bool mask per ORIGINAL
    residual block over its original observations (False for culled observations and removed blocks).  block_map: the original
    block of every final block.  removed_blocks / removed_views: original indices (views: the bundle chain has none).
    rounds: (threshold_px, dropped, global_rms) of every solve, dropped = observations newly over the threshold after it.
    converged: the last round dropped nothing (False when max_rounds ended the loop)."""
    flat: FlatProblem
    summary: object
    keep: List[np.ndarray]
    block_map: np.ndarray
    removed_blocks: List[int] = field(default_factory=list)
    removed_views: List[int] = field(default_factory=list)
    rounds: List[Tuple[float, int, float]] = field(default_factory=list)
    converged: bool = False


def _gpu_round(flat: FlatProblem, opts, robust: RobustOptions, device: int):
    """One solve and the flags of its observations: (summary, threshold, global RMS, keep [n_obs] bool)."""
    with ReprojHandle(flat, device) as h:
        s = h.solve(opts)
        st = h.residual_stats()
        rms = st.global_rms
        thr = float(robust.threshold_px) if robust.threshold_px is not None else float(robust.k_sigma) * rms
        _, keep = h.residuals_fetch_blocks(0, flat.n_blocks, thr)
    return s, thr, rms, keep


def subset_problem(flat: FlatProblem, keep_blocks: Sequence[np.ndarray], blocks: Optional[Sequence[int]] = None) -> FlatProblem:
    """The problem of the kept observations (keep_blocks[b]: mask over block b's observations) of the listed blocks (default: all),
    at flat's current parameters.  Views without a block left are dropped and the remaining ones renumbered in order."""
    blocks = list(range(flat.n_blocks)) if blocks is None else [int(b) for b in blocks]
    views = []
    for b in blocks:
        lo, hi = int(flat.blk_offset[b]), int(flat.blk_offset[b + 1])
        k = np.asarray(keep_blocks[b], bool)
        views.append(np.stack([flat.X[lo:hi][k], flat.Y[lo:hi][k], flat.u[lo:hi][k], flat.v[lo:hi][k]], axis=1))
    bcam = flat.blk_cam[blocks]
    bview, vpose = None, None
    if flat.blk_view is not None and flat.chain != capi.CHAIN_BUNDLE:
        used = sorted(set(int(v) for v in flat.blk_view[blocks]))
        remap = {v: i for i, v in enumerate(used)}
        bview = np.array([remap[int(v)] for v in flat.blk_view[blocks]], dtype=np.int32)
        vpose = flat.view_pose.reshape(-1, 7)[used] if len(used) else np.zeros((0, 7))
    btg = None if flat.blk_b_T_g is None else flat.blk_b_T_g.reshape(-1, 12)[blocks]
    return FlatProblem(flat.chain, flat.model, views, bcam, bview, flat.intr, flat.cam_pose, vpose, flat.target_pose, btg,
                       first_view_global=flat.first_view_global)


def refine_with_outlier_rejection(flat: FlatProblem, opts, robust: Optional[RobustOptions] = None, device: int = 0,
                                  round_fn: Optional[Callable] = None) -> RobustResult:
    """Solve, cull, re-solve, for any of the three reprojection chains.

    Every round solves the current problem (from the previous round's solution), takes thr = robust.threshold_px or
    k_sigma x global RMS, and fetches the keep flags (sqrt(e2) <= thr) of every observation.  The loop stops when no observation is
    dropped (or after max_rounds solves); otherwise the next problem holds the kept observations at the solved parameters.  A
    block left with fewer than min_block_points observations is removed; a view that loses all its blocks is removed and reported.
    ValueError when a camera loses all its blocks, or an intrinsic chain keeps fewer than 4 views (intrinsics.cpp validate_input).
    ``flat`` is not modified.  ``round_fn(flat, opts, robust, device) -> (summary, thr, rms, keep)`` replaces the GPU round (tests,
    custom solvers)."""
    robust = robust or RobustOptions()
    if robust.max_rounds < 1:
        raise ValueError("max_rounds must be >= 1")
    round_fn = round_fn or _gpu_round
    orig_counts = np.diff(flat.blk_offset).astype(np.int64)
    keep_orig = [np.ones(int(n), bool) for n in orig_counts]
    obs_idx = [np.arange(int(n)) for n in orig_counts]  # per current block: its observations' original indices
    block_map = np.arange(flat.n_blocks)
    view_of = (lambda f, b: int(f.blk_view[b])) if flat.chain != capi.CHAIN_BUNDLE and flat.blk_view is not None else (lambda f, b: int(b))
    view_map = np.arange(flat.n_views if flat.chain != capi.CHAIN_BUNDLE else flat.n_blocks)  # current view -> original view
    removed_blocks: List[int] = []
    removed_views: List[int] = []
    rounds = []
    cur = copy.deepcopy(flat)
    converged = False
    s = None
    for rnd in range(int(robust.max_rounds)):
        s, thr, rms, keep = round_fn(cur, opts, robust, device)
        keep = np.asarray(keep, bool).reshape(-1)
        if keep.shape[0] != cur.n_obs:
            raise ValueError("keep flags must cover every observation of the round's problem")
        dropped = int(keep.size - np.count_nonzero(keep))
        rounds.append((float(thr), dropped, float(rms)))
        if dropped == 0:
            converged = True
            break
        if rnd == robust.max_rounds - 1:
            break
        # ---- cull: new per-block masks, blocks under min_block_points, views without blocks ----------------------------
        kb, keep_blocks, new_obs = [], [], []
        for b in range(cur.n_blocks):
            kk = keep[cur.blk_offset[b]:cur.blk_offset[b + 1]]
            ob = block_map[b]
            keep_orig[ob][obs_idx[b][~kk]] = False
            if int(np.count_nonzero(kk)) < int(robust.min_block_points):
                keep_orig[ob][:] = False
                removed_blocks.append(int(ob))
                continue
            kb.append(b)
            keep_blocks.append(kk)
            new_obs.append(obs_idx[b][kk])
        cams_left = set(int(cur.blk_cam[b]) for b in kb)
        lost = [c for c in range(cur.n_cams) if c not in cams_left]
        if lost:
            raise ValueError(f"camera(s) {lost} lost every residual block to outlier rejection")
        views_left = sorted(set(view_of(cur, b) for b in kb))
        if cur.chain != capi.CHAIN_BUNDLE:
            left = set(views_left)
            removed_views += [int(view_map[v]) for v in range(len(view_map)) if v not in left]
        if cur.chain == capi.CHAIN_INTRINSIC and len(views_left) < 4:
            raise ValueError("Insufficient views for calibration (at least 4 required) after outlier rejection.")
        full_keep = [None] * cur.n_blocks
        for b, kk in zip(kb, keep_blocks):
            full_keep[b] = kk
        cur = subset_problem(cur, full_keep, kb)
        block_map = block_map[kb]
        obs_idx = new_obs
        view_map = view_map[views_left]
    return RobustResult(cur, s, keep_orig, block_map, sorted(removed_blocks), sorted(removed_views), rounds, converged)

