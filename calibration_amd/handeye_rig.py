"""Seed and calibration of a robot-mounted rig: the reference's ``compute_handeye_initialization`` and ``choose_initial_target``
(src/pipeline/detail/bundle_utils.cpp:154-237) on the C ABI (``cba_estimate_bundle_seed``), and the numerical bodies of
``HandEyeCalibrationStage::run`` (src/pipeline/stages/handeye_stage.cpp) and ``BundleAdjustmentStage::run``
(src/pipeline/stages/bundle_stage.cpp) for one rig.

``views[v][c]`` is an (N, 4) array [X, Y, u, v] of robot pose v seen by camera c, or None when camera c has no image there;
``base_poses[v]`` is the 4x4 b_se3_g of robot pose v.  Poses are 4x4 matrices: g_se3_c maps camera c to the gripper, b_se3_t the
target to the robot base.  Reading configuration files and matching image names is not done here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .capi import dptr, i32ptr, i64ptr
from .geometry import pose_from_matrix
from .optim import BundleObservation, BundleOptions, BundleResult, HandeyeResult, OptimOptions, optimize_bundle, optimize_handeye
from .rig import _kmtx5, pose7_to_matrix

NO_PAIRS_ERROR = "No valid motion pairs after filtering. Increase motion or relax thresholds."  # handeyedlt.cpp:76-79
SINGULAR_ERROR = "Tsai-Lenz system is singular"
_SOURCE = {capi.TARGET_ESTIMATED: "estimated", capi.TARGET_CONFIG: "config", capi.TARGET_IDENTITY: "identity"}


@dataclass
class BundleSeedBlocks:
    """Everything cba_estimate_bundle_seed returns, poses as pose7 rows [qw, qx, qy, qz, tx, ty, tz]."""
    g_T_c: np.ndarray       # [n_cams][7]
    cam_status: np.ndarray  # [n_cams]: capi.HANDEYE_*
    cam_pairs: np.ndarray   # [n_cams]: motion pairs that passed the filter
    b_T_t: np.ndarray       # [7]
    target_source: int      # capi.TARGET_*
    blk_pose: np.ndarray    # [n_blocks][7]: each block's planar pose c_T_t
    blk_ok: np.ndarray      # [n_blocks]: 0 for fewer than 4 points or a failed fit (the pose is then the identity)


@dataclass
class BundleSeed:
    """HandeyeInitializationResult + TargetInitializationResult (bundle_utils.h)."""
    g_se3_c: List[np.ndarray]
    report: List[dict]              # per camera: source ("handeye" / "dlt" / "identity"), success, error (when failed)
    failed: bool
    b_se3_t: np.ndarray
    initial_target_source: str      # "estimated" / "config" / "identity"
    blocks: Optional[BundleSeedBlocks] = None


@dataclass
class HandeyeSensorResult:
    status: str                     # no_observations / insufficient_observations / estimation_error / optimization_failed / ok
    used_observations: int
    view_status: List[str]          # per robot pose: missing_image_reference / insufficient_points / ok
    result: Optional[HandeyeResult] = None
    error: str = ""


@dataclass
class HandeyeRigResult:
    status: str                     # ok / partial_success / failed
    sensors: List[HandeyeSensorResult] = field(default_factory=list)

    def successful(self) -> List[Optional[np.ndarray]]:
        """g_se3_c of the sensors whose refinement succeeded (None elsewhere): what the bundle stage reads as "handeye"."""
        return [s.result.g_se3_c if s.result is not None and s.result.core.success else None for s in self.sensors]


@dataclass
class BundleRigResult:
    status: str                     # no_valid_observations / optimization_failed / ok
    success: bool
    requested_views: int
    used_views: int
    view_status: List[List[str]]    # [view][camera]: missing_image_reference / insufficient_points / ok
    view_used: List[bool]
    seed: Optional[BundleSeed] = None
    result: Optional[BundleResult] = None


def estimate_bundle_seed_blocks(n_cams: int, blk_offset, blk_cam, blk_b_T_g, X, Y, u, v, kmtx5, min_angle_deg: float = 1.0,
                                given_mask=None, g_T_c_given=None, b_T_t_given=None) -> BundleSeedBlocks:
    """cba_estimate_bundle_seed on the blocked layout of cba_optimize_bundle (blk_b_T_g: [n_blocks][12] row-major R, t)."""
    lib = capi.load_library()
    off = np.ascontiguousarray(blk_offset, dtype=np.int64)
    nb = len(off) - 1
    bc = np.ascontiguousarray(blk_cam, dtype=np.int32)
    btg = np.ascontiguousarray(np.asarray(blk_b_T_g, dtype=np.float64).reshape(-1, 12))
    cols = [np.ascontiguousarray(a, dtype=np.float64) for a in (X, Y, u, v)]
    K = np.ascontiguousarray(np.asarray(kmtx5, dtype=np.float64).reshape(-1, 5))
    gm = None if given_mask is None else np.ascontiguousarray(given_mask, dtype=np.int32)
    gg = None if g_T_c_given is None else np.ascontiguousarray(np.asarray(g_T_c_given, dtype=np.float64).reshape(-1, 7))
    bt = None if b_T_t_given is None else np.ascontiguousarray(np.asarray(b_T_t_given, dtype=np.float64).reshape(7))
    m = max(int(n_cams), 1)
    g, st, pr = np.zeros((m, 7)), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    out_t, src = np.zeros(7), np.zeros(1, dtype=np.int32)
    bp, ok = np.zeros((max(nb, 1), 7)), np.zeros(max(nb, 1), dtype=np.int32)
    capi.check(lib, lib.cba_estimate_bundle_seed(int(n_cams), nb, i64ptr(off), i32ptr(bc), dptr(btg), *(dptr(a) for a in cols), dptr(K),
                                                 float(min_angle_deg), i32ptr(gm), dptr(gg), dptr(bt), dptr(g), i32ptr(st), i32ptr(pr),
                                                 dptr(out_t), i32ptr(src), dptr(bp), i32ptr(ok)))
    return BundleSeedBlocks(g[:n_cams], st[:n_cams], pr[:n_cams], out_t, int(src[0]), bp[:nb], ok[:nb])


def _given(handeye, n_cams: int):
    """handeye: None, a HandeyeRigResult, or one 4x4 (or None) per camera -> (mask, pose7 rows) or (None, None)"""
    if handeye is None:
        return None, None
    if isinstance(handeye, HandeyeRigResult):
        handeye = handeye.successful()
    if len(handeye) != n_cams:
        raise capi.CbaInvalidArgument(capi.CBA_ERR_INVALID_ARGUMENT, "one hand-eye entry per camera")
    mask = np.array([0 if T is None else 1 for T in handeye], dtype=np.int32)
    rows = np.stack([np.r_[1.0, 0, 0, 0, 0, 0, 0] if T is None else pose_from_matrix(T) for T in handeye])
    return mask, rows


def _flatten(observations: Sequence[BundleObservation]):
    blocks = [np.asarray(o.view, dtype=np.float64).reshape(-1, 4) for o in observations]
    off = np.zeros(len(blocks) + 1, dtype=np.int64)
    np.cumsum([b.shape[0] for b in blocks], out=off[1:])
    allp = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, 4))
    bcam = np.array([int(o.camera_index) for o in observations], dtype=np.int32)
    btg = (np.stack([np.concatenate([np.asarray(o.b_se3_g, dtype=np.float64)[:3, :3].reshape(-1), np.asarray(o.b_se3_g)[:3, 3]])
                     for o in observations]) if observations else np.zeros((0, 12)))
    return off, bcam, btg, [allp[:, k] for k in range(4)]


def estimate_bundle_seed(observations: Sequence[BundleObservation], cameras: Sequence, min_angle_deg: float = 1.0, handeye=None,
                         initial_target=None) -> BundleSeed:
    """compute_handeye_initialization + choose_initial_target (bundle_utils.cpp:154-237) from bundle observations listed
    view-major (as collect_bundle_observations lists them).  ``cameras``: intrinsic vectors or [fx, fy, cx, cy, skew]; only K is
    read.  ``handeye``: a calibrate_handeye_rig result, or one 4x4 (None: not available) per camera.  ``initial_target``: the
    configured 4x4 b_se3_t, or None to estimate it."""
    n_cams = len(cameras)
    K = np.stack([_kmtx5(c) for c in cameras]) if n_cams else np.zeros((0, 5))
    off, bcam, btg, cols = _flatten(observations)
    mask, rows = _given(handeye, n_cams)
    bt = None if initial_target is None else pose_from_matrix(initial_target)
    r = estimate_bundle_seed_blocks(n_cams, off, bcam, btg, *cols, K, min_angle_deg, mask, rows, bt)
    report, failed = [], False
    for c in range(n_cams):
        s = int(r.cam_status[c])
        if s == capi.HANDEYE_GIVEN:
            report.append({"source": "handeye", "success": True})
        elif s == capi.HANDEYE_DLT:
            report.append({"source": "dlt", "success": True})
        elif s == capi.HANDEYE_TOO_FEW_VIEWS:
            report.append({"source": "identity", "success": False, "error": "insufficient_observations"})
            failed = True
        else:
            report.append({"source": "dlt", "success": False, "error": NO_PAIRS_ERROR if s == capi.HANDEYE_NO_PAIRS else SINGULAR_ERROR})
            failed = True
    return BundleSeed([pose7_to_matrix(p) for p in r.g_T_c], report, failed, pose7_to_matrix(r.b_T_t), _SOURCE[r.target_source], r)


def _collect(views, base_poses, n_cams: int):
    """view-major blocks of >= 4 points (collect_bundle_observations, bundle_utils.cpp:46-146) with the per-(view, camera) status"""
    if len(views) != len(base_poses):
        raise capi.CbaInvalidArgument(capi.CBA_ERR_INVALID_ARGUMENT, "one base pose per view")
    obs, status, used = [], [], []
    for v, mv in enumerate(views):
        if len(mv) != n_cams:
            raise capi.CbaInvalidArgument(capi.CBA_ERR_INVALID_ARGUMENT, f"view {v}: one entry per camera")
        row, any_ok = [], False
        for c, pv in enumerate(mv):
            if pv is None:
                row.append("missing_image_reference")
                continue
            a = np.asarray(pv, dtype=np.float64).reshape(-1, 4)
            if a.shape[0] < 4:
                row.append("insufficient_points")
                continue
            obs.append(BundleObservation(a, np.asarray(base_poses[v], dtype=np.float64), c))
            row.append("ok")
            any_ok = True
        status.append(row)
        used.append(any_ok)
    return obs, status, used


def calibrate_handeye_rig(views, base_poses, cameras: Sequence, min_angle_deg: float = 1.0,
                          options: Optional[OptimOptions] = None) -> HandeyeRigResult:
    """The body of HandEyeCalibrationStage::run for one rig: every sensor's block poses and Tsai-Lenz seed come from one
    cba_estimate_bundle_seed call, then optimize_handeye refines each sensor from its seed (estimate_and_optimize_handeye)."""
    n_cams = len(cameras)
    obs, status, _ = _collect(views, base_poses, n_cams)
    seed = estimate_bundle_seed(obs, cameras, min_angle_deg) if obs else None
    sensors, any_ok, all_ok = [], False, True
    for c in range(n_cams):
        vs = [status[v][c] for v in range(len(views))]
        mine = [k for k, o in enumerate(obs) if o.camera_index == c]
        n_used = len(mine)
        if n_used < 2:
            sensors.append(HandeyeSensorResult("no_observations" if n_used == 0 else "insufficient_observations", n_used, vs))
            all_ok = False
            continue
        st = int(seed.blocks.cam_status[c])
        if st != capi.HANDEYE_DLT:
            sensors.append(HandeyeSensorResult("estimation_error", n_used, vs,
                                               error=NO_PAIRS_ERROR if st == capi.HANDEYE_NO_PAIRS else SINGULAR_ERROR))
            all_ok = False
            continue
        base = [obs[k].b_se3_g for k in mine]
        cam = [pose7_to_matrix(seed.blocks.blk_pose[k]) for k in mine]
        try:
            res = optimize_handeye(base, cam, seed.g_se3_c[c], options)
        except capi.CbaError as e:
            sensors.append(HandeyeSensorResult("estimation_error", n_used, vs, error=e.message))
            all_ok = False
            continue
        ok = bool(res.core.success)
        sensors.append(HandeyeSensorResult("ok" if ok else "optimization_failed", n_used, vs, res))
        any_ok = any_ok or ok
        all_ok = all_ok and ok
    return HandeyeRigResult("ok" if any_ok and all_ok else ("partial_success" if any_ok else "failed"), sensors)


def calibrate_bundle_rig(views, base_poses, cameras: Sequence, opts: Optional[BundleOptions] = None, min_angle_deg: float = 1.0,
                         handeye=None, initial_target=None, device: int = 0) -> BundleRigResult:
    """The body of BundleAdjustmentStage::run for one rig: collect the view-major observations, seed (compute_handeye_initialization
    with ``handeye``'s successful sensors as "handeye", choose_initial_target with ``initial_target`` as "config"), then
    optimize_bundle from the seed with the full ``cameras``.  A failed hand-eye initialisation without a configured target makes
    ``success`` false even when the solve succeeds (bundle_stage.cpp:91-93, 111-113)."""
    opts = opts or BundleOptions()
    n_cams = len(cameras)
    obs, status, used = _collect(views, base_poses, n_cams)
    if not obs:
        return BundleRigResult("no_valid_observations", False, len(views), 0, status, used)
    seed = estimate_bundle_seed(obs, cameras, min_angle_deg, handeye, initial_target)
    res = optimize_bundle(obs, [np.asarray(c, dtype=np.float64) for c in cameras], seed.g_se3_c, seed.b_se3_t, opts, device)
    ok = bool(res.core.success)
    success = ok and not (seed.failed and initial_target is None)
    return BundleRigResult("ok" if ok else "optimization_failed", success, len(views), sum(used), status, used, seed, res)
