"""numpy restatement of the reference's hand-eye / bundle seed (TEST INFRASTRUCTURE: the checker of bundle_seed_math.hpp and of
cba_estimate_bundle_seed):
  compute_handeye_initialization   src/pipeline/detail/bundle_utils.cpp:154-200
  choose_initial_target            src/pipeline/detail/bundle_utils.cpp:202-237
  estimate_handeye_dlt             tests/helpers.py tsai_lenz_dlt (handeyedlt.cpp:84-137)
  average_isometries               tests/extrinsic_dlt_ref.py (se3_utils.h:75-95)
Accumulators are per camera: base[c] (4x4 b_T_g) and cam[c] (4x4 c_T_t), in the order the reference appends them.
"""
import numpy as np

from tests import helpers
from tests.extrinsic_dlt_ref import IDENTITY7, average_isometries, matrix_of

NO_PAIRS = "No valid motion pairs after filtering. Increase motion or relax thresholds."


def accumulators(observations, blk_pose, n_cams):
    """collect_bundle_observations' SensorAccumulators from bundle observations listed view-major and each one's pose7."""
    base, cam = [[] for _ in range(n_cams)], [[] for _ in range(n_cams)]
    for o, p in zip(observations, blk_pose):
        if len(o.view) < 4:
            continue
        base[o.camera_index].append(np.asarray(o.b_se3_g, dtype=np.float64))
        cam[o.camera_index].append(matrix_of(p))
    return base, cam


def handeye_initialization(base, cam, min_angle_deg=1.0, handeye=None):
    """-> (transforms [4x4], report [dict], failed, pairs [int]).  handeye[c]: a successful hand-eye g_se3_c or None."""
    n = len(base)
    out, report, pairs, failed = [np.eye(4) for _ in range(n)], [], [0] * n, False
    for c in range(n):
        if handeye is not None and handeye[c] is not None:
            out[c] = np.asarray(handeye[c], dtype=np.float64)
            report.append({"source": "handeye", "success": True})
            continue
        if len(cam[c]) >= 2:
            pairs[c] = len(helpers.build_all_pairs(base[c], cam[c], min_angle_deg))
            try:
                out[c] = helpers.tsai_lenz_dlt(base[c], cam[c], min_angle_deg)
                report.append({"source": "dlt", "success": True})
            except RuntimeError as e:
                report.append({"source": "dlt", "success": False, "error": str(e)})
                failed = True
        else:
            report.append({"source": "identity", "success": False, "error": "insufficient_observations"})
            failed = True
    return out, report, failed, pairs


def candidates(base, cam, g):
    """b_T_g * g_T_c * c_T_t over the accumulators, camera-major then in each camera's order"""
    return [b @ g[c] @ t for c in range(len(base)) for b, t in zip(base[c], cam[c])]


def initial_target(base, cam, g, config=None):
    """-> (pose7, source)"""
    if config is not None:
        return np.asarray(config, dtype=np.float64), "config"
    cand = candidates(base, cam, g)
    if not cand:
        return IDENTITY7.copy(), "identity"
    return average_isometries(cand), "estimated"
