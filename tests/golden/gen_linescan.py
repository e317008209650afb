"""Writes tests/golden/linescan_kats.json: the scenes of the reference's line-scan KATs, restated with this repository's own
geometry (tests/linescan_ref.py: target plane x laser plane, the line clipped to the [-0.5, 0.5]^2 target, sampled, projected).
  plane_fit_multiple_views  LineScanCalibration.PlaneFitMultipleViews (linescan_test.cpp): K = I, n = (0.1, 1, -0.1)/|.|,
                            d = 0.5, views at z = 1 m (identity, and rotated 0.2 rad about x), 400 samples per unit
  plane_fit_single_view     LineScanCalibration.PlaneFitFailsSingleView: one view, laser plane y = 0.5
  facade                    LinescanFacade.CalibratesFromViews (linescan_facade_test.cpp): fx 400, fy 402,
                            n = (0.1, 1, -0.05)/|.|, d = 0.4, 200 samples per unit
  points_from_view          LinescanUtils.PointsFromViewProduces3DPoints (as written in linescan_utils_test.cpp)
  fit_plane_svd_grid        LinescanUtils.FitPlaneSVDDetectsPlane: the 5 x 5 integer grid on z = 0
  plane_rms_exact           LinescanUtils.PlaneRMSZeroForExactPoints
  svd_ideal_plane           PlaneFit.SvdMatchesIdealPlane (planefit_test.cpp): 11 x 11 points on the plane through
                            (0.5, -0.2, 0.8) with normal (0.4, 0.1, 1)
usage: python -m tests.golden.gen_linescan   (from the repository root)
"""
import json
import os

import numpy as np

from tests import linescan_ref as ref

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "linescan_kats.json")


def _views(intr, n, d, spu):
    poses = [ref.pose(np.eye(3), [0.0, 0.0, 1.0]), ref.pose(ref.rot_x(0.2), [0.0, 0.0, 1.0])]
    return [{"target_view": tv.tolist(), "laser_uv": lv.tolist()} for tv, lv in (ref.make_view(p, n, d, intr, samples_per_unit=spu) for p in poses)]


def _unit(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


def build():
    k_id = [1.0, 1.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0]
    n1 = _unit([0.1, 1.0, -0.1])
    k_f = [400.0, 402.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0]
    n2 = _unit([0.1, 1.0, -0.05])
    tv1, lv1 = ref.make_view(np.eye(4), np.array([0.0, 1.0, 0.0]), -0.5, np.array(k_id))
    ns = _unit([0.4, 0.1, 1.0])
    gt = np.r_[ns, -ns @ np.array([0.5, -0.2, 0.8])]
    svd_pts = []
    for i in range(-5, 6):
        for j in range(-5, 6):
            x, y = 0.1 * i, 0.1 * j
            svd_pts.append([x, y, (-gt[3] - gt[0] * x - gt[1] * y) / gt[2]])
    return {
        "plane_fit_multiple_views": {"intr": k_id, "inverse_coeffs": [0.0] * 5, "plane": list(n1) + [0.5],
                                     "views": _views(np.array(k_id), n1, 0.5, 400.0)},
        "plane_fit_single_view": {"intr": k_id, "inverse_coeffs": [0.0] * 5, "views": [{"target_view": tv1.tolist(), "laser_uv": lv1.tolist()}]},
        "facade": {"intr": k_f, "plane": list(n2) + [0.4], "views": _views(np.array(k_f), n2, 0.4, 200.0)},
        "points_from_view": {"intr": [400.0, 400.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0], "inverse_coeffs": [0.0, 0.0],
                             "target_view": [[-0.5, -0.5, -200, -200], [0.5, -0.5, 200, -200], [0.5, 0.5, 200, 200], [-0.5, 0.5, -200, 200]],
                             "laser_uv": [[-50, 0], [0, 0], [50, 0]]},
        "fit_plane_svd_grid": {"points": [[float(i), float(j), 0.0] for i in range(5) for j in range(5)], "plane": [0.0, 0.0, 1.0, 0.0]},
        "plane_rms_exact": {"points": [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]},
        "svd_ideal_plane": {"points": svd_pts, "plane": list(gt)},
    }


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(build(), f)
        f.write("\n")
