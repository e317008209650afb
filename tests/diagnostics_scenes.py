"""Scenes of the reprojection-diagnostics tests: block sizes that straddle the Mode R tile edges, gross outliers at known
indices, and the outlier-rejection round run on the CPU oracle (used to set the GPU tests' margins)."""
import numpy as np

from calibration_amd import capi
from calibration_amd import diagnostics as D
from tests import helpers, synth

EDGE_SIZES = (1, 63, 64, 65, 2047, 2048, 2049)


def edge_scene(chain, model, seed=5):
    """A problem whose residual blocks hold EDGE_SIZES observations (cycled) of a 50 x 50 grid."""
    kw = dict(rows=50, cols=50, spacing=0.004, model=model, seed=seed, noise_px=0.1)
    if chain == capi.CHAIN_INTRINSIC:
        sc = synth.scene_intrinsics(n_views=7, **kw)
    elif chain == capi.CHAIN_EXTRINSIC:
        sc = synth.scene_extrinsics(n_views=4, n_cams=2, **kw)
    else:
        kw.pop("noise_px")
        sc = synth.scene_bundle(n_poses=4, n_cams=2, noise_px=0.1, distortion=True, **kw)
    f = sc.flat
    masks = []
    for b in range(f.n_blocks):
        n = int(f.blk_offset[b + 1] - f.blk_offset[b])
        m = np.zeros(n, bool)
        m[:min(n, EDGE_SIZES[b % len(EDGE_SIZES)])] = True
        masks.append(m)
    return D.subset_problem(f, masks)


def contaminate(flat, frac=0.02, lo=20.0, hi=50.0, seed=11):
    """Adds gross errors of lo..hi px in a random direction to a fraction of the observations; returns their global indices."""
    rng = np.random.default_rng(seed)
    n = flat.n_obs
    idx = np.sort(rng.choice(n, size=int(round(frac * n)), replace=False))
    mag = rng.uniform(lo, hi, idx.size)
    ang = rng.uniform(0.0, 2.0 * np.pi, idx.size)
    flat.u[idx] += mag * np.cos(ang)
    flat.v[idx] += mag * np.sin(ang)
    return idx


def oracle_round(flat, opts, robust, device):
    """refine_with_outlier_rejection's round on the CPU oracle: orc_reproj_solve, then the raw residuals of orc_reproj_eval."""
    orc = helpers.load_oracle()
    s = helpers.oracle_solve(orc, flat, opts)
    r, _ = helpers.oracle_eval(orc, flat)
    e2 = r[0::2] * r[0::2] + r[1::2] * r[1::2]
    counts = np.diff(flat.blk_offset)
    key = flat.blk_view if flat.chain != capi.CHAIN_BUNDLE else np.arange(flat.n_blocks)
    nv = int(key.max()) + 1 if len(key) else 0
    sums = np.bincount(np.repeat(key, counts), weights=e2, minlength=nv)
    ns = np.bincount(key, weights=counts, minlength=nv)
    rms_v = np.sqrt(sums / (2.0 * np.maximum(ns, 1)))
    rms = D.compute_global_rms(list(rms_v), list(ns.astype(int)))
    thr = robust.threshold_px if robust.threshold_px is not None else robust.k_sigma * rms
    return s, thr, rms, np.sqrt(e2) <= thr


def intr_error(flat, gt_intr):
    """max |fx, fy, cx, cy - ground truth| over the cameras (px)."""
    a = flat.intr.reshape(gt_intr.shape)
    return float(np.abs(a[:, :4] - gt_intr[:, :4]).max())
