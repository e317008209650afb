"""GPU tier of stereo depth: cba_stereo_matcher and cba_stereo_points on the device against the numpy restatement
tests/stereo_ref.py, bitwise (NaN positions equal): the sizes and options of the issue, planted cases, independence of the pairs,
determinism, the handle's xyz against cba_stereo_points, the handle's life cycle, and the chain calibrated rig -> rectified pair ->
disparity -> points on a rendered plane."""
import numpy as np
import pytest

from calibration_amd import capi, stereo
from calibration_amd.stereo import StereoMatcher, StereoMatchOptions, stereo_points
from tests import camera_ref as R
from tests import stereo_ref as S

pytestmark = pytest.mark.gpu


def _opts(o):
    return StereoMatchOptions(o.min_disparity, o.num_disparities, o.half_window, o.uniqueness_percent, o.lr_max_diff, bool(o.subpixel))


def _run(left, right, o, geom=None, pose=None, max_pairs=None):
    with StereoMatcher(left.shape[2], left.shape[1], max_pairs or left.shape[0], _opts(o), geom, pose) as m:
        r = m.process(left, right)
    return dict(disparity=r.disparity, cost=r.cost, xyz=r.xyz)


@pytest.mark.parametrize("case", S.option_cases(), ids=lambda c: f"{c[0]}x{c[1]}_n{c[2]}_{c[3]}")
def test_matcher_matches_restatement(gpu_lib, case):
    H, W, n, o = case
    left, right = S.random_pairs(n, H, W)
    pose = S.POSE if o.half_window != 4 else None
    ref = S.match_cached((H, W, n, repr(o)), left, right, o, S.GEOM, pose)
    got = _run(left, right, o, S.GEOM, pose)
    for k in ("disparity", "cost", "xyz"):
        assert S.bitwise(got[k], ref[k]), k


# ---- planted cases ------------------------------------------------------------------------------------------------------------------
def _both(left, right, o):
    ref = S.match(left, right, o)
    got = _run(left, right, o)
    assert S.bitwise(got["disparity"], ref["disparity"]) and S.bitwise(got["cost"], ref["cost"])
    return ref


def test_constant_images(gpu_lib):
    img = np.full((1, 16, 40), 77, np.uint8)
    r, dmin = 2, -3
    ref = _both(img, img, S.Options(dmin, 12, r, 0, -1, 1))
    d = ref["disparity"][0]
    xs = np.arange(40)
    adm = (xs >= r) & (xs <= 39 - r) & (xs + r - dmin <= 39)  # the columns that admit min_disparity
    assert (d[r:16 - r][:, adm] == dmin).all() and (ref["cost"][0][r:16 - r, r:40 - r] == 0).all()
    assert (d[r:16 - r, 37] == 0.0).all()  # x = 37 admits d >= 0 only: the lowest admissible candidate
    ref = _both(img, img, S.Options(dmin, 12, r, 10, -1, 1))
    assert np.isnan(ref["disparity"]).all() and (ref["cost"][0][r:16 - r, r:40 - r] == 0).all()


def test_periodic_texture_ties_choose_the_lowest(gpu_lib):
    row = (np.arange(80) % 8 * 30).astype(np.uint8)
    img = np.ascontiguousarray(np.broadcast_to(row, (1, 12, 80)))
    ref = _both(img, img, S.Options(-8, 24, 1, 0, -1, 0))
    d = ref["disparity"][0, 5]
    assert d[40] == -8 and d[4] == -8 and d[78] == 0  # d = -8, 0, 8 tie where admissible (x = 78 admits d >= 0 only): the lowest wins


def test_best_at_either_end_and_flat_costs(gpu_lib):
    left, right = S.random_pairs(1, 16, 64, shift=4)
    for dmin, D in ((4, 8), (-3, 8)):  # the true shift is the first / the last candidate: no sub-pixel step
        ref = _both(left, right, S.Options(dmin, D, 2, 0, -1, 1))
        d = ref["disparity"][0, 4:12, 16:48]
        assert (d == 4.0).mean() > 0.9
    # flat costs: den == 0 (left constant, right constant of another level: every candidate costs the same)
    a, b = np.full((1, 12, 30), 10, np.uint8), np.full((1, 12, 30), 200, np.uint8)
    ref = _both(a, b, S.Options(0, 6, 1, 0, -1, 1))
    assert (ref["disparity"][0, 1:11, 8:28] == 0.0).all() and (ref["cost"][0, 1:11, 8:28] == 9 * 190).all()
    # a saturated pair: the largest cost there is
    a, b = np.zeros((1, 21, 40), np.uint8), np.full((1, 21, 40), 255, np.uint8)
    ref = _both(a, b, S.Options(0, 4, 10, 0, 1, 1))
    assert ref["cost"].max() == 255 * 441


def test_occlusion_and_single_candidate(gpu_lib):
    # the right image is the left one moved by 6 columns, except a strip that shows other content: the left-right check removes it
    L, Rr, _ = S.truth_pair(lambda x, y: 6.0, H=24, W=96)
    Rr = Rr.copy()
    Rr[:, 40:52] = S.truth_pair(lambda x, y: 6.0, H=24, W=96, seed=9)[1][:, 10:22]
    off = _both(L[None], Rr[None], S.Options(0, 16, 2, 0, -1, 1))["disparity"][0]
    on = _both(L[None], Rr[None], S.Options(0, 16, 2, 0, 1, 1))["disparity"][0]
    strip = (slice(2, 22), slice(48, 56))  # left columns whose match lies in the strip
    assert np.isfinite(off[strip]).all() and np.isnan(on[strip]).mean() > 0.5
    assert np.isfinite(on[2:22, 20:40]).mean() > 0.95
    # one admissible candidate: x = r with min_disparity = 0 admits d = 0 alone
    ref = _both(L[None], Rr[None], S.Options(0, 16, 2, 10, -1, 1))
    assert (ref["disparity"][0, 2:22, 2] == 0.0).all()


# ---- independence, determinism, the handle ---------------------------------------------------------------------------------------------
def test_independence_determinism_and_handle(gpu_lib):
    left, right = S.random_pairs(3, 33, 131)
    o = S.Options(-2, 20, 3, 10, 1, 1)
    with StereoMatcher(131, 33, 4, _opts(o), S.GEOM, S.POSE) as m:
        a = m.process(left, right)
        b = m.process(left, right)
        for x, y in ((a.disparity, b.disparity), (a.cost, b.cost), (a.xyz, b.xyz)):
            assert S.bitwise(x, y)
        one = m.process(left[1], right[1])
        assert S.bitwise(one.disparity[0], a.disparity[1]) and S.bitwise(one.cost[0], a.cost[1]) and S.bitwise(one.xyz[0], a.xyz[1])
        none = m.process(left[:0], right[:0])
        assert none.disparity.shape == (0, 33, 131)
        with pytest.raises(ValueError):
            m.process(np.concatenate([left, left]), np.concatenate([right, right]))
        five = np.zeros((5, 33, 131), np.uint8)
        fp = capi.C.POINTER(capi.C.c_float)
        assert gpu_lib.cba_stereo_matcher_process(m._h, 5, capi.u8ptr(five), capi.u8ptr(five), capi.C.cast(None, fp), None,
                                                  capi.C.cast(None, fp)) == capi.CBA_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        m.process(left, right)  # closed
    with StereoMatcher(131, 33, 3, _opts(o)) as m2:  # no geometry: xyz is an error, the rest is the same
        r = m2.process(left, right)
        assert r.xyz is None and S.bitwise(r.disparity, a.disparity)
        with pytest.raises(ValueError):
            m2.process(left, right, want_xyz=True)
        out = np.empty((3, 33, 131, 3), np.float32)
        fp = capi.C.POINTER(capi.C.c_float)
        assert gpu_lib.cba_stereo_matcher_process(m2._h, 3, capi.u8ptr(left), capi.u8ptr(right), capi.C.cast(None, fp), None,
                                                  out.ctypes.data_as(fp)) == capi.CBA_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("pose", [None, S.POSE], ids=["no_pose", "pose"])
def test_xyz_is_stereo_points_of_the_disparity(gpu_lib, pose):
    left, right = S.random_pairs(2, 21, 70)
    got = _run(left, right, S.Options(0, 16, 2, 10, 1, 1), S.GEOM, pose)
    yy, xx = np.indices((21, 70))
    d = got["disparity"].astype(np.float64)
    uvd = np.stack([np.broadcast_to(xx, d.shape), np.broadcast_to(yy, d.shape), d], axis=-1).reshape(-1, 3)
    pts = stereo_points(uvd, S.GEOM, pose)
    assert S.bitwise(pts.astype(np.float32).reshape(got["xyz"].shape), got["xyz"]) and np.isfinite(pts).any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_stereo_points_match_restatement(gpu_lib, n):
    rng = np.random.default_rng(n)
    uvd = np.c_[rng.uniform(0, 200, (n, 2)), rng.uniform(-2, 60, n)]
    if n:
        uvd[::7, 2] = [0.0, np.nan, np.inf, -1.0][n % 4]
        uvd[n // 2, 0] = np.nan
    for pose in (None, S.POSE):
        assert S.bitwise(stereo_points(uvd, S.GEOM, pose), S.points(uvd, S.GEOM, pose))


# ---- end to end: calibrated rig -> rectified pair -> disparity -> points on a plane -------------------------------------------------------
E2E_W, E2E_H = 200, 120
PLANE_N, PLANE_D = np.array([0.15, -0.05, 1.0]) / np.linalg.norm([0.15, -0.05, 1.0]), -1.0  # n.P + d = 0, about 1 m in front
# The restatement's chain (camera_ref maps and resampling, stereo_ref matching and points), measured on this scene: RMS distance of the
# valid interior points to the plane 4.21e-3 (the plane is ~1 m away, the baseline 0.1 m and f' = 180 px: a disparity error of 0.076 px),
# valid share 1.000, worst point 1.22e-2.
E2E_REF_RMS = 4.21e-3


def _e2e_rig():
    """intrinsics and c_T_r in the layout cba_optimize_extrinsics returns them: [n_cams][10] and [n_cams][7]"""
    intr = np.array([[182.0, 180.0, 99.0, 60.5, 0.0, -0.12, 0.03, 0.0, 8e-4, -5e-4], [179.0, 181.0, 101.5, 58.0, 0.0, -0.10, 0.02, 0.0, -6e-4, 7e-4]])
    rows = []
    for q, o in ((np.array([1.0, 0.004, 0.012, -0.003]), np.zeros(3)), (np.array([1.0, -0.006, -0.02, 0.005]), np.array([0.1, 0.003, -0.002]))):
        q = q / np.linalg.norm(q)
        rows.append(np.r_[q, -S.quat_to_rotmat(q) @ o])
    return intr, np.array(rows)


def _e2e_render(intr, c_T_r):
    """both camera images of the textured plane, by unprojecting every source pixel"""
    yy, xx = np.indices((E2E_H, E2E_W))
    uv = np.c_[xx.ravel(), yy.ravel()].astype(float)
    a = np.cross(PLANE_N, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(PLANE_N, a)
    out = []
    for c in range(2):
        Rm = S.quat_to_rotmat(c_T_r[c, :4])
        o = -Rm.T @ c_T_r[c, 4:]
        ray = np.c_[R.unproject(R.PINHOLE, intr[c], uv), np.ones(len(uv))] @ Rm  # R^T ray per row
        s = -(PLANE_N @ o + PLANE_D) / (ray @ PLANE_N)
        P = o + s[:, None] * ray
        p, q = P @ a, P @ b
        t = (np.sin(41 * p) + np.sin(67 * q + 1) + np.sin(29 * (p + q)) + np.sin(53 * (p - q) + 2) + np.sin(97 * p + 13 * q)) / 5
        out.append(np.clip(np.rint(127.5 + 120 * t), 0, 255).astype(np.uint8).reshape(E2E_H, E2E_W))
    return np.stack(out)


def _e2e_score(xyz, o):
    r, dmax = o.half_window, o.min_disparity + o.num_disparities - 1
    inner = xyz[0, r + 8:E2E_H - r - 8, dmax + r + 8:E2E_W - r - 8].reshape(-1, 3).astype(np.float64)
    valid = ~np.isnan(inner).any(1)
    dist = np.abs(inner[valid] @ PLANE_N + PLANE_D)
    return float(np.sqrt(np.mean(dist ** 2))), float(valid.mean()), float(dist.max())


def e2e_restatement():
    intr, c_T_r = _e2e_rig()
    src = _e2e_render(intr, c_T_r)
    ref = S.rectify(intr, c_T_r, E2E_W, E2E_H)
    rect = [R.apply(src[c], *R.undistort_map(R.PINHOLE, intr[c], E2E_W, E2E_H, ref["R"][c], ref["new_k5"][c])) for c in range(2)]
    return intr, c_T_r, src, rect


def test_end_to_end_plane(gpu_lib):
    intr, c_T_r, src, rect_ref = e2e_restatement()
    o = S.Options(0, 40, 4, 10, 1, 1)
    rec = stereo.rectify(intr, c_T_r, E2E_W, E2E_H)
    ref = S.match(rect_ref[0][None], rect_ref[1][None], o, (rec.new_K[0, 0], rec.new_K[0, 2], rec.new_K[0, 3], rec.baseline), rec.r_T_rect)
    rms_ref, share_ref, worst_ref = _e2e_score(ref["xyz"], o)
    print(f"restatement: rms {rms_ref:.3e} valid share {share_ref:.4f} worst {worst_ref:.3e}")
    assert abs(rms_ref / E2E_REF_RMS - 1.0) < 0.01  # the value written above is the one measured
    with stereo.rectify_maps(intr, rec, E2E_W, E2E_H) as maps:
        rect = maps.apply(src, [0, 1])
    with StereoMatcher(E2E_W, E2E_H, 1, _opts(o), rec, rec.r_T_rect) as m:
        got = m.process(rect[0], rect[1])
    rms, share, worst = _e2e_score(got.xyz, o)
    print(f"device: rms {rms:.3e} valid share {share:.4f} worst {worst:.3e}")
    assert rms <= 3 * E2E_REF_RMS
    assert share >= 0.95
    assert worst <= 10 * E2E_REF_RMS
