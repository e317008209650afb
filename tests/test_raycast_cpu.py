"""CPU tier of the TSDF ray cast (cba_tsdf_raycast): the numpy restatement (tests/raycast_ref.py) against the host build of
tsdf_ray_math.hpp (tests/raycast_cpu) to the bit at every size and planted case of the GPU tier (which imports the cases from here),
the planted cases against what the rule gives by hand, ground truth on the rendered scenes of tests/fusion_ref.py, the restatement's
own frame-to-model chain, the stand-alone driver under the sanitizers, and what the library checks before it asks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.capi import dptr
from tests import cloud_ref as R
from tests import fusion_ref as F
from tests import host_build
from tests import raycast_ref as RC
from tests import test_fusion_cpu as cpu
from tests.test_fusion_cpu import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("depth", "xyz", "normals", "status")

# Ground truth, measured on the restatement with the rays of tests/camera_ref.py's unprojection: the scenes of test_fusion_cpu fused
# without their held-out last view and ray cast at the held-out pose with the default options (half-voxel steps, skip 0.5).
# (scene, model) -> over the pixels that are hits and have a rendered depth: the rms and the largest difference between the cast and the
# rendered depth in voxels, and the largest angle in rad between a cast normal and the true one (tests/fusion_ref.surface_error, which
# leaves the bumpy surface's step out).  The largest depth errors sit at silhouette pixels, where a ray grazes the band: the sphere's
# rim and the bumpy surface's step.  The figures are the measured values rounded up in their fourth digit; the bars are these times
# cpu.MARGIN, and the device, which must give the restatement's bits from rays that agree to 1e-12, needs no wider ones.  Also
# measured (printed by the test, asserted only as the condition "at least half"): hits among the truth-finite pixels.
# Sphere, pinhole: 1927 of 1977 truth pixels hit, 7-33 samples per hit ray (mean 19.7; 25.3 at skip 0, 17.2 at skip 1); bumpy, pinhole:
# 4561 of 4757, 6-18 samples (mean 8.67; 21.5 at skip 0, 4.54 at skip 1).  The hit sets differ slightly between skip values.
RAYCAST_ERROR = {("sphere", F.PINHOLE): (0.4453, 2.531, 0.4196), ("sphere", F.SCHEIMPFLUG): (0.4028, 2.646, 0.4650),
                 ("bumpy", F.PINHOLE): (0.2329, 2.754, 0.06795), ("bumpy", F.SCHEIMPFLUG): (0.2300, 2.305, 0.08078)}

# The chain: cpu.chain's held-out view tracked against the model's ray cast at cpu.chain's perturbed start, point to plane within
# cpu.CHAIN_MD, TRACK_ITERATIONS updates (the pose stands still to 1e-9 after six; the step never falls below 1e-10, so the status is
# NOT_CONVERGED), every second pixel of every second row as the source (the restatement's search is quadratic).  TRACK: what
# track_truth_error gives for the restatement's result, rounded up in the fourth digit: the sphere's centre; the bumpy surface's
# rotation (rad) and translation (0.0064 is a tenth of a voxel: the model's own depth error is 0.23 voxel rms).
TRACK_ITERATIONS = 6
TRACK = {"sphere": (0.01338, 0.0), "bumpy": (0.004350, 0.006354)}


@pytest.fixture(scope="module")
def host():
    return host_build.load("raycast_cpu")


def same_cast(a, b, keys=KEYS):
    return all(same(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])) for k in keys)


# ---- cases shared with the GPU tier ------------------------------------------------------------------------------------------------------
VIEW_SIZES = [(1, 1), (7, 5), (8, 8), (9, 8), (8, 9), (17, 9), (33, 9), (65, 17)]
VOLUMES = [(2, 2, 2), (3, 2, 2), (5, 4, 3), (64, 3, 2), (65, 3, 2)]


def field(shape, seed, dense):
    """cpu.field_volume over F.random_field; dense: every voxel observed (W + 1), so that most cells can be sampled"""
    D, W = F.random_field(shape, seed)
    return cpu.field_volume(shape, D, W + np.float32(1.0) if dense else W)


def views_for(vol, model, Wd, H, n_views):
    """intrinsics under which the volume's middle plane overfills a Wd x H view from one of its diagonals away (so nearly every ray
    enters the box, obliquely towards the view's edges), and n_views poses around that place looking at its centre; from two views on,
    the second one looks away from the volume"""
    ext = np.array([(n - 1) * vol.vs for n in vol.shape])
    centre = vol.origin + 0.5 * ext
    dist = np.linalg.norm(ext)
    intr = np.array([1.2 * max(Wd, 2) * dist / ext[0], 1.2 * max(H, 2) * dist / ext[1], (Wd - 1) / 2.0, (H - 1) / 2.0, 0.01] + [0.1 * v for v in F.DIST]
                    + ([0.003, -0.002] if model == F.SCHEIMPFLUG else []))
    poses = []
    for m in range(n_views):
        eye = centre + np.array([0.05 * ext[0] * (m - 1), 0.04 * ext[1] * (2 - m), -dist * (1.0 + 0.05 * m)])
        poses.append(F.look_at(eye, 2 * eye - centre if m == 1 else centre, up=(0.0, -1.0, 0.0)))
    return intr, np.array(poses)


def size_cases():
    """(name, volume shape, view (width, height), model, n_views, dense, options)"""
    out = []
    for k, (view, n_views) in enumerate(zip(VIEW_SIZES, (1, 2, 5, 1, 2, 5, 2, 1))):
        shape, model = VOLUMES[(k + 2) % len(VOLUMES)], F.PINHOLE if k % 2 == 0 else F.SCHEIMPFLUG
        out.append(("view%dx%d" % view, shape, view, model, n_views, True, {}))
    for k, shape in enumerate(VOLUMES):
        model = F.SCHEIMPFLUG if k % 2 == 0 else F.PINHOLE
        out.append(("vol%dx%dx%d" % shape, shape, (17, 9), model, 2, True, dict(skip=(0.0, 0.5, 1.0)[k % 3])))
        out.append(("vol%dx%dx%d_sparse" % shape, shape, (33, 9), model, 1, False, dict(skip=1.0 if k % 2 else 0.5)))
    out.append(("vol65x3x2_w2", (65, 3, 2), (33, 9), F.PINHOLE, 2, True, dict(min_weight=2.0, step=0.125 / 16)))
    out.append(("vol32x8x5_near_far", (32, 8, 5), (33, 9), F.PINHOLE, 5, True, dict(near_depth=3.9, far_depth=4.2, skip=0.0)))
    return out


SEED = 83  # of the random fields: every dense case has hits, BEHIND rays and misses under it


def size_case(case):
    _, shape, (Wd, H), model, n_views, dense, opts = case
    vol = field(shape, SEED + shape[0], dense)
    intr, poses = views_for(vol, model, Wd, H, n_views)
    return vol, model, intr, poses, (H, Wd), opts


# The planted volume: 9 x 9 x 9 voxels of 1/8 at (-0.5, -0.5, 1) with D = (4 - k) / 4 (zero on the plane z = 1.5) and W = 1, seen through
# a pinhole without distortion, fx = fy = 8 and c = (4, 4) over 9 x 9 pixels: the ray of pixel (col, row) is ((col - 4) / 8,
# (row - 4) / 8) exactly, also by the iterative undistortion, whose every step is then exact.  Poses have unit or half-unit
# quaternion entries, so R holds 0 and +-1 alone and every value below is exact.
PLANTED_INTR = np.array([8.0, 8.0, 4.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
PLANTED_SHAPE = (9, 9)
IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])


def planted_rays():
    v, u = np.mgrid[0:9, 0:9].astype(np.float64)
    return np.stack([(u - 4.0) / 8.0, (v - 4.0) / 8.0], -1)


def planted_volume():
    vol = F.Volume((9, 9, 9), np.array([-0.5, -0.5, 1.0]), 0.125, 0.5)
    vol.D[:] = ((4.0 - np.arange(9)) / 4.0).astype(np.float32)[:, None, None]
    vol.W[:] = 1.0
    return vol


def planted_cases():
    """name -> (volume, pose7, options, expected (status, depth, count, normal) of the centre pixel (4, 4); normal: True = (0, 0, -1),
    False = NaN)"""
    out = {}
    fixed = dict(skip=0.0)
    nan = np.nan
    # along z through the lattice points (4, 4, k): parallel to x and y inside the slab, f = 0; sixteenths from z = 1: the ninth sample
    # is F = 0 exactly (F_prev == 0), the tenth is negative
    out["axis"] = (planted_volume(), IDENTITY, fixed, (RC.HIT, 1.5, 10, True))
    out["axis_skip_half"] = (planted_volume(), IDENTITY, dict(skip=0.5), (RC.HIT, 1.5, None, True))
    out["axis_skip_one"] = (planted_volume(), IDENTITY, dict(skip=1.0), (RC.HIT, 1.5, None, True))
    v = planted_volume()
    v.D[4, 4, 4] = np.float32(-0.0)
    out["minus_zero"] = (v, IDENTITY, fixed, (RC.HIT, 1.5, 10, None))
    out["outside_the_slab"] = (planted_volume(), np.array([1.0, 0, 0, 0, -1.0, 0, 0]), fixed, (RC.MISS, nan, 0, False))
    out["last_lattice_plane"] = (planted_volume(), np.array([1.0, 0, 0, 0, -0.5, 0, 0]), fixed, (RC.HIT, 1.5, 10, False))  # g_x = n - 1: no +x sample
    out["camera_inside"] = (planted_volume(), np.array([1.0, 0, 0, 0, 0, 0, -1.25]), fixed, (RC.HIT, 0.25, 6, True))
    out["near_cuts"] = (planted_volume(), IDENTITY, dict(skip=0.0, near_depth=1.625), (RC.BEHIND, nan, 1, False))  # the first route
    out["far_cuts"] = (planted_volume(), IDENTITY, dict(skip=0.0, far_depth=1.4375), (RC.MISS, nan, 8, False))
    out["far_camera"] = (planted_volume(), np.array([1.0, 0, 0, 0, 0, 0, 1e17]), {}, (RC.MISS, nan, 1, False))  # z + step == z: no progress
    out["looking_away"] = (planted_volume(), np.array([0.0, 1.0, 0, 0, 0, 0, 0]), {}, (RC.MISS, nan, 0, False))
    v = planted_volume()
    v.W[4, 4, 6] = 0.0  # voxel (6, 4, 4): in the cell of the hit's +x sample alone
    out["normals_cell_below_min_weight"] = (v, IDENTITY, fixed, (RC.HIT, 1.5, 10, False))
    out["min_weight_2"] = (planted_volume(), IDENTITY, dict(skip=0.0, min_weight=2.0), (RC.MISS, nan, 17, False))
    v = planted_volume()
    v.W[3, 4, 4] = 0.0  # the cells k = 2, 3 are invalid; the sample on the zero is valid again and the next one hits
    out["hole_before_the_surface"] = (v, IDENTITY, fixed, (RC.HIT, 1.5, 10, False))
    v = planted_volume()
    v.W[4, 4, 4] = 0.0  # the cells k = 3, 4 are invalid: "previous" is reset, and the first valid sample after them is negative
    out["hole_at_the_surface"] = (v, IDENTITY, fixed, (RC.BEHIND, nan, 11, False))
    v = planted_volume()  # the second route: F is NaN in the first planes, then negative, then positive
    v.D[:2], v.D[2], v.D[3:] = np.nan, -0.5, 0.5
    out["behind_second_route"] = (v, IDENTITY, fixed, (RC.BEHIND, nan, 6, False))
    return out


# the step's lower bound along the longest side a volume can have: 1024 x 2 x 2 free voxels and a camera that looks along +x through the
# lattice points (i, 0, 0): 1023 x 16 + 1 samples, under CBA_TSDF_RAY_MAX_SAMPLES.  A volume's longest diagonal is below 1024 sqrt(3)
# voxels, and a step of the depth is at least as long along the ray, so no ray inside a volume takes more than 16 x 1774 samples.
LONG_SHAPE, LONG_POSE, LONG_COUNT = (1024, 2, 2), np.array([0.5, -0.5, -0.5, -0.5, 0, 0, 0]), 1023 * 16 + 1
LONG_INTR = np.array([8.0, 8.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])  # a 1 x 1 view: the ray (0, 0)


def long_volume():
    vol = F.Volume(LONG_SHAPE, np.array([1.0, 0.0, 0.0]), 0.125, 0.5)
    vol.W[:] = 1.0
    return vol


def track_start(name):
    """the pose volume frame -> camera the chain starts from: the inverse of cpu.chain's perturbed start"""
    s = F.scene(name, F.PINHOLE)
    init = F.pose_inverse(s["poses"][cpu.CHAIN[name]["views"]]) + cpu.CHAIN_SHIFT
    return R.pose_inverse(np.concatenate([R.normalise(init[:4]), init[4:]]))


def track_source(name, rays):
    """the held-out depth map as an organised map [H][W][3] on the rays of a table, NaN but for every second pixel of every second row"""
    d = F.scene(name, F.PINHOLE)["depth"][cpu.CHAIN[name]["views"]]
    pts = np.concatenate([rays * d[..., None], d[..., None]], -1)
    pts[0::2], pts[:, 0::2] = np.nan, np.nan
    return pts


def track_ref(name, rays):
    """the restatement's frame-to-model chain over a rays table -> cloud_ref.register's result"""
    s, n = F.scene(name, F.PINHOLE), cpu.CHAIN[name]["views"]
    start = track_start(name)
    res = RC.cast_views(F.fused(name, F.PINHOLE, n), rays, start[None])
    target, normals = RC.cloud(res, 0, start)
    src = track_source(name, rays).reshape(-1, 3)
    src = src[R.valid(src)]
    return R.register(target, normals, src, cpu.CHAIN_MD, metric=0, max_iterations=TRACK_ITERATIONS, step_tolerance=1e-10,
                      init_pose7=R.pose_inverse(start))


def track_truth_error(name, pose7):
    """what cpu.chain_truth_error measures, of a pose camera -> volume frame: the sphere's centre under it against its true place; the
    bumpy surface's rotation (rad) and translation error"""
    view_pose = F.scene(name, F.PINHOLE)["poses"][cpu.CHAIN[name]["views"]]
    if name == "bumpy":
        return R.pose_error(pose7, F.pose_inverse(view_pose))
    in_camera = R.transform(F.rotation(view_pose[:4]), view_pose[4:], F.SPHERE_C)
    back = R.transform(R.rotation(R.normalise(pose7[:4])), pose7[4:], in_camera)
    return float(np.linalg.norm(back - F.SPHERE_C)), 0.0


def truth_error(name, model, res, pose7):
    """-> hits among the truth-finite pixels, those pixels, depth rms and worst in voxels, largest normal angle (rad) of one view's cast"""
    s, n = F.scene(name, model), cpu.CHAIN[name]["views"]
    truth = s["depth"][n]
    both = (res["status"][0] == RC.HIT) & np.isfinite(truth)
    err = np.abs(res["depth"][0][both] - truth[both]) / F.VOXEL
    xyz, nrm = RC.cloud(res, 0, pose7)
    angle = F.surface_error(name, xyz, nrm)[2]
    return int(both.sum()), int(np.isfinite(truth).sum()), float(np.sqrt((err ** 2).mean())), float(err.max()), angle


# ---- the constants the cases are built around ---------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    src = os.path.join(ROOT, "calibration_amd", "csrc")

    def const(name, file):
        return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(src, file)).read()).group(1))

    assert const("TSDF_RAY_WAVE_W", "tsdf_fusion.hip") == RC.WAVE_W and 64 // RC.WAVE_W == RC.WAVE_H
    assert const("TSDF_RAY_MAX_SAMPLES", "tsdf_ray_math.hpp") == RC.MAX_SAMPLES == capi.TSDF_RAY_MAX_SAMPLES
    header = open(os.path.join(ROOT, "include", "calibba.h")).read()
    assert "#define CBA_TSDF_RAY_MAX_SAMPLES %d\n" % RC.MAX_SAMPLES in header and "#define CBA_TSDF_MAX_RAYS (1 << 26)\n" in header
    widths, heights = {v[0] for v in VIEW_SIZES}, {v[1] for v in VIEW_SIZES}
    assert {1, RC.WAVE_W - 1, RC.WAVE_W, RC.WAVE_W + 1, 2 * RC.WAVE_W + 1, 8 * RC.WAVE_W + 1} <= widths  # 65 x 17: 27 tiles, 7 workgroups
    assert {1, RC.WAVE_H, RC.WAVE_H + 1, 2 * RC.WAVE_H + 1} <= heights
    assert LONG_COUNT < RC.MAX_SAMPLES and 16 * 1774 < RC.MAX_SAMPLES


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------
def test_driver_runs_clean_under_sanitizers():
    p = host_build.run_sanitized("raycast_cpu")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "raycast_driver: 0 mismatches" in p.stdout and not p.stderr.strip(), p.stdout + p.stderr


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", size_cases(), ids=lambda c: c[0])
def test_sizes_equal_the_host_build_to_the_bit(host, case):
    vol, model, intr, poses, (H, Wd), opts = size_case(case)
    rays = RC.pixel_rays(model, intr, Wd, H)
    hits = 0
    for m, pose in enumerate(poses):
        ref, got = RC.cast(vol, rays, pose, **opts), RC.host_cast(host, vol, rays, pose, **opts)
        assert same_cast(ref, got, KEYS + ("count",))
        assert ref["count"].max() < 200
        if m == 1:
            assert (ref["status"] == RC.MISS).all() and (ref["count"] == 0).all()  # the view that looks away
        hits += int((ref["status"] == RC.HIT).sum())
        assert np.isnan(ref["depth"][ref["status"] != RC.HIT]).all() and np.isfinite(ref["xyz"][ref["status"] == RC.HIT]).all()
    print(f"{case[0]}: {hits} hits of {len(poses) * H * Wd} rays")
    if case[5]:
        assert hits > 0


def test_rays_without_a_finite_value_have_no_ray(host):
    vol = field((5, 4, 3), 3, True)
    intr, poses = views_for(vol, F.PINHOLE, 7, 5, 1)
    rays = RC.pixel_rays(F.PINHOLE, intr, 7, 5)
    rays[1, 2, 0], rays[3, 4, 1], rays[0, 0, 1] = np.nan, np.inf, -np.inf
    ref, got = RC.cast(vol, rays, poses[0]), RC.host_cast(host, vol, rays, poses[0])
    assert same_cast(ref, got, KEYS + ("count",))
    assert ref["status"][1, 2] == ref["status"][3, 4] == ref["status"][0, 0] == RC.NO_RAY and (ref["status"] == RC.NO_RAY).sum() == 3
    assert np.isnan(ref["xyz"][1, 2]).all() and np.isnan(ref["xyz"][3, 4]).all()


# ---- planted cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(planted_cases()))
def test_planted_cases_by_hand_and_to_the_bit(host, name):
    vol, pose, opts, (status, depth, count, normal) = planted_cases()[name]
    rays = planted_rays()
    assert np.array_equal(rays, RC.pixel_rays(F.PINHOLE, PLANTED_INTR, 9, 9))  # exact, whichever unprojection
    ref, got = RC.cast(vol, rays, pose, **opts), RC.host_cast(host, vol, rays, pose, **opts)
    assert same_cast(ref, got, KEYS + ("count",))
    assert ref["status"][4, 4] == status and (count is None or ref["count"][4, 4] == count)
    assert np.array_equal(ref["depth"][4, 4], depth, equal_nan=True)
    if status == RC.HIT:
        assert np.array_equal(ref["xyz"][4, 4], [0.0, 0.0, depth])
    if normal is not None:
        assert np.array_equal(ref["normals"][4, 4], [0.0, 0.0, -1.0] if normal else [np.nan] * 3, equal_nan=True)
    if name == "axis":
        # the ray of pixel (0, 4) leaves the box where it enters it: z0 == z1 == 1, one sample, a miss; the plane is hit elsewhere
        assert ref["count"][4, 0] == 1 and ref["status"][4, 0] == RC.MISS
        inner = ref["status"][2:7, 2:7]
        assert (inner == RC.HIT).all() and np.abs(ref["depth"][2:7, 2:7] - 1.5).max() < 1e-15
    if name == "camera_inside":
        assert (ref["status"] == RC.HIT).all()


def test_step_at_its_lower_bound_along_the_longest_side(host):
    vol, rays = long_volume(), RC.pixel_rays(F.PINHOLE, LONG_INTR, 1, 1)
    assert np.array_equal(rays, np.zeros((1, 1, 2)))
    opts = dict(step=vol.vs / 16, skip=0.0)
    got = RC.host_cast(host, vol, rays, LONG_POSE, **opts)
    assert got["status"][0, 0] == RC.MISS and got["count"][0, 0] == LONG_COUNT
    ref = RC.cast(vol, rays, LONG_POSE, **opts)
    assert same_cast(ref, got, KEYS + ("count",))


# ---- ground truth and the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RAYCAST_ERROR))
def test_ground_truth_of_the_restatement(host, key):
    name, model = key
    s, n = F.scene(name, model), cpu.CHAIN[name]["views"]
    vol, pose = F.fused(name, model, n), s["poses"][n]
    rays = RC.pixel_rays(model, s["intr"], F.MAP_W, F.MAP_H)
    res = RC.cast_views(vol, rays, pose[None])
    got = RC.host_cast(host, vol, rays, pose)
    assert same_cast({k: res[k][0] for k in res}, got, KEYS + ("count",))
    hit, of, rms, worst, angle = truth_error(name, model, res, pose)
    counts = res["count"][0][res["status"][0] == RC.HIT]
    print(f"{name} model {model}: {hit} of {of} truth pixels hit, depth rms {rms:.4g} voxel, worst {worst:.4g} voxel, largest normal angle "
          f"{angle:.4g} rad, {counts.min()}-{counts.max()} samples per hit ray (mean {counts.mean():.3g})")
    for skip in (0.0, 1.0):
        other = RC.cast_views(vol, rays, pose[None], skip=skip)
        h2, _, r2, w2, a2 = truth_error(name, model, other, pose)
        c2 = other["count"][0][other["status"][0] == RC.HIT]
        print(f"    skip {skip}: {h2} hit, rms {r2:.4g}, worst {w2:.4g}, angle {a2:.4g}, mean {c2.mean():.3g} samples")
    bar = RAYCAST_ERROR[key]
    assert 2 * hit >= of  # the condition: at least half of the truth-finite pixels are hits
    assert rms <= cpu.MARGIN * bar[0] and worst <= cpu.MARGIN * bar[1] and angle <= cpu.MARGIN * bar[2]
    assert rms >= bar[0] / cpu.MARGIN  # the constants are the measurement, not a loose bound


@pytest.mark.parametrize("name", sorted(TRACK))
def test_track_chain_of_the_restatement(name):
    s = F.scene(name, F.PINHOLE)
    ref = track_ref(name, RC.pixel_rays(F.PINHOLE, s["intr"], F.MAP_W, F.MAP_H))
    err = track_truth_error(name, ref["pose7"])
    print(f"track {name}: status {ref['status']}, iterations {ref['iterations']}, pairs {ref['n_pairs']}, gap {ref['gap']:.3g}, against the truth "
          f"{err[0]:.4g}, {err[1]:.4g}")
    assert ref["gap"] >= 1e-9 * cpu.CHAIN_MD ** 2  # the condition under which the GPU tier compares
    assert ref["status"] == R.NOT_CONVERGED and ref["iterations"] == TRACK_ITERATIONS and ref["n_pairs"] > 400
    bar = TRACK[name]
    assert err[0] <= cpu.MARGIN * bar[0] and err[1] <= cpu.MARGIN * bar[1] and err[0] >= bar[0] / cpu.MARGIN


# ---- the package and the library without a device ----------------------------------------------------------------------------------------
def test_package_exports():
    for name in ("RayCast", "RayCastOptions", "track"):
        assert hasattr(cal, name)
    assert capi.TSDF_MAX_RAYS == 1 << 26 and C.sizeof(capi.CbaTsdfRaycastOptions) == 40
    assert (cal.fusion.MISS, cal.fusion.HIT, cal.fusion.BEHIND, cal.fusion.NO_RAY) == (RC.MISS, RC.HIT, RC.BEHIND, RC.NO_RAY)
    o = cal.RayCastOptions()
    assert (o.step, o.skip, o.near_depth, o.far_depth, o.min_weight) == tuple(RC.DEFAULTS[k] for k in ("step", "skip", "near_depth", "far_depth",
                                                                                                          "min_weight"))
    assert np.allclose(cal.fusion.pose_inverse(R.pose_inverse(F.sphere_poses()[2])), F.sphere_poses()[2], atol=1e-15)


def test_cloud_of_a_ray_cast_is_the_restatements():
    vol = field((5, 4, 3), 3, True)
    intr, poses = views_for(vol, F.PINHOLE, 17, 9, 2)
    res = RC.cast_views(vol, RC.pixel_rays(F.PINHOLE, intr, 17, 9), poses)
    cast = cal.RayCast(res["depth"], res["xyz"], res["normals"], res["status"], None)
    xyz, nrm = cast.cloud(0, poses[0])
    rx, rn = RC.cloud(res, 0, poses[0])
    assert len(xyz) == cast.hits[0].sum() > 20 and np.allclose(xyz, rx, atol=1e-14) and np.allclose(nrm, rn, atol=1e-14, equal_nan=True)
    assert cast.cloud(1, poses[1])[0].shape == (0, 3)
    # the hits lie inside the volume's box
    hi = vol.origin + (np.array(vol.shape) - 1) * vol.vs
    assert (xyz >= vol.origin - 1e-12).all() and (xyz <= hi + 1e-12).all()


def test_argument_errors_come_before_the_device(lib):
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    o = capi.CbaTsdfRaycastOptions()
    lib.cba_tsdf_raycast_options_default(C.byref(o))
    assert (o.step, o.skip, o.near_depth, o.far_depth, o.min_weight) == (0.0, 0.5, 0.0, np.inf, 1.0)
    lib.cba_tsdf_raycast_options_default(None)
    k, p = np.array(F.CAMERAS[F.PINHOLE]), np.ascontiguousarray(IDENTITY)
    assert lib.cba_tsdf_raycast(None, 0, dptr(k), 1, 4, 4, dptr(p), None) == bad and b"null" in lib.cba_last_error()
    assert lib.cba_tsdf_raycast(None, 0, dptr(k), 0, 4, 4, dptr(None), C.byref(o)) == bad
    assert lib.cba_tsdf_raycast_fetch(None, dptr(None), dptr(None), dptr(None), capi.u8ptr(None), dptr(None)) == bad
