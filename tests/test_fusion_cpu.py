"""CPU tier of scan fusion (cba_tsdf_volume, cba_tsdf_integrate, cba_tsdf_extract): the numpy restatement (tests/fusion_ref.py)
against the host build of tsdf_math.hpp (tests/fusion_cpu) to the bit at every size and planted case of the GPU tier (which imports
the cases from here), the planted cases against what the rule gives by hand, ground truth on rendered scenes, the condition under
which the GPU tier compares the chain's solve, the stand-alone driver under the sanitizers, and what the library checks before it
asks for a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.capi import dptr
from tests import camera_ref as CR
from tests import cloud_ref as R
from tests import fusion_ref as F
from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Ground truth, measured on the restatement: SHAPE = 32 x 28 x 24 voxels of 1/16, truncation four voxels, views of 80 x 60 (six of the
# sphere, five of the bumpy surface; one more of each is held out), (scene, model) -> the rms and the largest distance of the
# extracted points from the true surface in voxels, and the largest angle in rad between an extracted normal and the true one.  The
# sphere's largest errors sit at grazing silhouette pixels under nearest-pixel sampling (a numpy prototype of the rule on a like scene
# gave rms 0.22 and 1.13: these agree); the bumpy surface is seen from above, without silhouettes.  The figures are the measured
# values rounded up in their fourth digit; the bars are these times 1.25, and the device, which must give the restatement's bits,
# needs no wider ones.
SURFACE_ERROR = {("sphere", F.PINHOLE): (0.2617, 1.120, 0.8336), ("sphere", F.SCHEIMPFLUG): (0.2517, 1.117, 0.8026),
                 ("bumpy", F.PINHOLE): (0.02137, 0.09598, 0.08537), ("bumpy", F.SCHEIMPFLUG): (0.02045, 0.1139, 0.1008)}
MARGIN = 1.25

# The chain: the held-out view of a scene registered onto the model fused from the others, point to plane, from the true pose plus
# CHAIN_SHIFT.  A sphere leaves the rotation about its centre unobservable, so its solve wanders and ends at the cap (10 updates bound
# the wandering); what it does determine is where the centre goes.  The bumpy surface holds all six freedoms and converges.
# views: the fused ones (the next is held out).  truth: measured on the restatement and rounded up in the fourth digit - the sphere's
# centre under the returned pose against its true place; the bumpy surface's rotation (rad) and translation error (0.0035 is 0.06 voxel).
CHAIN_MD = 2 * F.VOXEL
CHAIN_SHIFT = np.array([0.0, 0.004, -0.003, 0.005, 0.02, -0.015, 0.01])
CHAIN = {"sphere": dict(views=6, max_iterations=10, truth=(0.01368, 0.0)), "bumpy": dict(views=5, max_iterations=60, truth=(0.0008589, 0.003455))}
SPHERE_VIEWS = CHAIN["sphere"]["views"]


@pytest.fixture(scope="module")
def host():
    return host_build.load("fusion_cpu")


def same(a, b):
    """equal bits (NaNs included)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- cases shared with the GPU tier ------------------------------------------------------------------------------------------------------
def generic_volume(shape, **kw):
    return F.Volume(shape, F.GENERIC_ORIGIN, F.GENERIC_VOXEL, 3 * F.GENERIC_VOXEL, **kw)


def size_cases():
    """(name, shape, model, n_maps): the lane's ownership and the wave along x, the workgroup's share, the extract tile"""
    out = [("nx%d" % s[0], s, F.PINHOLE if k % 2 == 0 else F.SCHEIMPFLUG, 2) for k, s in enumerate(F.NX_SIZES)]
    out += [("block%dx%dx%d" % s, s, F.SCHEIMPFLUG if k % 2 == 0 else F.PINHOLE, 2) for k, s in enumerate(F.BLOCK_SIZES)]
    out += [("maps%d" % n, (65, 3, 2), F.PINHOLE, n) for n in (0, 1, 7)]
    return out


def planted_update():
    """A pinhole with power-of-two intrinsics over a power-of-two lattice: on the plane k = 1 (z = 1) voxel i projects to
    u = i / 2 - 0.5 exactly and row j to v = 0.5, 1, 1.5, so px = 0 0 1 1 2 2 3 3 4 4 (4 is outside) and py = 1 1 2.
    -> volume arguments, intr, the depth map [3][4], the identity pose"""
    args = dict(shape=(10, 3, 3), origin=np.array([-0.125, -0.03125, 0.96875]), voxel_size=0.03125, truncation=0.25, max_weight=3.0, max_depth=4.0)
    intr = np.array([16.0, 16.0, 1.5, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    depth = np.array([[9.0, 9.0, 9.0, 9.0],
                      [0.75, np.nextafter(0.75, 0.0), 1.5, 5.0],  # s = -truncation: kept; the next below: skipped; s >= truncation; beyond max_depth
                      [1.125, 1.0, 0.875, 1.25]])
    return args, intr, depth, np.array([1.0, 0, 0, 0, 0, 0, 0])


def check_planted_update(D, W, n_maps):
    """the planes after n_maps >= 1 copies of the planted map, by hand"""
    w = float(min(n_maps, 3))
    assert np.array_equal(W[1, 0], [w, w, 0, 0, w, w, 0, 0, 0, 0]) and np.array_equal(W[1, 1], W[1, 0])
    assert np.array_equal(D[1, 0], [-1, -1, 1, 1, 1, 1, 1, 1, 1, 1]) and np.array_equal(D[1, 1], D[1, 0])
    assert np.array_equal(W[1, 2], [w, w, w, w, w, w, w, w, 0, 0])
    assert np.array_equal(D[1, 2], [0.5, 0.5, 0, 0, -0.5, -0.5, 1, 1, 1, 1])


def planted_fields():
    """name -> (shape, D, W, min_weight, expected count or None): planes for upload"""
    out = {}
    one = np.ones((2, 2, 2), np.float32)
    D, W = one.copy(), np.zeros_like(one)
    D[0, 0, 0], D[0, 0, 1], W[0, 0, 0], W[0, 0, 1] = -0.5, 0.5, 1, 1
    out["one_crossing_no_normal"] = ((2, 2, 2), D, W, 1.0, 1)
    out["below_min_weight"] = ((2, 2, 2), D, W, 2.0, 0)
    D2 = D.copy()
    D2[0, 0, 0], D2[0, 0, 1] = 0.0, -0.5
    out["zero_against_negative"] = ((2, 2, 2), D2, W, 1.0, 1)
    D3 = D2.copy()
    D3[0, 0, 0] = np.float32(-0.0)
    out["minus_zero_against_negative"] = ((2, 2, 2), D3, W, 1.0, 1)
    D4 = D3.copy()
    D4[0, 0, 1] = 0.5
    out["minus_zero_against_positive"] = ((2, 2, 2), D4, W, 1.0, 0)
    # 32 x 8 x 5: l = 1023 is voxel (31, 7, 3), the last of tile 0, whose only edge is +z; l = 1024 is (0, 0, 4), the first of tile 1
    shape = (32, 8, 5)
    D, W = np.full((5, 8, 32), 0.5, np.float32), np.full((5, 8, 32), 2.0, np.float32)
    D[3, 7, 31], D[4, 0, 0] = -0.25, -0.75
    W[3, 7, 30] = 1.0
    out["tile_edge"] = (shape, D, W, 1.0, 7)
    out["tile_edge_min_weight_2"] = (shape, D, W, 2.0, 6)  # (30, 7, 3) has W = 1: its +x edge goes
    # one interior crossing with every neighbour observed but one
    D, W = np.full((5, 8, 32), 0.5, np.float32), np.ones((5, 8, 32), np.float32)
    D[2, 3, 10:] = -0.5
    D[1, 3, 10:] = -0.25
    W[2, 4, 20] = 0.0
    out["missing_neighbour"] = (shape, D, W, 1.0, None)
    for k, s in enumerate(F.NX_SIZES + F.BLOCK_SIZES + [shape]):
        Dr, Wr = F.random_field(s, 50 + k)
        out["random%dx%dx%d" % s] = (s, Dr, Wr, 1.0, None)
        out["random%dx%dx%d_w2" % s] = (s, Dr, Wr, 2.0, None)
    return out


def field_volume(shape, D, W):
    v = F.Volume(shape, np.array([0.25, -0.5, 1.0]), 0.125, 0.5)
    v.D, v.W = D.copy(), W.copy()
    return v


def flat_field():
    """FLAT_SHAPE with a sparse random field: observed voxels in pairs along x, a twentieth of the volume"""
    nx, ny, nz = F.FLAT_SHAPE
    rng = np.random.default_rng(7)
    D = (rng.integers(-8, 9, (nz, ny, nx)) / 8.0).astype(np.float32)
    seen = rng.random((nz, ny, nx)) < 0.025
    seen[:, :, 1:] |= seen[:, :, :-1]
    return D, seen.astype(np.float32)


_chain = {}


def chain(name):
    """the chain's scene and the restatement's solve, computed once: target points and normals, the source, the initial pose, the
    truth, cloud_ref.register's result"""
    if name not in _chain:
        s, n = F.scene(name, F.PINHOLE), CHAIN[name]["views"]
        xyz, nrm = F.fused(name, F.PINHOLE, n).extract()
        src = F.camera_points(F.PINHOLE, s["intr"], s["depth"][n]).reshape(-1, 3)
        src = src[R.valid(src)]
        truth = F.pose_inverse(s["poses"][n])
        init = truth + CHAIN_SHIFT
        ref = R.register(xyz, nrm, src, CHAIN_MD, metric=0, max_iterations=CHAIN[name]["max_iterations"], step_tolerance=1e-10, init_pose7=init)
        _chain[name] = dict(target=xyz, normals=nrm, source=src, init=init, truth=truth, ref=ref, view_pose=s["poses"][n])
    return _chain[name]


def chain_truth_error(name, pose7):
    """what CHAIN[name]['truth'] bounds, of a returned pose"""
    c = chain(name)
    if name == "bumpy":
        return R.pose_error(pose7, c["truth"])
    in_camera = R.transform(F.rotation(c["view_pose"][:4]), c["view_pose"][4:], F.SPHERE_C)
    back = R.transform(R.rotation(R.normalise(pose7[:4])), pose7[4:], in_camera)
    return float(np.linalg.norm(back - F.SPHERE_C)), 0.0


# ---- the constants the cases are built around ---------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    src = os.path.join(ROOT, "calibration_amd", "csrc")
    def const(name, file):
        return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(src, file)).read()).group(1))
    assert const("TSDF_BLOCK", "tsdf_fusion.hip") == F.INTEGRATE_BLOCK
    assert const("TSDF_EXTRACT_TILE", "tsdf_math.hpp") == F.EXTRACT_TILE
    assert const("SCAN_TILE", "scan_tiles.hpp") == F.SCAN_TILE == R.SCAN_TILE
    pairs = [((s[0] + 1) // 2) * s[1] * s[2] for s in F.BLOCK_SIZES]
    voxels = [s[0] * s[1] * s[2] for s in F.BLOCK_SIZES]
    assert {F.INTEGRATE_BLOCK - 1, F.INTEGRATE_BLOCK, F.INTEGRATE_BLOCK + 2} <= set(pairs)
    assert {F.EXTRACT_TILE - 1, F.EXTRACT_TILE, F.EXTRACT_TILE + 1} <= set(voxels)
    nx, ny, nz = F.FLAT_SHAPE
    assert nx * ny * nz // F.EXTRACT_TILE > F.SCAN_TILE


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------
def test_driver_runs_clean_under_sanitizers():
    p = host_build.run_sanitized("fusion_cpu")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "fusion_driver: 0 mismatches" in p.stdout and not p.stderr.strip(), p.stdout + p.stderr


# ---- the projection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [F.PINHOLE, F.SCHEIMPFLUG])
def test_projection_agrees_with_the_reference_order(model):
    P = CR.points(500, seed=3)
    u, v = F.project(model, F.CAMERAS[model], P[:, 0], P[:, 1], P[:, 2])
    uv = CR.project(model, F.CAMERAS[model], P)
    assert np.abs(u - uv[:, 0]).max() < 1e-9 and np.abs(v - uv[:, 1]).max() < 1e-9
    if model == F.SCHEIMPFLUG:
        Rs, _ = F.sensor_consts(F.CAMERAS[model])
        assert np.allclose(np.array(Rs).reshape(3, 3), CR.rot_sensor(*F.CAMERAS[model][10:]), atol=1e-15)


# ---- integrate -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", size_cases(), ids=lambda c: c[0])
def test_integrate_and_extract_equal_the_host_build_to_the_bit(host, case):
    _, shape, model, n_maps = case
    intr, depth, poses = F.generic_views(model, n_maps, seed=shape[0])
    vol = generic_volume(shape)
    D, W = F.host_integrate(host, vol, model, intr, depth, poses)
    vol.integrate(model, intr, depth, poses)
    assert same(D, vol.D) and same(W, vol.W)
    assert (vol.W > 0).any() == (n_maps > 0)
    xyz, nrm = vol.extract()
    hx, hn = F.host_extract(host, vol)
    assert same(xyz, hx) and same(nrm, hn)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5)], ids=["1x1", "7x5"])
def test_small_and_odd_maps_and_an_all_nan_map_in_the_batch(host, shape):
    Wd, H = shape
    intr, depth, poses = F.generic_views(F.PINHOLE, 3, W=Wd, H=H, seed=5)
    depth[1] = np.nan
    vol = generic_volume((65, 3, 2))
    D, W = F.host_integrate(host, vol, F.PINHOLE, intr, depth, poses)
    vol.integrate(F.PINHOLE, intr, depth, poses)
    assert same(D, vol.D) and same(W, vol.W) and (vol.W > 0).any()
    two = generic_volume((65, 3, 2)).integrate(F.PINHOLE, intr, depth[[0, 2]], poses[[0, 2]])
    assert same(two.D, vol.D) and same(two.W, vol.W)  # the all-NaN map changes nothing


def test_batch_independence_of_the_restatement_and_the_host_build(host):
    intr, depth, poses = F.generic_views(F.SCHEIMPFLUG, 7, seed=2)
    one = generic_volume((65, 3, 2)).integrate(F.SCHEIMPFLUG, intr, depth, poses)
    each = generic_volume((65, 3, 2))
    hv = generic_volume((65, 3, 2))
    for m in range(7):
        each.integrate(F.SCHEIMPFLUG, intr, depth[m], poses[m])
        hv.D, hv.W = F.host_integrate(host, hv, F.SCHEIMPFLUG, intr, depth[m], poses[m])
    assert same(one.D, each.D) and same(one.W, each.W) and same(one.D, hv.D) and same(one.W, hv.W)
    assert one.W.max() == 7


@pytest.mark.parametrize("n_maps", [1, 2, 5])
def test_planted_update_decisions(host, n_maps):
    args, intr, depth, pose = planted_update()
    vol = F.Volume(**args)
    maps, poses = np.tile(depth, (n_maps, 1, 1)), np.tile(pose, (n_maps, 1))
    D, W = F.host_integrate(host, vol, F.PINHOLE, intr, maps, poses)
    vol.integrate(F.PINHOLE, intr, maps, poses)
    assert same(D, vol.D) and same(W, vol.W)
    check_planted_update(vol.D, vol.W, n_maps)
    # a camera one unit further along z: the planes z <= 1 have P_2 <= 0 and stay; on z = 33 / 32 voxel (4, 1) sees pixel (2, 1)
    behind = F.Volume(**args).integrate(F.PINHOLE, intr, depth, np.array([1.0, 0, 0, 0, 0, 0, -1.0]))
    assert (behind.W[:2] == 0).all() and behind.W[2, 1, 4] == 1 and behind.D[2, 1, 4] == 1
    Db, Wb = F.host_integrate(host, F.Volume(**args), F.PINHOLE, intr, depth, np.array([1.0, 0, 0, 0, 0, 0, -1.0]))
    assert same(Db, behind.D) and same(Wb, behind.W)


@pytest.mark.parametrize("tilt", [(0.03, -0.02), (0.9, -0.8)])
def test_scheimpflug_with_a_non_positive_denominator(host, tilt):
    intr, depth, poses = F.generic_views(F.SCHEIMPFLUG, 2, seed=4)
    intr[10:] = tilt
    vol = generic_volume((65, 5, 3))
    X = np.meshgrid(vol.axes[2], vol.axes[1], vol.axes[0], indexing="ij")
    Rm, t = F.rotation(poses[0, :4]), poses[0, 4:]
    P = [((Rm[r, 0] * X[2] + Rm[r, 1] * X[1]) + Rm[r, 2] * X[0]) + t[r] for r in range(3)]
    behind = (P[2] > 0) & ~(F.denominator(F.SCHEIMPFLUG, intr, *P) > 0)
    assert behind.any() == (tilt[0] > 0.5)  # the steep tilt puts voxels in front of the camera behind the sensor's plane
    D, W = F.host_integrate(host, vol, F.SCHEIMPFLUG, intr, depth, poses)
    vol.integrate(F.SCHEIMPFLUG, intr, depth, poses)
    assert same(D, vol.D) and same(W, vol.W)


# ---- extract -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(planted_fields()))
def test_planted_fields_equal_the_host_build_to_the_bit(host, name):
    shape, D, W, min_weight, count = planted_fields()[name]
    vol = field_volume(shape, D, W)
    xyz, nrm = vol.extract(min_weight)
    hx, hn = F.host_extract(host, vol, min_weight)
    assert same(xyz, hx) and same(nrm, hn)
    if count is not None:
        assert len(xyz) == count
    if name.startswith("random32"):
        assert len(xyz) > 100 and 0 < np.isnan(nrm[:, 0]).sum() < len(xyz)


def test_planted_fields_by_hand():
    f = planted_fields()
    xyz, nrm = field_volume(*f["one_crossing_no_normal"][:3]).extract()
    assert np.array_equal(xyz, [[0.25 + 0.5 * 0.125, -0.5, 1.0]]) and np.isnan(nrm).all()
    for name in ("zero_against_negative", "minus_zero_against_negative"):  # t = 0 (or -0): the point is the voxel
        xyz, _ = field_volume(*f[name][:3]).extract()
        assert np.array_equal(xyz, [[0.25, -0.5, 1.0]])
    # the tile edge: voxel (31, 7, 3) is negative among positives, as is (0, 0, 4); in visiting order
    shape, D, W, _, _ = f["tile_edge"]
    v = field_volume(shape, D, W)
    xyz, _ = v.extract()
    at = lambda i, j, k: np.array([v.axes[0][i], v.axes[1][j], v.axes[2][k]])
    want = [at(31, 7, 2) + [0, 0, 0.125 * (0.5 / 0.75)], at(31, 6, 3) + [0, 0.125 * (0.5 / 0.75), 0], at(30, 7, 3) + [0.125 * (0.5 / 0.75), 0, 0],
            at(31, 7, 3) + [0, 0, 0.125 * (0.25 / 0.75)]]
    order = [(31, 7, 2), (0, 0, 3), (31, 6, 3), (30, 7, 3), (31, 7, 3), (0, 0, 4), (0, 0, 4)]
    assert len(xyz) == len(order)
    assert np.allclose(xyz[0], want[0]) and np.allclose(xyz[2], want[1]) and np.allclose(xyz[3], want[2]) and np.allclose(xyz[4], want[3])
    assert len(v.extract(2.0)[0]) == len(order) - 1  # (30, 7, 3) has W = 1
    # the missing neighbour: with (20, 4, 2) unobserved its own crossing goes, and edges beside it keep their point without a normal
    shape, D, W, _, _ = f["missing_neighbour"]
    xyz, nrm = field_volume(shape, D, W).extract()
    full = W.copy()
    full[2, 4, 20] = 1.0
    xyz_full, nrm_full = field_volume(shape, D, full).extract()
    assert len(xyz) == len(xyz_full) - 1 and np.isnan(nrm[:, 0]).sum() > np.isnan(nrm_full[:, 0]).sum() - 1
    assert (~np.isnan(nrm_full[:, 0])).any()


def test_flat_volume_extraction_equals_the_host_build(host):
    D, W = flat_field()
    vol = field_volume(F.FLAT_SHAPE, D, W)
    xyz, nrm = vol.extract()
    hx, hn = F.host_extract(host, vol)
    assert same(xyz, hx) and same(nrm, hn)
    tiles = (np.floor((xyz[:, 1] + 0.5) / 0.125 + 0.5) * 1024 + np.floor((xyz[:, 2] - 1.0) / 0.125 + 0.5) * 1024 * 1024) // F.EXTRACT_TILE
    assert tiles.max() >= F.SCAN_TILE + 1 and len(xyz) > 1000  # crossings in tiles past the scan's first level


# ---- ground truth and the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(SURFACE_ERROR))
def test_ground_truth_of_the_restatement(key):
    name, model = key
    xyz, nrm = F.fused(name, model, CHAIN[name]["views"]).extract()
    rms, worst, angle = F.surface_error(name, xyz, nrm)
    print(f"{name} model {model}: {len(xyz)} points, {int((~np.isnan(nrm[:, 0])).sum())} normals, rms {rms:.4g} voxel, largest {worst:.4g} voxel, "
          f"largest normal angle {angle:.4g} rad")
    bar = SURFACE_ERROR[key]
    assert len(xyz) > 500 and rms <= MARGIN * bar[0] and worst <= MARGIN * bar[1] and angle <= MARGIN * bar[2]
    assert rms >= bar[0] / MARGIN  # the constants are the measurement, not a loose bound


def test_xyz_maps_give_the_depth_maps():
    s = F.scene("sphere", F.PINHOLE)
    pts = F.camera_points(F.PINHOLE, s["intr"], s["depth"][0])
    assert np.array_equal(F.depth_from_xyz(pts), s["depth"][0], equal_nan=True)
    pts[3, 4, 0] = np.inf
    assert np.isnan(F.depth_from_xyz(pts)[3, 4])
    assert np.array_equal(cal.depth_from_xyz(pts), F.depth_from_xyz(pts), equal_nan=True)


@pytest.mark.parametrize("name", sorted(CHAIN))
def test_chain_solve_of_the_restatement(name):
    c = chain(name)
    ref = c["ref"]
    err = chain_truth_error(name, ref["pose7"])
    print(f"chain {name}: {len(c['target'])} target points, {len(c['source'])} source points, status {ref['status']}, iterations "
          f"{ref['iterations']}, pairs {ref['n_pairs']}, gap {ref['gap']:.3g}, against the truth {err[0]:.4g}, {err[1]:.4g}")
    assert ref["gap"] >= 1e-9 * CHAIN_MD ** 2  # the condition under which the GPU tier compares
    assert ref["status"] == (R.OK if name == "bumpy" else R.NOT_CONVERGED) and ref["n_pairs"] > 1000
    bar = CHAIN[name]["truth"]
    assert err[0] <= MARGIN * bar[0] and err[1] <= MARGIN * bar[1] and err[0] >= bar[0] / MARGIN


# ---- the package and the library without a device ----------------------------------------------------------------------------------------
def test_package_exports():
    for name in ("TsdfOptions", "TsdfVolume", "fuse", "depth_from_xyz"):
        assert hasattr(cal, name)
    assert capi.TSDF_MAX_VOXELS == 1 << 28 and C.sizeof(capi.CbaTsdfOptions) == 32


def test_argument_errors_come_before_the_device(lib):
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    o = capi.CbaTsdfOptions()
    lib.cba_tsdf_options_default(C.byref(o))
    assert (o.voxel_size, o.truncation, o.max_weight, o.max_depth) == (0.0, 0.0, 64.0, np.inf)
    h = C.c_void_p()
    origin = np.zeros(3)

    def create(nx=8, ny=8, nz=8, org=origin, out=True, **kw):
        c = capi.CbaTsdfOptions(0.1, 0.3, 64.0, np.inf)
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.cba_tsdf_volume_create(nx, ny, nz, dptr(org), C.byref(c), 0, C.byref(h) if out else None)

    assert create(out=False) == bad and create(org=None) == bad
    assert lib.cba_tsdf_volume_create(8, 8, 8, dptr(origin), None, 0, C.byref(h)) == bad
    for sides in ((1, 8, 8), (8, 1025, 8), (8, 8, 0), (1024, 1024, 512)):
        assert create(*sides) == bad
    assert b"2^28" in lib.cba_last_error()
    for org in (np.array([0.0, np.nan, 0.0]), np.array([np.inf, 0.0, 0.0])):
        assert create(org=org) == bad and b"origin" in lib.cba_last_error()
    for kw in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=np.nan), dict(voxel_size=np.inf)):
        assert create(**kw) == bad and b"voxel_size" in lib.cba_last_error()
    for kw in (dict(truncation=0.0), dict(truncation=np.nan), dict(truncation=np.inf)):
        assert create(**kw) == bad and b"truncation" in lib.cba_last_error()
    for kw in (dict(max_weight=0.0), dict(max_weight=2.5), dict(max_weight=2.0 ** 24 + 2), dict(max_weight=np.nan)):
        assert create(**kw) == bad and b"max_weight" in lib.cba_last_error()
    for kw in (dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=np.nan)):
        assert create(**kw) == bad and b"max_depth" in lib.cba_last_error()
    assert not h.value
    # every call on a handle refuses NULL
    n = np.zeros(1, np.int64)
    k = np.array(F.CAMERAS[F.PINHOLE])
    assert lib.cba_tsdf_integrate(None, 0, dptr(k), 0, 4, 4, dptr(None), dptr(None)) == bad
    assert lib.cba_tsdf_fetch(None, None, None) == bad and lib.cba_tsdf_upload(None, None, None) == bad and lib.cba_tsdf_reset(None) == bad
    assert lib.cba_tsdf_extract(None, 1.0, capi.i64ptr(n)) == bad and lib.cba_tsdf_extract_fetch(None, dptr(None), dptr(None)) == bad
    lib.cba_tsdf_volume_destroy(None)
    # with everything in order the answer is the device's: a handle, or CBA_ERR_NO_DEVICE where there is none
    st = create()
    if lib.cba_device_count() > 0:
        assert st == capi.CBA_OK and h.value
        lib.cba_tsdf_volume_destroy(h)
    else:
        assert st == capi.CBA_ERR_NO_DEVICE and not h.value
