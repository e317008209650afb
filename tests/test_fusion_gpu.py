"""GPU tier of scan fusion (cba_tsdf_volume, cba_tsdf_integrate, cba_tsdf_extract) through the Python layer: D, W, the point count,
the points and the normals of the device against the numpy restatement (tests/fusion_ref.py) and the host build of tsdf_math.hpp, to
the bit, at the sizes where a kernel changes path (nx around the lane's two voxels and the wave, pairs around the workgroup's 256,
voxels around the extract tile of 1024, a flat volume whose tile counts need the scan's second level), map shapes and batch counts,
batch independence and repeatability, the planted update and extraction decisions, both camera models, the chain into registration,
and the argument errors that need a live handle.  The cases are those of tests/test_fusion_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.fusion import TsdfOptions, TsdfVolume, fuse
from calibration_amd.registration import CloudIndex, IcpOptions, default_cell_size
from tests import cloud_ref as R
from tests import fusion_ref as F
from tests import host_build
from tests import test_fusion_cpu as cpu
from tests.test_fusion_cpu import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return host_build.load("fusion_cpu")


def device_volume(ref):
    """a device volume with the arguments of a restatement's Volume"""
    return TsdfVolume(ref.shape, ref.origin, TsdfOptions(float(ref.vs), float(ref.trunc), float(ref.max_weight), float(ref.max_depth)))


def assert_volume(vol, ref):
    D, W = vol.fetch()
    assert same(D, ref.D) and same(W, ref.W)


def assert_extract(vol, ref, host, min_weight=1.0):
    xyz, nrm = vol.extract(min_weight)
    rx, rn = ref.extract(min_weight)
    assert len(xyz) == len(rx) and same(xyz, rx) and same(nrm, rn)
    hx, hn = F.host_extract(host, ref, min_weight)
    assert same(xyz, hx) and same(nrm, hn)
    return xyz, nrm


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cpu.size_cases(), ids=lambda c: c[0])
def test_sizes_equal_restatement_and_host_build_to_the_bit(gpu_lib, host, case):
    _, shape, model, n_maps = case
    intr, depth, poses = F.generic_views(model, n_maps, seed=shape[0])
    ref = cpu.generic_volume(shape)
    hD, hW = F.host_integrate(host, ref, model, intr, depth, poses)
    ref.integrate(model, intr, depth, poses)
    with device_volume(ref) as vol:
        vol.integrate(model, intr, poses, depth=depth)
        assert_volume(vol, ref)
        D, W = vol.fetch()
        assert same(D, hD) and same(W, hW)
        assert_extract(vol, ref, host)
        assert_extract(vol, ref, host)  # again: the same bits, the buffers reused


def test_flat_volume_needs_the_second_scan_level(gpu_lib, host):
    intr, depth, poses = F.generic_views(F.PINHOLE, 1, seed=9)
    ref = cpu.generic_volume(F.FLAT_SHAPE).integrate(F.PINHOLE, intr, depth, poses)
    with device_volume(ref) as vol:
        vol.integrate(F.PINHOLE, intr, poses, depth=depth)
        assert_volume(vol, ref)
        assert (ref.W > 0).sum() > 100
        xyz, nrm = vol.extract()
        rx, rn = ref.extract()
        assert same(xyz, rx) and same(nrm, rn)
        # crossings in tiles past the scan's first level: a sparse random field, uploaded
        D, W = cpu.flat_field()
        field = cpu.field_volume(F.FLAT_SHAPE, D, W)
    with device_volume(field) as vol:
        vol.upload(D, W)
        assert_volume(vol, field)
        xyz, nrm = vol.extract()
        rx, rn = field.extract()
        assert len(xyz) == len(rx) > 1000 and same(xyz, rx) and same(nrm, rn)


# ---- maps and batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 5)], ids=["1x1", "7x5"])
def test_small_and_odd_maps_and_an_all_nan_map_in_the_batch(gpu_lib, shape):
    Wd, H = shape
    intr, depth, poses = F.generic_views(F.PINHOLE, 3, W=Wd, H=H, seed=5)
    depth[1] = np.nan
    ref = cpu.generic_volume((65, 3, 2)).integrate(F.PINHOLE, intr, depth, poses)
    with device_volume(ref) as vol:
        vol.integrate(F.PINHOLE, intr, poses, depth=depth)
        assert_volume(vol, ref)
        assert (ref.W > 0).any()


@pytest.mark.parametrize("model", [F.PINHOLE, F.SCHEIMPFLUG])
def test_batch_independence_and_repeatability(gpu_lib, model):
    intr, depth, poses = F.generic_views(model, 7, seed=2)
    ref = cpu.generic_volume((65, 3, 2)).integrate(model, intr, depth, poses)
    with device_volume(ref) as one, device_volume(ref) as each, device_volume(ref) as split:
        one.integrate(model, intr, poses, depth=depth)
        for m in range(7):
            each.integrate(model, intr, poses[m], depth=depth[m])
        split.integrate(model, intr, poses[:2], depth=depth[:2])
        split.integrate(model, intr, poses[2:], depth=depth[2:])
        for vol in (one, each, split):
            assert_volume(vol, ref)
        one.reset()
        assert same(one.fetch()[0], np.ones_like(ref.D)) and same(one.fetch()[1], np.zeros_like(ref.W))
        one.integrate(model, intr, poses, depth=depth)  # a repeated run gives equal bits
        assert_volume(one, ref)
        assert ref.W.max() == 7
        one.integrate(model, intr, np.zeros((0, 7)), depth=np.zeros((0, 9, 33)))  # n_maps == 0: no work
        assert_volume(one, ref)


def test_xyz_maps_and_the_facade(gpu_lib):
    s = F.scene("sphere", F.PINHOLE)
    n = cpu.SPHERE_VIEWS
    ref = F.fused("sphere", F.PINHOLE, n)
    maps = np.stack([F.camera_points(F.PINHOLE, s["intr"], d) for d in s["depth"][:n]])
    maps[0, 3, 4, 0] = np.inf  # a pixel with a non-finite coordinate is invalid: that pixel was a miss anyway
    assert np.isnan(s["depth"][0, 3, 4])
    xyz, nrm = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), F.PINHOLE, s["intr"], s["poses"][:n], xyz=maps)
    rx, rn = ref.extract()
    assert same(xyz, rx) and same(nrm, rn)


# ---- planted update decisions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_maps", [1, 2, 5])
def test_planted_update_decisions(gpu_lib, n_maps):
    args, intr, depth, pose = cpu.planted_update()
    ref = F.Volume(**args)
    maps, poses = np.tile(depth, (n_maps, 1, 1)), np.tile(pose, (n_maps, 1))
    ref.integrate(F.PINHOLE, intr, maps, poses)
    with device_volume(ref) as vol:
        vol.integrate(F.PINHOLE, intr, poses, depth=maps)
        assert_volume(vol, ref)
        cpu.check_planted_update(*vol.fetch(), n_maps)  # u = k + 0.5 up, -0.5 in, width - 0.5 out, s = -truncation kept, f = 1, max_depth, max_weight
        vol.reset()
        D, W = vol.fetch()
        assert (D == 1).all() and (W == 0).all()
        # P_2 <= 0: a camera one unit further along z
        behind = F.Volume(**args).integrate(F.PINHOLE, intr, depth, np.array([1.0, 0, 0, 0, 0, 0, -1.0]))
        vol.integrate(F.PINHOLE, intr, np.array([1.0, 0, 0, 0, 0, 0, -1.0]), depth=depth)
        assert_volume(vol, behind)
        assert (vol.fetch()[1][:2] == 0).all() and vol.fetch()[1][2, 1, 4] == 1


@pytest.mark.parametrize("tilt", [(0.03, -0.02), (0.9, -0.8)])
def test_scheimpflug_with_a_non_positive_denominator(gpu_lib, tilt):
    intr, depth, poses = F.generic_views(F.SCHEIMPFLUG, 2, seed=4)
    intr[10:] = tilt
    ref = cpu.generic_volume((65, 5, 3)).integrate(F.SCHEIMPFLUG, intr, depth, poses)
    with device_volume(ref) as vol:
        vol.integrate(F.SCHEIMPFLUG, intr, poses, depth=depth)
        assert_volume(vol, ref)


@pytest.mark.parametrize("name", ["sphere", "bumpy"])
@pytest.mark.parametrize("model", [F.PINHOLE, F.SCHEIMPFLUG])
def test_scenes_with_distortion_and_ground_truth(gpu_lib, host, name, model):
    s, n = F.scene(name, model), cpu.CHAIN[name]["views"]
    ref = F.fused(name, model, n)
    with device_volume(ref) as vol:
        vol.integrate(model, s["intr"], s["poses"][:n], depth=s["depth"][:n])
        assert_volume(vol, ref)
        xyz, nrm = assert_extract(vol, ref, host)
    rms, worst, angle = F.surface_error(name, xyz, nrm)
    bar = cpu.SURFACE_ERROR[(name, model)]
    assert rms <= cpu.MARGIN * bar[0] and worst <= cpu.MARGIN * bar[1] and angle <= cpu.MARGIN * bar[2]


# ---- planted extraction cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cpu.planted_fields()))
def test_planted_fields(gpu_lib, host, name):
    shape, D, W, min_weight, count = cpu.planted_fields()[name]
    ref = cpu.field_volume(shape, D, W)
    with device_volume(ref) as vol:
        vol.upload(D, W)
        assert_volume(vol, ref)
        xyz, nrm = assert_extract(vol, ref, host, min_weight)
        if count is not None:
            assert len(xyz) == count
        if count == 0:
            assert xyz.shape == (0, 3) and nrm.shape == (0, 3)
        if name == "one_crossing_no_normal":
            assert np.isnan(nrm).all() and not np.isnan(xyz).any()
        if name == "minus_zero_against_negative":
            assert np.array_equal(xyz, [ref.origin])
            vol.upload(None, np.full_like(W, 2.0))  # one plane alone: D stays
            assert same(vol.fetch()[0], D)


def test_no_crossing_gives_an_empty_fetch(gpu_lib):
    with TsdfVolume((5, 4, 3), [0.0, 0.0, 0.0], TsdfOptions(0.1, 0.3)) as vol:
        xyz, nrm = vol.extract()
        assert xyz.shape == (0, 3) and nrm.shape == (0, 3)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cpu.CHAIN))
def test_chain_fuse_extract_index_register(gpu_lib, name):
    c, s, n = cpu.chain(name), F.scene(name, F.PINHOLE), cpu.CHAIN[name]["views"]
    ref = c["ref"]
    assert ref["gap"] >= 1e-9 * cpu.CHAIN_MD ** 2  # the condition: no search decision of the restatement was closer than this
    xyz, nrm = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), F.PINHOLE, s["intr"], s["poses"][:n], depth=s["depth"][:n])
    assert same(xyz, c["target"]) and same(nrm, c["normals"])
    opts = IcpOptions(cpu.CHAIN_MD, metric=0, max_iterations=cpu.CHAIN[name]["max_iterations"], step_tolerance=1e-10)
    with CloudIndex(xyz, nrm, default_cell_size(cpu.CHAIN_MD)) as index:
        got = index.register([c["source"]], opts, init_pose7=c["init"][None])[0]
    drot, dtr = R.pose_error(got.pose7, ref["pose7"])
    print(f"chain {name}: status {got.status}, iterations {got.iterations}, pairs {got.n_pairs}; against the restatement {drot:.3g} rad, {dtr:.3g}")
    assert (got.status, got.iterations, got.n_pairs) == (ref["status"], ref["iterations"], ref["n_pairs"])
    assert drot <= 1e-9 and dtr <= 1e-9
    err, bar = cpu.chain_truth_error(name, got.pose7), cpu.CHAIN[name]["truth"]
    assert err[0] <= cpu.MARGIN * bar[0] and err[1] <= cpu.MARGIN * bar[1]


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_with_a_live_handle_and_use_after_close(gpu_lib):
    intr, depth, poses = F.generic_views(F.PINHOLE, 2, seed=1)
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.CbaInvalidArgument, match="2\\^28"):
        TsdfVolume((1024, 1024, 512), [0.0, 0, 0], TsdfOptions(0.1, 0.3))
    with pytest.raises(capi.CbaInvalidArgument, match="max_weight"):
        TsdfVolume((4, 4, 4), [0.0, 0, 0], TsdfOptions(0.1, 0.3, max_weight=1.5))
    with pytest.raises(capi.CbaInvalidArgument):
        TsdfVolume((4, 4, 4), [0.0, 0, 0], TsdfOptions(0.1, 0.3), device=99)
    with TsdfVolume((4, 4, 4), [0.0, 0, 0], TsdfOptions(0.1, 0.3)) as vol:
        h, lib = vol._h, gpu_lib
        k, d, p = capi.dptr(np.ascontiguousarray(intr)), capi.dptr(np.ascontiguousarray(depth)), capi.dptr(np.ascontiguousarray(poses))
        with pytest.raises(capi.CbaInvalidArgument, match="extract"):
            capi.check(lib, lib.cba_tsdf_extract_fetch(h, capi.dptr(np.zeros((1, 3))), capi.dptr(None)))
        assert lib.cba_tsdf_integrate(h, 7, k, 2, 9, 33, d, p) == bad and b"camera model" in lib.cba_last_error()
        assert lib.cba_tsdf_integrate(h, 0, capi.dptr(None), 2, 9, 33, d, p) == bad
        zero_f = intr.copy()
        zero_f[1] = 0.0
        assert lib.cba_tsdf_integrate(h, 0, capi.dptr(zero_f), 2, 9, 33, d, p) == bad and b"fx and fy" in lib.cba_last_error()
        assert lib.cba_tsdf_integrate(h, 0, k, -1, 9, 33, d, p) == bad and b"n_maps" in lib.cba_last_error()
        assert lib.cba_tsdf_integrate(h, 0, k, 2, 0, 33, d, p) == bad and lib.cba_tsdf_integrate(h, 0, k, 2, 9, 32769, d, p) == bad
        assert lib.cba_tsdf_integrate(h, 0, k, 2, 9, 33, capi.dptr(None), p) == bad and lib.cba_tsdf_integrate(h, 0, k, 2, 9, 33, d, capi.dptr(None)) == bad
        assert lib.cba_tsdf_integrate(h, 0, k, 0, 9, 33, capi.dptr(None), capi.dptr(None)) == capi.CBA_OK  # no work
        for q in ([0.0, 0, 0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0]):
            broken = poses.copy()
            broken[1, :4] = q
            with pytest.raises(capi.CbaInvalidArgument, match="quaternion"):
                vol.integrate(F.PINHOLE, intr, broken, depth=depth)
        assert (vol.fetch()[1] == 0).all()  # nothing ran
        n = np.zeros(1, np.int64)
        for mw in (0.0, 0.999, -1.0, np.nan):
            with pytest.raises(capi.CbaInvalidArgument, match="min_weight"):
                vol.extract(mw)
        assert lib.cba_tsdf_extract(h, 1.0, capi.i64ptr(None)) == bad
        with pytest.raises(ValueError):
            vol.integrate(F.PINHOLE, intr, poses[:1], depth=depth)
        with pytest.raises(ValueError):
            vol.integrate(F.PINHOLE, intr, poses)
        with pytest.raises(ValueError):
            vol.upload(np.zeros((2, 2, 2), np.float32))
        # points and no room for them
        vol.upload(np.linspace(-1, 1, 64, dtype=np.float32).reshape(4, 4, 4), np.ones((4, 4, 4), np.float32))
        assert lib.cba_tsdf_extract(h, 1.0, capi.i64ptr(n)) == capi.CBA_OK and n[0] > 0
        assert lib.cba_tsdf_extract_fetch(h, capi.dptr(None), capi.dptr(None)) == bad
        xyz = np.zeros((int(n[0]), 3))
        assert lib.cba_tsdf_extract_fetch(h, capi.dptr(xyz), capi.dptr(None)) == capi.CBA_OK and same(xyz, vol.extract()[0])  # normals may be NULL
    for call in (vol.fetch, vol.extract, vol.reset, lambda: vol.upload(None, None), lambda: vol.integrate(F.PINHOLE, intr, poses, depth=depth)):
        with pytest.raises(ValueError, match="closed"):
            call()
