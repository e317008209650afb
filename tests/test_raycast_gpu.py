"""GPU tier of the TSDF ray cast (cba_tsdf_raycast) through the Python layer: the device's depth, xyz, normals and status against the
numpy restatement (tests/raycast_ref.py) and the host build of tsdf_ray_math.hpp, to the bit, both fed the device's fetched rays table;
the table against tests/camera_ref.py's unprojection at the 1e-12 relative that tests/test_camera_gpu.py uses; the view sizes around a
wavefront's 8 x 8 pixel block and a workgroup's four blocks, batches with a view that looks away, volumes with odd rows, both camera
models, the planted cases, batch independence, repeatability, what other calls leave alone, ground truth, the frame-to-model chain, and
the argument errors that need a live handle.  The cases are those of tests/test_raycast_cpu.py."""
import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.fusion import RayCastOptions, track
from calibration_amd.registration import IcpOptions
from tests import cloud_ref as R
from tests import fusion_ref as F
from tests import host_build
from tests import raycast_ref as RC
from tests import test_fusion_cpu as cpu
from tests import test_raycast_cpu as rcpu
from tests.test_fusion_cpu import same
from tests.test_fusion_gpu import device_volume
from tests.test_raycast_cpu import KEYS, same_cast

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return host_build.load("raycast_cpu")


def uploaded(ref):
    """a device volume holding a restatement's planes"""
    vol = device_volume(ref)
    vol.upload(ref.D, ref.W)
    return vol


def as_dict(cast):
    return dict(depth=cast.depth, xyz=cast.xyz, normals=cast.normals, status=cast.status)


def rel(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def assert_cast(cast, ref_vol, host, model, intr, poses, opts):
    """the device's result against the restatement and the host build over the device's rays, and those rays against the unprojection"""
    got = as_dict(cast)
    assert rel(cast.rays, RC.pixel_rays(model, intr, cast.rays.shape[1], cast.rays.shape[0])) <= 1e-12
    ref = RC.cast_views(ref_vol, cast.rays, poses, **opts)
    assert same_cast(got, ref)
    for m, pose in enumerate(poses):
        assert same_cast({k: got[k][m] for k in KEYS}, RC.host_cast(host, ref_vol, cast.rays, pose, **opts))
    assert np.array_equal(cast.hits, ref["status"] == RC.HIT)
    return ref


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rcpu.size_cases(), ids=lambda c: c[0])
def test_sizes_equal_restatement_and_host_build_to_the_bit(gpu_lib, host, case):
    ref_vol, model, intr, poses, shape, opts = rcpu.size_case(case)
    with uploaded(ref_vol) as vol:
        cast = vol.raycast(model, intr, poses, shape, RayCastOptions(**opts))
        ref = assert_cast(cast, ref_vol, host, model, intr, poses, opts)
        if case[5]:
            assert cast.hits.sum() > 0
        if len(poses) > 1:
            assert (cast.status[1] == RC.MISS).all()  # the view that looks away
        # n views in one call equal each view alone, and a repeated call gives equal bits
        for m in range(len(poses)):
            one = vol.raycast(model, intr, poses[m], shape, RayCastOptions(**opts))
            assert same_cast(as_dict(one), {k: ref[k][m:m + 1] for k in KEYS}) and same(one.rays, cast.rays)
        assert same_cast(as_dict(vol.raycast(model, intr, poses, shape, RayCastOptions(**opts))), ref)


# ---- planted cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rcpu.planted_cases()))
def test_planted_cases(gpu_lib, host, name):
    ref_vol, pose, opts, (status, depth, count, normal) = rcpu.planted_cases()[name]
    with uploaded(ref_vol) as vol:
        cast = vol.raycast(F.PINHOLE, rcpu.PLANTED_INTR, pose, rcpu.PLANTED_SHAPE, RayCastOptions(**opts))
    assert np.array_equal(cast.rays, rcpu.planted_rays())  # exact on the device too
    assert_cast(cast, ref_vol, host, F.PINHOLE, rcpu.PLANTED_INTR, pose[None], opts)
    assert cast.status[0, 4, 4] == status and np.array_equal(cast.depth[0, 4, 4], depth, equal_nan=True)
    if normal is not None:
        assert np.array_equal(cast.normals[0, 4, 4], [0.0, 0.0, -1.0] if normal else [np.nan] * 3, equal_nan=True)


def test_step_at_its_lower_bound_along_the_longest_side(gpu_lib, host):
    ref_vol = rcpu.long_volume()
    opts = dict(step=float(ref_vol.vs) / 16, skip=0.0)
    with uploaded(ref_vol) as vol:
        cast = vol.raycast(F.PINHOLE, rcpu.LONG_INTR, rcpu.LONG_POSE, (1, 1), RayCastOptions(**opts))
    assert np.array_equal(cast.rays, np.zeros((1, 1, 2))) and cast.status[0, 0, 0] == RC.MISS
    assert same_cast(as_dict(cast), {k: v[None] for k, v in RC.host_cast(host, ref_vol, cast.rays, rcpu.LONG_POSE, **opts).items() if k in KEYS})


# ---- what other calls leave alone -----------------------------------------------------------------------------------------------------------
def test_integrate_between_two_ray_casts_and_a_mesh_before_one(gpu_lib, host):
    model = F.PINHOLE
    intr, depth, poses = F.generic_views(model, 3, seed=6)
    ref_vol = cpu.generic_volume((65, 5, 3)).integrate(model, intr, depth[:2], poses[:2])
    with device_volume(ref_vol) as vol:
        vol.integrate(model, intr, poses[:2], depth=depth[:2])
        mesh = vol.mesh()
        first = vol.raycast(model, intr, poses[:2], (9, 33))
        assert_cast(first, ref_vol, host, model, intr, poses[:2], {})
        assert first.hits.sum() > 20
        # the mesh made before the ray cast still fetches
        tri = np.empty((len(mesh.triangles), 3), np.int32)
        xyz = np.empty_like(mesh.xyz)
        capi.check(gpu_lib, gpu_lib.cba_tsdf_mesh_fetch(vol._h, capi.i32ptr(tri)))
        capi.check(gpu_lib, gpu_lib.cba_tsdf_extract_fetch(vol._h, capi.dptr(xyz), capi.dptr(None)))
        assert same(tri, mesh.triangles) and same(xyz, mesh.xyz)
        # an integrate changes the second ray cast only: the first one's arrays are the handle's until the next cast
        vol.integrate(model, intr, poses[2], depth=depth[2])
        kept = [np.empty_like(a) for a in (first.depth, first.xyz, first.normals, first.status, first.rays)]
        capi.check(gpu_lib, gpu_lib.cba_tsdf_raycast_fetch(vol._h, capi.dptr(kept[0]), capi.dptr(kept[1]), capi.dptr(kept[2]), capi.u8ptr(kept[3]),
                                                           capi.dptr(kept[4])))
        assert all(same(a, b) for a, b in zip(kept, (first.depth, first.xyz, first.normals, first.status, first.rays)))
        vol.extract()
        vol.reset()
        capi.check(gpu_lib, gpu_lib.cba_tsdf_raycast_fetch(vol._h, capi.dptr(kept[0]), capi.dptr(None), capi.dptr(None), capi.u8ptr(None), capi.dptr(None)))
        assert same(kept[0], first.depth)
        vol.integrate(model, intr, poses, depth=depth)
        ref_vol.integrate(model, intr, depth[2], poses[2])
        second = vol.raycast(model, intr, poses[:2], (9, 33))
        assert_cast(second, ref_vol, host, model, intr, poses[:2], {})
        assert not same(second.depth, first.depth)


# ---- ground truth and the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(rcpu.RAYCAST_ERROR))
def test_scenes_and_ground_truth(gpu_lib, host, key):
    name, model = key
    s, n = F.scene(name, model), cpu.CHAIN[name]["views"]
    ref_vol, pose = F.fused(name, model, n), s["poses"][n]
    with device_volume(ref_vol) as vol:
        vol.integrate(model, s["intr"], s["poses"][:n], depth=s["depth"][:n])
        cast = vol.raycast(model, s["intr"], pose, (F.MAP_H, F.MAP_W))
    assert_cast(cast, ref_vol, host, model, s["intr"], pose[None], {})
    hit, of, rms, worst, angle = rcpu.truth_error(name, model, as_dict(cast), pose)
    print(f"{name} model {model}: {hit} of {of} truth pixels hit, depth rms {rms:.4g} voxel, worst {worst:.4g} voxel, largest normal angle {angle:.4g} rad")
    bar = rcpu.RAYCAST_ERROR[key]
    assert 2 * hit >= of
    assert rms <= cpu.MARGIN * bar[0] and worst <= cpu.MARGIN * bar[1] and angle <= cpu.MARGIN * bar[2]
    # the organised map is what the front ends write: the product's own consumers take it
    xyz, nrm = cast.cloud(0, pose)
    rx, rn = RC.cloud(as_dict(cast), 0, pose)
    assert len(xyz) == cast.hits.sum() >= hit
    assert np.allclose(xyz, rx, atol=1e-13) and np.allclose(nrm, rn, atol=1e-13, equal_nan=True)


@pytest.mark.parametrize("name", sorted(rcpu.TRACK))
def test_chain_track_against_the_model(gpu_lib, name):
    s, n = F.scene(name, F.PINHOLE), cpu.CHAIN[name]["views"]
    start = rcpu.track_start(name)
    icp = IcpOptions(cpu.CHAIN_MD, metric=0, max_iterations=rcpu.TRACK_ITERATIONS, step_tolerance=1e-10)
    with device_volume(F.fused(name, F.PINHOLE, n)) as vol:
        vol.integrate(F.PINHOLE, s["intr"], s["poses"][:n], depth=s["depth"][:n])
        rays = vol.raycast(F.PINHOLE, s["intr"], start, (F.MAP_H, F.MAP_W)).rays
        pose, got = track(vol, F.PINHOLE, s["intr"], start, xyz=rcpu.track_source(name, rays), icp=icp)
    ref = rcpu.track_ref(name, rays)
    assert ref["gap"] >= 1e-9 * cpu.CHAIN_MD ** 2  # the condition: no search decision of the restatement was closer than this
    drot, dtr = R.pose_error(got.pose7, ref["pose7"])
    print(f"track {name}: status {got.status}, iterations {got.iterations}, pairs {got.n_pairs}; against the restatement {drot:.3g} rad, {dtr:.3g}")
    assert (got.status, got.iterations, got.n_pairs) == (ref["status"], ref["iterations"], ref["n_pairs"])
    assert drot <= 1e-9 and dtr <= 1e-9
    back = R.pose_error(pose, R.pose_inverse(got.pose7))
    assert back[0] <= 1e-12 and back[1] <= 1e-12  # the returned pose is the result's inverse: volume frame -> camera
    err, bar = rcpu.track_truth_error(name, got.pose7), rcpu.TRACK[name]
    assert err[0] <= cpu.MARGIN * bar[0] and err[1] <= cpu.MARGIN * bar[1]


def test_track_takes_a_depth_map(gpu_lib):
    s, n = F.scene("bumpy", F.PINHOLE), cpu.CHAIN["bumpy"]["views"]
    start = rcpu.track_start("bumpy")
    icp = IcpOptions(cpu.CHAIN_MD, metric=0, max_iterations=2, step_tolerance=1e-10)
    with device_volume(F.fused("bumpy", F.PINHOLE, n)) as vol:
        vol.integrate(F.PINHOLE, s["intr"], s["poses"][:n], depth=s["depth"][:n])
        rays = vol.raycast(F.PINHOLE, s["intr"], start, (F.MAP_H, F.MAP_W)).rays
        d = s["depth"][n]
        by_depth = track(vol, F.PINHOLE, s["intr"], start, depth=d, icp=icp)
        by_xyz = track(vol, F.PINHOLE, s["intr"], start, xyz=np.concatenate([rays * d[..., None], d[..., None]], -1), icp=icp)
        assert same(by_depth[0], by_xyz[0]) and by_depth[1].n_pairs == by_xyz[1].n_pairs > 1000
        with pytest.raises(ValueError):
            track(vol, F.PINHOLE, s["intr"], start)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_with_a_live_handle_and_use_after_close(gpu_lib):
    lib, bad = gpu_lib, capi.CBA_ERR_INVALID_ARGUMENT
    ref_vol = rcpu.planted_volume()
    intr, pose = rcpu.PLANTED_INTR, np.ascontiguousarray(rcpu.IDENTITY)
    with uploaded(ref_vol) as vol:
        h, k, p = vol._h, capi.dptr(np.ascontiguousarray(intr)), capi.dptr(pose)
        none = (capi.dptr(None), capi.dptr(None), capi.dptr(None), capi.u8ptr(None), capi.dptr(None))
        assert lib.cba_tsdf_raycast_fetch(h, *none) == bad and b"no ray cast" in lib.cba_last_error()  # it fails before any ray cast
        assert lib.cba_tsdf_raycast(h, 0, k, 0, 9, 9, capi.dptr(None), None) == capi.CBA_OK  # no work ...
        assert lib.cba_tsdf_raycast_fetch(h, *none) == bad  # ... and no result
        first = vol.raycast(F.PINHOLE, intr, pose, (9, 9))  # opts None: the defaults
        assert same_cast(as_dict(first), RC.cast_views(ref_vol, first.rays, pose[None]))
        assert lib.cba_tsdf_raycast_fetch(h, *none) == capi.CBA_OK  # every pointer may be NULL
        assert lib.cba_tsdf_raycast(h, 7, k, 1, 9, 9, p, None) == bad and b"camera model" in lib.cba_last_error()
        assert lib.cba_tsdf_raycast(h, 0, capi.dptr(None), 1, 9, 9, p, None) == bad
        zero_f = intr.copy()
        zero_f[0] = 0.0
        assert lib.cba_tsdf_raycast(h, 0, capi.dptr(zero_f), 1, 9, 9, p, None) == bad and b"fx and fy" in lib.cba_last_error()
        assert lib.cba_tsdf_raycast(h, 0, k, -1, 9, 9, p, None) == bad and b"n_views" in lib.cba_last_error()
        assert lib.cba_tsdf_raycast(h, 0, k, 1, 0, 9, p, None) == bad and lib.cba_tsdf_raycast(h, 0, k, 1, 9, 32769, p, None) == bad
        assert lib.cba_tsdf_raycast(h, 0, k, 9, 4096, 2048, p, None) == bad and b"2^26" in lib.cba_last_error()
        assert lib.cba_tsdf_raycast(h, 0, k, 1, 9, 9, capi.dptr(None), None) == bad
        for q in ([0.0, 0, 0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0]):
            broken = pose.copy()
            broken[:4] = q
            with pytest.raises(capi.CbaInvalidArgument, match="quaternion"):
                vol.raycast(F.PINHOLE, intr, broken, (9, 9))
        vs = float(ref_vol.vs)
        for field, values in (("step", (-1.0, vs / 17, np.nan, np.inf)), ("skip", (-0.1, 1.5, np.nan)), ("near_depth", (-1.0, np.nan, np.inf)),
                              ("far_depth", (0.0, -1.0, np.nan)), ("min_weight", (0.0, 0.5, np.nan))):
            for v in values:
                with pytest.raises(capi.CbaInvalidArgument, match=field):
                    vol.raycast(F.PINHOLE, intr, pose, (9, 9), RayCastOptions(**{field: v}))
        with pytest.raises(capi.CbaInvalidArgument, match="far_depth"):
            vol.raycast(F.PINHOLE, intr, pose, (9, 9), RayCastOptions(near_depth=2.0, far_depth=2.0))
        vol.raycast(F.PINHOLE, intr, pose, (9, 9), RayCastOptions(step=vs / 16))  # the lower bound itself is allowed
        with pytest.raises(ValueError):
            vol.raycast(F.PINHOLE, intr[:9], pose, (9, 9))
        # an error leaves earlier results untouched
        vol.raycast(F.PINHOLE, intr, pose, (9, 9))
        assert lib.cba_tsdf_raycast(h, 0, k, 1, 9, 9, p, None) == capi.CBA_OK and lib.cba_tsdf_raycast(h, 7, k, 1, 9, 9, p, None) == bad
        depth = np.empty((1, 9, 9))
        assert lib.cba_tsdf_raycast_fetch(h, capi.dptr(depth), *none[1:]) == capi.CBA_OK and same(depth, first.depth)
    for call in (lambda: vol.raycast(F.PINHOLE, intr, pose, (9, 9)), lambda: track(vol, F.PINHOLE, intr, pose, depth=np.ones((9, 9)))):
        with pytest.raises(ValueError, match="closed"):
            call()
