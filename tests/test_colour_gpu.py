"""GPU tier of colour in scan fusion (cba_tsdf_integrate_colour, the colour of the extract's points, of the mesh and of the ray cast)
through the Python layer and the C ABI: the records, the point colours and the hit colours of the device against the numpy
restatement (tests/colour_ref.py) and the host build of tsdf_colour_math.hpp, to the bit, at the sizes where a kernel changes path,
map shapes and batch counts, the planted step-7, edge and cell cases, both camera models, partial pixel blocks, what one call leaves
for the next, the facade chain into a PLY file, and the argument errors that need a live handle.  The cases are those of
tests/test_colour_cpu.py."""
import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.fusion import RayCastOptions, TsdfOptions, TsdfVolume, fuse
from tests import colour_ref as K
from tests import fusion_ref as F
from tests import host_build
from tests import raycast_ref as RC
from tests import test_colour_cpu as cpu
from tests import test_fusion_cpu as fusion_cpu
from tests.test_fusion_cpu import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return host_build.load("colour_cpu")


def device_volume(ref):
    """a device volume with the arguments of a restatement's Volume"""
    return TsdfVolume(ref.shape, ref.origin, TsdfOptions(float(ref.vs), float(ref.trunc), float(ref.max_weight), float(ref.max_depth)))


def assert_volume(vol, ref):
    D, W = vol.fetch()
    assert same(D, ref.D) and same(W, ref.W)
    assert vol.has_colour == (ref.C is not None)
    if ref.C is not None:
        assert same(vol.fetch_colour(), ref.C)


def assert_points(vol, ref, host, min_weight=1.0):
    xyz, nrm, rgba = vol.extract(min_weight, colour=True)
    rx, rn = ref.extract(min_weight)
    assert same(xyz, rx) and same(nrm, rn)
    assert rgba.shape == (len(rx), 4) and same(rgba, K.point_colours(ref, min_weight)) and same(rgba, K.host_point_colours(host, ref, min_weight))
    return xyz, rgba


def assert_cast(vol, ref, host, model, intr, poses, shape, opts=None):
    """the device's hit colours against rule 8 applied to the device's own stored outputs -> the RayCast"""
    poses = np.asarray(poses).reshape(-1, 7)
    out = vol.raycast(model, intr, poses, shape, opts)
    assert out.rgba.shape == (len(poses),) + tuple(shape) + (4,)
    for v, pose in enumerate(poses):
        want = K.hit_colours(ref, out.rays, pose, out.status[v], out.depth[v])
        assert same(out.rgba[v], want) and same(out.rgba[v], K.host_hit_colours(host, ref, out.rays, pose, out.status[v], out.depth[v]))
        assert not out.rgba[v][out.status[v] != RC.HIT].any()
    return out


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fusion_cpu.size_cases(), ids=lambda c: c[0])
def test_sizes_equal_restatement_and_host_build_to_the_bit(gpu_lib, host, case):
    shape, model, intr, depth, rgba, poses = cpu.size_case(case)
    ref = cpu.generic_volume(shape)
    hD, hW, hC = K.host_integrate_colour(host, ref, model, intr, depth, rgba, poses)
    ref.integrate_colour(model, intr, depth, rgba, poses)
    with device_volume(ref) as vol, device_volume(ref) as plain:
        vol.integrate(model, intr, poses, depth=depth, colour=rgba)
        assert_volume(vol, ref)
        plain.integrate(model, intr, poses, depth=depth)
        assert same(vol.fetch()[0], plain.fetch()[0]) and same(vol.fetch()[1], plain.fetch()[1]) and not plain.has_colour
        if len(depth) == 0:  # no work: nothing was allocated
            with pytest.raises(capi.CbaInvalidArgument, match="no colour"):
                vol.fetch_colour()
            return
        assert same(vol.fetch_colour(), hC) and same(vol.fetch()[0], hD)
        assert_points(vol, ref, host)
        assert_points(vol, ref, host)  # again: the same bits, the buffers reused
        assert_cast(vol, ref, host, model, intr, poses[:1], (9, 33))


@pytest.mark.parametrize("shape", [(1, 1), (7, 5)], ids=["1x1", "7x5"])
def test_small_and_odd_maps_and_a_map_without_colour_in_the_batch(gpu_lib, shape):
    Wd, H = shape
    intr, depth, poses = F.generic_views(F.PINHOLE, 3, W=Wd, H=H, seed=5)
    rgba = K.generic_images(3, W=Wd, H=H, seed=5)
    rgba[..., 3] = 255
    rgba[1, ..., 3] = 0
    ref = cpu.generic_volume((65, 3, 2)).integrate_colour(F.PINHOLE, intr, depth, rgba, poses)
    with device_volume(ref) as vol:
        vol.integrate(F.PINHOLE, intr, poses, depth=depth, colour=rgba)
        assert_volume(vol, ref)
        assert (ref.C[..., 3] > 0).any()


@pytest.mark.parametrize("model", [F.PINHOLE, F.SCHEIMPFLUG])
def test_batch_independence_and_repeatability(gpu_lib, model):
    intr, depth, poses = F.generic_views(model, 7, seed=2)
    rgba = K.generic_images(7, seed=2)
    ref = cpu.generic_volume((65, 3, 2)).integrate_colour(model, intr, depth, rgba, poses)
    with device_volume(ref) as one, device_volume(ref) as each, device_volume(ref) as split:
        one.integrate(model, intr, poses, depth=depth, colour=rgba)
        for m in range(7):
            each.integrate(model, intr, poses[m], depth=depth[m], colour=rgba[m])
        split.integrate(model, intr, poses[:2], depth=depth[:2], colour=rgba[:2, ..., :3])  # the [..][3] form: A = 255
        split.integrate(model, intr, poses[2:], depth=depth[2:], colour=rgba[2:])
        for vol in (one, each):
            assert_volume(vol, ref)
        opaque = rgba.copy()
        opaque[:2, ..., 3] = 255
        assert_volume(split, cpu.generic_volume((65, 3, 2)).integrate_colour(model, intr, depth, opaque, poses))
        one.reset()  # zeroes the colour and keeps it allocated
        assert one.has_colour and not one.fetch_colour().any() and (one.fetch()[1] == 0).all()
        one.integrate(model, intr, poses, depth=depth, colour=rgba)  # a repeated run gives equal bits
        assert_volume(one, ref)
        assert ref.C[..., 3].max() == 7


# ---- planted cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_maps", [1, 2, 3, 5])
def test_planted_step_7_decisions(gpu_lib, n_maps):
    args, intr, depth, rgba, poses = cpu.planted_colour(n_maps)
    ref = K.Volume(**args).integrate_colour(F.PINHOLE, intr, depth, rgba, poses)
    with device_volume(ref) as vol:
        h = vol._h
        k, d, c, p = np.ascontiguousarray(intr), np.ascontiguousarray(depth), np.ascontiguousarray(rgba), np.ascontiguousarray(poses)
        capi.check(gpu_lib, gpu_lib.cba_tsdf_integrate_colour(h, F.PINHOLE, capi.dptr(k), n_maps, 3, 4, capi.dptr(d), capi.u8ptr(c), capi.dptr(p)))
        assert_volume(vol, ref)
        cpu.check_planted_colour(vol.fetch_colour(), *vol.fetch(), n_maps)
        before = vol.fetch_colour()
        vol.integrate(F.PINHOLE, intr, poses, depth=depth)  # a plain integrate on a handle with colour leaves the colour as it was
        assert same(vol.fetch_colour(), before)
        assert_volume(vol, ref.integrate(F.PINHOLE, intr, depth, poses))  # D and W moved on, as the restatement's


@pytest.mark.parametrize("name", sorted(cpu.planted_records()))
def test_planted_records_through_upload(gpu_lib, host, name):
    shape, D, W, Cv, want = cpu.planted_records()[name]
    ref = cpu.record_volume(shape, D, W, Cv)
    with device_volume(ref) as vol:
        vol.upload(D, W)
        assert not vol.has_colour
        vol.upload_colour(Cv)  # allocates; the records are taken as they are, NaN included
        assert_volume(vol, ref)
        _, rgba = assert_points(vol, ref, host)
        if want is not None:
            assert rgba.tolist() == want
        else:
            assert_points(vol, ref, host, 2.0)
            mesh = vol.mesh()
            assert same(mesh.colours, K.point_colours(ref)) and same(mesh.compact().colours, mesh.colours[np.unique(mesh.triangles)])


def test_planted_cast_with_one_voxel_of_a_cell_uncoloured(gpu_lib, host):
    ref, _, pose, want = cpu.planted_cast()
    intr = np.array([5.0, 5.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])  # columns 0, 1, 2 -> x = -0.2, 0, 0.2; rows 0, 1 -> y = 0, 0.2
    with device_volume(ref) as vol:
        vol.upload(ref.D, ref.W)
        vol.upload_colour(ref.C)
        out = assert_cast(vol, ref, host, F.PINHOLE, intr, pose, (2, 3))
        assert (out.status == RC.HIT).all() and np.allclose(out.depth, 5.5, atol=1e-6)
        full = want[0, 1].tolist()
        assert out.rgba[0].tolist() == [[[0] * 4, [0] * 4, full], [full, full, full]]


# ---- the painted sphere: partial pixel blocks, views in one call, the chain ---------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere(gpu_lib):
    s = K.painted_scene("sphere", F.PINHOLE)
    n = cpu.VIEWS
    ref = K.fused("sphere", F.PINHOLE, n)
    with device_volume(ref) as vol:
        vol.integrate(F.PINHOLE, s["intr"], s["poses"][:n], depth=s["depth"][:n], colour=s["rgba"][:n])
        yield vol, ref, s


def test_painted_sphere_volume_points_and_ground_truth(sphere, host):
    vol, ref, s = sphere
    assert_volume(vol, ref)
    xyz, rgba = assert_points(vol, ref, host)
    out = assert_cast(vol, ref, host, F.PINHOLE, s["intr"], s["poses"][cpu.VIEWS], (F.MAP_H, F.MAP_W))
    cast = dict(status=out.status[0], xyz=out.xyz[0])
    p, h, n_points, n_hits = cpu.sphere_truth(ref, F.PINHOLE, rgba, cast, out.rgba[0])
    print(f"device: {n_points} points: mean {p[0]:.6g}, largest {p[1]:.6g}, without colour {p[2]:.4g}; {n_hits} hits: mean {h[0]:.6g}, "
          f"largest {h[1]:.6g}, without colour {h[2]:.4g}")
    bar = cpu.COLOUR_ERROR[F.PINHOLE]
    assert p[0] <= cpu.MARGIN * bar["points"][0] and p[1] <= cpu.MARGIN * bar["points"][1] and p[2] <= cpu.UNCOLOURED_CAP
    assert h[0] <= cpu.MARGIN * bar["hits"][0] and h[1] <= cpu.MARGIN * bar["hits"][1] and h[2] <= cpu.UNCOLOURED_CAP and n_hits > 500


@pytest.mark.parametrize("shape", [(5, 7), (17, 9)], ids=["7x5", "9x17"])
def test_partial_pixel_blocks_and_two_views_in_one_call(sphere, host, shape):
    vol, ref, s = sphere
    H, W = shape
    intr = s["intr"].copy()
    intr[:4] = [intr[0] * W / F.MAP_W, intr[1] * H / F.MAP_H, (W - 1) / 2.0, (H - 1) / 2.0]
    poses = s["poses"][[cpu.VIEWS, 2]]
    both = assert_cast(vol, ref, host, F.PINHOLE, intr, poses, shape)
    assert (both.status == RC.HIT).sum() > H * W // 4 and both.rgba[..., 3].any()
    for v in range(2):
        one = vol.raycast(F.PINHOLE, intr, poses[v], shape)
        assert same(one.rgba[0], both.rgba[v]) and same(one.depth[0], both.depth[v])
    again = vol.raycast(F.PINHOLE, intr, poses, shape, RayCastOptions(skip=0.0))
    # other options give other stored outputs: the colours are rule 8 of those
    assert same(again.rgba[0], K.hit_colours(ref, again.rays, poses[0], again.status[0], again.depth[0]))


@pytest.mark.parametrize("model", [F.PINHOLE, F.SCHEIMPFLUG])
def test_facade_chain_fuse_mesh_ply(gpu_lib, tmp_path, model):
    s, n = K.painted_scene("sphere", model), cpu.VIEWS
    ref = K.fused("sphere", model, n)
    mesh = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), model, s["intr"], s["poses"][:n], depth=s["depth"][:n], mesh=True,
                colour=s["rgba"][:n])
    assert same(mesh.xyz, ref.extract()[0]) and same(mesh.colours, K.point_colours(ref)) and len(mesh.triangles) > 1000
    path = str(tmp_path / "sphere.ply")
    cal.write_ply(path, mesh)
    back = cal.read_ply(path)
    assert same(back.colours, mesh.colours) and same(back.xyz, mesh.xyz) and same(back.triangles, mesh.triangles)
    mean, worst, none = K.colour_error(back.xyz, back.colours)
    bar = cpu.COLOUR_ERROR[model]["points"]
    assert mean <= cpu.MARGIN * bar[0] and worst <= cpu.MARGIN * bar[1] and none <= cpu.UNCOLOURED_CAP
    xyz, nrm, rgba = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), model, s["intr"], s["poses"][:n], depth=s["depth"][:n],
                          colour=s["rgba"][:n, ..., 0])  # grey: replicated
    assert same(xyz, mesh.xyz) and (rgba[:, 0] == rgba[:, 1]).all() and (rgba[:, 1] == rgba[:, 2]).all() and rgba[:, 3].all()
    plain = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), model, s["intr"], s["poses"][:n], depth=s["depth"][:n], mesh=True)
    assert plain.colours is None and same(plain.xyz, mesh.xyz)
    none = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), model, s["intr"], s["poses"][:0], depth=s["depth"][:0], colour=s["rgba"][:0])
    assert [a.shape for a in none] == [(0, 3), (0, 3), (0, 4)] and none[2].dtype == np.uint8  # no maps: no points, no colours, no error


# ---- what one call leaves for the next ----------------------------------------------------------------------------------------------------
def test_cross_call_cases(gpu_lib):
    lib, bad = gpu_lib, capi.CBA_ERR_INVALID_ARGUMENT
    intr, depth, poses = F.generic_views(F.PINHOLE, 3, seed=65)
    rgba = K.generic_images(3, seed=65)
    ref = cpu.generic_volume((65, 3, 2)).integrate_colour(F.PINHOLE, intr, depth[:2], rgba[:2], poses[:2])
    with device_volume(ref) as vol:
        h = vol._h
        buf = np.zeros((4096, 4), np.uint8)
        # a handle without colour: the colour fetches fail, extract, mesh and ray cast give what they always gave
        assert lib.cba_tsdf_extract_fetch_colour(h, capi.u8ptr(buf)) == bad and b"no extract" in lib.cba_last_error()
        assert lib.cba_tsdf_raycast_fetch_colour(h, capi.u8ptr(buf)) == bad and b"no ray cast" in lib.cba_last_error()
        vol.integrate(F.PINHOLE, intr, poses[:2], depth=depth[:2])
        xyz, _ = vol.extract()
        assert len(xyz) > 0 and not vol.has_colour
        assert lib.cba_tsdf_extract_fetch_colour(h, capi.u8ptr(buf)) == bad and b"without colour" in lib.cba_last_error()
        with pytest.raises(capi.CbaInvalidArgument, match="without colour"):
            vol.extract(colour=True)
        assert vol.mesh().colours is None
        cast = vol.raycast(F.PINHOLE, intr, poses[:1], (9, 33))
        assert cast.rgba is None
        assert lib.cba_tsdf_raycast_fetch_colour(h, capi.u8ptr(buf)) == bad and b"without colour" in lib.cba_last_error()
        with pytest.raises(capi.CbaInvalidArgument, match="no colour"):
            vol.fetch_colour()
        # n_maps == 0 allocates nothing, and an argument error neither
        vol.integrate(F.PINHOLE, intr, np.zeros((0, 7)), depth=np.zeros((0, 9, 33)), colour=np.zeros((0, 9, 33, 4), np.uint8))
        k, d, p = capi.dptr(np.ascontiguousarray(intr)), capi.dptr(np.ascontiguousarray(depth)), capi.dptr(np.ascontiguousarray(poses))
        c = capi.u8ptr(np.ascontiguousarray(rgba))
        assert lib.cba_tsdf_integrate_colour(h, F.PINHOLE, k, 3, 9, 33, d, capi.u8ptr(None), p) == bad and b"null argument" in lib.cba_last_error()
        assert lib.cba_tsdf_integrate_colour(h, 7, k, 3, 9, 33, d, c, p) == bad and b"camera model" in lib.cba_last_error()
        assert lib.cba_tsdf_integrate_colour(h, F.PINHOLE, k, -1, 9, 33, d, c, p) == bad and b"n_maps" in lib.cba_last_error()
        assert lib.cba_tsdf_integrate_colour(h, F.PINHOLE, k, 3, 0, 33, d, c, p) == bad
        assert lib.cba_tsdf_integrate_colour(h, F.PINHOLE, k, 3, 9, 33, capi.dptr(None), c, p) == bad
        broken = poses.copy()
        broken[1, :4] = 0.0
        with pytest.raises(capi.CbaInvalidArgument, match="quaternion"):
            vol.integrate(F.PINHOLE, intr, broken, depth=depth, colour=rgba)
        assert lib.cba_tsdf_colour_upload(h, None) == bad and lib.cba_tsdf_has_colour(h, capi.i32ptr(None)) == bad
        assert not vol.has_colour
        with pytest.raises(ValueError):
            vol.integrate(F.PINHOLE, intr, poses, depth=depth, colour=rgba[:2])
        with pytest.raises(ValueError):
            vol.upload_colour(np.zeros((2, 3, 65, 3), np.float32))
        # colour from here on: the extract's colours stay as they are through a later integrate
        vol.reset()
        vol.integrate(F.PINHOLE, intr, poses[:2], depth=depth[:2], colour=rgba[:2])
        assert vol.has_colour
        xyz, _, first = vol.extract(colour=True)
        assert same(first, K.point_colours(ref)) and first[:, 3].any()
        assert lib.cba_tsdf_extract_fetch_colour(h, capi.u8ptr(None)) == bad and b"null argument" in lib.cba_last_error()
        cast = vol.raycast(F.PINHOLE, intr, poses[:1], (9, 33))
        vol.integrate(F.PINHOLE, intr, poses[2:], depth=depth[2:], colour=rgba[2:])
        later = np.zeros_like(first)
        capi.check(lib, lib.cba_tsdf_extract_fetch_colour(h, capi.u8ptr(later)))
        rays = np.zeros_like(cast.rgba)
        capi.check(lib, lib.cba_tsdf_raycast_fetch_colour(h, capi.u8ptr(rays)))
        assert same(later, first) and same(rays, cast.rgba)
        assert lib.cba_tsdf_raycast_fetch_colour(h, capi.u8ptr(None)) == bad
        ref.integrate_colour(F.PINHOLE, intr, depth[2:], rgba[2:], poses[2:])
        assert_volume(vol, ref)
        vol.reset()
        assert vol.has_colour and not vol.fetch_colour().any()
    for call in (vol.fetch_colour, lambda: vol.has_colour, lambda: vol.upload_colour(ref.C), lambda: vol.extract(colour=True),
                 lambda: vol.integrate(F.PINHOLE, intr, poses, depth=depth, colour=rgba)):
        with pytest.raises(ValueError, match="closed"):
            call()
