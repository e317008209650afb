"""CPU tier of colour in scan fusion (cba_tsdf_integrate_colour, rules 6 to 8 of calibba.h's scan-fusion section): the numpy
restatement (tests/colour_ref.py) against the host build of tsdf_colour_math.hpp (tests/colour_cpu) to the bit at every size and
planted case of the GPU tier (which imports the cases from here), the planted cases against what the rule gives by hand, ground truth
on the painted sphere, PLY files with colours, the stand-alone driver under the sanitizers, and what the library checks before it asks
for a device."""
import ctypes as C

import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.capi import dptr
from tests import colour_ref as K
from tests import fusion_ref as F
from tests import host_build
from tests import mesh_ref as M
from tests import raycast_ref as RC
from tests import test_fusion_cpu as fusion_cpu
from tests.test_fusion_cpu import same

# Ground truth, measured on the restatement: the painted sphere of colour_ref fused from the six views of the chain test (SHAPE =
# 32 x 28 x 24 voxels of 1/16, truncation four voxels, maps of 80 x 60), model -> (mean, largest) absolute channel error in byte units
# of the colours of the extract's points against the paint at each point, and the same of the hits of a ray cast from the held-out
# seventh view.  The paint moves by up to 19 units per voxel, and a voxel's colour is the mean over the views of nearest-pixel samples
# of the surface where each view's ray through the voxel meets it, up to four voxels away: the largest errors sit where views see a
# voxel's neighbourhood at a slant.  A ray cast's hit blends eight voxels where a point blends two, so its errors are smaller.  The
# figures are the measured values rounded up in their fourth digit; the bars are these times MARGIN, as in test_fusion_cpu.  The
# share of points and hits with A == 0 is held to a cap, not a tolerance: measured 0 of the points, 0.0015 and 0.0020 of the hits.
COLOUR_ERROR = {F.PINHOLE: dict(points=(2.506, 28.51), hits=(1.365, 16.57)), F.SCHEIMPFLUG: dict(points=(2.530, 28.51), hits=(1.339, 14.35))}
UNCOLOURED_CAP = 0.02
MARGIN = fusion_cpu.MARGIN
VIEWS = fusion_cpu.SPHERE_VIEWS


@pytest.fixture(scope="module")
def host():
    return host_build.load("colour_cpu")


# ---- cases shared with the GPU tier ------------------------------------------------------------------------------------------------------
def generic_volume(shape, **kw):
    return K.Volume(shape, F.GENERIC_ORIGIN, F.GENERIC_VOXEL, 3 * F.GENERIC_VOXEL, **kw)


def size_case(case):
    """a size case of test_fusion_cpu with images behind its maps -> shape, model, intr, depth, rgba, poses"""
    _, shape, model, n_maps = case
    intr, depth, poses = F.generic_views(model, n_maps, seed=shape[0])
    return shape, model, intr, depth, K.generic_images(n_maps, seed=shape[0]), poses


def generic_cast(vol, model, intr, pose, shape=(9, 33)):
    """the restatement's ray cast of one view -> rays [H][W][2], status, depth"""
    rays = RC.pixel_rays(model, intr, shape[1], shape[0])
    res = RC.cast(vol, rays, pose)
    return rays, res["status"], res["depth"]


def planted_colour(n_maps=1):
    """test_fusion_cpu.planted_update's lattice and camera with max_weight = 2 and a map whose row 2 decides step 7 on the plane k = 1
    (s = d - 1): pixel 0 has s == truncation, pixel 1 the next double above it, pixel 2 s == -truncation, pixel 3 s = 0 and A == 0.
    Rows j = 0, 1 see row 1 of the map, far behind: observed free space.  The R bytes of the maps are 10, 20, 40, 40, 40.
    -> volume arguments, intr, depth [n][3][4], rgba [n][3][4][4], poses [n][7]"""
    args, intr, _, pose = fusion_cpu.planted_update()
    args = dict(args, max_weight=2.0)
    depth = np.array([[9.0, 9.0, 9.0, 9.0], [3.0, 3.0, 3.0, 3.0], [1.25, np.nextafter(1.25, 2.0), 0.75, 1.0]])
    rgba = np.zeros((n_maps, 3, 4, 4), np.uint8)
    for m in range(n_maps):
        rgba[m, :, :] = [(10, 20, 40, 40, 40)[m], 7, 200, 255]
        rgba[m, 2, 3, 3] = 0
    return args, intr, np.tile(depth, (n_maps, 1, 1)), rgba, np.tile(pose, (n_maps, 1))


def check_planted_colour(vol_C, D, W, n_maps):
    """the records of the plane k = 1 after n_maps planted maps, by hand"""
    w = float(min(n_maps, 2))
    red = np.float32(0.0)
    for m in range(n_maps):  # the running mean with the old Wc, capped at 2: 10, 15, float32(70 / 3), then it keeps following
        wc = float(min(m, 2))
        red = np.float32((wc * float(red) + (10.0, 20.0, 40.0, 40.0, 40.0)[m]) / (wc + 1.0))
    if n_maps >= 3:
        assert red >= np.float32(70.0 / 3.0) and (n_maps == 3) == (red == np.float32(70.0 / 3.0))
    row = vol_C[1, 2]
    for i in (0, 1, 4, 5):  # s == truncation and s == -truncation: coloured
        assert row[i].tolist() == [red, 7.0, 200.0, w]
    for i in (2, 3, 6, 7, 8, 9):  # the next double above the truncation; A == 0; outside the map
        assert not row[i].any()
    assert not vol_C[1, :2].any()  # free space in front of the band
    assert (W[1, 2, :8] == w).all() and (W[1, :2, :8] == w).all() and D[1, 2, 6] == 0.0 and D[1, 2, 2] == 1.0  # D moved where the colour did not


def planted_records():
    """name -> (shape, D, W, C, expected point colours or None): volumes for upload whose extract is checked by hand"""
    out = {}
    shape, D, W, _, _ = fusion_cpu.planted_fields()["one_crossing_no_normal"]  # a = (0, 0, 0) at -0.5, b = (1, 0, 0) at 0.5: t = 0.5
    Cv = np.zeros((2, 2, 2, 4), np.float32)
    Cv[0, 0, 0], Cv[0, 0, 1] = [10, 20, 31, 1], [20, 21, 32, 3]
    out["both_ends_and_a_half"] = (shape, D, W, Cv.copy(), [[15, 21, 32, 255]])  # 15, 20.5 and 31.5: x.5 goes up
    Cv[0, 0, 1, 3] = 0
    out["one_end"] = (shape, D, W, Cv.copy(), [[10, 20, 31, 255]])
    Cv[0, 0, 0, 3], Cv[0, 0, 1, 3] = 0, 2
    out["other_end"] = (shape, D, W, Cv.copy(), [[20, 21, 32, 255]])
    Cv[0, 0, 1, 3] = 0
    out["neither_end"] = (shape, D, W, Cv.copy(), [[0, 0, 0, 0]])
    Cv[0, 0, 0], Cv[0, 0, 1] = [-40, 300, np.nan, 1], [-40, 300, 5, 1]
    out["clamped"] = (shape, D, W, Cv.copy(), [[0, 255, 0, 255]])
    for k, s in enumerate(F.NX_SIZES + F.BLOCK_SIZES):
        Dr, Wr = F.random_field(s, 50 + k)
        out["random%dx%dx%d" % s] = (s, Dr, Wr, K.random_colour(s, k), None)
    return out


def record_volume(shape, D, W, Cv):
    v = K.Volume(shape, np.array([0.25, -0.5, 1.0]), 0.125, 0.5)
    v.D, v.W, v.C = D.copy(), W.copy(), Cv.copy()
    return v


def planted_cast():
    """A 4 x 4 x 6 unit lattice with D = (2.5 - k) / 3, seen along +z from (1.5, 1.5, -3): every ray hits the plane z = 2.5 at depth 5.5.
    All records are {100, 50, 25.5, 1} but voxel (1, 1, 2)'s, which has Wc = 0.  -> the volume, rays [2][3][2], pose7, expected rgba"""
    D = np.broadcast_to(((2.5 - np.arange(6)) / 3.0)[:, None, None], (6, 4, 4)).astype(np.float32)
    v = K.Volume((4, 4, 6), np.zeros(3), 1.0, 3.0)
    v.D, v.W = np.ascontiguousarray(D), np.ones((6, 4, 4), np.float32)
    v.C = np.tile(np.array([100, 50, 25.5, 1], np.float32), (6, 4, 4, 1))
    v.C[2, 1, 1, 3] = 0.0
    pose = np.array([1.0, 0, 0, 0, -1.5, -1.5, 3.0])
    # x = 0: p = (1.5, 1.5, 2.5), cell (1, 1, 2), which holds the voxel without colour; x = 0.2: p_x = 2.6, cell (2, 1, 2); x = -0.2:
    # p_x = 0.4, cell (0, 1, 2), whose +x corner is voxel (1, 1, 2) again; y = 0.2: cell (., 2, 2)
    rays = np.array([[[0.0, 0.0], [0.2, 0.0], [-0.2, 0.0]], [[0.0, 0.2], [0.2, 0.2], [np.nan, 0.0]]])
    full = [100, 50, 26, 255]
    return v, rays, pose, np.array([[[0] * 4, full, [0] * 4], [full, full, [0] * 4]], np.uint8)


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------
def test_driver_runs_clean_under_sanitizers():
    p = host_build.run_sanitized("colour_cpu")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "colour_driver: 0 mismatches" in p.stdout and not p.stderr.strip(), p.stdout + p.stderr


# ---- integrate -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fusion_cpu.size_cases(), ids=lambda c: c[0])
def test_sizes_equal_the_host_build_to_the_bit(host, case):
    shape, model, intr, depth, rgba, poses = size_case(case)
    vol = generic_volume(shape)
    D, W, Cv = K.host_integrate_colour(host, vol, model, intr, depth, rgba, poses)
    vol.integrate_colour(model, intr, depth, rgba, poses)
    plain = fusion_cpu.generic_volume(shape).integrate(model, intr, depth, poses)
    assert same(vol.D, plain.D) and same(vol.W, plain.W) and same(D, vol.D) and same(W, vol.W)  # steps 1 to 6 are rule 2's
    if len(depth) == 0:
        assert vol.C is None and not Cv.any()  # no work: nothing allocated
        return
    assert same(Cv, vol.C)
    coloured = vol.C[..., 3] > 0
    assert coloured.any() and (coloured <= (vol.W > 0)).all()
    if shape[0] >= 63:  # a pixel with A == 0, or free space in front of the band: D moved there and the colour did not
        assert (vol.C[..., 3] < vol.W).any()
    assert same(K.point_colours(vol), K.host_point_colours(host, vol)) and len(K.point_colours(vol)) == len(vol.extract()[0])
    rays, status, z = generic_cast(vol, model, intr, poses[0])
    got = K.hit_colours(vol, rays, poses[0], status, z)
    assert same(got, K.host_hit_colours(host, vol, rays, poses[0], status, z))
    assert not got[status != RC.HIT].any()


@pytest.mark.parametrize("shape", [(1, 1), (7, 5)], ids=["1x1", "7x5"])
def test_small_and_odd_maps_and_a_map_without_colour_in_the_batch(host, shape):
    Wd, H = shape
    intr, depth, poses = F.generic_views(F.PINHOLE, 3, W=Wd, H=H, seed=5)
    rgba = K.generic_images(3, W=Wd, H=H, seed=5)
    rgba[..., 3] = 255
    rgba[1, ..., 3] = 0
    vol = generic_volume((65, 3, 2))
    D, W, Cv = K.host_integrate_colour(host, vol, F.PINHOLE, intr, depth, rgba, poses)
    vol.integrate_colour(F.PINHOLE, intr, depth, rgba, poses)
    assert same(D, vol.D) and same(W, vol.W) and same(Cv, vol.C) and (vol.C[..., 3] > 0).any()
    two = generic_volume((65, 3, 2)).integrate_colour(F.PINHOLE, intr, depth[[0, 2]], rgba[[0, 2]], poses[[0, 2]])
    assert same(two.C, vol.C) and not same(two.W, vol.W)  # the map with A == 0 everywhere moves D and W and leaves the colour


def test_batch_independence_of_the_restatement_and_the_host_build(host):
    intr, depth, poses = F.generic_views(F.SCHEIMPFLUG, 7, seed=2)
    rgba = K.generic_images(7, seed=2)
    one = generic_volume((65, 3, 2)).integrate_colour(F.SCHEIMPFLUG, intr, depth, rgba, poses)
    each, hv = generic_volume((65, 3, 2)), generic_volume((65, 3, 2))
    for m in range(7):
        each.integrate_colour(F.SCHEIMPFLUG, intr, depth[m], rgba[m], poses[m])
        hv.D, hv.W, hv.C = K.host_integrate_colour(host, hv, F.SCHEIMPFLUG, intr, depth[m], rgba[m], poses[m])
    assert same(one.C, each.C) and same(one.C, hv.C) and same(one.D, hv.D) and same(one.W, hv.W)
    assert one.C[..., 3].max() == 7


@pytest.mark.parametrize("n_maps", [1, 2, 3, 5])
def test_planted_step_7_decisions(host, n_maps):
    args, intr, depth, rgba, poses = planted_colour(n_maps)
    vol = K.Volume(**args)
    D, W, Cv = K.host_integrate_colour(host, vol, F.PINHOLE, intr, depth, rgba, poses)
    vol.integrate_colour(F.PINHOLE, intr, depth, rgba, poses)
    assert same(D, vol.D) and same(W, vol.W) and same(Cv, vol.C)
    check_planted_colour(vol.C, vol.D, vol.W, n_maps)
    plain = F.Volume(**args).integrate(F.PINHOLE, intr, depth, poses)
    assert same(plain.D, vol.D) and same(plain.W, vol.W)
    before = vol.C.copy()
    vol.integrate(F.PINHOLE, intr, depth, poses)  # a plain integrate leaves the colour
    assert same(before, vol.C)
    vol.reset()
    assert not vol.C.any() and (vol.W == 0).all()


# ---- points and hits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(planted_records()))
def test_planted_records_equal_the_host_build_and_the_hand(host, name):
    shape, D, W, Cv, want = planted_records()[name]
    vol = record_volume(shape, D, W, Cv)
    got = K.point_colours(vol)
    assert same(got, K.host_point_colours(host, vol)) and len(got) == len(vol.extract()[0])
    if want is not None:
        assert got.tolist() == want
    else:
        has = got[:, 3] != 0
        assert 0 < has.sum() < len(got) and not got[~has].any()
        assert same(K.point_colours(vol, 2.0), K.host_point_colours(host, vol, 2.0))


def test_planted_cast_with_one_voxel_of_a_cell_uncoloured(host):
    vol, rays, pose, want = planted_cast()
    res = RC.cast(vol, rays, pose)
    assert (res["status"] == [[RC.HIT] * 3, [RC.HIT, RC.HIT, RC.NO_RAY]]).all() and (res["depth"][res["status"] == RC.HIT] == 5.5).all()
    got = K.hit_colours(vol, rays, pose, res["status"], res["depth"])
    assert got.tolist() == want.tolist()
    assert same(got, K.host_hit_colours(host, vol, rays, pose, res["status"], res["depth"]))
    vol.W[:] = 0.0  # the D weight is not asked again: the colours are a function of the stored outputs and the colour volume
    assert same(got, K.hit_colours(vol, rays, pose, res["status"], res["depth"]))


# ---- ground truth ------------------------------------------------------------------------------------------------------------------------
def sphere_truth(vol, model, point_rgba, cast, hit_rgba):
    """-> the colour errors of the points and of the held-out view's hits against the paint"""
    s = K.painted_scene("sphere", model)
    xyz, _ = vol.extract()
    pose = s["poses"][VIEWS]
    hit = cast["status"] == RC.HIT
    Rm, t = F.rotation(pose[:4] / np.linalg.norm(pose[:4])), pose[4:]
    return K.colour_error(xyz, point_rgba), K.colour_error((cast["xyz"][hit] - t) @ Rm, hit_rgba[hit]), len(xyz), int(hit.sum())


def sphere_cast(vol, model):
    s = K.painted_scene("sphere", model)
    x, y = F.pixel_rays(model, s["intr"])
    return np.stack([x, y], -1), RC.cast(vol, np.stack([x, y], -1), s["poses"][VIEWS])


@pytest.mark.parametrize("model", sorted(COLOUR_ERROR))
def test_ground_truth_of_the_restatement_and_the_host_build(host, model):
    s = K.painted_scene("sphere", model)
    vol = K.fused("sphere", model, VIEWS)
    rays, cast = sphere_cast(vol, model)
    pose = s["poses"][VIEWS]
    bar = COLOUR_ERROR[model]
    got = {}
    for who, points, hits in (("restatement", K.point_colours(vol), K.hit_colours(vol, rays, pose, cast["status"], cast["depth"])),
                              ("host build", K.host_point_colours(host, vol), K.host_hit_colours(host, vol, rays, pose, cast["status"], cast["depth"]))):
        p, h, n_points, n_hits = sphere_truth(vol, model, points, cast, hits)
        print(f"{who}, model {model}: {n_points} points: mean {p[0]:.6g}, largest {p[1]:.6g}, without colour {p[2]:.4g}; "
              f"{n_hits} hits: mean {h[0]:.6g}, largest {h[1]:.6g}, without colour {h[2]:.4g}")
        assert n_points > 500 and n_hits > 500
        assert p[0] <= MARGIN * bar["points"][0] and p[1] <= MARGIN * bar["points"][1] and p[2] <= UNCOLOURED_CAP
        assert h[0] <= MARGIN * bar["hits"][0] and h[1] <= MARGIN * bar["hits"][1] and h[2] <= UNCOLOURED_CAP
        assert p[0] >= bar["points"][0] / MARGIN and h[0] >= bar["hits"][0] / MARGIN  # the constants are the measurement, not a loose bound
        got[who] = (points, hits)
    assert same(got["restatement"][0], got["host build"][0]) and same(got["restatement"][1], got["host build"][1])


# ---- PLY -------------------------------------------------------------------------------------------------------------------------------------
def write_ply_without_colours(path, mesh, normals=None):
    """the writer as it was before meshes had colours, kept here: a mesh without colours must give these bytes"""
    if normals is None:
        normals = bool(np.isfinite(mesh.normals).all())
    xyz_f, nrm_f = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")], [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
    fields = xyz_f + (nrm_f if normals else [])
    v = np.empty(len(mesh.xyz), np.dtype(fields))
    for c, (name, _) in enumerate(xyz_f):
        v[name] = mesh.xyz[:, c]
    if normals:
        for c, (name, _) in enumerate(nrm_f):
            v[name] = mesh.normals[:, c]
    f = np.empty(len(mesh.triangles), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    f["n"], f["v"] = 3, mesh.triangles
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property double {name}" for name, _ in fields]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def test_ply_with_and_without_colours(tmp_path):
    xyz, nrm, tri = M.mesh(M.solid("sphere"))
    rng = np.random.default_rng(3)
    colours = rng.integers(0, 256, (len(xyz), 4), dtype=np.uint8)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    for normals in (None, False):
        plain = cal.Mesh(xyz, nrm, tri)
        cal.write_ply(a, plain, normals)
        write_ply_without_colours(b, plain, normals)
        assert open(a, "rb").read() == open(b, "rb").read()
        back = cal.read_ply(a)
        assert back.colours is None
        painted = cal.Mesh(xyz, nrm, tri, colours)
        cal.write_ply(a, painted, normals)
        head = open(a, "rb").read(600)
        tail = b"property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face"
        assert (b"property double nz\n" + tail if normals is None else b"property double z\n" + tail) in head
        back = cal.read_ply(a)
        assert same(back.colours, colours) and same(back.xyz, xyz) and same(back.triangles, tri) and back.colours.dtype == np.uint8
        assert same(back.normals, nrm) if normals is None else np.isnan(back.normals).all()
    # compact carries the colours of the points it keeps
    loose = cal.Mesh(xyz, nrm, tri[: len(tri) // 2], colours)
    used = np.zeros(len(xyz), bool)
    used[loose.triangles.ravel()] = True
    small = loose.compact()
    assert same(small.colours, colours[used]) and len(small.xyz) == used.sum() < len(xyz)
    assert cal.Mesh(xyz, nrm, tri).compact().colours is None
    empty = cal.Mesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 4), np.uint8))
    cal.write_ply(a, empty)
    assert cal.read_ply(a).colours.shape == (0, 4)
    with open(a, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty double x\nproperty double y\nproperty double z\n"
                b"property uchar red\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError):
        cal.read_ply(a)


# ---- the package and the library without a device ----------------------------------------------------------------------------------------
def test_package_exports_and_the_image_forms():
    assert hasattr(cal, "rgba_maps")
    for name in ("has_colour", "fetch_colour", "upload_colour"):
        assert hasattr(cal.TsdfVolume, name)
    assert cal.Mesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32)).colours is None
    assert "rgba" in cal.RayCast.__dataclass_fields__ and "colours" in cal.Mesh.__dataclass_fields__
    rng = np.random.default_rng(0)
    grey = rng.integers(0, 256, (2, 3, 5), dtype=np.uint8)
    out = cal.rgba_maps(grey, (2, 3, 5))
    assert out.shape == (2, 3, 5, 4) and (out[..., :3] == grey[..., None]).all() and (out[..., 3] == 255).all() and out.flags["C_CONTIGUOUS"]
    rgb = rng.integers(0, 256, (2, 3, 5, 3), dtype=np.uint8)
    out = cal.rgba_maps(rgb, (2, 3, 5))
    assert (out[..., :3] == rgb).all() and (out[..., 3] == 255).all()
    rgba = rng.integers(0, 256, (2, 3, 5, 4), dtype=np.uint8)
    assert same(cal.rgba_maps(rgba, (2, 3, 5)), rgba)
    assert cal.rgba_maps(grey[0], (1, 3, 5)).shape == (1, 3, 5, 4) and cal.rgba_maps(rgb[0], (1, 3, 5)).shape == (1, 3, 5, 4)
    one = np.array([[[9]]], np.uint8)  # n = H = W = 1: [1][1][1] is the grey batch form, not one image with a channel axis
    assert cal.rgba_maps(one, (1, 1, 1)).tolist() == [[[[9, 9, 9, 255]]]] and cal.rgba_maps(one[0], (1, 1, 1)).tolist() == [[[[9, 9, 9, 255]]]]
    assert cal.rgba_maps(np.zeros((1, 1, 3), np.uint8), (1, 1, 1)).shape == (1, 1, 1, 4)
    for wrong in (grey.astype(np.float32), grey[:1], rgb[..., :2], np.zeros((2, 3, 5, 5), np.uint8), np.zeros((2, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            cal.rgba_maps(wrong, (2, 3, 5))


def test_argument_errors_come_before_the_device(lib):
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    k = np.array(F.CAMERAS[F.PINHOLE])
    out = np.zeros(1, np.int32)
    assert lib.cba_tsdf_integrate_colour(None, 0, dptr(k), 0, 4, 4, dptr(None), capi.u8ptr(None), dptr(None)) == bad
    assert lib.cba_tsdf_has_colour(None, capi.i32ptr(out)) == bad
    assert lib.cba_tsdf_colour_fetch(None, None) == bad and lib.cba_tsdf_colour_upload(None, None) == bad
    assert lib.cba_tsdf_extract_fetch_colour(None, capi.u8ptr(None)) == bad and lib.cba_tsdf_raycast_fetch_colour(None, capi.u8ptr(None)) == bad
    assert b"null argument" in lib.cba_last_error()
