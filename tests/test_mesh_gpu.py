"""GPU tier of scan meshing (cba_tsdf_mesh, cba_tsdf_mesh_fetch) through the Python layer: the device's triangles, points and counts
against the numpy restatement (tests/mesh_ref.py) and the host build of tsdf_mesh_math.hpp, to the bit: all 256 cases in one odd row
wider than a wave, single cells, the sizes where a kernel changes path (nx around the wave, a row end inside a wave, voxels around the
tile of 1024, a flat volume whose tile counts need the scan's second level), weights below min_weight, a sphere, a torus and a fused
scene with their statistics, repeatability, which calls invalidate a mesh, and the argument errors that need a live handle.  The
fields are those of tests/test_mesh_cpu.py."""
import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.fusion import Mesh, TsdfOptions, TsdfVolume, fuse
from tests import fusion_ref as F
from tests import host_build
from tests import mesh_ref as M
from tests import test_fusion_cpu as fcpu
from tests import test_mesh_cpu as cpu
from tests.test_mesh_cpu import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return host_build.load("mesh_cpu")


def device_volume(ref):
    return TsdfVolume(ref.shape, ref.origin, TsdfOptions(float(ref.vs), float(ref.trunc), float(ref.max_weight), float(ref.max_depth)))


def assert_mesh(vol, ref, host, min_weight=1.0, want=None):
    """the device's mesh of vol against the restatement's of ref (or `want`, computed before) and the host build's -> the Mesh"""
    got = vol.mesh(min_weight)
    xyz, nrm, tri = M.mesh(ref, min_weight) if want is None else want
    assert got.triangles.dtype == np.int32 and got.triangles.shape == tri.shape and got.xyz.shape == xyz.shape
    assert same(got.xyz, xyz) and same(got.normals, nrm) and same(got.triangles, tri)
    n, ht = M.host_triangles(host, ref, min_weight)
    assert n == len(got.xyz) and same(got.triangles, ht)
    return got


def uploaded(name):
    ref, mw = cpu.field_volume(name)
    vol = device_volume(ref)
    vol.upload(ref.D, ref.W)
    return vol, ref, mw


# ---- cases, cells, sizes ------------------------------------------------------------------------------------------------------------------
def test_all_cases_in_one_odd_row_wider_than_a_wave(gpu_lib, host):
    vol, ref, mw = uploaded("all_cases")
    with vol:
        got = assert_mesh(vol, ref, host, mw)
    count = M.table()[0]
    case, live = M.cell_cases(ref, mw)
    assert live.all() and np.array_equal(case[0, 0, ::3], np.arange(256)) and len(got.triangles) == count[case].sum() > 820


@pytest.mark.parametrize("case", [0, 1, 0x69, 0x96, 255], ids=lambda c: "%02x" % c)
def test_one_cell(gpu_lib, host, case):
    vol, ref, mw = uploaded("one_cell_%02x" % case)
    with vol:
        got = assert_mesh(vol, ref, host, mw)
    assert len(got.triangles) == M.table()[0][case]
    if case == 1:
        assert got.triangles.tolist() == [[0, 1, 2]]
    if case in (0, 255):
        assert got.triangles.shape == (0, 3) and got.xyz.shape == (0, 3)


@pytest.mark.parametrize("name", [n for n in sorted(cpu.fields()) if n.startswith("signs") or n.startswith("random")])
def test_sizes_equal_restatement_and_host_build_to_the_bit(gpu_lib, host, name):
    vol, ref, mw = uploaded(name)
    with vol:
        got = assert_mesh(vol, ref, host, mw)
        assert len(got.triangles) > 0 or name.startswith("random")
        assert same(vol.mesh(mw).triangles, got.triangles)  # again: the same bits, the buffers reused


def test_flat_volume_needs_the_second_scan_level(gpu_lib, host):
    ref, want = cpu.flat_volume()
    assert len(want[2]) > 1000 and cpu.first_tile_of(ref, want[2]).max() >= F.SCAN_TILE + 1  # triangles in tiles past the scan's first level
    with device_volume(ref) as vol:
        vol.upload(ref.D, ref.W)
        assert_mesh(vol, ref, host, want=want)


# ---- weights --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["weights", "weights_rows"])
def test_weights_below_min_weight_kill_their_cells(gpu_lib, host, name):
    vol, ref, mw = uploaded(name)
    assert mw == 2.0 and set(np.unique(ref.W)) == {0.0, 1.0, 2.0}
    with vol:
        got = assert_mesh(vol, ref, host, mw)
        all_live = assert_mesh(vol, ref, host, 1.0)
    assert 0 < len(got.triangles) < len(all_live.triangles)


def test_nothing_live_gives_no_triangles_and_an_empty_fetch(gpu_lib, host):
    vol, ref, mw = uploaded("nothing_live")
    with vol:
        got = assert_mesh(vol, ref, host, mw)
        assert got.triangles.shape == (0, 3) and got.xyz.shape == (0, 3)
        n, m = np.zeros(1, np.int64), np.zeros(1, np.int64)
        assert gpu_lib.cba_tsdf_mesh(vol._h, 2.0, capi.i64ptr(n), capi.i64ptr(m)) == capi.CBA_OK and (n[0], m[0]) == (0, 0)
        assert gpu_lib.cba_tsdf_mesh_fetch(vol._h, capi.i32ptr(None)) == capi.CBA_OK  # a fetch of nothing succeeds
        # points but no live cell: W = 0 in every second plane along x leaves the y and z edges of the other planes
        W = ref.W.copy()
        W[:, :, ::2] = 0.0
        vol.upload(None, W)
        holed = M.unit_volume(ref.shape, ref.D, W)
        got = assert_mesh(vol, holed, host, 1.0)
        assert got.triangles.shape == (0, 3) and len(got.xyz) > 0
        assert gpu_lib.cba_tsdf_mesh_fetch(vol._h, capi.i32ptr(None)) == capi.CBA_OK


# ---- solids and a fused scene ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus", "weight_hole", "zero_sphere"])
def test_solids_and_their_statistics(gpu_lib, host, name):
    vol, ref, mw = uploaded(name)
    with vol:
        got = assert_mesh(vol, ref, host, mw)
        packed = vol.mesh(mw, compact=True)
    if name in ("sphere", "torus"):
        truth, bar = M.SOLID_TRUTH[name], cpu.SOLID_DEFICIT[name]
        assert (len(got.xyz), len(got.triangles)) == cpu.SOLID_COUNTS[name]
        assert got.boundary_edges().shape == (0, 2) and M.euler_characteristic(got.triangles) == truth["euler"]
        assert bar[0] / cpu.MARGIN <= truth["volume"] - got.volume() <= cpu.MARGIN * bar[0]
        assert bar[1] / cpu.MARGIN <= truth["area"] - got.area() <= cpu.MARGIN * bar[1]
        vec = M.triangle_vectors(got.xyz, got.triangles)
        assert (np.einsum("ij,ij->i", vec, M.solid_gradient(name, got.xyz[got.triangles.astype(np.int64)].mean(axis=1))) > 0).all()
        assert same(packed.xyz, got.xyz) and same(packed.triangles, got.triangles)  # all points are referenced
    if name == "weight_hole":
        assert len(got.boundary_edges()) > 8 and len(packed.xyz) == len(np.unique(got.triangles)) < len(got.xyz)
        assert same(packed.xyz[packed.triangles.astype(np.int64)], got.xyz[got.triangles.astype(np.int64)])
    if name == "zero_sphere":
        zero = np.linalg.norm(M.triangle_vectors(got.xyz, got.triangles), axis=1) == 0.0
        assert (len(got.triangles), int(zero.sum())) == cpu.ZERO_SPHERE  # the zero-area triangles are kept


def test_fused_scene_through_integrate(gpu_lib, host):
    s, n = F.scene("sphere", F.PINHOLE), fcpu.SPHERE_VIEWS
    ref = F.fused("sphere", F.PINHOLE, n)
    want = M.mesh(ref)
    with device_volume(ref) as vol:
        vol.integrate(F.PINHOLE, s["intr"], s["poses"][:n], depth=s["depth"][:n])
        got = assert_mesh(vol, ref, host, want=want)
    assert len(got.triangles) > 1000
    assert got.area() == M.area(want[0], want[2]) and got.volume() == M.volume(want[0], want[2])
    stats = (len(got.boundary_edges()), M.euler_characteristic(got.triangles), len(np.unique(got.triangles)))
    print(f"fused sphere: {len(got.xyz)} points, {len(got.triangles)} triangles, {stats[0]} boundary edges, Euler characteristic {stats[1]}, "
          f"area {got.area():.4g} against {4.0 * np.pi * F.SPHERE_R ** 2:.4g}")
    unbalanced = M.unbalanced_edges(want[2])
    assert stats == (int(unbalanced[:, 2].sum()), M.euler_characteristic(want[2]), len(np.unique(want[2])))
    assert stats[0] > 0  # six views leave unobserved voxels next to the surface: the mesh has a boundary there
    facade = fuse(F.SHAPE, F.ORIGIN, TsdfOptions(F.VOXEL, F.TRUNCATION), F.PINHOLE, s["intr"], s["poses"][:n], depth=s["depth"][:n], mesh=True)
    assert isinstance(facade, Mesh) and same(facade.triangles, got.triangles) and same(facade.xyz, got.xyz)


# ---- repeatability and validity -------------------------------------------------------------------------------------------------------------
def test_repeatability_and_which_calls_invalidate_a_mesh(gpu_lib, host):
    vol, ref, _ = uploaded("weights")
    intr, depth, poses = F.generic_views(F.PINHOLE, 1, seed=3)
    with vol:
        h, lib = vol._h, gpu_lib
        first = assert_mesh(vol, ref, host, 1.0)
        again = vol.mesh(1.0)
        assert same(again.triangles, first.triangles) and same(again.xyz, first.xyz) and same(again.normals, first.normals)
        second = assert_mesh(vol, ref, host, 2.0)
        assert len(second.triangles) < len(first.triangles)
        third = vol.mesh(1.0)
        assert same(third.triangles, first.triangles) and same(third.xyz, first.xyz)
        tri = np.zeros_like(first.triangles)
        assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(tri)) == capi.CBA_OK and same(tri, first.triangles)  # a mesh may be fetched twice
        # a plain extract after a mesh is the extract as it was: the restatement's, and the mesh is gone
        xyz, nrm = vol.extract(2.0)
        rx, rn = ref.extract(2.0)
        assert same(xyz, rx) and same(nrm, rn)
        kept = first.triangles.copy()
        for name, call in (("extract", lambda: vol.extract(1.0)), ("integrate", lambda: vol.integrate(F.PINHOLE, intr, poses, depth=depth)),
                           ("upload", lambda: vol.upload(ref.D, ref.W)), ("reset", vol.reset)):
            if name != "extract":
                vol.upload(ref.D, ref.W)
                vol.mesh(1.0)
            call()
            assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(tri)) == capi.CBA_ERR_INVALID_ARGUMENT and b"mesh" in lib.cba_last_error(), name
        assert same(first.triangles, kept)  # arrays already fetched are the caller's
        vol.upload(ref.D, ref.W)
        assert same(vol.mesh(1.0).triangles, first.triangles)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_with_a_live_handle_and_use_after_close(gpu_lib):
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    vol, ref, _ = uploaded("signs16x8x4")
    with vol:
        h, lib = vol._h, gpu_lib
        n, m = np.zeros(1, np.int64), np.zeros(1, np.int64)
        tri = np.zeros((4096, 3), np.int32)
        assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(tri)) == bad and b"mesh" in lib.cba_last_error()  # before any mesh
        assert lib.cba_tsdf_mesh(h, 1.0, capi.i64ptr(None), capi.i64ptr(m)) == bad
        assert lib.cba_tsdf_mesh(h, 1.0, capi.i64ptr(n), capi.i64ptr(None)) == bad
        for mw in (0.0, 0.999, -1.0, np.nan):
            with pytest.raises(capi.CbaInvalidArgument, match="min_weight"):
                vol.mesh(mw)
        assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(tri)) == bad  # nothing ran: still no mesh
        assert lib.cba_tsdf_mesh(h, 1.0, capi.i64ptr(n), capi.i64ptr(m)) == capi.CBA_OK and n[0] > 0 and 0 < m[0] <= len(tri)
        assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(None)) == bad  # triangles and no room for them
        assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(tri)) == capi.CBA_OK and same(tri[:m[0]], M.triangles(ref))
        assert lib.cba_tsdf_mesh(h, 0.5, capi.i64ptr(n), capi.i64ptr(m)) == bad
        assert lib.cba_tsdf_mesh_fetch(h, capi.i32ptr(tri)) == capi.CBA_OK  # a refused call leaves the mesh as it was
    with pytest.raises(ValueError, match="closed"):
        vol.mesh()
