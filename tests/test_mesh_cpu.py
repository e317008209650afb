"""CPU tier of scan meshing (cba_tsdf_mesh): the table of tsdf_mesh_math.hpp against the one the numpy restatement (tests/mesh_ref.py)
generates from the rule with its own code, the facts calibba.h states about it, the restatement against the host build of the header
(tests/mesh_cpu) to the bit on every field of the GPU tier (which imports the fields from here), a sphere and a torus against their
analytic volume, area, topology and orientation, the guarantees (balanced half-edges, a boundary only next to cells that are not live,
zero-area triangles kept), the Python layer's statistics, compaction and PLY files, the stand-alone driver under the sanitizers, and
what the library checks before it asks for a device."""
import os
import re

import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from tests import fusion_ref as F
from tests import host_build
from tests import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on the restatement (float32 field D = clip(distance / 3), W = 1, 20^3 voxels, centre (9.3, 9.7, 10.1), in voxels): the
# sphere of radius 6 gives 676 points, all referenced, and 1348 triangles, volume 889.776 against 904.779, area 448.445 against
# 452.389; the torus R = 5.5, r = 2.2 gives 740 points and 1480 triangles, volume 502.304 against 525.458, area 471.713 against
# 477.689.  A mesh of chords lies inside a convex surface, so both fall short.  (volume deficit, area deficit), rounded up in the
# fourth digit; the bars are these times MARGIN both ways, as test_fusion_cpu.SURFACE_ERROR's are.
SOLID_COUNTS = {"sphere": (676, 1348), "torus": (740, 1480)}
SOLID_DEFICIT = {"sphere": (15.01, 3.944), "torus": (23.16, 5.976)}
MARGIN = 1.25
ZERO_SPHERE = (1304, 96)  # triangles, of them with zero area: the sphere centred on the lattice point (10, 10, 10)


@pytest.fixture(scope="module")
def host():
    return host_build.load("mesh_cpu")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- fields shared with the GPU tier -------------------------------------------------------------------------------------------------------
_fields = {}


def fields():
    """name -> (shape, D, W, min_weight): planes for upload (computed once)"""
    if _fields:
        return _fields
    out = _fields
    out["all_cases"] = (M.ALL_CASES_SHAPE, *M.all_cases_field(), 1.0)
    for case in (0, 1, 0x69, 0x96, 255):
        out["one_cell_%02x" % case] = ((2, 2, 2), *M.one_cell_field(case), 1.0)
    for n, s in enumerate(F.NX_SIZES + F.BLOCK_SIZES):
        out["signs%dx%dx%d" % s] = (s, *M.sign_field(s, 100 + n), 1.0)
        D, W = F.random_field(s, 200 + n)  # zeros and -0.0 among the values, W in {0, 1, 2, 3}
        out["random%dx%dx%d" % s] = (s, D, W, 1.0)
    out["weights"] = ((41, 5, 5), *M.weight_field((41, 5, 5), 3), 2.0)
    out["weights_rows"] = ((65, 3, 2), *M.weight_field((65, 3, 2), 4), 2.0)
    D, W = M.sign_field((16, 8, 4), 5)
    out["nothing_live"] = ((16, 8, 4), D, W, 2.0)
    for name in ("sphere", "torus"):
        v = M.solid(name)
        out[name] = (M.SOLID_SHAPE, v.D, v.W, 1.0)
    out["weight_hole"] = (M.SOLID_SHAPE, *M.weight_hole(), 1.0)
    z = M.zero_sphere()
    out["zero_sphere"] = (M.SOLID_SHAPE, z.D, z.W, 1.0)
    return out


def field_volume(name):
    shape, D, W, min_weight = fields()[name]
    return M.unit_volume(shape, D, W), min_weight


_flat = {}


def flat_volume():
    """FLAT_SHAPE with a sparse field and its restated mesh (computed once)"""
    if not _flat:
        D, W = M.flat_sparse_field()
        v = M.unit_volume(F.FLAT_SHAPE, D, W)
        _flat.update(vol=v, mesh=M.mesh(v))
    return _flat["vol"], _flat["mesh"]


def first_tile_of(vol, tri, min_weight=1.0):
    """the tile (of the dense order) of the cell that gave each triangle's first vertex's edge: enough to tell that late tiles have some"""
    q, _, _ = M.edge_mask(vol, min_weight)
    l_of_point = np.nonzero(q.reshape(-1, 3))[0]
    return l_of_point[tri[:, 0].astype(np.int64)] // M.MESH_TILE


# ---- the constants and the table ------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    src = os.path.join(ROOT, "calibration_amd", "csrc")

    def const(name, file):
        return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(src, file)).read()).group(1))

    assert const("TSDF_BLOCK", "tsdf_fusion.hip") == M.MESH_BLOCK
    assert const("TSDF_EXTRACT_TILE", "tsdf_math.hpp") == M.MESH_TILE == F.EXTRACT_TILE
    assert const("TSDF_MESH_GROUP", "tsdf_mesh_math.hpp") == M.GROUP
    assert const("TSDF_MESH_SLOTS", "tsdf_mesh_math.hpp") == M.SLOTS
    voxels = [s[0] * s[1] * s[2] for s in F.BLOCK_SIZES]
    assert {M.MESH_TILE - 1, M.MESH_TILE, M.MESH_TILE + 1} <= set(voxels)
    assert {M.GROUP - 1, M.GROUP, M.GROUP + 1} <= {s[0] for s in F.NX_SIZES}  # the wave along x, a row end inside a wave
    nx, ny, nz = F.FLAT_SHAPE
    assert nx * ny * nz // M.MESH_TILE > F.SCAN_TILE
    assert M.ALL_CASES_SHAPE[0] > M.GROUP and M.ALL_CASES_SHAPE[0] % M.GROUP != 0 and M.ALL_CASES_SHAPE[0] % 2 == 1


def test_header_table_equals_the_restatement(host):
    _, _, words = M.table()
    assert same(M.host_table(host), words)


def test_no_table_is_typed_in():
    text = open(os.path.join(ROOT, "calibration_amd", "csrc", "tsdf_mesh_math.hpp")).read()
    assert "tsdf_mesh_case_word(c)" in text and len(re.findall(r"0x[0-9a-fA-F]+", text)) < 8


def test_facts_of_the_rule():
    count, edges, _ = M.table()
    loops = [M.case_loops(c) for c in range(256)]  # asserts inside: every crossing edge is one tail and one head, so the loops close
    assert loops[0] == [] and loops[255] == [] and all(loops[c] for c in range(1, 255))
    assert max(len(lp) for lp in loops) == 4
    assert max(len(e) for lp in loops for e in lp) == 7 and min(len(e) for lp in loops for e in lp) == 3
    assert count.max() == 5 and count.sum() == 820
    assert np.bincount(count).tolist() == [2, 16, 50, 80, 76, 32]
    assert M.case_triangles(1) == [(0, 4, 8)]
    assert M.case_triangles(5) == [(0, 1, 10), (0, 10, 8)]
    assert M.case_triangles(0x69) == [(0, 4, 8), (1, 5, 11), (2, 7, 9), (3, 6, 10)]
    assert M.case_triangles(0x96) == [(0, 9, 5), (1, 10, 4), (2, 8, 6), (3, 11, 7)]
    for c in range(256):  # a loop visits the crossing edges of its case, each once
        crossing = {M.edge_number(p, q) for p in np.ndindex(2, 2, 2) for q in np.ndindex(2, 2, 2)
                    if sum(abs(a - b) for a, b in zip(p, q)) == 1 and ((c >> M.corner_number(p)) & 1) != ((c >> M.corner_number(q)) & 1)}
        assert sorted(e for lp in loops[c] for e in lp) == sorted(crossing)


def test_shared_face_segments_are_reversed_for_every_pattern():
    """Cell A and its neighbour B across axis a share A's face on side 1, which is B's face on side 0: for all 2^8 patterns of A (B takes
    A's far corners as its near ones, and the rest as they come) B draws A's segments reversed."""
    for a in range(3):
        across = {}  # A's local edge in the shared face -> B's number for it
        for p in np.ndindex(2, 2, 2):
            for q in np.ndindex(2, 2, 2):
                if p[a] == 1 and q[a] == 1 and sum(abs(x - y) for x, y in zip(p, q)) == 1:
                    pb, qb = list(p), list(q)
                    pb[a] = qb[a] = 0
                    across[M.edge_number(p, q)] = M.edge_number(tuple(pb), tuple(qb))
        assert len(across) == 4
        for case in range(256):
            neg_a = lambda p: bool((case >> M.corner_number(p)) & 1)

            def neg_b(p):
                q = list(p)
                q[a] = 1 - q[a]  # B's near corners are A's far ones
                return neg_a(tuple(q))

            seg_a = sorted((across[t], across[h]) for t, h in M.face_segments(a, 1, neg_a))
            seg_b = sorted((h, t) for t, h in M.face_segments(a, 0, neg_b))
            assert seg_a == seg_b


# ---- the restatement against the host build ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fields()))
def test_fields_equal_the_host_build_to_the_bit(host, name):
    vol, mw = field_volume(name)
    xyz, _, tri = M.mesh(vol, mw)
    n, ht = M.host_triangles(host, vol, mw)
    assert n == len(xyz) and same(ht, tri)
    assert tri.dtype == np.int32 and (len(tri) == 0 or (0 <= tri.min() and tri.max() < n))
    count = M.table()[0]
    if name == "all_cases":
        assert len(tri) > 820  # the table's 820 and what the cells between the planted ones give
        for c in range(256):  # cell 3 c alone gives the table's row
            cell = M.unit_volume((2, 2, 2), vol.D[:, :, 3 * c:3 * c + 2])
            assert len(M.triangles(cell)) == count[c]
    if name.startswith("one_cell"):
        assert len(tri) == count[int(name[-2:], 16)]
    if name == "nothing_live":
        assert len(tri) == 0 and n == 0 and len(M.triangles(vol, 1.0)) > 0
    if name.startswith("weights"):
        assert 0 < len(tri) < len(M.triangles(M.unit_volume(vol.shape, vol.D)))
    if name.startswith("signs"):
        assert len(tri) > 0


def test_one_cell_cases_by_hand():
    for case, want in ((1, [[0, 1, 2]]), (0x69, [[0, 4, 8], [1, 5, 11], [2, 7, 9], [3, 6, 10]]), (0x96, [[0, 9, 5], [1, 10, 4], [2, 8, 6], [3, 11, 7]])):
        vol, _ = field_volume("one_cell_%02x" % case)
        xyz, _, tri = M.mesh(vol)
        if case == 1:
            assert tri.tolist() == want and (np.nonzero(xyz)[1] == [0, 1, 2]).all() and (xyz.sum(axis=1) > 0).all()  # one point on each axis from corner 0
        else:
            # all twelve edges cross: the point order is voxel by voxel, +x +y +z; local edge -> its place
            place = {}
            q, _, _ = M.edge_mask(vol, 1.0)
            for n, (k, j, i, axis) in enumerate(zip(*np.nonzero(q))):
                u, v = [c for a, c in enumerate((i, j, k)) if a != axis]
                place[4 * axis + u + 2 * v] = n
            assert tri.tolist() == [[place[e] for e in t] for t in want]


def test_flat_volume_has_triangles_past_the_first_scan_level(host):
    vol, (xyz, _, tri) = flat_volume()
    n, ht = M.host_triangles(host, vol)
    assert n == len(xyz) and same(ht, tri)
    assert len(tri) > 1000 and first_tile_of(vol, tri).max() >= F.SCAN_TILE + 1


# ---- ground truth ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_solids_against_the_analytic_surface(name):
    vol, _ = field_volume(name)
    xyz, nrm, tri = M.mesh(vol)
    truth = M.SOLID_TRUTH[name]
    vol_deficit, area_deficit = truth["volume"] - M.volume(xyz, tri), truth["area"] - M.area(xyz, tri)
    print(f"{name}: {len(xyz)} points, {len(tri)} triangles, volume {M.volume(xyz, tri):.6g} against {truth['volume']:.6g} (deficit {vol_deficit:.5g}), "
          f"area {M.area(xyz, tri):.6g} against {truth['area']:.6g} (deficit {area_deficit:.5g})")
    assert (len(xyz), len(tri)) == SOLID_COUNTS[name]
    assert len(np.unique(tri)) == len(xyz)                 # all points referenced
    assert len(M.unbalanced_edges(tri)) == 0               # closed and oriented
    assert M.max_half_edge_multiplicity(tri) == 1          # a 2-manifold: every directed edge once
    assert M.euler_characteristic(tri) == truth["euler"]
    vec = M.triangle_vectors(xyz, tri)
    assert (np.einsum("ij,ij->i", vec, M.solid_gradient(name, xyz[tri.astype(np.int64)].mean(axis=1))) > 0).all()  # along the gradient: into positive D
    has = ~np.isnan(nrm[:, 0])
    assert has.all() and (np.einsum("ij,ij->i", nrm, M.solid_gradient(name, xyz)) > 0.9).all()  # rule 3's normals point the same way
    bar = SOLID_DEFICIT[name]
    assert bar[0] / MARGIN <= vol_deficit <= MARGIN * bar[0] and bar[1] / MARGIN <= area_deficit <= MARGIN * bar[1]


def test_random_field_has_balanced_half_edges():
    """random signs inside a shell of positive voxels: no crossing reaches the grid's boundary, so the mesh has none"""
    D, W = M.sign_field((14, 13, 12), 21)
    shell = np.ones_like(D, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    D[shell] = np.abs(D[shell])
    xyz, _, tri = M.mesh(M.unit_volume((14, 13, 12), D, W))
    assert len(tri) > 2000 and len(M.unbalanced_edges(tri)) == 0
    assert M.max_half_edge_multiplicity(tri) == 2  # non-manifold along fan diagonals, as stated: never more than 2
    # without the shell the boundary is on the grid's faces alone
    D, W = M.sign_field((14, 13, 12), 21)
    xyz, _, tri = M.mesh(M.unit_volume((14, 13, 12), D, W))
    open_edges = M.unbalanced_edges(tri)
    assert len(open_edges) > 0
    for u, v, _ in open_edges:
        on_face = [(xyz[u, c] == xyz[v, c]) and xyz[u, c] in (0.0, float(n - 1)) for c, n in enumerate((14, 13, 12))]
        assert any(on_face)


def test_weight_hole_opens_a_boundary_next_to_dead_cells_only():
    vol, _ = field_volume("weight_hole")
    xyz, _, tri = M.mesh(vol)
    _, live = M.cell_cases(vol, 1.0)
    open_edges = M.unbalanced_edges(tri)
    assert len(open_edges) > 8 and (open_edges[:, 2] == 1).all()
    assert not live.all() and len(np.unique(tri)) < len(xyz)  # points of the extract that no live cell touches stay, unreferenced
    for u, v, _ in open_edges:
        pu, pv = xyz[u], xyz[v]
        axes = [c for c in range(3) if pu[c] == pv[c] and pu[c] == np.floor(pu[c])]
        assert len(axes) == 1  # the segment lies in one lattice plane: a cell face
        a = axes[0]
        cell = np.floor(0.5 * (pu + pv)).astype(int)
        sides = []
        for s in (-1, 0):
            c = cell.copy()
            c[a] = int(pu[a]) + s
            inside = all(0 <= c[d] < n - 1 for d, n in enumerate(vol.shape))
            sides.append(bool(inside and live[c[2], c[1], c[0]]))
        assert sorted(sides) == [False, True]  # one cell of the face is live, the other is not


def test_exact_zeros_keep_their_zero_area_triangles():
    vol, _ = field_volume("zero_sphere")
    assert (vol.D == 0).sum() >= 6  # the lattice points at distance exactly 6 along the axes, and more
    xyz, _, tri = M.mesh(vol)
    zero = np.linalg.norm(M.triangle_vectors(xyz, tri), axis=1) == 0.0
    assert (len(tri), int(zero.sum())) == ZERO_SPHERE
    assert len(M.unbalanced_edges(tri)) == 0 and M.euler_characteristic(tri) == 2


# ---- the Python layer on the host ----------------------------------------------------------------------------------------------------------
def test_mesh_statistics_and_compact():
    vol, _ = field_volume("weight_hole")
    xyz, nrm, tri = M.mesh(vol)
    m = cal.Mesh(xyz, nrm, tri)
    assert m.area() == M.area(xyz, tri) and m.volume() == M.volume(xyz, tri)
    want = M.unbalanced_edges(tri)
    assert np.array_equal(m.boundary_edges(), np.repeat(want[:, :2], want[:, 2], axis=0))
    c = m.compact()
    used = np.unique(tri)
    assert len(c.xyz) == len(used) < len(xyz) and same(c.xyz, xyz[used]) and same(c.normals, nrm[used])
    assert c.triangles.dtype == np.int32 and same(c.xyz[c.triangles.astype(np.int64)], xyz[tri.astype(np.int64)])  # the same corners, in order
    assert c.area() == m.area() and len(c.compact().xyz) == len(c.xyz)
    closed = cal.Mesh(*M.mesh(field_volume("sphere")[0]))
    assert closed.boundary_edges().shape == (0, 2) and same(closed.compact().triangles, closed.triangles)
    empty = cal.Mesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert empty.area() == 0.0 and empty.volume() == 0.0 and empty.boundary_edges().shape == (0, 2) and len(empty.compact().xyz) == 0


def test_ply_round_trip(tmp_path):
    closed = cal.Mesh(*M.mesh(field_volume("sphere")[0]))
    path = str(tmp_path / "sphere.ply")
    cal.write_ply(path, closed)
    head = open(path, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 676\nproperty double x\n") and b"property double nz\n" in head
    assert b"element face 1348\nproperty list uchar int vertex_indices\nend_header\n" in head
    assert os.path.getsize(path) == head.index(b"end_header\n") + 11 + 676 * 48 + 1348 * 13
    back = cal.read_ply(path)
    assert same(back.xyz, closed.xyz) and same(back.normals, closed.normals) and same(back.triangles, closed.triangles)
    # a mesh with NaN normals: left out by default, written when asked for
    holed = cal.Mesh(*M.mesh(field_volume("weight_hole")[0]))
    assert np.isnan(holed.normals).any()
    cal.write_ply(path, holed)
    back = cal.read_ply(path)
    assert b"property double nx" not in open(path, "rb").read(300)
    assert same(back.xyz, holed.xyz) and same(back.triangles, holed.triangles) and np.isnan(back.normals).all()
    cal.write_ply(path, holed, normals=True)
    assert same(cal.read_ply(path).normals, holed.normals)
    cal.write_ply(path, closed, normals=False)
    assert np.isnan(cal.read_ply(path).normals).all()
    empty = cal.Mesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    cal.write_ply(path, empty)
    back = cal.read_ply(path)
    assert back.xyz.shape == (0, 3) and back.triangles.shape == (0, 3) and back.triangles.dtype == np.int32
    with open(path, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        cal.read_ply(path)


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------
def test_driver_runs_clean_under_sanitizers():
    p = host_build.run_sanitized("mesh_cpu")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mesh_driver: 0 mismatches" in p.stdout and not p.stderr.strip(), p.stdout + p.stderr


# ---- the package and the library without a device ----------------------------------------------------------------------------------------
def test_package_exports():
    for name in ("Mesh", "write_ply", "read_ply"):
        assert hasattr(cal, name)
    assert hasattr(cal.TsdfVolume, "mesh")


def test_argument_errors_come_before_the_device(lib):
    bad = capi.CBA_ERR_INVALID_ARGUMENT
    n, m = np.zeros(1, np.int64), np.zeros(1, np.int64)
    assert lib.cba_tsdf_mesh(None, 1.0, capi.i64ptr(n), capi.i64ptr(m)) == bad and b"null" in lib.cba_last_error()
    assert lib.cba_tsdf_mesh_fetch(None, capi.i32ptr(np.zeros((1, 3), np.int32))) == bad
