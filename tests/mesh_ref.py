"""Independent numpy restatement of scan meshing as calibba.h states it (cba_tsdf_mesh, item 4 of the scan-fusion block): the table of
triangles per sign pattern, generated from the rule with code of its own (corners and edges as coordinate tuples, face cycles rotated
to start outside a run; tsdf_mesh_math.hpp works on bit patterns), and the mesh of a fusion_ref.Volume, vectorised: the index of an
edge is a cumulative sum over the extract's mask, the cases and the table lookups are array operations.  Every output is an integer,
so the device and the host build are held to it bit for bit.  Also the fields of both tiers (sphere, torus, all cases, random signs,
the weight hole), the mesh statistics the tests use as checks, and the wrappers of the host build (tests/mesh_cpu).  Test
infrastructure: no product code is imported here.
"""

import numpy as np

from tests import fusion_ref as F
from tests.host_build import ptr

MESH_BLOCK = 256  # lanes per workgroup of k_tsdf_mesh (tsdf_fusion.hip: TSDF_BLOCK)
MESH_TILE = 1024  # cells per workgroup (tsdf_math.hpp: TSDF_EXTRACT_TILE; the mesh walks the extract's tiles)
GROUP = 64        # voxels per edge record (tsdf_mesh_math.hpp: TSDF_MESH_GROUP)
SLOTS = 15        # edge numbers per table word (tsdf_mesh_math.hpp: TSDF_MESH_SLOTS)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def corner_number(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def edge_number(p, q):
    """the local edge between two corners (coordinate triples) that differ along one axis"""
    axis = [c for c in range(3) if p[c] != q[c]]
    assert len(axis) == 1
    axis = axis[0]
    lower = min(p, q)
    u, v = [lower[c] for c in range(3) if c != axis]
    return 4 * axis + u + 2 * v


def face_cycle(a, s):
    """the four corners of the face across axis a on side s, counter-clockwise seen from outside for s = 1, reversed for s = 0"""
    b, c = (a + 1) % 3, (a + 2) % 3
    out = []
    for ub, uc in ((0, 0), (1, 0), (1, 1), (0, 1)):
        p = [0, 0, 0]
        p[a], p[b], p[c] = s, ub, uc
        out.append(tuple(p))
    return out if s == 1 else out[::-1]


def face_segments(a, s, negative):
    """the directed segments (from edge, to edge) of one face; negative: corner triple -> bool"""
    cyc = face_cycle(a, s)
    signs = [negative(p) for p in cyc]
    if all(signs) or not any(signs):
        return []
    start = signs.index(False)  # rotate: the walk starts at a positive corner, so no run wraps around
    cyc, signs = cyc[start:] + cyc[:start], signs[start:] + signs[:start]
    cyc, signs = cyc + cyc[:1], signs + signs[:1]
    out, enter = [], None
    for n in range(4):
        if not signs[n] and signs[n + 1]:
            enter = edge_number(cyc[n], cyc[n + 1])
        if signs[n] and not signs[n + 1]:
            out.append((enter, edge_number(cyc[n], cyc[n + 1])))
    return out


def case_loops(case):
    """the closed loops of one case, in ascending order of their lowest edge, each from its lowest edge"""
    negative = lambda p: bool((case >> corner_number(p)) & 1)
    follow, heads = {}, []
    for a in range(3):
        for s in range(2):
            for tail, head in face_segments(a, s, negative):
                assert tail not in follow  # every crossing edge is the tail of exactly one segment
                follow[tail] = head
                heads.append(head)
    assert sorted(heads) == sorted(follow)  # and the head of exactly one: the loops are closed
    loops, left = [], set(follow)
    while left:
        first = min(left)
        loop, e = [first], follow[first]
        while e != first:
            loop.append(e)
            e = follow[e]
        left -= set(loop)
        loops.append(loop)
    return loops


def case_triangles(case):
    return [(lp[0], lp[n], lp[n + 1]) for lp in case_loops(case) for n in range(1, len(lp) - 1)]


_table = {}


def table():
    """-> count [256], edges [256][SLOTS] (three per triangle), words uint64 [256] in the header's packing"""
    if not _table:
        count, edges, words = np.zeros(256, np.int64), np.zeros((256, SLOTS), np.int64), np.zeros(256, np.uint64)
        for c in range(256):
            flat = [e for t in case_triangles(c) for e in t]
            count[c] = len(flat) // 3
            edges[c, :len(flat)] = flat
            words[c] = np.uint64(sum(e << (4 * n) for n, e in enumerate(flat)) | (len(flat) // 3) << 60)
        _table.update(count=count, edges=edges, words=words)
    return _table["count"], _table["edges"], _table["words"]


# ---- the mesh of a volume --------------------------------------------------------------------------------------------------------------
def edge_mask(vol, min_weight):
    """rule 3's qualifying edges [nz][ny][nx][3]"""
    nx, ny, nz = vol.shape
    heavy, neg = vol.W.astype(np.float64) >= min_weight, vol.D.astype(np.float64) < 0.0
    q = np.zeros((nz, ny, nx, 3), bool)
    q[:, :, :-1, 0] = heavy[:, :, :-1] & heavy[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    q[:, :-1, :, 1] = heavy[:, :-1, :] & heavy[:, 1:, :] & (neg[:, :-1, :] != neg[:, 1:, :])
    q[:-1, :, :, 2] = heavy[:-1, :, :] & heavy[1:, :, :] & (neg[:-1, :, :] != neg[1:, :, :])
    return q, heavy, neg


def cell_cases(vol, min_weight):
    """-> case [nz-1][ny-1][nx-1], live of the same shape"""
    nx, ny, nz = vol.shape
    _, heavy, neg = edge_mask(vol, min_weight)
    case, live = np.zeros((nz - 1, ny - 1, nx - 1), np.int64), np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
                case |= neg[sl].astype(np.int64) << corner_number((dx, dy, dz))
                live &= heavy[sl]
    return case, live


def triangles(vol, min_weight=1.0):
    """-> int32 [n][3] indices into vol.extract(min_weight)'s points: cells in ascending l, the table's order inside a cell"""
    q, _, _ = edge_mask(vol, min_weight)
    index = (np.cumsum(q.ravel(), dtype=np.int64) - 1).reshape(q.shape)
    case, live = cell_cases(vol, min_weight)
    count, edges, _ = table()
    n_tri = np.where(live, count[case], 0)
    k, j, i = np.nonzero(n_tri)  # row-major: ascending l of corner 0
    cs, nt = case[k, j, i], n_tri[k, j, i]
    slot = np.arange(5)[None, :] < nt[:, None]
    cell, t = np.nonzero(slot)   # per cell, its triangles in order
    out = np.zeros((len(cell), 3), np.int64)
    for c in range(3):
        e = edges[cs[cell], 3 * t + c]
        axis, u, v = e >> 2, e & 1, (e >> 1) & 1
        di = np.where(axis == 0, 0, u)
        dj = np.where(axis == 0, u, np.where(axis == 1, 0, v))
        dk = np.where(axis == 2, 0, v)
        assert q[k[cell] + dk, j[cell] + dj, i[cell] + di, axis].all()  # every crossing edge of a live cell is a point of the extract
        out[:, c] = index[k[cell] + dk, j[cell] + dj, i[cell] + di, axis]
    return out.astype(np.int32)


def mesh(vol, min_weight=1.0):
    """-> xyz [n][3], normals [n][3], triangles int32 [m][3]"""
    xyz, nrm = vol.extract(min_weight)
    return xyz, nrm, triangles(vol, min_weight)


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def half_edges(tri):
    """the directed edges of all triangles [3 m][2]"""
    t = np.asarray(tri, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def unbalanced_edges(tri):
    """the directed edges u -> v whose count differs from that of v -> u, with the difference: [n][3] (u, v, count(u->v) - count(v->u) > 0)"""
    h = half_edges(tri)
    if len(h) == 0:
        return np.zeros((0, 3), np.int64)
    both = np.concatenate([h, h[:, ::-1]])
    sign = np.concatenate([np.ones(len(h), np.int64), -np.ones(len(h), np.int64)])
    uniq, inv = np.unique(both, axis=0, return_inverse=True)
    net = np.bincount(inv.ravel(), weights=sign).astype(np.int64)
    keep = net > 0
    return np.column_stack([uniq[keep], net[keep]])


def max_half_edge_multiplicity(tri):
    h = half_edges(tri)
    return int(np.unique(h, axis=0, return_counts=True)[1].max()) if len(h) else 0


def euler_characteristic(tri):
    """V - E + F over the referenced vertices and the undirected edges"""
    t = np.asarray(tri, dtype=np.int64)
    und = np.sort(half_edges(t), axis=1)
    return len(np.unique(t)) - len(np.unique(und, axis=0)) + len(t)


def triangle_vectors(xyz, tri):
    """(p1 - p0) x (p2 - p0) per triangle"""
    p = xyz[np.asarray(tri, dtype=np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def area(xyz, tri):
    return float(0.5 * np.linalg.norm(triangle_vectors(xyz, tri), axis=1).sum())


def volume(xyz, tri):
    """the enclosed volume by the divergence theorem; the triangles' vectors point into positive D, out of the solid where D < 0"""
    p = xyz[np.asarray(tri, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- fields ----------------------------------------------------------------------------------------------------------------------------
SOLID_SHAPE, SOLID_CENTRE = (20, 20, 20), np.array([9.3, 9.7, 10.1])
SPHERE_RADIUS = 6.0
TORUS_R, TORUS_r = 5.5, 2.2


def unit_volume(shape, D, W=None):
    """a Volume on the unit lattice (origin 0, voxel 1: points are in voxels) holding the planes given"""
    v = F.Volume(shape, np.zeros(3), 1.0, 3.0)
    v.D = np.ascontiguousarray(D, dtype=np.float32)
    v.W = np.ones_like(v.D) if W is None else np.ascontiguousarray(W, dtype=np.float32)
    return v


def lattice(shape):
    nx, ny, nz = shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    return x, y, z


def sphere_distance(x, y, z, centre=SOLID_CENTRE):
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - SPHERE_RADIUS


def torus_distance(x, y, z, centre=SOLID_CENTRE):
    ring = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - TORUS_R
    return np.sqrt(ring ** 2 + (z - centre[2]) ** 2) - TORUS_r


def solid(name, centre=SOLID_CENTRE):
    """'sphere' | 'torus' -> the Volume with D = clip(distance / 3) in float32 and W = 1"""
    dist = (sphere_distance if name == "sphere" else torus_distance)(*lattice(SOLID_SHAPE), centre=centre)
    return unit_volume(SOLID_SHAPE, np.clip(dist / 3.0, -1.0, 1.0))


def solid_gradient(name, p):
    """the analytic gradient direction of a solid's distance at points [n][3]"""
    d = p - SOLID_CENTRE
    if name == "sphere":
        return d / np.linalg.norm(d, axis=1)[:, None]
    rho = np.linalg.norm(d[:, :2], axis=1)
    ring = rho - TORUS_R
    g = np.column_stack([ring * d[:, 0] / rho, ring * d[:, 1] / rho, d[:, 2]])
    return g / np.linalg.norm(g, axis=1)[:, None]


SOLID_TRUTH = {"sphere": dict(volume=4.0 / 3.0 * np.pi * SPHERE_RADIUS ** 3, area=4.0 * np.pi * SPHERE_RADIUS ** 2, euler=2),
               "torus": dict(volume=2.0 * np.pi ** 2 * TORUS_R * TORUS_r ** 2, area=4.0 * np.pi ** 2 * TORUS_R * TORUS_r, euler=0)}

ALL_CASES_SHAPE = (767, 2, 2)


def all_cases_field(seed=0):
    """nx = 767, ny = nz = 2: cell i = 3 c carries case c; magnitudes random in [0.1, 1]; W = 1"""
    nx, ny, nz = ALL_CASES_SHAPE
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.1, 1.0, (nz, ny, nx)).astype(np.float32)
    for c in range(256):
        for q in range(8):
            if (c >> q) & 1:
                D[q >> 2, (q >> 1) & 1, 3 * c + (q & 1)] *= -1
    return D, np.ones_like(D)


def one_cell_field(case):
    """2 x 2 x 2 with the sign pattern given, magnitudes 0.25 + q / 16"""
    D = np.array([(-1.0 if (case >> q) & 1 else 1.0) * (0.25 + q / 16.0) for q in range(8)], np.float32).reshape(2, 2, 2)
    return D, np.ones_like(D)


def sign_field(shape, seed, negative=0.5):
    """random signs with magnitudes in [0.1, 1]; W = 1"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.1, 1.0, (nz, ny, nx)).astype(np.float32)
    D[rng.random((nz, ny, nx)) < negative] *= -1
    return D, np.ones_like(D)


def weight_field(shape, seed):
    """random signs and W of 0, 1 and 2 scattered (mostly 2, so that cells stay live at min_weight = 2)"""
    D, _ = sign_field(shape, seed)
    rng = np.random.default_rng(seed + 500)
    W = rng.choice(np.array([0, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2], np.float32), D.shape)
    return D, W


def flat_sparse_field():
    """FLAT_SHAPE: observed blocks of 3 x 3 x 2 voxels scattered thinly, random multiples of 1/8 inside them"""
    nx, ny, nz = F.FLAT_SHAPE
    rng = np.random.default_rng(11)
    D = (rng.integers(-8, 9, (nz, ny, nx)) / 8.0).astype(np.float32)
    seed = rng.random((ny, nx)) < 0.01
    seen = seed.copy()
    for dj in range(3):
        for di in range(3):
            seen[dj:, di:] |= seed[:ny - dj, :nx - di]
    return D, np.ascontiguousarray(np.broadcast_to(seen, (nz, ny, nx))).astype(np.float32)


def weight_hole():
    """the sphere with a block of unobserved voxels across its surface, and the four diagonal neighbours of voxel (3, 10, 10) unobserved,
    so that no cell around the crossing edge (3, 10, 10) - (4, 10, 10) is live and its point stays unreferenced -> D, W"""
    v = solid("sphere")
    W = v.W.copy()
    W[9:12, 8:12, 14:18] = 0.0
    for dk, dj in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
        W[10 + dk, 10 + dj, 3] = 0.0
    return v.D, W


def zero_sphere():
    """a sphere of radius 6 centred on the lattice point (10, 10, 10): the corners at distance exactly 6 have D = 0"""
    return solid("sphere", centre=np.array([10.0, 10.0, 10.0]))


# ---- the host build (tests/mesh_cpu) ---------------------------------------------------------------------------------------------------
def host_table(L):
    import ctypes as C

    words = np.zeros(256, np.uint64)
    L.mesh_host_table(words.ctypes.data_as(C.c_void_p))
    return words


def host_triangles(L, vol, min_weight=1.0):
    """the host build's triangles of vol's planes -> n_points, int32 [m][3]"""
    import ctypes as C

    D, W = np.ascontiguousarray(vol.D), np.ascontiguousarray(vol.W)
    nx, ny, nz = vol.shape
    L.mesh_host_triangles.restype = C.c_int64
    n_points = np.zeros(1, np.int64)
    args = (C.c_int(nx), C.c_int(ny), C.c_int(nz), ptr(D), ptr(W), C.c_double(min_weight), ptr(n_points))
    m = L.mesh_host_triangles(*args, C.c_int64(0), None)
    tri = np.zeros((m, 3), np.int32)
    assert L.mesh_host_triangles(*args, C.c_int64(m), ptr(tri)) == m
    return int(n_points[0]), tri
