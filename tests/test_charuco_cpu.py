"""CPU tier of ChArUco detection: the host build of marker_math.hpp / marker_board.hpp (tests/charuco_cpu) and the library's host-only
entry points against the numpy restatement (tests/charuco_ref.py), on the cases the GPU tier runs and on planted lattices and votes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from calibration_amd import capi, detect
from tests import charuco_ref as S
from tests import host_build

READ_CASES = S.read_cases()
ARM_CASES = S.arm_cases()


@pytest.fixture(scope="module")
def host():
    return host_build.load("charuco_cpu")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _claims(case, rd):
    for t, e in enumerate(case["expect"] or []):
        if e is None:
            continue
        have = (int(rd[t]["flags"]), int(rd[t]["id"]), int(rd[t]["rotation"]), int(rd[t]["distance"]))
        assert all(x is None or x == h for x, h in zip(e, have)), (case["name"], t, e, have)


@pytest.mark.parametrize("case", READ_CASES, ids=[c["name"] for c in READ_CASES])
def test_host_read_matches_restatement(host, case):
    ref = S.read_reference(case)
    _claims(case, ref)  # the case is what it claims to be
    got = S.host_read(host, case["images"], case["cell_image"], case["quads"], case["board"], case["opts"])
    assert S.same_readings(got, ref, tol=1e-9)


def test_read_cases_cover_the_wave_and_workgroup_edges():
    """the constants the cases are built round are the ones in the kernel source"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "marker_read.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(MRK_BLOCK|MRK_WAVE) = (\d+)", src)}
    assert const["MRK_WAVE"] == S.WAVE and const["MRK_BLOCK"] // const["MRK_WAVE"] == S.WAVES_PER_GROUP
    cells = {(c["board"].marker_bits + 2) ** 2 for c in READ_CASES}
    assert any(v < S.WAVE for v in cells) and S.WAVE in cells and any(S.WAVE < v <= 2 * S.WAVE for v in cells)
    entries = {4 * len(c["board"].codes) for c in READ_CASES}
    assert {4, S.WAVE, S.WAVE + 4} <= entries and max(entries) >= 4000
    counts = {len(c["cell_image"]) for c in READ_CASES}
    assert {0, 1, S.WAVES_PER_GROUP - 1, S.WAVES_PER_GROUP, S.WAVES_PER_GROUP + 1} <= counts
    assert {c["opts"].cell_samples for c in READ_CASES} >= {1, 3, 5}


@pytest.mark.parametrize("case", ARM_CASES, ids=[c[0] for c in ARM_CASES])
def test_host_arms_match_restatement(host, case):
    name, images, m = case
    det, dirs, ref = S.arm_reference(name, images, m)
    got = S.host_arms(host, images, det["xy"], det["count"], dirs, S.DEFAULT)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and (np.abs(np.nan_to_num(got) - np.nan_to_num(ref)) <= 1e-9).all()
    assert np.array_equal(detect.arm_directions(det["angle"], S.DEFAULT.arm_fan_deg), dirs)


def test_arm_cases_are_what_they_claim():
    det, _, sc = S.arm_reference(*ARM_CASES[-1])  # junctions 12 px from a border: every arm counted, the full contrast, both polarities
    assert (det["count"][:8] == 1).all() and det["count"][8] == 0 and np.isnan(sc[8]).all() and np.isnan(sc[:8, 1:]).all()
    assert np.allclose(sc[:8, 0], 170.0, atol=1e-6)
    det, _, sc = S.arm_reference(*ARM_CASES[0])
    assert np.isnan(sc).all()  # 23 x 23 of smooth noise: no corner


# ---- dictionary ----------------------------------------------------------------------------------------------------------------------
def _lib_dictionary(lib, bits, count, dist, seed):
    return detect.marker_dictionary(bits, count, dist, seed)


@pytest.mark.parametrize("bits,count,dist,seed", [(4, 70, 4, 11), (3, 8, 2, 1), (6, 40, 10, 123456789012345), (7, 17, 14, 2 ** 64 - 1)])
def test_dictionary_reproducible_and_distant(lib, host, bits, count, dist, seed):
    ref = S.dictionary(bits, count, dist, seed)
    got = _lib_dictionary(lib, bits, count, dist, seed)
    assert np.array_equal(got, ref) and len(ref) == count
    buf = np.zeros(count, np.uint64)
    host.ch_dictionary.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
    assert host.ch_dictionary(bits, count, dist, seed, buf.ctypes.data_as(C.c_void_p)) == count and np.array_equal(buf, ref)
    table = S.rotated_table(ref, bits)
    for a, c in enumerate(ref):
        d = S.popcount(table ^ np.uint64(c))
        d[4 * a] = bits * bits
        assert d.min() >= dist
    assert not np.array_equal(_lib_dictionary(lib, bits, count, dist, seed ^ 1), ref)


def test_dictionary_reports_what_the_budget_found(lib):
    got = _lib_dictionary(lib, 3, 1000, 3, 1)  # 9 bits cannot hold 1000 codes three bits apart
    assert 0 < len(got) < 1000 and np.array_equal(got, S.dictionary(3, 1000, 3, 1))
    with pytest.raises(ValueError):
        _lib_dictionary(lib, 8, 4, 2, 0)
    with pytest.raises(ValueError):
        _lib_dictionary(lib, 4, 0, 2, 0)


# ---- lattice and board index ---------------------------------------------------------------------------------------------------------
def _plant(nx, ny, turn_deg=0.0, step=30.0, origin=(200.0, 160.0), shear=0.0):
    """the inner corners of a board: xy [nx ny][2], angle, the true (i, j); the board's x axis points along turn_deg in the image"""
    t = math.radians(turn_deg)
    a, b = np.array([math.cos(t), math.sin(t)]) * step, np.array([-math.sin(t) + shear, math.cos(t)]) * step
    jj, ii = np.divmod(np.arange(nx * ny), nx)
    xy = np.array(origin) + ii[:, None] * a + jj[:, None] * b
    mid = 0.5 * (math.atan2(a[1], a[0]) + math.atan2(b[1], b[0]) + (2 * math.pi if math.atan2(b[1], b[0]) < math.atan2(a[1], a[0]) else 0))
    ang = np.array([S.CR._wrap(mid + (0 if (i + j) % 2 == 0 else math.pi / 2), math.pi) for i, j in zip(ii, jj)])
    return xy, ang, np.stack([ii, jj], axis=1)


def _all_lattices(host, xy, ang, min_component=4):
    ref = S.lattice(xy, ang, min_component)
    comp, ij, k = detect.chessboard_lattice(xy, ang, min_component)
    n = len(ang)
    hc, hij = np.full(max(n, 1), -1, np.int32), np.zeros((max(n, 1), 2), np.int32)
    xyc, angc = np.ascontiguousarray(xy, float), np.ascontiguousarray(ang, float)
    host.ch_lattice.restype = C.c_int
    hk = host.ch_lattice(C.c_int(n), host_build.ptr(xyc), host_build.ptr(angc), C.c_int(min_component), host_build.ptr(hc), host_build.ptr(hij))
    for got in ((comp, ij, k), (hc[:n], hij[:n], hk)):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    return ref


def _right_handed(xy, comp, ij, k):
    at = {(int(i), int(j)): c for c, (i, j) in enumerate(ij) if comp[c] == k}
    si = [xy[at[(i + 1, j)]] - xy[c] for (i, j), c in at.items() if (i + 1, j) in at]
    sj = [xy[at[(i, j + 1)]] - xy[c] for (i, j), c in at.items() if (i, j + 1) in at]
    mi, mj = np.mean(si, axis=0), np.mean(sj, axis=0)
    return mi[0] * mj[1] - mi[1] * mj[0] > 0


def _plant_readings(board, xy, comp, ij, true_ij, drop=()):
    """the readings an ideal marker read would give: per complete lattice cell of a bright interior square its id and rotation"""
    cells, quads = S.cells_of(xy, comp, ij)
    at = {(int(comp[c]), int(ij[c, 0]), int(ij[c, 1])): c for c in range(len(comp)) if comp[c] >= 0}
    sq = S.marker_squares(board)
    flags, ids, rots = [], [], []
    for (k, i, j) in cells:
        c00, c10 = at[(k, i, j)], at[(k, i + 1, j)]
        corners = [at[(k, i, j)], at[(k, i + 1, j)], at[(k, i + 1, j + 1)], at[(k, i, j + 1)]]
        step = tuple(true_ij[c10] - true_ij[c00])
        r = {(1, 0): 0, (0, -1): 1, (-1, 0): 2, (0, 1): 3}[step]
        s = (int(true_ij[corners, 0].min()) + 1, int(true_ij[corners, 1].min()) + 1)
        bright = s in sq and len(ids) not in drop
        flags.append(0 if bright else S.LOW_CONTRAST)
        ids.append(sq.index(s) if s in sq else 0)
        rots.append(r)
    return cells, np.array(flags, np.int32), np.array(ids, np.int32), np.array(rots, np.int32)


def _all_matches(host, board, comp, ij, xy, cells, flags, ids, rots, min_markers=2):
    ref = S.match(board, comp, ij, xy, cells, flags, ids, rots, min_markers)
    b = detect.CharucoBoard(board.squares_x, board.squares_y, board.square, board.codes, board.marker_bits, board.marker_ratio)
    got = detect.charuco_match(b, comp, ij, xy, cells, flags, ids, rots, min_markers)
    nb = (board.squares_x - 1) * (board.squares_y - 1)
    oi, oxy, nm = np.full(nb, -1, np.int32), np.full((nb, 2), np.nan), np.zeros(1, np.int32)
    a = [np.ascontiguousarray(v, np.int32) for v in (comp, ij, cells, flags, ids, rots)]
    host.ch_match.restype = C.c_int
    cnt = host.ch_match(C.c_int(board.squares_x), C.c_int(board.squares_y), C.c_int(min_markers), C.c_int(len(comp)), host_build.ptr(a[0]), host_build.ptr(a[1]),
                        host_build.ptr(np.ascontiguousarray(xy, float)), C.c_int(len(cells)), host_build.ptr(a[2]), host_build.ptr(a[3]), host_build.ptr(a[4]), host_build.ptr(a[5]), host_build.ptr(oi), host_build.ptr(oxy),
                        host_build.ptr(nm))
    for g in (got, (oi[:cnt], oxy[:cnt], int(nm[0]))):
        assert np.array_equal(g[0], ref[0]) and np.array_equal(g[1], ref[1]) and g[2] == ref[2]
    return ref


BOARD = S.Board(8, 6, 0.025, 4, 0.6, S.cached_dictionary(4, 24, 3, 3))  # 7 x 5 inner corners


@pytest.mark.parametrize("turn", [8.0, 98.0, 188.0, 278.0])
def test_full_lattice_in_each_quarter_turn(host, turn):
    xy, ang, true_ij = _plant(7, 5, turn, shear=0.1)
    comp, ij, k = _all_lattices(host, xy, ang)
    assert k == 1 and (comp == 0).all() and len({tuple(v) for v in ij}) == 35 and _right_handed(xy, comp, ij, 0)
    cells, flags, ids, rots = _plant_readings(BOARD, xy, comp, ij, true_ij)
    assert len(cells) == 24 and (flags == 0).sum() == 12
    out_ids, out_xy, nm = _all_matches(host, BOARD, comp, ij, xy, cells, flags, ids, rots)
    assert np.array_equal(out_ids, np.arange(35)) and np.array_equal(out_xy, xy) and nm == 12


@pytest.mark.parametrize("side", ["left", "right", "top", "bottom"])
def test_lattice_cut_by_an_image_side(host, side):
    xy, ang, true_ij = _plant(7, 5, 20.0, origin=(60.0, 40.0))
    keep = {"left": xy[:, 0] > 95, "right": xy[:, 0] < 170, "top": xy[:, 1] > 100, "bottom": xy[:, 1] < 150}[side]
    assert 8 <= keep.sum() < 35
    xy, ang, true_ij = xy[keep], ang[keep], true_ij[keep]
    comp, ij, k = _all_lattices(host, xy, ang)
    assert k == 1 and _right_handed(xy, comp, ij, 0)
    cells, flags, ids, rots = _plant_readings(BOARD, xy, comp, ij, true_ij)
    out_ids, out_xy, nm = _all_matches(host, BOARD, comp, ij, xy, cells, flags, ids, rots)
    labelled = np.flatnonzero(comp == 0)
    assert len(out_ids) == len(labelled) >= keep.sum() - 4 and nm >= 2  # a corner tip with one link may leave
    assert np.array_equal(out_ids, np.sort(true_ij[labelled, 1] * 7 + true_ij[labelled, 0]))
    order = np.argsort(true_ij[labelled, 1] * 7 + true_ij[labelled, 0])
    assert np.array_equal(out_xy, xy[labelled][order])


def test_two_components_and_a_clash(host):
    xa, aa, ta = _plant(4, 5, 5.0, origin=(40.0, 40.0))
    xb, ab, tb = _plant(2, 5, 5.0, origin=(40.0 + 30.0 * 5.2, 60.0))  # the right part of the same board, too far to link
    tb = tb + np.array([5, 0])
    xy, ang, true_ij = np.concatenate([xa, xb]), np.concatenate([aa, ab]), np.concatenate([ta, tb])
    comp, ij, k = _all_lattices(host, xy, ang)
    assert k == 2 and (comp[:20] == 0).all() and (comp[20:] == 1).all()
    cells, flags, ids, rots = _plant_readings(BOARD, xy, comp, ij, true_ij)
    out_ids, _, nm = _all_matches(host, BOARD, comp, ij, xy, cells, flags, ids, rots)
    assert np.array_equal(out_ids, np.sort(true_ij[:, 1] * 7 + true_ij[:, 0]))
    # the smaller component claims the larger one's indices: it is dropped whole
    out_ids, _, _ = _all_matches(host, BOARD, comp, ij, xy, cells, flags, np.where(cells[:, 0] == 1, ids - 2, ids), rots)
    assert np.array_equal(out_ids, np.sort(ta[:, 1] * 7 + ta[:, 0]))


def test_a_false_corner_costs_itself_and_its_cell_mates(host):
    xy, ang, true_ij = _plant(7, 5, 12.0)
    for dx, dy, pol in ((11.0, 9.0, 0), (14.0, 15.0, 1), (6.0, 20.0, 1)):
        t = math.radians(12.0)
        p = xy[7 * 2 + 3] + np.array([dx * math.cos(t) - dy * math.sin(t), dx * math.sin(t) + dy * math.cos(t)])
        xy2, ang2 = np.concatenate([xy, p[None]]), np.concatenate([ang, [ang[pol]]])
        comp, ij, k = _all_lattices(host, xy2, ang2)
        lost = np.flatnonzero(comp[:35] != 0)
        cell_mates = {7 * 2 + 3, 7 * 2 + 4, 7 * 3 + 3, 7 * 3 + 4}
        assert set(lost) <= cell_mates, lost
        true2 = np.concatenate([true_ij, [[-9, -9]]])
        if comp[35] >= 0:  # it may keep a label only if that never becomes a board index
            continue
        cells, flags, ids, rots = _plant_readings(BOARD, xy2, comp, ij, true2)
        out_ids, out_xy, _ = _all_matches(host, BOARD, comp, ij, xy2, cells, flags, ids, rots)
        kept = np.flatnonzero(comp[:35] == 0)
        assert np.array_equal(out_ids, kept) and np.array_equal(out_xy, xy[kept])


def test_a_mirrored_lattice_is_made_right_handed(host):
    xy, ang, _ = _plant(6, 4, 15.0)
    xy_m = xy * np.array([-1.0, 1.0]) + np.array([600.0, 0.0])  # the picture mirrored: angles mirror too
    ang_m = np.array([S.CR._wrap(math.pi - a, math.pi) for a in ang])
    for p, a in ((xy, ang), (xy_m, ang_m), (xy[::-1].copy(), ang[::-1].copy())):
        comp, ij, k = _all_lattices(host, p, a)
        assert k == 1 and (comp == 0).all() and _right_handed(p, comp, ij, 0)


def test_votes_two_to_one_tie_and_foreign_ids(host):
    xy, ang, true_ij = _plant(7, 5, 3.0)
    comp, ij, _ = _all_lattices(host, xy, ang)
    cells, flags, ids, rots = _plant_readings(BOARD, xy, comp, ij, true_ij)
    good = np.flatnonzero(flags == 0)
    only = lambda keep: np.where(np.isin(np.arange(len(flags)), good[keep]), 0, S.NO_MATCH).astype(np.int32)
    wrong = ids.copy()
    wrong[good[2]] = ids[good[2]] + 1  # another square: another shift
    out_ids, _, nm = _all_matches(host, BOARD, comp, ij, xy, cells, only([0, 1, 2]), wrong, rots)
    assert np.array_equal(out_ids, np.arange(35)) and nm == 2  # 2 : 1
    out_ids, _, nm = _all_matches(host, BOARD, comp, ij, xy, cells, only([0, 2]), wrong, rots, min_markers=1)
    assert len(out_ids) == 0 and nm == 0  # 1 : 1 is rejected
    out_ids, _, _ = _all_matches(host, BOARD, comp, ij, xy, cells, only([0]), ids, rots)
    assert len(out_ids) == 0  # fewer than min_markers
    foreign = ids.copy()
    foreign[good[1:]] = 24 + np.arange(len(good) - 1)  # ids the board does not carry do not vote
    out_ids, _, nm = _all_matches(host, BOARD, comp, ij, xy, cells, flags, foreign, rots, min_markers=1)
    assert np.array_equal(out_ids, np.arange(35)) and nm == 1
    turned = (rots + 1) % 4  # every reading claims another quarter-turn: the corners land elsewhere or off the board, never doubled
    out_ids, _, _ = _all_matches(host, BOARD, comp, ij, xy, cells, flags, ids, turned)
    assert len(set(out_ids)) == len(out_ids)


def test_small_components_are_discarded(host):
    xy, ang, _ = _plant(2, 2, 0.0)
    assert _all_lattices(host, xy, ang, 4)[2] == 1 and _all_lattices(host, xy, ang, 5)[2] == 0
    assert _all_lattices(host, xy[:3], ang[:3], 1)[2] in (0, 1)
    assert _all_lattices(host, xy[:0], ang[:0])[2] == 0


def test_host_calls_reject_bad_arguments(lib):
    xy, ang, _ = _plant(3, 3)
    with pytest.raises(ValueError):
        detect.chessboard_lattice(xy, ang[:-1])
    with pytest.raises(ValueError):
        detect.chessboard_lattice(np.where(np.arange(18).reshape(9, 2) == 3, np.nan, xy), ang)
    with pytest.raises(ValueError):
        detect.chessboard_lattice(xy, ang, 0)
    b = detect.CharucoBoard(2, 6, 0.025, BOARD.codes)
    with pytest.raises(ValueError):
        detect.charuco_match(b, [0], [[0, 0]], [[1.0, 1.0]], np.zeros((0, 3)), [], [], [])
    b = detect.CharucoBoard(8, 6, 0.025, BOARD.codes)
    with pytest.raises(ValueError):
        detect.charuco_match(b, [0], [[0, 0]], [[1.0, 1.0]], np.zeros((1, 3)), [0], [0], [])
    with pytest.raises(ValueError):
        detect.charuco_match(b, [0], [[0, 0]], [[np.inf, 1.0]], np.zeros((0, 3)), [], [], [])
    assert b.object_points.shape == (35, 2) and tuple(b.object_points[8]) == (2 * 0.025, 2 * 0.025) and len(b.marker_squares) == 24


def test_selfcheck_under_sanitizers():
    """the stand-alone driver program (its own main), built under the address and undefined-behaviour sanitizers, runs clean over the
    planted cases"""
    r = host_build.run_sanitized("charuco_cpu")
    assert r.returncode == 0 and "charuco self-check: ok" in r.stdout, r.stdout + r.stderr


# ---- the scene of the GPU tier, by the restatement alone ----------------------------------------------------------------------------
def test_restatement_meets_the_scene_conditions():
    """In every view of the end-to-end scene (a board larger than the view) the restatement alone, with the default options,
    returns no wrong id, at least 80 % of the inner corners that lie 12 px or more inside the image, and at least 10 accepted
    readings.  Measured on seeds 1-3: 90-115 of 117 corners per view, 34-47 readings, RMS 0.033-0.093 px."""
    sc = S.scene("big", S.SCENE_SEED)
    res = S.detect(sc["images"], sc["board"], key=("scene", "big", S.SCENE_SEED))
    for r, truth in zip(res, sc["truth"]):
        err = np.linalg.norm(r["xy"] - truth[r["ids"]], axis=1)
        assert (err < 1.0).all()  # a wrong id is at least a square (26 px) off
        inside = np.flatnonzero((truth[:, 0] >= 12) & (truth[:, 0] <= S.W_IMG - 13) & (truth[:, 1] >= 12) & (truth[:, 1] <= S.H_IMG - 13))
        assert np.isin(inside, r["ids"]).sum() >= 0.8 * len(inside)
        assert (r["readings"]["flags"] == 0).sum() >= 10 and len(inside) < len(truth)
