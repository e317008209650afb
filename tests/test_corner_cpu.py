"""CPU tier of chessboard detection: the host build of calibration_amd/csrc/corner_math.hpp and corner_grid.hpp (tests/corner_cpu,
compiled here) against the independent numpy restatement tests/corner_ref.py, the grid order of cba_chessboard_order (host code of
the library, needs no device) on hand-made lattices, the restatement against rendered boards, and the argument errors of the C ABI
and of the Python layer (raised before any device work)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from calibration_amd import capi, detect
from tests import corner_ref as S
from tests import host_build


@pytest.fixture(scope="module")
def host():
    return host_build.load("corner_cpu")


# ---- the header against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [S.NONE, S.COG, S.GRADIENT])
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}_n{s[2]}")
def test_header_matches_restatement(host, size, refine):
    H, W, n = size
    o = S.Options(1, 2, 2, refine, 3, 4)
    images = S.smooth_random(n, H, W)
    ref = S.detect_cached((H, W, n, o), images, o, 64)
    got = S.host_detect(host, images, o, 64, want_response=True)
    assert np.array_equal(got["R"], np.stack([S.response(im) for im in images]))
    # response, peaks, COG and angle to the bit; GRADIENT within the fp64 parity bar with equal flags
    assert S.same_result(got, ref, xy_tol=1e-9 if refine == S.GRADIENT else 0.0)
    if min(H, W) >= 31:
        assert ref["count"].min() > 0


@pytest.mark.parametrize("case", S.planted_cases(), ids=lambda c: c[0])
def test_header_planted_cases(host, case):
    name, images, o, max_corners = case
    ref = S.detect_cached(name, images, o, max_corners)
    got = S.host_detect(host, images, o, max_corners)
    assert S.same_result(got, ref, xy_tol=1e-9 if o.refine == S.GRADIENT else 0.0)


def test_planted_cases_are_what_they_claim():
    cases = {c[0]: c for c in S.planted_cases()}
    _, images, o, m = cases["ties_on_tile_edges"]
    ref = S.detect_cached("ties_on_tile_edges", images, o, m)
    for i, (px, py) in enumerate(((63, 15), (64, 16))):  # four equal responses round the tile corner (64, 16): the lowest index wins
        Rm = S.response(images[i])
        assert len({int(Rm[py + a, px + b]) for a in (0, 1) for b in (0, 1)}) == 1 and Rm[py, px] > 0
        assert [px + 0.5, py + 0.5] in ref["xy"][i, :ref["count"][i]].tolist()  # the COG of a symmetric tie
    none = S.detect(images, o._replace(refine=S.NONE), m)
    assert [63.0, 15.0] in none["xy"][0].tolist() and [64.0, 16.0] in none["xy"][1].tolist()
    assert [64.0, 15.0] not in none["xy"][0].tolist() and [63.0, 16.0] not in none["xy"][0].tolist()
    ref = S.detect_cached("constant_and_split", *cases["constant_and_split"][1:])
    assert (ref["count"] == 0).all() and np.isnan(ref["xy"]).all()
    ref = S.detect_cached("borders", *cases["borders"][1:])
    for i, (_, expected) in enumerate(S.border_images()):
        assert [(int(y), int(x)) for x, y in ref["xy"][i, :ref["count"][i]]] == expected
    ref = S.detect_cached("overflow", *cases["overflow"][1:])
    full = S.detect_cached("ties_on_tile_edges", images, o, m)
    assert (ref["count"] == 16).all() and (ref["status"] == 1).all()
    assert np.array_equal(ref["xy"][0], full["xy"][1, :3]) and np.array_equal(ref["xy"][1], full["xy"][0, :3])  # the first ones are kept
    ref = S.detect_cached("empty_between", *cases["empty_between"][1:])
    assert ref["count"].tolist() == [16, 0, 16]
    ref = S.detect_cached("gradient_window_flag", *cases["gradient_window_flag"][1:])
    assert ref["flags"][:, 0].tolist() == [S.FLAG_WINDOW, 0]


def test_sizes_cover_the_kernels_tile_and_strip_edges():
    """the tile and strip constants that SIZES and the planted cases are built round are the ones in the kernel source, and SIZES
    holds every edge they define: a change of CRN_TX, CRN_TY or CRN_SH fails here until the sizes follow"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "corner_detect.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(CRN_TX|CRN_TY|CRN_SH) = (\d+)", src)}
    assert (const["CRN_TX"], const["CRN_TY"], const["CRN_SH"]) == (S.TILE_W, S.TILE_H, S.STRIP_H)
    heights, widths = {s[0] for s in S.SIZES}, {s[1] for s in S.SIZES}
    for edge in {S.STRIP_H, S.TILE_H}:  # one row less and one more than a strip (a tile), one strip, and the same round two
        assert {edge - 1, edge, edge + 1, 2 * edge - 1, 2 * edge, 2 * edge + 1} <= heights
    assert {S.TILE_W - 1, S.TILE_W, S.TILE_W + 1, 2 * S.TILE_W - 1, 2 * S.TILE_W, 2 * S.TILE_W + 1} <= widths
    assert any(w % 4 and w > S.TILE_W for w in widths) and any(w % 16 == 0 and w % S.TILE_W for w in widths)
    assert 11 in heights and 11 in widths and max(s[2] for s in S.SIZES) >= 3
    # the planted ties of 16-pixel squares lie on a tile edge and on a strip edge
    assert 64 % S.TILE_W == 0 and 16 % S.TILE_H == 0 and 16 % S.STRIP_H == 0


def test_tables(host):
    for w in (1, 5, 10):
        wt, trig = np.empty((2 * w + 1, 2 * w + 1)), np.empty(16)
        host.cr_tables(C.c_int(w), wt.ctypes.data_as(C.c_void_p), trig.ctypes.data_as(C.c_void_p))
        c, s = S.trig_table()
        assert np.array_equal(wt, S.weight_table(w)) and np.array_equal(trig, np.array(c + s))
    th = [math.atan2(dy, dx) for dx, dy in S.RING[:8]]
    assert np.abs(np.cos(2 * np.array(th)) - np.array(c)).max() < 1e-15 and np.abs(np.sin(2 * np.array(th)) - np.array(s)).max() < 1e-15


def test_selfcheck_under_sanitizers():
    """the stand-alone driver program (its own main), built under the address and undefined-behaviour sanitizers, runs clean"""
    r = host_build.run_sanitized("corner_cpu")
    assert r.returncode == 0 and "corner self-check: ok" in r.stdout, r.stdout + r.stderr


# ---- grid order -------------------------------------------------------------------------------------------------------------------------
def _lattice(rows, cols, turn_deg=0.0, mirror=False, pitch=20.0, origin=(100.0, 80.0), shear=0.0):
    """corners of a rows x cols lattice in a shuffled order with the angles a chessboard gives them: the bisector lies at 45 degrees to
    the lattice axes and turns by pi/2 from a corner to its neighbour"""
    jj, ii = np.divmod(np.arange(rows * cols), cols)
    base = np.stack([ii * pitch + shear * jj * pitch, jj * pitch], axis=1)
    ang = np.pi / 4 + ((ii + jj) % 2) * (np.pi / 2)
    if mirror:
        base[:, 0] = -base[:, 0]
        ang = np.pi - ang
    t = math.radians(turn_deg)
    Rm = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
    xy = base @ Rm.T + np.asarray(origin)
    ang = ang + t
    perm = np.random.default_rng(int(turn_deg) + rows).permutation(rows * cols)
    return xy[perm], ang[perm]


def _all_orders(lib, host, xy, ang, rows, cols):
    out = [detect.order_chessboard(xy, ang, rows, cols), S.host_order(host, xy, ang, rows, cols), S.order(xy, ang, rows, cols)]
    if out[0] is None:
        assert out[1] is None and out[2] is None
        return None
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    return out[0]


def _check_canonical(xy, index, rows, cols, pitch=20.0):
    """index orders all of an unsheared rows x cols lattice of xy: every step along i and along j is one pitch (to the rounding of
    coordinates of a few hundred px, far below 1e-9 px) and the frame is right-handed; returns the mean steps"""
    assert sorted(index.tolist()) == list(range(rows * cols))  # every corner exactly once
    P = xy[index].reshape(rows, cols, 2)
    di, dj = P[:, 1:] - P[:, :-1], P[1:] - P[:-1]
    assert np.abs(np.linalg.norm(di, axis=2) - pitch).max() < 1e-9  # neighbours along i are lattice neighbours
    assert np.abs(np.linalg.norm(dj, axis=2) - pitch).max() < 1e-9  # and along j
    mi, mj = di.mean(axis=(0, 1)), dj.mean(axis=(0, 1))
    assert mi[0] * mj[1] - mi[1] * mj[0] > 0  # right-handed with x right, y down
    return mi, mj


@pytest.mark.parametrize("turn", [0.0, 100.0, 180.0, 250.0])
@pytest.mark.parametrize("rows,cols", [(6, 9), (4, 7), (5, 5)])
def test_order_turned_lattices(lib, host, rows, cols, turn):
    xy, ang = _lattice(rows, cols, turn)
    index = _all_orders(lib, host, xy, ang, rows, cols)
    assert index is not None
    mi, mj = _check_canonical(xy, index, rows, cols)
    assert np.abs(np.linalg.norm(mi) - 20.0) < 1e-9 and np.abs(np.linalg.norm(mj) - 20.0) < 1e-9
    if rows == cols:  # four turns remain: the i-step is the lattice direction with the largest x
        assert mi[0] >= 20.0 * math.cos(math.radians(45.0)) - 1e-9
    else:  # a half turn remains
        assert mi[0] >= -1e-9


def test_order_perfect_lattice_is_the_identity(lib, host):
    xy, ang = _lattice(6, 9)
    inv = np.lexsort((xy[:, 0], xy[:, 1]))  # the row-major order of the unshuffled lattice
    assert np.array_equal(_all_orders(lib, host, xy, ang, 6, 9), inv)
    assert np.array_equal(_all_orders(lib, host, xy[inv], ang[inv], 6, 9), np.arange(54))


def test_order_missing_spurious_and_mirrored(lib, host):
    xy, ang = _lattice(6, 9, 30.0, shear=0.15)
    assert _all_orders(lib, host, xy[1:], ang[1:], 6, 9) is None  # one corner removed
    assert _all_orders(lib, host, xy, ang, 5, 9) is None  # another board
    far = np.array([[400.0, 300.0]])
    index = _all_orders(lib, host, np.r_[xy, far], np.r_[ang, 0.3], 6, 9)  # one spurious corner off the board: found, and ignored
    assert index is not None and 54 not in index.tolist()
    assert np.array_equal(index, _all_orders(lib, host, xy, ang, 6, 9))
    xm, am = _lattice(6, 9, 30.0, mirror=True)
    index = _all_orders(lib, host, xm, am, 6, 9)
    assert index is not None
    _check_canonical(xm, index, 6, 9)  # still right-handed after labelling
    with pytest.raises(ValueError):
        detect.order_chessboard(xy, ang, 1, 9)
    with pytest.raises(ValueError):
        detect.order_chessboard(np.r_[xy, [[np.nan, 0.0]]], np.r_[ang, 0.0], 6, 9)
    with pytest.raises(ValueError):
        detect.order_chessboard(xy, ang[:-1], 6, 9)


# ---- the restatement on rendered boards ------------------------------------------------------------------------------------------------
SCENE_SEED, restatement_boards = S.SCENE_SEED, S.restatement_boards


@pytest.mark.parametrize("refine", [S.NONE, S.COG, S.GRADIENT])
def test_restatement_finds_every_rendered_board(refine):
    sc = S.scene(SCENE_SEED)
    rms = []
    for (found, uv, n_peaks), truth in zip(restatement_boards(refine), sc["truth"]):
        assert found and n_peaks == S.ROWS * S.COLS  # every board, zero false peaks
        rms.append(S.match_truth(uv, truth))
    print("refine", refine, "per view (rms, max) px:", [(round(a, 3), round(b, 3)) for a, b in rms])
    # the corner is a saddle of the blurred image, so every mode must beat rounding to a pixel (RMS 0.41 px) except NONE, which is it
    assert max(r for r, _ in rms) < (0.5 if refine == S.NONE else 0.25)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
def test_create_rejects_bad_arguments(lib):
    def create(W=64, H=48, n=1, m=16, **kw):
        o = capi.CbaCornerOptions(400, 3, 2, 2, 5, 5)
        for k, v in kw.items():
            setattr(o, k, v)
        h = C.c_void_p()
        return lib.cba_corner_detector_create(W, H, n, m, C.byref(o), 0, C.byref(h))

    bad = [dict(W=10), dict(H=10), dict(W=40000), dict(n=0), dict(m=0), dict(min_response=0), dict(min_response=10201), dict(nms_radius=0),
           dict(nms_radius=11), dict(cog_radius=0), dict(cog_radius=6), dict(refine=3), dict(refine=-1), dict(refine_half_window=0),
           dict(refine_half_window=11), dict(refine_iterations=0), dict(n=70000, W=32768, H=32768)]
    for kw in bad:
        assert create(**kw) == capi.CBA_ERR_INVALID_ARGUMENT, kw
    assert lib.cba_corner_detector_create(64, 48, 1, 16, None, 0, C.byref(C.c_void_p())) == capi.CBA_ERR_INVALID_ARGUMENT
    assert lib.cba_corner_detector_process(None, 1, None, None, None, None, None, None, None) == capi.CBA_ERR_INVALID_ARGUMENT
    lib.cba_corner_detector_destroy(None)
    o = capi.CbaCornerOptions()
    lib.cba_corner_options_default(C.byref(o))
    assert (o.min_response, o.nms_radius, o.cog_radius, o.refine, o.refine_half_window, o.refine_iterations) == (400, 3, 2, 2, 5, 5)
    d = detect.CornerOptions()
    assert (d.min_response, d.nms_radius, d.cog_radius, d.refine, d.refine_half_window, d.refine_iterations) == (400, 3, 2, 2, 5, 5)
    if lib.cba_device_count() <= 0:  # without a device a valid create fails loudly
        assert create() == capi.CBA_ERR_NO_DEVICE
