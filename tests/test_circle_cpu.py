"""CPU tier of circle-grid detection: the host build of calibration_amd/csrc/blob_math.hpp and circle_grid.hpp (tests/circle_cpu,
compiled here) against the independent numpy restatement tests/circle_ref.py, the grid order of cba_circle_grid_order (host code of
the library, needs no device) on hand-made lattices, the restatement against rendered views, and the argument errors of the C ABI
and of the Python layer (raised before any device work)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from calibration_amd import capi, detect
from tests import circle_ref as S
from tests import host_build


@pytest.fixture(scope="module")
def host():
    return host_build.load("circle_cpu")


# ---- the header against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}_n{s[2]}")
def test_header_matches_restatement(host, size):
    H, W, n = size
    images = S.blobs_random(n, H, W)
    ref = S.detect_cached((H, W, n, S.SMALL), images, S.SMALL, 64)
    got = S.host_detect(host, images, S.SMALL, 64, want_response=True)
    Rm = [S.response(im, S.SMALL) for im in images]
    assert np.array_equal(got["R"], np.stack([r for r, _ in Rm])) and np.array_equal(got["S"], np.stack([s for _, s in Rm]))
    # g++ with -ffp-contract=off and numpy do the same IEEE operations in the same order: equal to the bit, well inside the 1e-9 bar
    for k in ref:
        assert S.bitwise(got[k], ref[k]), k
    if min(H, W) >= 31:
        assert ref["count"].min() > 0


@pytest.mark.parametrize("case", S.planted_cases(), ids=lambda c: c[0])
def test_header_planted_cases(host, case):
    name, images, o, max_blobs = case
    ref = S.detect_cached(name, images, o, max_blobs)
    got = S.host_detect(host, images, o, max_blobs)
    assert S.same_result(got, ref, 1e-9)


def test_planted_cases_are_what_they_claim():
    cases = {c[0]: c for c in S.planted_cases()}
    ref = {name: S.detect_cached(name, *c[1:]) for name, c in cases.items()}

    def clean(name, i=0):
        r = ref[name]
        k = min(int(r["count"][i]), r["xy"].shape[1])
        return [r["xy"][i, j].tolist() for j in range(k) if r["flags"][i, j] == 0]

    _, images, o, _ = cases["tie_on_tile_corner"]
    Rm, _ = S.response(images[0], o)
    assert 64 % S.TILE_W == 0 and 16 % S.TILE_H == 0 and 16 % S.STRIP_H == 0
    assert len({int(Rm[y, x]) for y in (15, 16) for x in (63, 64)}) == 1 and Rm[15, 63] > 0  # four tied responses round (64, 16)
    thr = o.min_contrast * 25 * (17 * 17 - 25)
    assert S.peaks(Rm, thr, o.nms_radius, o.b) == [(15, 63)]  # the lowest index wins
    (c,) = clean("tie_on_tile_corner")
    # one blob at the half-pixel centre: the start is 0.71 px off, and three centroid rounds of a 32-ray polygon leave a few 1e-3 px
    assert np.abs(np.array(c) - [63.5, 15.5]).max() < 0.01
    r = ref["constant_and_half_plane"]
    assert r["count"][0] == 0 and r["count"][1] > 0 and not clean("constant_and_half_plane", 1)
    assert (r["flags"][1, :r["count"][1]] & S.FLAG_NO_EDGE).all()
    r = ref["borders"]
    for i, (_, (cx, cy), inside) in enumerate(S.border_images(cases["borders"][2])):
        assert r["count"][i] == (1 if inside else 0)
        if inside:
            assert r["flags"][i, 0] == 0 and np.abs(r["xy"][i, 0] - [cx, cy]).max() < 0.05
    r = ref["ray_leaves_image"]
    assert r["count"][0] > 0 and (r["flags"][0, :r["count"][0]] == S.FLAG_WINDOW).all()
    r, full = ref["overflow"], ref["empty_between"]
    assert r["count"][0] == 3 and r["status"][0] == 1 and np.array_equal(r["xy"][0], full["xy"][0, :2])  # the first are kept
    assert full["count"].tolist() == [3, 0, 1] and full["status"].tolist() == [0, 0, 0]
    b = ref["bright"]
    assert np.array_equal(b["count"], full["count"]) and np.array_equal(b["flags"], full["flags"])
    assert np.nanmax(np.abs(b["xy"] - full["xy"])) <= 1e-9
    r = ref["wide_disc_duplicates"]
    k = int(r["count"][0])
    assert k > 1 and r["flags"][0, 0] == 0 and (r["flags"][0, 1:k] == S.FLAG_DUPLICATE).all()
    assert np.abs(r["xy"][0, 0] - [40.0, 34.0]).max() < 0.05
    r = ref["square"]
    k = int(r["count"][0])
    # an ideal square has fit_error 0.5 (its corner lies at q = 3/2); the bilinear image rounds a corner inside its pixel, which pulls
    # it in by less than half a pixel diagonal of the 8.1 px to the corner: q >= 1.5 (1 - 0.71 / 8.1)^2 = 1.25
    assert k > 0 and (r["flags"][0, :k] & S.FLAG_SHAPE).all() and (r["fit_error"][0, :k] > 0.25).all() and (r["fit_error"][0, :k] <= 0.5).all()
    r = ref["bar"]
    k = int(r["count"][0])
    assert k > 0 and (r["flags"][0, :k] & S.FLAG_RATIO).all()
    r = ref["dot"]
    assert r["count"][0] == 1 and r["flags"][0, 0] == S.FLAG_SIZE
    r = ref["widest_boxes"]
    assert r["count"][0] == 1 and r["flags"][0, 0] == 0 and np.abs(r["xy"][0, 0] - [60.0, 35.0]).max() < 0.05


def test_sizes_cover_the_kernels_tile_and_strip_edges():
    """the tile and strip constants that SIZES and the planted cases are built round are the ones in the kernel source, and SIZES
    holds every edge they define: a change of BLB_TX, BLB_TY or BLB_SH fails here until the sizes follow"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "csrc", "blob_detect.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"\b(BLB_TX|BLB_TY|BLB_SH) = (\d+)", src)}
    assert (const["BLB_TX"], const["BLB_TY"], const["BLB_SH"]) == (S.TILE_W, S.TILE_H, S.STRIP_H)
    heights, widths = {s[0] for s in S.SIZES}, {s[1] for s in S.SIZES}
    for edge in {S.STRIP_H, S.TILE_H}:
        assert {edge - 1, edge, edge + 1, 2 * edge - 1, 2 * edge, 2 * edge + 1} <= heights
    assert {S.TILE_W - 1, S.TILE_W, S.TILE_W + 1, 2 * S.TILE_W - 1, 2 * S.TILE_W, 2 * S.TILE_W + 1} <= widths
    assert any(w % 4 and w > S.TILE_W for w in widths) and any(w % 16 == 0 and w % S.TILE_W for w in widths)
    assert 11 in heights and 11 in widths and max(s[2] for s in S.SIZES) >= 3
    assert 11 >= 2 * (S.SMALL.b + S.SMALL.nms_radius) + 1


def test_ray_table(host):
    rays = np.empty(64)
    host.cc_rays(rays.ctypes.data_as(C.c_void_p))
    c, s = S.ray_table()
    assert np.array_equal(rays, np.array(c + s))
    assert np.abs(np.hypot(rays[:32], rays[32:]) - 1.0).max() < 1e-15 and rays[0] == 1.0 and rays[32] == 0.0


def test_selfcheck_under_sanitizers():
    """the stand-alone driver program (its own main), built under the address and undefined-behaviour sanitizers, runs clean"""
    r = host_build.run_sanitized("circle_cpu")
    assert r.returncode == 0 and "circle self-check: ok" in r.stdout, r.stdout + r.stderr


# ---- grid order -------------------------------------------------------------------------------------------------------------------------
def _lattice(pattern, rows, cols, turn_deg=0.0, mirror=False, pitch=20.0, origin=(300.0, 260.0), tilt=0.0, radius=5.0, seed=0):
    """the pattern's points through a homography (an in-plane turn, then a tilt about an oblique axis seen from 600 px away), with the
    ellipse shape M = r^2 J J^T a small circle gets from the local Jacobian J, in a shuffled order -> (xy, shape, perm)"""
    p = S.pattern_points(pattern, rows, cols, pitch)
    p = p - p.mean(axis=0)
    if mirror:
        p = p * [-1.0, 1.0]
    t = math.radians(turn_deg)
    Rz = np.array([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]])
    Rt = S.K.rodrigues(tilt * np.array([math.cos(0.6), math.sin(0.6), 0.0]))
    Rm, f, z = Rt @ Rz, 600.0, 600.0
    Hm = np.array([[f, 0, origin[0]], [0, f, origin[1]], [0, 0, 1.0]]) @ np.c_[Rm[:, :2], [0.0, 0.0, z]]

    def proj(q):
        h = np.c_[q, np.ones(len(q))] @ Hm.T
        return h[:, :2] / h[:, 2:3]

    xy, e = proj(p), 1e-4
    Jx, Jy = (proj(p + [e, 0.0]) - proj(p - [e, 0.0])) / (2 * e), (proj(p + [0.0, e]) - proj(p - [0.0, e])) / (2 * e)
    J = np.stack([Jx, Jy], axis=2)  # [n][2][2]
    M = radius * radius * (J @ J.transpose(0, 2, 1))
    shape = np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 1, 1]], axis=1)
    perm = np.random.default_rng(seed + int(turn_deg) + rows).permutation(rows * cols)
    return xy[perm], shape[perm], perm


def _all_orders(lib, host, xy, shape, pattern, rows, cols):
    out = [detect.order_circle_grid(xy, shape, pattern, rows, cols), S.host_order(host, xy, shape, pattern, rows, cols),
           S.order(xy, shape, pattern, rows, cols)]
    if out[0][0] is None:
        assert out[1][0] is None and out[2][0] is None
        return None, False
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][0], out[2][0])
    assert int(out[0][1]) == out[1][1] == out[2][1]
    return out[0]


@pytest.mark.parametrize("tilt", [0.0, 0.8])
@pytest.mark.parametrize("turn", [30.0 * k for k in range(12)])
def test_order_turned_and_tilted_lattices(lib, host, turn, tilt):
    # the asymmetric pattern with odd rows: one labelling, so every physical point keeps its (j, i) whatever the turn
    xy, shape, perm = _lattice(S.ASYMMETRIC, 11, 4, turn, tilt=tilt)
    index, unique = _all_orders(lib, host, xy, shape, S.ASYMMETRIC, 11, 4)
    assert index is not None and unique and np.array_equal(perm[index], np.arange(44))
    # even rows and the symmetric pattern: a half turn maps the pattern onto itself, the chessboard's rule decides
    for pattern, rows, cols in ((S.ASYMMETRIC, 6, 5), (S.SYMMETRIC, 5, 7), (S.SYMMETRIC, 5, 5)):
        xy, shape, perm = _lattice(pattern, rows, cols, turn, tilt=tilt)
        index, unique = _all_orders(lib, host, xy, shape, pattern, rows, cols)
        assert index is not None and not unique and sorted(index.tolist()) == list(range(rows * cols))
        phys = perm[index].reshape(rows, cols)
        turns = [np.arange(rows * cols).reshape(rows, cols)]
        turns.append(turns[0][::-1, ::-1])
        if rows == cols and pattern == S.SYMMETRIC:
            turns += [turns[0].T[::-1], turns[0].T[:, ::-1]]
        assert any(np.array_equal(phys, g) for g in turns)  # a rotation of the construction, never a reflection
        P = xy[index].reshape(rows, cols, 2)
        mi, mj = (P[:, 1:] - P[:, :-1]).mean(axis=(0, 1)), (P[1:] - P[:-1]).mean(axis=(0, 1))
        assert mi[0] * mj[1] - mi[1] * mj[0] > 0 and mi[0] >= -1e-9


def test_order_half_turn_keeps_every_label(lib, host):
    xy, shape, perm = _lattice(S.ASYMMETRIC, 11, 4, 20.0, tilt=0.5)
    a, ua = _all_orders(lib, host, xy, shape, S.ASYMMETRIC, 11, 4)
    c = np.array([300.0, 260.0])
    b, ub = _all_orders(lib, host, 2 * c - xy, shape, S.ASYMMETRIC, 11, 4)  # the image turned by a half turn: same blobs, same shapes
    assert ua and ub and np.array_equal(a, b)


def test_order_null_shapes_strays_missing_and_mirrored(lib, host):
    xy, shape, perm = _lattice(S.ASYMMETRIC, 11, 4, 40.0, tilt=0.25)
    index, unique = _all_orders(lib, host, xy, None, S.ASYMMETRIC, 11, 4)  # mild tilt: the identity metric is enough
    assert unique and np.array_equal(perm[index], np.arange(44))
    far = np.array([[900.0, 40.0], [20.0, 700.0]])
    fs = np.array([[25.0, 0.0, 25.0]] * 2)
    i2, u2 = _all_orders(lib, host, np.r_[xy, far], np.r_[shape, fs], S.ASYMMETRIC, 11, 4)  # stray blobs far from the grid are ignored
    assert u2 and np.array_equal(i2, _all_orders(lib, host, xy, shape, S.ASYMMETRIC, 11, 4)[0])
    assert _all_orders(lib, host, xy[1:], shape[1:], S.ASYMMETRIC, 11, 4)[0] is None  # one blob missing
    assert _all_orders(lib, host, xy, shape, S.ASYMMETRIC, 11, 3)[0] is None  # another grid
    assert _all_orders(lib, host, xy, shape, S.SYMMETRIC, 11, 4)[0] is None  # another pattern
    # Mirrored: the asymmetric pattern with even rows has a half turn but no mirror line, so its mirror image is not found.  (With odd
    # rows the pattern is symmetric about its middle row, and the symmetric pattern about both axes: a mirror image of those is a
    # rotated copy, which no detector can tell from the pattern.)
    xm, sm, _ = _lattice(S.ASYMMETRIC, 6, 5, 70.0, mirror=True, tilt=0.3)
    assert _all_orders(lib, host, xm, sm, S.ASYMMETRIC, 6, 5)[0] is None
    xo, so, _ = _lattice(S.ASYMMETRIC, 6, 5, 70.0, tilt=0.3)
    assert _all_orders(lib, host, xo, so, S.ASYMMETRIC, 6, 5)[0] is not None
    with pytest.raises(ValueError):
        detect.order_circle_grid(xy, shape, S.ASYMMETRIC, 1, 4)
    with pytest.raises(ValueError):
        detect.order_circle_grid(xy, shape, 2, 11, 4)
    with pytest.raises(ValueError):
        detect.order_circle_grid(np.r_[xy, [[np.nan, 0.0]]], None, S.ASYMMETRIC, 11, 4)
    with pytest.raises(ValueError):
        detect.order_circle_grid(xy, shape[:-1], S.ASYMMETRIC, 11, 4)
    with pytest.raises(ValueError):
        detect.order_circle_grid(xy, -shape, S.ASYMMETRIC, 11, 4)


# ---- the restatement on rendered views ----------------------------------------------------------------------------------------------------
def test_restatement_finds_every_rendered_grid():
    sc = S.scene(S.SCENE_SEED)
    for (found, unique, uv, uvc, n_peaks, n_good), truth in zip(S.restatement_boards(), sc["truth"]):
        assert found and unique and n_good == S.ROWS * S.COLS  # every blob, no unflagged false blob
        (r0, m0), (r1, m1) = S.rms(uv, truth), S.rms(uvc, truth)  # the truth's own labelling: no half-turn allowance
        print(f"peaks {n_peaks} rms px uncorrected {r0:.4f} (max {m0:.4f}) bias-corrected {r1:.4f} (max {m1:.4f})")
        assert m0 < 0.5  # the labelling is the truth's: a wrong one is off by a whole pitch
        assert r1 <= r0


def test_circle_centre_bias_matches_the_restatement_and_geometry():
    sc = S.scene(S.SCENE_SEED)
    obj = S.grid_points()
    assert np.abs(detect.circle_grid_points(S.ROWS, S.COLS, S.SPACING, detect.CIRCLES_ASYMMETRIC) - (obj - obj[0])).max() < 1e-15
    Hm = S.homography(obj, sc["truth"][0])
    assert np.abs(detect._dlt_homography(obj, sc["truth"][0]) - Hm).max() < 1e-6 * np.abs(Hm).max()
    bias = detect.circle_centre_bias(Hm, obj, S.RADIUS)
    assert np.abs(bias - S.centre_bias(Hm, obj, S.RADIUS)).max() < 1e-9
    # geometry: the centre of the ellipse through 64 projected rim points (the mean of antipodal tangent points is not it; fit the conic)
    X, Y = obj[5]
    th = 2 * np.pi * np.arange(64) / 64
    rim = np.c_[X + S.RADIUS * np.cos(th), Y + S.RADIUS * np.sin(th), np.ones(64)] @ Hm.T
    rim = rim[:, :2] / rim[:, 2:3]
    m = rim.mean(axis=0)
    x, y = (rim - m).T
    A = np.c_[x * x, x * y, y * y, x, y, np.ones(64)]
    q = np.linalg.svd(A)[2][-1]
    centre = np.linalg.solve([[2 * q[0], q[1]], [q[1], 2 * q[2]]], [-q[3], -q[4]]) + m
    p = Hm @ [X, Y, 1.0]
    assert np.abs((centre - p[:2] / p[2]) - bias[5]).max() < 1e-6
    assert np.abs(detect.circle_centre_bias(np.diag([500.0, 500.0, 1.0]), obj, S.RADIUS)).max() < 1e-9  # fronto-parallel: none


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
def test_create_rejects_bad_arguments(lib):
    def create(W=64, H=48, n=1, m=16, **kw):
        o = capi.CbaBlobOptions()
        lib.cba_blob_options_default(C.byref(o))
        o.outer_half, o.nms_radius = 8, 3
        for k, v in kw.items():
            setattr(o, k, v)
        h = C.c_void_p()
        return lib.cba_blob_detector_create(W, H, n, m, C.byref(o), 0, C.byref(h))

    bad = [dict(W=22), dict(H=22), dict(W=40000), dict(n=0), dict(m=0), dict(polarity=2), dict(polarity=-1), dict(inner_half=0),
           dict(inner_half=8), dict(outer_half=2), dict(outer_half=16), dict(min_contrast=0), dict(min_contrast=256), dict(nms_radius=0),
           dict(nms_radius=11), dict(max_radius=1), dict(max_radius=33), dict(rounds=0), dict(rounds=9), dict(max_fit_error=0.0),
           dict(max_axis_ratio=0.5), dict(min_radius=-1.0), dict(max_fit_error=float("nan")), dict(n=70000, W=32768, H=32768),
           dict(outer_half=12, nms_radius=4, W=32)]
    for kw in bad:
        assert create(**kw) == capi.CBA_ERR_INVALID_ARGUMENT, kw
    assert lib.cba_blob_detector_create(64, 48, 1, 16, None, 0, C.byref(C.c_void_p())) == capi.CBA_ERR_INVALID_ARGUMENT
    assert lib.cba_blob_detector_process(None, 1, None, None, None, None, None, None, None, None) == capi.CBA_ERR_INVALID_ARGUMENT
    lib.cba_blob_detector_destroy(None)
    o = capi.CbaBlobOptions()
    lib.cba_blob_options_default(C.byref(o))
    d = detect.BlobOptions()
    for got in ((o.polarity, o.inner_half, o.outer_half, o.min_contrast, o.nms_radius, o.max_radius, o.rounds, o.max_fit_error,
                 o.max_axis_ratio, o.min_radius),
                (d.polarity, d.inner_half, d.outer_half, d.min_contrast, d.nms_radius, d.max_radius, d.rounds, d.max_fit_error,
                 d.max_axis_ratio, d.min_radius), tuple(S.DEFAULT)):
        assert got == (0, 2, 12, 30, 4, 20, 3, 0.2, 3.0, 1.5)
    idx = np.zeros(44, np.int32)
    assert lib.cba_circle_grid_order(0, None, None, 1, 11, 4, None, None) == capi.CBA_ERR_INVALID_ARGUMENT
    assert lib.cba_circle_grid_order(0, None, None, 1, 11, 4, capi.i32ptr(idx), None) == capi.CBA_OK and (idx == -1).all()
    for kw in (dict(width=22), dict(opts=detect.BlobOptions(outer_half=2)), dict(opts=detect.BlobOptions(rounds=0)), dict(max_blobs=0)):
        with pytest.raises(ValueError):  # the Python layer raises before any device work, with or without a device
            detect.BlobDetector(**{**dict(width=64, height=64), **kw})
    with pytest.raises(ValueError):
        detect.detect_circle_grid(np.zeros((1, 64, 64), np.uint8), 1, 4)
    with pytest.raises(ValueError):
        detect.detect_circle_grid(np.zeros((64,), np.uint8), 11, 4)
    with pytest.raises(ValueError):
        detect.detect_circle_grid(np.zeros((1, 64, 64), np.uint8), 11, 4, pattern=5)
    assert detect.detect_circle_grid(np.zeros((0, 64, 64), np.uint8), 11, 4) == ([], [])
    if lib.cba_device_count() <= 0:  # without a device a valid create fails loudly
        assert create() == capi.CBA_ERR_NO_DEVICE
