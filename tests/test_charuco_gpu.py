"""GPU tier of ChArUco detection: cba_charuco_detector on the device against the numpy restatement tests/charuco_ref.py.  The two
device stages are compared alone through the handle's mid-level calls (arm scores and marker readings to the bit: integers, codes,
flags, levels), then determinism and the handle's life cycle, then the chain rendered views of a board larger than the image ->
detect_charuco -> intrinsic seed -> optimize_intrinsics against the camera that rendered the views."""
import numpy as np
import pytest

from calibration_amd import detect, linear, optim
from calibration_amd.detect import CharucoBoard, CharucoDetector, CharucoOptions, CornerOptions
from tests import charuco_ref as S

pytestmark = pytest.mark.gpu

READ_CASES = S.read_cases()
ARM_CASES = S.arm_cases()


def _board(b):
    return CharucoBoard(b.squares_x, b.squares_y, b.square, b.codes, b.marker_bits, b.marker_ratio)


def _opts(o):
    return CharucoOptions(*o)


@pytest.mark.parametrize("case", READ_CASES, ids=[c["name"] for c in READ_CASES])
def test_marker_read_matches_restatement(gpu_lib, case):
    ref = S.read_reference(case)
    images = case["images"]
    n, H, W = images.shape
    with CharucoDetector(W, H, _board(case["board"]), n + 1, 16, 16, opts=_opts(case["opts"])) as d:  # max_images larger than n_images
        d.process(images)
        got = d.read(case["cell_image"], case["quads"])
    assert S.same_readings(got, ref)


@pytest.mark.parametrize("case", ARM_CASES, ids=[c[0] for c in ARM_CASES])
def test_corner_arms_match_restatement(gpu_lib, case):
    name, images, m = case
    det, dirs, ref = S.arm_reference(name, images, m)
    n, H, W = images.shape
    board = S.Board(3, 3, 1.0, 4, 0.6, S.cached_dictionary(4, 17, 3, 3))
    with CharucoDetector(W, H, _board(board), n, m, 8, CornerOptions(*S.ARM_CORNERS), _opts(S.DEFAULT)) as d:
        res = d.process(images)
        got = d.arms(dirs)
    assert np.array_equal(res.n_corners, det["count"])
    assert np.array_equal(np.isnan(got), np.isnan(ref))  # NaN past the kept corners
    assert np.array_equal(np.nan_to_num(got), np.nan_to_num(ref))


def _same(a, b):
    for k in ("count", "status", "ids", "n_markers", "n_corners", "cells"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert S.CR.bitwise(a.xy, b.xy) and a.n_cells == b.n_cells and a.readings.tobytes() == b.readings.tobytes()


def test_determinism_independence_and_handle(gpu_lib):
    sc = S.scene("small", 3, 2)
    images, board = sc["images"], _board(sc["board"])
    with CharucoDetector(S.W_IMG, S.H_IMG, board, 3, 512, 256) as d:
        a = d.process(images)
        _same(a, d.process(images))  # run to run
        assert (a.count == 54).all() and (a.status == 0).all() and a.n_cells == len(a.cells) >= 80
        one = d.process(images[1])  # fewer images than before on the same handle; an image alone equals itself in a batch
        assert np.array_equal(one.ids[0], a.ids[1]) and S.CR.bitwise(one.xy[0], a.xy[1]) and one.n_markers[0] == a.n_markers[1]
        k = a.cells[:, 0] == 1
        assert np.array_equal(one.cells[:, 1:], a.cells[k, 1:]) and one.readings.tobytes() == a.readings[k].tobytes()
        with pytest.raises(ValueError):
            d.arms(np.zeros((2, 512, 12, 2)))  # not the images of the last process
        with pytest.raises(ValueError):
            d.read([1], np.zeros((1, 4, 2)))  # an image the last process did not have
        assert d.process(images[:0]).xy.shape == (0, 54, 2)
        with pytest.raises(ValueError):
            d.process(np.concatenate([images, images]))
        with pytest.raises(ValueError):
            d.process(images.astype(np.float32))
        with pytest.raises(ValueError):
            d.process(images[:, :, :100])
    with pytest.raises(ValueError):
        d.process(images)  # closed
    for _ in range(3):  # create and destroy
        with CharucoDetector(S.W_IMG, S.H_IMG, board, 1, 512, 256) as d2:
            assert d2.process(images[0]).count[0] == 54
    with CharucoDetector(S.W_IMG, S.H_IMG, board, 2, 512, 30) as d3:  # cells overflow: the first are kept, the count stays true
        r = d3.process(images)
        assert r.n_cells == a.n_cells and len(r.cells) == 30 and (r.status & detect.CHARUCO_STATUS_CELL_OVERFLOW).any()
        assert np.array_equal(r.cells, a.cells[:30]) and r.readings.tobytes() == a.readings[:30].tobytes()
    with pytest.raises(ValueError):
        CharucoDetector(10, 45, board)
    with pytest.raises(ValueError):
        CharucoDetector(64, 64, board, opts=CharucoOptions(cell_samples=6))
    with pytest.raises(ValueError):
        CharucoDetector(64, 64, CharucoBoard(10, 7, 0.025, sc["board"].codes, marker_bits=3))  # codes wider than the marker


def test_small_board_fully_in_view(gpu_lib):
    """the 10 x 7 board fully in view gives all 54 inner corners, the set a plain 6 x 9 chessboard detection orders, on their indices"""
    sc = S.scene("small", 3, 2)
    ref = S.detect(sc["images"], sc["board"], key=("scene", "small", 3, 2))
    out = detect.detect_charuco(sc["images"], _board(sc["board"]), max_corners=512, max_cells=256)
    for b, r, truth in zip(out, ref, sc["truth"]):
        assert b.found and np.array_equal(b.ids, np.arange(54)) and np.array_equal(r["ids"], np.arange(54))
        assert np.abs(b.image_uv - r["xy"]).max() <= 1e-9 and b.n_markers == r["n_markers"]
        assert np.linalg.norm(b.image_uv - truth, axis=1).max() < 0.5
        assert b.view.shape == (54, 4) and np.array_equal(b.object_xy, S.object_points(sc["board"]))


def _calibrate(views):
    est = linear.estimate_intrinsics(views)
    assert est.success and len(est.views) == len(views)
    init = np.r_[est.kmtx, np.zeros(5)]
    res = optim.optimize_intrinsics(views, init, [v.c_se3_t for v in est.views])
    assert res.core.success
    return res.camera


def test_board_larger_than_the_view_end_to_end(gpu_lib):
    sc = S.scene("big", S.SCENE_SEED)
    board = sc["board"]
    ref = S.detect(sc["images"], board, key=("scene", "big", S.SCENE_SEED))
    out = detect.detect_charuco(sc["images"], _board(board), max_corners=1024, max_cells=1024)
    obj = S.object_points(board)
    for b, r, truth in zip(out, ref, sc["truth"]):
        assert b.found and np.array_equal(b.ids, r["ids"]) and len(b.ids) < len(truth)  # a partial view, the restatement's ids
        assert np.abs(b.image_uv - r["xy"]).max() <= 1e-9 and b.n_markers == r["n_markers"]
        err, err_ref = np.linalg.norm(b.image_uv - truth[b.ids], axis=1), np.linalg.norm(r["xy"] - truth[r["ids"]], axis=1)
        assert err.max() < 1.0  # no wrong id: the next corner is a square away
        rms, rms_ref = float(np.sqrt((err ** 2).mean())), float(np.sqrt((err_ref ** 2).mean()))
        print("corners", len(b.ids), "markers", b.n_markers, "rms px device", rms, "restatement", rms_ref)
        assert rms <= 1.5 * rms_ref
        assert np.array_equal(b.object_xy, obj[b.ids])
    cam = _calibrate([b.view for b in out])
    cam_ref = _calibrate([np.c_[obj[r["ids"]], r["xy"]] for r in ref])
    dev, dev_ref = np.abs(cam[:4] - S.CAMERA[:4]), np.abs(cam_ref[:4] - S.CAMERA[:4])
    print("fx fy cx cy device", cam[:4], "restatement", cam_ref[:4], "true", S.CAMERA[:4])
    assert (dev <= 3.0 * dev_ref).all()
