"""GPU tier of chessboard detection: cba_corner_detector on the device against the numpy restatement tests/corner_ref.py.  count,
status, peak pixels, response, flags and the NONE and COG positions are compared to the bit; the angle too (the device makes the two
fp64 sums, the host of the library halves their atan2, as the restatement does); GRADIENT positions are held to 1e-9 px with equal
flags.  Then the sizes and planted cases of the issue, independence of the images, determinism, the handle's life cycle, and the chain
rendered boards -> detect_chessboard -> intrinsic seed -> optimize_intrinsics against the camera that rendered the views."""
import numpy as np
import pytest

from calibration_amd import detect, linear, optim
from calibration_amd.detect import CornerDetector, CornerOptions
from tests import corner_ref as S

pytestmark = pytest.mark.gpu


def _opts(o):
    return CornerOptions(*o)


def _as_dict(r):
    return dict(count=r.count, status=r.status, xy=r.xy, angle=r.angle, response=r.response, flags=r.flags)


def _run(images, o, max_corners, max_images=None):
    with CornerDetector(images.shape[2], images.shape[1], max_images or images.shape[0], max_corners, _opts(o)) as d:
        return _as_dict(d.process(images))


def _tol(o):
    return 1e-9 if o.refine == S.GRADIENT else 0.0


@pytest.mark.parametrize("refine", [S.NONE, S.COG, S.GRADIENT])
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}_n{s[2]}")
def test_detector_matches_restatement(gpu_lib, size, refine):
    H, W, n = size
    o = S.Options(1, 2, 2, refine, 3, 4)
    images = S.smooth_random(n, H, W)
    ref = S.detect_cached((H, W, n, o), images, o, 64)
    got = _run(images, o, 64, max_images=n + 2)  # max_images larger than n_images
    assert S.same_result(got, ref, _tol(o))


@pytest.mark.parametrize("case", S.planted_cases(), ids=lambda c: c[0])
def test_planted_cases(gpu_lib, case):
    name, images, o, max_corners = case
    ref = S.detect_cached(name, images, o, max_corners)
    got = _run(images, o, max_corners)
    assert S.same_result(got, ref, _tol(o))


def test_wide_window_and_radii(gpu_lib):
    """the largest suppression, COG and GRADIENT windows"""
    images = S.smooth_random(2, 70, 150, seed=5, sigma=2.5)
    o = S.Options(200, 10, 5, S.GRADIENT, 10, 3)
    ref = S.detect_cached(("wide", o), images, o, 32)
    assert ref["count"].min() > 0
    assert S.same_result(_run(images, o, 32), ref, 1e-9)


def test_independence_determinism_and_handle(gpu_lib):
    images = S.smooth_random(3, 45, 131, seed=2)
    o = S.Options(1, 2, 2, S.GRADIENT, 3, 4)
    ref = S.detect_cached(("handle", o), images, o, 48)
    with CornerDetector(131, 45, 4, 48, _opts(o)) as d:
        a = _as_dict(d.process(images))
        b = _as_dict(d.process(images))
        assert S.same_result(a, ref, 1e-9)
        for k in a:
            assert S.bitwise(a[k], b[k]), k  # run to run
        one = _as_dict(d.process(images[1]))  # fewer images than before on the same handle; an image alone equals itself in a batch
        for k in a:
            assert S.bitwise(one[k][0], a[k][1]), k
        last = _as_dict(d.process(images[2:]))
        for k in a:
            assert S.bitwise(last[k][0], a[k][2]), k
        none = d.process(images[:0])
        assert none.xy.shape == (0, 48, 2)
        with pytest.raises(ValueError):
            d.process(np.concatenate([images, images]))
        with pytest.raises(ValueError):
            d.process(images.astype(np.float32))
        with pytest.raises(ValueError):
            d.process(images[:, :, :100])
    with pytest.raises(ValueError):
        d.process(images)  # closed
    for _ in range(3):  # create and destroy
        with CornerDetector(131, 45, 1, 8, _opts(o)) as d2:
            r = d2.process(images[0])
            assert r.count[0] == ref["count"][0]
    with pytest.raises(ValueError):
        CornerDetector(10, 45)
    with pytest.raises(ValueError):
        CornerDetector(64, 64, opts=CornerOptions(min_response=0))


# ---- end to end on rendered boards ---------------------------------------------------------------------------------------------------------
def _calibrate(views):
    est = linear.estimate_intrinsics(views)
    assert est.success and len(est.views) == len(views)
    init = np.r_[est.kmtx, np.zeros(5)]
    res = optim.optimize_intrinsics(views, init, [v.c_se3_t for v in est.views])
    assert res.core.success
    return res.camera


@pytest.mark.parametrize("refine", [S.NONE, S.COG, S.GRADIENT])
def test_rendered_boards_end_to_end(gpu_lib, refine):
    sc = S.scene(S.SCENE_SEED)
    o = S.DEFAULT._replace(refine=refine)
    ref = S.restatement_boards(refine)
    boards = detect.detect_chessboard(sc["images"], S.ROWS, S.COLS, S.SQUARE, _opts(o), max_corners=128)
    obj = S.board_points()
    for b, (found, uv, n_peaks), truth in zip(boards, ref, sc["truth"]):
        assert b.found and found and b.n_corners == n_peaks == S.ROWS * S.COLS
        assert np.array_equal(b.object_xy, obj)
        assert np.abs(b.image_uv - uv).max() <= _tol(o)  # the device equals the restatement, the grid order included
        rms, _ = S.match_truth(b.image_uv, truth)
        rms_ref, _ = S.match_truth(uv, truth)
        print("refine", refine, "rms px device", rms, "restatement", rms_ref)
        assert rms <= 1.5 * rms_ref
    cam = _calibrate([b.view for b in boards])
    cam_ref = _calibrate([np.c_[obj, uv] for _, uv, _ in ref])
    dev, dev_ref = np.abs(cam[:4] - S.CAMERA[:4]), np.abs(cam_ref[:4] - S.CAMERA[:4])
    print("refine", refine, "fx fy cx cy device", cam[:4], "restatement", cam_ref[:4], "true", S.CAMERA[:4])
    assert (dev <= 3.0 * dev_ref).all()
