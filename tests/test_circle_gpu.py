"""GPU tier of circle-grid detection: cba_blob_detector on the device against the numpy restatement tests/circle_ref.py.  count, status,
peak pixels (through the responses), response and flags are compared to the bit; positions, shapes and fit_error are held to 1e-9 with
equal flags.  Then the sizes and planted cases of the CPU tier, independence of the images, determinism, the handle's life cycle, and
the chain rendered views -> detect_circle_grid -> intrinsic seed -> optimize_intrinsics against the camera that rendered the views."""
import numpy as np
import pytest

from calibration_amd import detect, linear, optim
from calibration_amd.detect import BlobDetector, BlobOptions
from tests import circle_ref as S

pytestmark = pytest.mark.gpu


def _opts(o):
    return BlobOptions(*o)


def _as_dict(r):
    return dict(count=r.count, status=r.status, xy=r.xy, shape=r.shape, fit_error=r.fit_error, response=r.response, flags=r.flags)


def _run(images, o, max_blobs, max_images=None):
    with BlobDetector(images.shape[2], images.shape[1], max_images or images.shape[0], max_blobs, _opts(o)) as d:
        return _as_dict(d.process(images))


@pytest.mark.parametrize("polarity", [S.DARK, S.BRIGHT])
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}_n{s[2]}")
def test_detector_matches_restatement(gpu_lib, size, polarity):
    H, W, n = size
    o = S.SMALL._replace(polarity=polarity)
    images = S.blobs_random(n, H, W)
    ref = S.detect_cached((H, W, n, o), images, o, 64)
    got = _run(images, o, 64, max_images=n + 2)  # max_images larger than n_images
    assert S.same_result(got, ref, 1e-9)


@pytest.mark.parametrize("case", S.planted_cases(), ids=lambda c: c[0])
def test_planted_cases(gpu_lib, case):
    name, images, o, max_blobs = case
    ref = S.detect_cached(name, images, o, max_blobs)
    got = _run(images, o, max_blobs)
    assert S.same_result(got, ref, 1e-9)


def test_widest_boxes_and_longest_rays(gpu_lib):
    images = S.K.smooth_random(2, 70, 150, seed=5, sigma=4.0)
    o = S.DEFAULT._replace(a=7, b=15, min_contrast=10, nms_radius=10, max_radius=32, rounds=8)
    ref = S.detect_cached(("wide", o), images, o, 32)
    assert ref["count"].min() > 0
    assert S.same_result(_run(images, o, 32), ref, 1e-9)


def test_independence_determinism_and_handle(gpu_lib):
    images = S.blobs_random(3, 45, 131, seed=2)
    o = S.SMALL
    ref = S.detect_cached(("handle", o), images, o, 48)
    with BlobDetector(131, 45, 4, 48, _opts(o)) as d:
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
        assert none.xy.shape == (0, 48, 2) and none.shape.shape == (0, 48, 3)
        with pytest.raises(ValueError):
            d.process(np.concatenate([images, images]))
        with pytest.raises(ValueError):
            d.process(images.astype(np.float32))
        with pytest.raises(ValueError):
            d.process(images[:, :, :100])
    with pytest.raises(ValueError):
        d.process(images)  # closed
    for _ in range(3):  # create and destroy
        with BlobDetector(131, 45, 1, 8, _opts(o)) as d2:
            r = d2.process(images[0])
            assert r.count[0] == ref["count"][0]
    with pytest.raises(ValueError):
        BlobDetector(32, 45)
    with pytest.raises(ValueError):
        BlobDetector(64, 64, opts=BlobOptions(min_contrast=0))


def test_result_properties(gpu_lib):
    images = S.disc(60, 90, 41.3, 30.6, 6.0)[None]
    with BlobDetector(90, 60, 1, 4) as d:
        r = d.process(images)
    assert r.count[0] == 1 and r.flags[0, 0] == 0
    assert np.abs(r.semi_axes[0, 0] - 6.0).max() < 0.3 and np.abs(r.xy[0, 0] - [41.3, 30.6]).max() < 0.05
    major, minor = S.semi_axes(r.shape[0, 0])
    assert np.array_equal(r.semi_axes[0, 0], [major, minor]) and -np.pi / 2 < r.angle[0, 0] <= np.pi / 2


# ---- end to end on rendered views ----------------------------------------------------------------------------------------------------------
def _calibrate(views):
    est = linear.estimate_intrinsics(views)
    assert est.success and len(est.views) == len(views)
    init = np.r_[est.kmtx, np.zeros(5)]
    res = optim.optimize_intrinsics(views, init, [v.c_se3_t for v in est.views])
    assert res.core.success
    return res.camera


@pytest.mark.parametrize("correct", [False, True], ids=["centres", "bias_corrected"])
def test_rendered_grids_end_to_end(gpu_lib, correct):
    sc = S.scene(S.SCENE_SEED)
    ref = S.restatement_boards()
    boards, unique = detect.detect_circle_grid(sc["images"], S.ROWS, S.COLS, S.SPACING, detect.CIRCLES_ASYMMETRIC, _opts(S.DEFAULT),
                                               circle_radius=S.RADIUS if correct else None, max_blobs=S.MAX_BLOBS)
    obj = detect.circle_grid_points(S.ROWS, S.COLS, S.SPACING, detect.CIRCLES_ASYMMETRIC)
    ref_uv = [(uvc if correct else uv) for _, _, uv, uvc, _, _ in ref]
    for b, u, (found, runique, _, _, n_peaks, _), uv, truth in zip(boards, unique, ref, ref_uv, sc["truth"]):
        assert b.found and found and u and runique and b.n_corners == n_peaks
        assert np.array_equal(b.object_xy, obj)
        assert np.abs(b.image_uv - uv).max() <= 1e-9  # the device equals the restatement, the grid order included
        rms, _ = S.rms(b.image_uv, truth)
        rms_ref, _ = S.rms(uv, truth)
        print("corrected", correct, "rms px device", rms, "restatement", rms_ref)
        assert rms <= 1.5 * rms_ref
    cam = _calibrate([b.view for b in boards])
    cam_ref = _calibrate([np.c_[obj, uv] for uv in ref_uv])
    dev, dev_ref = np.abs(cam[:4] - S.CAMERA[:4]), np.abs(cam_ref[:4] - S.CAMERA[:4])
    print("corrected", correct, "fx fy cx cy device", cam[:4], "restatement", cam_ref[:4], "true", S.CAMERA[:4], "deviations", dev, dev_ref)
    assert (dev <= 3.0 * dev_ref).all()
