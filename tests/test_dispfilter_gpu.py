"""GPU tier of the disparity filters: cba_disparity_filter on the device, through DisparityFilter, against the numpy restatement
tests/dispfilter_ref.py, bitwise (NaN positions equal): the option grid and planted scenes of the CPU tier, out == in, determinism,
independence of the maps, the handle's life cycle, the filter attached to both matchers, and the occluded strip of
tests/test_sgm_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi
from calibration_amd.stereo import DisparityFilter, DisparityFilterOptions, SgmMatcher, SgmOptions, StereoMatcher, StereoMatchOptions
from tests import dispfilter_ref as G
from tests import sgm_ref as S

pytestmark = pytest.mark.gpu


def _opts(o):
    return DisparityFilterOptions(o.median_half, o.speckle_max_size, o.speckle_max_diff)


def _run(maps, o, max_images=None):
    with DisparityFilter(maps.shape[2], maps.shape[1], max_images or maps.shape[0], _opts(o)) as f:
        return f.process(maps, want_stats=True)


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_matches_restatement(gpu_lib, size):
    for key, maps, o in G.grid_cases(size):
        assert G.same(_run(maps, o), G.filter_cached(key, maps, o)), key


@pytest.mark.parametrize("case", G.planted_cases(), ids=lambda c: c.name)
def test_planted(gpu_lib, case):
    ref = G.filter_cached("planted_" + case.name, case.maps, case.o)
    got = _run(case.maps, case.o)
    assert G.same(got, ref) and case.check(*got)


def test_in_place_determinism_independence_and_handle(gpu_lib):
    H, W = G.SIZES[-1]
    maps, other = G.random_maps(3, H, W), G.random_maps(3, H, W, seed=5)
    o = G.Options(1, 5, 0.5)
    ref, ref_other = G.filter_maps(maps, o), G.filter_maps(other, o)
    fp = C.POINTER(C.c_float)
    with DisparityFilter(W, H, 4, _opts(o)) as f:  # n < max_images
        a = f.process(maps, want_stats=True)
        b = f.process(maps, want_stats=True)
        assert G.same(a, ref) and G.same(b, a)  # two calls are equal to the bit
        assert G.same(f.process(other, want_stats=True), ref_other)  # a second call with other data sees nothing stale
        one = f.process(maps[1], want_stats=True)  # a smaller n after a larger one
        assert G.bitwise(one[0][0], a[0][1]) and np.array_equal(one[1][0], a[1][1])
        assert G.same(f.process(maps, want_stats=True), ref)
        buf = maps.copy()  # out == in
        assert gpu_lib.cba_disparity_filter_process(f._h, 3, buf.ctypes.data_as(fp), buf.ctypes.data_as(fp), None) == capi.CBA_OK
        assert G.bitwise(buf, ref[0])
        none = f.process(maps[:0])
        assert none.shape == (0, H, W)
        with pytest.raises(ValueError):
            f.process(np.concatenate([maps, maps]))
        five = np.zeros((5, H, W), np.float32)
        assert gpu_lib.cba_disparity_filter_process(f._h, 5, five.ctypes.data_as(fp), five.ctypes.data_as(fp), None) == capi.CBA_ERR_INVALID_ARGUMENT
        assert gpu_lib.cba_disparity_filter_process(f._h, -1, five.ctypes.data_as(fp), five.ctypes.data_as(fp), None) == capi.CBA_ERR_INVALID_ARGUMENT
        assert gpu_lib.cba_disparity_filter_process(f._h, 1, C.cast(None, fp), five.ctypes.data_as(fp), None) == capi.CBA_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            f.process(maps.astype(np.float64))
        with pytest.raises(ValueError):
            f.process(maps[:, :-1])
    with pytest.raises(ValueError):
        f.process(maps)  # closed


def test_many_small_maps(gpu_lib):
    """more tiles and chunks than the median and apply launches have workgroups (4096): a workgroup then walks a run of them, here two
    maps, and must add each map's counts to that map"""
    maps = G.random_maps(4100, 3, 5)
    o = G.Options(1, 2, 0.5)
    ref = G.filter_maps(maps, o)
    assert (ref[1][:, 2] > 0).sum() > 1000 and len({tuple(r) for r in ref[1].tolist()}) > 50  # the counts differ from map to map
    assert G.same(_run(maps, o), ref)


# ---- attached to a matcher ---------------------------------------------------------------------------------------------------------------
# The scene: three textured pairs with a strip of the right images replaced by noise, so that both matchers leave islands there.  On the
# restatements the median and speckle filter of the test removes 3 components (11 pixels) of the block matcher's maps and 66 (189) of
# SGM's.  SGM's workspace of 1 MiB holds two of the three pairs (33 * 130 * (3 * 32 + 16) bytes each), so its kernels run in two groups
# and the filter after both.
@pytest.mark.parametrize("matcher,mopts", [(StereoMatcher, StereoMatchOptions(-2, 32, 3, 0, 3, True)),
                                           (SgmMatcher, SgmOptions(-2, 32, 4, 32, 8, 10, 1, True, 1))], ids=["block", "sgm"])
def test_filter_attached_to_a_matcher(gpu_lib, matcher, mopts):
    left, right = S.random_pairs(3, 33, 130)
    right = right.copy()
    right[:, :, 60:76] = np.random.default_rng(3).integers(0, 256, (3, 33, 16), dtype=np.uint8)
    with matcher(130, 33, 3, mopts, S.GEOM, S.POSE) as m:
        plain = m.process(left, right)
    # Without the median the filtered map is the unfiltered one with holes, and so are its points.  With it the values move too: the
    # points are then those of the filtered map (the restatement's stereo points), NaN wherever it is NaN.
    fo = G.Options(0, 20, 1.0)
    with DisparityFilter(130, 33, 3, _opts(fo)) as f:
        want = f.process(plain.disparity)
    assert G.bitwise(want, G.filter_maps(plain.disparity, fo)[0])
    removed = np.isnan(want) & ~np.isnan(plain.disparity)
    assert removed.any() and np.isfinite(want).any()  # the filter has work to do on this scene, and leaves something
    with matcher(130, 33, 3, mopts, S.GEOM, S.POSE, filter=_opts(fo)) as m:
        got = m.process(left, right)
        assert G.bitwise(got.disparity, want)
        assert G.bitwise(got.xyz, np.where(np.isnan(want)[..., None], np.float32(np.nan), plain.xyz))
        assert np.array_equal(got.cost, plain.cost)
    fo = G.Options(1, 20, 1.0)
    with DisparityFilter(130, 33, 3, _opts(fo)) as f:
        want = f.process(plain.disparity)
    assert G.bitwise(want, G.filter_maps(plain.disparity, fo)[0]) and not G.bitwise(np.isnan(want), np.isnan(plain.disparity))
    yy, xx = np.indices((33, 130))
    uvd = np.stack([np.broadcast_to(xx, want.shape), np.broadcast_to(yy, want.shape), want.astype(np.float64)], axis=-1)
    want_xyz = S.points(uvd.reshape(-1, 3), S.GEOM, S.POSE).astype(np.float32).reshape(3, 33, 130, 3)
    with matcher(130, 33, 3, mopts, S.GEOM, S.POSE, filter=_opts(fo)) as m:
        got = m.process(left, right)
        assert G.bitwise(got.disparity, want)
        assert G.bitwise(got.xyz, want_xyz) and np.isnan(got.xyz[np.isnan(want)]).all()
        assert np.array_equal(got.cost, plain.cost)
        again = m.process(left[:2], right[:2])  # a smaller n, the same workspace
        assert G.bitwise(again.disparity, want[:2]) and G.bitwise(again.xyz, got.xyz[:2])
        only = m.process(left, right, want_xyz=False)
        assert only.xyz is None and G.bitwise(only.disparity, want)
        with pytest.raises(ValueError):
            m.set_filter(DisparityFilterOptions(median_half=3))
        bad = capi.CbaDisparityFilterOptions(1, -1, 1.0)
        assert getattr(gpu_lib, matcher._FN + "_set_filter")(m._h, C.byref(bad)) == capi.CBA_ERR_INVALID_ARGUMENT
        assert G.bitwise(m.process(left, right).disparity, want)  # a refused call leaves the filter as it was
        m.set_filter(None)
        back = m.process(left, right)
        for k in ("disparity", "cost", "xyz"):
            assert G.bitwise(getattr(back, k), getattr(plain, k)), k
        m.set_filter(_opts(G.Options(0, 0, 0.0)))  # both steps off: reading alone, which a matcher's output passes unchanged
        assert G.bitwise(m.process(left, right).disparity, plain.disparity)


# ---- the occluded strip ------------------------------------------------------------------------------------------------------------------
# tests/test_sgm_gpu.py::test_occluded_strip with p1 = p2 = 0 (D = 16, 8 paths, u = 0, lr = 1, sub-pixel), the strip [2:22, 48:56], wrong =
# finite with |d - 6| > 1, elsewhere = [2:22, 20:40].  Measured on the restatements (tests/sgm_ref.py, tests/dispfilter_ref.py), shares of
# the strip finite / wrong and of elsewhere finite:
#   left-right check alone                              0.3375  0.2812  0.9975
#   + median 3 x 3, speckle size <= 20, diff <= 1.0     0.0625  0.0250  0.9975
STRIP_MEASURED = ((0.3375, 0.2812, 0.9975), (0.0625, 0.0250, 0.9975))


def test_occluded_strip(gpu_lib):
    L, R = G.strip_pair()
    o = S.Options(0, 16, 0, 0, 8, 0, 1, 1)
    ref = S.match(L[None], R[None], o)["disparity"]
    ref_filtered = G.filter_maps(ref, G.STRIP_FILTER)[0]
    for disp, written in zip((ref[0], ref_filtered[0]), STRIP_MEASURED):
        print("restatement: strip finite %.4f wrong %.4f, elsewhere finite %.4f" % G.strip_shares(disp))
        assert np.allclose(G.strip_shares(disp), written, atol=5e-5)  # the values written above are the ones measured
    so = SgmOptions(0, 16, 0, 0, 8, 0, 1, True)
    with SgmMatcher(96, 24, 1, so) as m:
        before = m.process(L, R).disparity[0]
        m.set_filter(_opts(G.STRIP_FILTER))
        after = m.process(L, R).disparity[0]
    assert G.bitwise(before, ref[0]) and G.bitwise(after, ref_filtered[0])
    (_, wrong_before, _), (_, wrong_after, elsewhere) = G.strip_shares(before), G.strip_shares(after)
    print(f"device: strip wrong {wrong_before:.4f} -> {wrong_after:.4f}, elsewhere finite {elsewhere:.4f}")
    assert wrong_after <= 0.5 * wrong_before
    assert elsewhere >= 0.95
