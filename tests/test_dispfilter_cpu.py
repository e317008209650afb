"""CPU tier of the disparity filters: the host build of calibration_amd/csrc/disparity_filter_math.hpp (tests/dispfilter_cpu, compiled
here; it runs the device's tile-local, border-merge and flatten sequence over the tiles one after the other) against the independent
numpy restatement tests/dispfilter_ref.py, bitwise, over the option grid and the planted scenes; the self-check program; and the
argument errors of the C ABI and of the Python layer (raised before any device work)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from calibration_amd import capi, stereo
from tests import dispfilter_ref as G
from tests import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return host_build.load("dispfilter_cpu")


def test_tile_constants_match_the_header():
    src = open(os.path.join(ROOT, "calibration_amd", "csrc", "disparity_filter_math.hpp")).read()
    m = re.search(r"DF_TW = (\d+), DF_TH = (\d+);", src)
    assert (int(m.group(1)), int(m.group(2))) == (G.TW, G.TH)


@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_build_matches_restatement(host, size):
    cases = G.grid_cases(size)
    assert len(cases) == 2 * 36
    for key, maps, o in cases:
        ref = G.filter_cached(key, maps, o)
        assert G.same(G.host_filter(host, maps, o), ref), key
        assert G.bitwise(G.host_filter(host, maps, o, inplace=True)[0], ref[0]), key + " in place"


def test_grid_removes_and_keeps(host):
    """the grid is no empty exercise: at the largest size speckle removal deletes some components and keeps others"""
    key, maps, o = next(c for c in G.grid_cases(G.SIZES[-1]) if repr(c[2]) == "m0_S5_d0.5" and c[1].shape[0] == 3)
    out, stats = G.filter_cached(key, maps, o)
    assert (stats[:, 1] > 0).all() and (stats[:, 2] < stats[:, 0]).all() and np.isfinite(out).any()


@pytest.mark.parametrize("case", G.planted_cases(), ids=lambda c: c.name)
def test_planted(host, case):
    ref = G.filter_cached("planted_" + case.name, case.maps, case.o)
    assert case.check(*ref), "the restatement misses the planted property"
    got = G.host_filter(host, case.maps, case.o)
    assert G.same(got, ref) and case.check(*got)


def test_selfcheck_program(host):
    """the stand-alone program of tests/dispfilter_cpu (its own main), built under the address and undefined-behaviour sanitizers, runs
    clean"""
    r = host_build.run_sanitized("dispfilter_cpu")
    assert r.returncode == 0, r.stdout + r.stderr


# ---- argument errors, all before any device work ------------------------------------------------------------------------------------
def test_abi_defaults_and_argument_errors(lib):
    o = capi.CbaDisparityFilterOptions()
    lib.cba_disparity_filter_options_default(C.byref(o))
    assert (o.median_half, o.speckle_max_size, o.speckle_max_diff) == (1, 100, 1.0)
    lib.cba_disparity_filter_options_default(None)
    I = capi.CBA_ERR_INVALID_ARGUMENT

    def options(**fields):
        co = capi.CbaDisparityFilterOptions()
        lib.cba_disparity_filter_options_default(C.byref(co))
        for k, v in fields.items():
            setattr(co, k, v)
        return co

    def create(W=64, H=48, max_images=2, opts=True, out=True, **fields):
        co = options(**fields) if opts else None
        h = C.c_void_p()
        st = lib.cba_disparity_filter_create(W, H, max_images, None if co is None else C.byref(co), 0, C.byref(h) if out else None)
        assert st != capi.CBA_OK or h.value
        if h.value:
            lib.cba_disparity_filter_destroy(h)
        return st

    assert create(opts=False) == I and create(out=False) == I
    assert create(W=0) == I and create(H=0) == I and create(W=capi.IMAGE_MAX_SIDE + 1) == I and create(H=capi.IMAGE_MAX_SIDE + 1) == I
    assert create(max_images=0) == I and create(max_images=-1) == I
    assert create(W=32768, H=32768, max_images=2) == I  # 2^31 > 2^31 - 1
    assert create(W=32768, H=16384, max_images=4) == I
    assert create(median_half=-1) == I and create(median_half=3) == I
    assert create(speckle_max_size=-1) == I
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        assert create(speckle_max_diff=bad) == I, bad
    fp = C.POINTER(C.c_float)
    assert lib.cba_disparity_filter_process(None, 1, C.cast(None, fp), C.cast(None, fp), None) == I
    lib.cba_disparity_filter_destroy(None)
    good = options()
    for fn in (lib.cba_stereo_matcher_set_filter, lib.cba_sgm_matcher_set_filter):
        assert fn(None, C.byref(good)) == I and fn(None, None) == I
    if lib.cba_device_count() <= 0:  # every argument is fine: the device is looked for last
        assert create() == capi.CBA_ERR_NO_DEVICE
        assert create(median_half=0, speckle_max_size=0, speckle_max_diff=0.0) == capi.CBA_ERR_NO_DEVICE
        assert create(speckle_max_size=2**31 - 1) == capi.CBA_ERR_NO_DEVICE
        assert create(W=32768, H=32768, max_images=1) == capi.CBA_ERR_NO_DEVICE  # 2^30 pixels


def test_python_layer_validates(lib):
    assert stereo.DisparityFilterOptions() == stereo.DisparityFilterOptions(1, 100, 1.0)
    import calibration_amd

    assert calibration_amd.DisparityFilter is stereo.DisparityFilter and calibration_amd.DisparityFilterOptions is stereo.DisparityFilterOptions
    F = stereo.DisparityFilterOptions
    for bad in (F(median_half=3), F(median_half=-1), F(speckle_max_size=-1), F(speckle_max_size=2**31), F(speckle_max_diff=-1.0),
                F(speckle_max_diff=float("nan")), F(speckle_max_diff=float("inf"))):
        with pytest.raises(ValueError):
            stereo.DisparityFilter(64, 48, opts=bad)
        with pytest.raises(ValueError):  # the keyword of the matchers is checked before the matcher is created
            stereo.StereoMatcher(64, 48, filter=bad)
        with pytest.raises(ValueError):
            stereo.SgmMatcher(64, 48, filter=bad)
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.DisparityFilter(0, 48)
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.DisparityFilter(64, 48, max_images=0)
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.DisparityFilter(32768, 32768, max_images=2)
