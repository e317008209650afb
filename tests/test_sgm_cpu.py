"""CPU tier of semi-global matching: the host build of calibration_amd/csrc/sgm_math.hpp (tests/sgm_cpu, compiled here) against the
independent numpy restatement tests/sgm_ref.py, bitwise; the ranges the rule promises (path costs past 8 bits, sums past 10); the
restatement and the host build against rendered ground truth; and the argument errors of the C ABI and of the Python layer (raised
before any device work)."""
import ctypes as C

import numpy as np
import pytest

from calibration_amd import capi, stereo
from tests import host_build
from tests import sgm_ref as G


@pytest.fixture(scope="module")
def host():
    return host_build.load("sgm_cpu")


def test_option_cases_cover_every_value_at_every_size():
    cases = G.option_cases()
    for size in G.SIZES:
        at = [c for c in cases if (c[0], c[1]) == size]
        assert {(c[3].min_disparity, c[3].num_disparities) for c in at} == set(G.MD)
        assert {(c[3].p1, c[3].p2) for c in at} == set(G.PEN)
        for name, values in (("paths", {4, 8}), ("uniqueness_percent", {0, 10}), ("lr_max_diff", {-1, 1}), ("subpixel", {0, 1})):
            assert {getattr(c[3], name) for c in at} == values, (size, name)
        assert {c[2] for c in at} == {1, 3} and {c[4] for c in at} == {False, True}


@pytest.mark.parametrize("case", G.option_cases(), ids=G.case_id)
def test_host_build_matches_restatement(host, case):
    H, W, n, o, with_pose = case
    left, right = G.random_pairs(n, H, W)
    pose = G.POSE if with_pose else None
    ref = G.match_cached(G.case_id(case), left, right, o, G.GEOM, pose)
    assert G.same_result(G.host_match(host, left, right, o, G.GEOM, pose), ref)


def test_selfcheck_program(host):
    """the stand-alone program of tests/sgm_cpu (its own main), built under the address and undefined-behaviour sanitizers, runs
    clean"""
    r = host_build.run_sanitized("sgm_cpu")
    assert r.returncode == 0, r.stdout + r.stderr


def test_path_costs_leave_8_bits_and_sums_leave_10(host):
    """independent noise left and right with p1 = p2 = 1023: an 8-bit path cost or a 10-bit sum would show"""
    left, right = G.noise_pair()
    o = G.Options(0, 24, 1023, 1023, 8, 0, -1, 0)
    ref = G.match_cached("noise_16x64", left, right, o)
    print(f"largest S {ref['smax']}, largest L_r {ref['lmax']}")
    assert ref["smax"] > 1023 and ref["lmax"] > 255
    assert G.same_result(G.host_match(host, left, right, o), ref)


# ---- ground truth -----------------------------------------------------------------------------------------------------------------------
# Measured on the restatement (scene seed 2, D = 24, 8 paths, (4, 32), u = 10, lr = 1, sub-pixel, interior [4, H-4) x [28, W-4)): the
# valid share and the largest error and RMS in px are printed by the test; DESIGN.md section 7m lists them.
@pytest.mark.parametrize("noise", [0.0, 2.0])
@pytest.mark.parametrize("truth", ["constant", "slanted"])
def test_ground_truth(host, truth, noise):
    fn = (lambda x, y: 7.0) if truth == "constant" else (lambda x, y: 5 + 0.05 * x + 0.03 * y)
    L, R, d = G.truth_pair(fn, noise=noise)
    o = G.Options(0, 24, 4, 32, 8, 10, 1, 1)
    ref = G.match_cached(f"truth_{truth}_{noise}", L[None], R[None], o)
    got = G.host_match(host, L[None], R[None], o)
    H, W = L.shape
    inner = (slice(4, H - 4), slice(28, W - 4))
    for name, disp in (("restatement", ref["disparity"][0]), ("host build", got["disparity"][0])):
        valid = ~np.isnan(disp[inner])
        err = np.abs(disp[inner] - d[inner])[valid]
        print(f"{name}: truth {truth} noise {noise}: valid share {valid.mean():.4f} max error {err.max():.3f} px rms {np.sqrt(np.mean(err ** 2)):.3f}")
        assert valid.mean() >= 0.99
        assert err.max() <= 1.0
    assert G.same_result(got, ref)


# ---- argument errors, all before any device work ------------------------------------------------------------------------------------
def test_sgm_abi_defaults_and_argument_errors(lib):
    o = capi.CbaSgmOptions()
    lib.cba_sgm_options_default(C.byref(o))
    assert [getattr(o, f) for f, _ in capi.CbaSgmOptions._fields_] == [0, 64, 4, 32, 8, 10, 1, 1, 0]
    lib.cba_sgm_options_default(None)
    I = capi.CBA_ERR_INVALID_ARGUMENT
    geom = capi.CbaStereoGeometry(*G.GEOM)

    def create(W=64, H=48, max_pairs=2, opts=True, g=geom, pose=None, out=True, **fields):
        co = None
        if opts:
            co = capi.CbaSgmOptions()
            lib.cba_sgm_options_default(C.byref(co))
            for k, v in fields.items():
                setattr(co, k, v)
        h = C.c_void_p()
        st = lib.cba_sgm_matcher_create(W, H, max_pairs, None if co is None else C.byref(co), None if g is None else C.byref(g),
                                        capi.dptr(None if pose is None else np.ascontiguousarray(pose, float)), 0, C.byref(h) if out else None)
        assert st != capi.CBA_OK or h.value
        if h.value:
            lib.cba_sgm_matcher_destroy(h)
        return st

    assert create(opts=False) == I and create(out=False) == I
    assert create(W=0) == I and create(H=0) == I and create(W=capi.IMAGE_MAX_SIDE + 1) == I and create(max_pairs=0) == I
    assert create(W=32768, H=32768, max_pairs=3, num_disparities=1) == I
    assert create(min_disparity=-32769) == I and create(min_disparity=32769) == I
    assert create(num_disparities=0) == I and create(num_disparities=257) == I
    assert create(p2=-1) == I and create(p2=1024, p1=0) == I and create(p1=-1) == I
    assert create(p1=33) == I and create(p1=5, p2=4) == I  # p1 > p2
    for paths in (0, 1, 2, 5, 7, 16, -8):
        assert create(paths=paths) == I, paths
    assert create(uniqueness_percent=-1) == I and create(uniqueness_percent=101) == I
    assert create(lr_max_diff=-2) == I and create(subpixel=2) == I and create(subpixel=-1) == I
    assert create(workspace_mb=-1) == I and create(workspace_mb=(1 << 20) + 1) == I
    assert create(W=4096, H=4096, max_pairs=1, num_disparities=129) == I  # width height D > 2^31
    assert create(W=32768, H=32768, max_pairs=1, num_disparities=3) == I
    assert create(g=None, pose=G.POSE) == I
    for k in ("focal", "cx", "cy", "baseline"):
        bad = capi.CbaStereoGeometry(*G.GEOM)
        setattr(bad, k, np.nan)
        assert create(g=bad) == I, k
    assert create(g=capi.CbaStereoGeometry(0.0, 1.0, 1.0, 0.1)) == I and create(g=capi.CbaStereoGeometry(100.0, 1.0, 1.0, -0.1)) == I
    assert create(pose=np.r_[G.POSE[:6], np.inf]) == I
    fp = C.POINTER(C.c_float)
    assert lib.cba_sgm_matcher_process(None, 1, None, None, C.cast(None, fp), None, C.cast(None, fp)) == I
    lib.cba_sgm_matcher_destroy(None)
    if lib.cba_device_count() <= 0:  # every argument is fine: the device is looked for last
        assert create() == capi.CBA_ERR_NO_DEVICE and create(g=None) == capi.CBA_ERR_NO_DEVICE
        assert create(W=4096, H=4096, max_pairs=1, num_disparities=128) == capi.CBA_ERR_NO_DEVICE  # exactly 2^31


def test_python_layer_validates(lib):
    assert stereo.SgmOptions() == stereo.SgmOptions(0, 64, 4, 32, 8, 10, 1, True, 0)
    import calibration_amd

    assert calibration_amd.SgmMatcher is stereo.SgmMatcher and calibration_amd.SgmOptions is stereo.SgmOptions
    with pytest.raises(ValueError):
        stereo.SgmMatcher(64, 48, pose=G.POSE)
    with pytest.raises(ValueError):
        stereo.SgmMatcher(64, 48, opts=stereo.SgmOptions(paths=6))
    with pytest.raises(ValueError):
        stereo.SgmMatcher(64, 48, opts=stereo.SgmOptions(p1=40, p2=32))
    with pytest.raises(ValueError):
        stereo.SgmMatcher(64, 48, opts=stereo.SgmOptions(p1=-1))
    with pytest.raises(ValueError):
        stereo.SgmMatcher(64, 48, geometry=(1.0, 2.0, 3.0))
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.SgmMatcher(64, 48, opts=stereo.SgmOptions(num_disparities=0))
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.SgmMatcher(64, 48, opts=stereo.SgmOptions(p2=1024))
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.SgmMatcher(64, 48, opts=stereo.SgmOptions(workspace_mb=-1))
    with pytest.raises(capi.CbaInvalidArgument):
        stereo.SgmMatcher(4096, 4096, opts=stereo.SgmOptions(num_disparities=129))
