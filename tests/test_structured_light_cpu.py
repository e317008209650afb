"""CPU tier of structured-light scanning: the patterns of the library and of the host build of
calibration_amd/csrc/structured_light_math.hpp (tests/sl_cpu, compiled here) against the independent numpy restatement
tests/sl_ref.py, the host build's decode against the restatement's on rendered scenes and on planted pixels, the accuracy of the rule
against the renderer's exact projector coordinates, and the argument errors of the C ABI and of the Python layer (raised before any
device work)."""
import ctypes as C
import math

import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.structured_light import StructuredLightDecoder, StructuredLightOptions
from tests import camera_ref as R
from tests import host_build
from tests import sl_ref as S

PROJECTORS = [(2, 2), (37, 21), (200, 120), (1024, 8)]

# Ground truth: |decoded - exact projector coordinate| over the valid pixels of the rendered plane (pinhole, 67 x 37 camera, 200 x 120
# projector, gain 0.7, offset 20, noise sigma 1, seed 0), measured on the restatement: it belongs to the rule (8-bit patterns sampled
# bilinearly, three or four noisy samples of a cosine), not to an implementation.  Maxima: (s, N, T) = (0, 4, 16): 0.0798 px;
# (3, 3, 16): 0.0926 px.  Valid shares 0.9617 and 0.9956.  The bars are twice the maxima.
ACCURACY = {(0, 4, 16): 0.0798, (3, 3, 16): 0.0926}


@pytest.fixture(scope="module")
def host():
    return host_build.load("sl_cpu")


def _lib_options(o):
    return StructuredLightOptions(o.proj_width, o.proj_height, o.axes, o.s, o.N, o.T, o.min_contrast, o.min_bit_diff, o.min_modulation)


def _all_options(pw, ph):
    for axes in (1, 2, 3):
        for s in (0, 2, 3):
            for N, T in [(0, 16)] + [(N, T) for N in (3, 4, 8) for T in (8, 16, 32)]:
                o = S.Options(pw, ph, axes, s, N, T)
                if o.allowed():
                    yield o


# ---- 1. patterns --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", PROJECTORS)
def test_patterns_match_restatement(lib, host, proj):
    n_checked = 0
    for o in _all_options(*proj):
        ref = S.patterns(o)
        assert cal.image_count(_lib_options(o)) == S.image_count(o) == len(ref)
        got = cal.patterns(_lib_options(o))
        assert S.bitwise(got, ref), vars(o)
        assert S.bitwise(S.host_patterns(host, o), ref), vars(o)
        i = 2
        for a, P in o.sides():
            for _ in range(o.nbits(P)):
                assert np.array_equal(got[i].astype(int), 255 - got[i + 1].astype(int))
                i += 2
            i += o.N
        assert i == len(got) and (got[0] == 255).all() and (got[1] == 0).all()
        n_checked += 1
    assert n_checked >= (10 if proj == (2, 2) else 30)


@pytest.mark.parametrize("proj", [(37, 21), (200, 120)])
def test_patterns_decode_to_their_own_index(host, proj):
    """a camera that is the projector: Gray only gives the stripe's centre exactly; with phase |x - j| stays under the bound of the
    patterns' rounding: each sample is off by at most 0.5 of 127.5 of amplitude, the N errors add to at most N / 2 against a sum of
    length 127.5 N / 2, so the phase is off by at most asin(1 / 127.5) and the coordinate by T / (2 pi) of that"""
    pw, ph = proj
    for s, N, T in [(0, 0, 16), (3, 0, 16), (0, 4, 16), (3, 3, 16), (2, 8, 32)]:
        o = S.Options(pw, ph, 3, s, N, T)
        pats = S.patterns(o)
        ref, got = S.decode(o, pats), S.host_decode(host, o, pats[None])
        for a, P in enumerate((pw, ph)):
            j = np.arange(P)
            centre = (j >> s) * 2.0 ** s + (2 ** s - 1) / 2
            inside = centre <= P - 1
            line = ref["coord"][a][0, :] if a == 0 else ref["coord"][a][:, 0]
            assert np.array_equal(np.isfinite(line), inside)
            if N == 0:
                assert np.array_equal(line[inside], centre[inside])
            else:
                assert np.abs(line - j)[inside].max() <= T / (2 * math.pi) * math.asin(1 / 127.5) * 1.001
        _compare(got, ref, o, batch=False)


# ---- 2. the host build against the restatement -------------------------------------------------------------------------------------
def _compare(got, ref, o, batch=True):
    """the bars of the issue: status and Gray-only coordinates bitwise (NaN positions included); with phase coordinates to 1e-9 px and
    modulation to 1e-12 relative, after the two conditions on the restatement's own numbers"""
    coord, mod, status = (got[k] if batch else got[k][0] for k in ("coord", "modulation", "status"))
    assert ref["unwrap_margin"] >= 1e-6 and ref["mod_margin"] >= 1e-9, (ref["unwrap_margin"], ref["mod_margin"])
    assert np.array_equal(status, ref["status"])
    assert S.same_nan(coord, ref["coord"]) and S.same_nan(mod, ref["modulation"])
    if o.N == 0:
        assert np.array_equal(coord, ref["coord"], equal_nan=True) and np.isnan(mod).all()
    else:
        assert S.max_abs(coord, ref["coord"]) <= 1e-9
        assert S.max_rel(mod, ref["modulation"]) <= 1e-12
    sel = [a for a, _ in o.sides()]
    for i, a in enumerate(sel):
        bits = (ref["status"] >> (1 + 3 * a)) & 7
        assert np.array_equal(np.isfinite(ref["coord"][..., i, :, :]), (bits == 0) & (ref["status"] & 1 == 0))


@pytest.mark.parametrize("size", [(3, 2), (67, 37), (130, 33)])
@pytest.mark.parametrize("proj", [(37, 21), (200, 120)])
@pytest.mark.parametrize("model", [R.PINHOLE, R.SCHEIMPFLUG])
def test_host_build_matches_restatement(host, model, proj, size):
    W, H = size
    for axes in (1, 2, 3):
        for s, N in [(0, 0), (3, 0), (0, 3), (0, 4), (3, 3), (3, 4)]:
            o = S.Options(proj[0], proj[1], axes, s, N, 16)
            sc = S.scene(model, W, H, o, n_seq=2, two_planes=True, seed=3)
            _compare(S.host_decode(host, o, sc["images"]), S.decode_batch(o, sc["images"]), o)


# ---- 3. planted pixels ----------------------------------------------------------------------------------------------------------------
def test_planted_pixels(host):
    o = S.Options(**S.PLANT_OPTIONS)
    plants = S.plants()
    img, want = S.planted_images(len(plants) + 3, 2, [(i % 2, i + 1) for i in range(len(plants))])
    ref = S.decode(o, img)
    for i, (name, _, st) in enumerate(plants):
        assert ref["status"][i % 2, i + 1] == st, name
    assert np.array_equal(ref["status"], want)
    _compare(S.host_decode(host, o, img[None]), ref, o, batch=False)
    clean = want == 0
    assert np.isfinite(ref["coord"][:, clean]).all() and clean.sum() >= 8
    # without the two thresholds an all-255 stack has contrast and every bit is a tie: p == q is "not greater", so every bit is 0
    o0 = S.Options(16, 17, min_contrast=0, min_bit_diff=0)  # Gray only: the phase of a flat stack is rounding noise
    flat = np.full((S.image_count(o0), 1, 5), 255, np.uint8)
    ref0 = S.decode(o0, flat)
    assert (ref0["status"] == 0).all() and np.array_equal(ref0["coord"], np.zeros((2, 1, 5)))
    got0 = S.host_decode(host, o0, flat[None])
    assert (got0["status"] == 0).all() and np.array_equal(got0["coord"][0], ref0["coord"])
    o1 = S.Options(16, 17, min_contrast=0)  # ... and with the bit threshold every bit is uncertain
    assert (S.decode(o1, flat)["status"] == 18).all() and (S.host_decode(host, o1, flat[None])["status"] == 18).all()


def test_modulation_just_under_the_threshold(host):
    """the threshold 1e-7 relative above the pixel's restated modulation marks the axis, 1e-7 below does not: a `<=` for `<`, or a
    modulation that differs from the restatement's by more than the 1e-12 of the bar, would move it"""
    v, cases = S.modulation_plant()
    for min_modulation, st in cases:
        o = S.Options(**S.PLANT_OPTIONS, min_modulation=min_modulation)
        img, want = S.planted_images(5, 2, [(1, 3)], [("modulation at the threshold", v, st)])
        ref = S.decode(o, img)
        assert ref["status"][1, 3] == st and np.array_equal(ref["status"], want)
        assert 0.5 * S.MOD_STEP <= ref["mod_margin"] <= 2 * S.MOD_STEP  # just under or over, and outside the 1e-9 of the condition
        _compare(S.host_decode(host, o, img[None]), ref, o, batch=False)


# ---- 4. accuracy of the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snt", sorted(ACCURACY))
def test_coordinates_against_ground_truth(host, snt):
    s, N, T = snt
    o = S.Options(200, 120, 3, s, N, T)
    sc = S.scene(R.PINHOLE, 67, 37, o, seed=0)
    ref = S.decode(o, sc["images"][0])
    got = S.host_decode(host, o, sc["images"])
    truth = np.stack([sc["xp"][0], sc["yp"][0]])
    valid = ref["status"] == 0
    err = np.abs(ref["coord"] - truth)[:, valid].max()
    print(f"(s, N, T) = {snt}: max |x - x_true| = {err:.4f} px over a valid share of {valid.mean():.4f}")
    assert valid.mean() >= 0.95
    assert err <= ACCURACY[snt] + 5e-5  # the recorded maximum, to its last printed digit
    assert np.abs(got["coord"][0] - truth)[:, valid].max() <= 2 * ACCURACY[snt]


# ---- 5. argument errors, all before any device work -----------------------------------------------------------------------------------
def _d(a):
    return capi.dptr(None if a is None else np.ascontiguousarray(a, float))


def test_sl_abi_defaults_and_argument_errors(lib):
    d = capi.CbaSlOptions()
    lib.cba_sl_options_default(C.byref(d))
    assert (d.axes, d.gray_skip_bits, d.phase_steps, d.phase_period, d.min_contrast, d.min_bit_diff, d.min_modulation) == (3, 0, 0, 16, 10, 4, 5.0)
    I, OK = capi.CBA_ERR_INVALID_ARGUMENT, capi.CBA_OK

    def opts(**fields):
        co = capi.CbaSlOptions()
        lib.cba_sl_options_default(C.byref(co))
        co.proj_width, co.proj_height = 37, 21
        for k, v in fields.items():
            setattr(co, k, v)
        return co

    def count(**fields):
        n = C.c_int32(-1)
        return lib.cba_sl_image_count(C.byref(opts(**fields)), C.byref(n)), n.value

    assert count() == (OK, 2 + 2 * 6 + 2 * 5) and count(axes=1, phase_steps=3) == (OK, 2 + 12 + 3)
    bad = [dict(proj_width=1), dict(proj_height=1), dict(proj_width=capi.IMAGE_MAX_SIDE + 1), dict(axes=0), dict(axes=4), dict(gray_skip_bits=-1),
           dict(phase_steps=2), dict(phase_steps=9), dict(phase_steps=-1), dict(min_contrast=-1), dict(min_contrast=256), dict(min_bit_diff=-1),
           dict(min_bit_diff=256), dict(min_modulation=-1.0), dict(min_modulation=math.nan), dict(min_modulation=math.inf),
           dict(gray_skip_bits=5), dict(gray_skip_bits=6, axes=1), dict(gray_skip_bits=40),  # nbits < 1
           dict(phase_steps=4, gray_skip_bits=3, phase_period=8), dict(phase_steps=3, phase_period=1), dict(phase_steps=3, phase_period=0)]
    for b in bad:
        assert count(**b)[0] == I, b
    assert count(gray_skip_bits=5, axes=1)[0] == OK and count(phase_steps=4, gray_skip_bits=3, phase_period=16)[0] == OK
    assert count(gray_skip_bits=3, phase_period=1)[0] == OK  # the period is not used without phase steps
    assert lib.cba_sl_image_count(None, C.byref(C.c_int32())) == I and lib.cba_sl_image_count(C.byref(opts()), None) == I
    assert lib.cba_sl_patterns(None, capi.u8ptr(np.zeros(8, np.uint8))) == I and lib.cba_sl_patterns(C.byref(opts()), capi.u8ptr(None)) == I
    assert lib.cba_sl_patterns(C.byref(opts(axes=0)), capi.u8ptr(np.zeros(8, np.uint8))) == I

    def create(W=64, H=48, max_sequences=2, o=True, out=True, **fields):
        h = C.c_void_p()
        st = lib.cba_sl_decoder_create(C.byref(opts(**fields)) if o else None, W, H, max_sequences, 0, C.byref(h) if out else None)
        assert st != OK or h.value
        if h.value:
            lib.cba_sl_decoder_destroy(h)
        return st

    assert create(o=False) == I and create(out=False) == I
    for b in bad:
        assert create(**b) == I, b
    assert create(W=0) == I and create(H=0) == I and create(W=capi.IMAGE_MAX_SIDE + 1) == I and create(max_sequences=0) == I
    assert create(W=4096, H=4096, max_sequences=6) == I  # 6 * 24 * 2^24 > 2^31 - 1, while 6 * 2^24 is not
    none = capi.dptr(None)
    assert lib.cba_sl_decoder_process(None, 1, capi.u8ptr(None), none, none, capi.u8ptr(None), none, none, capi.i32ptr(None)) == I
    t = capi.CbaTriangulateOptions()
    lib.cba_triangulate_options_default(C.byref(t))
    assert lib.cba_sl_decoder_set_rig(None, 0, _d(np.ones((2, 10))), 0, none, _d(np.ones((2, 7))), C.byref(t)) == I
    lib.cba_sl_decoder_destroy(None)
    if lib.cba_device_count() <= 0:
        assert create() == capi.CBA_ERR_NO_DEVICE


def test_python_layer_validates(lib):
    with pytest.raises(capi.CbaInvalidArgument):
        cal.image_count(StructuredLightOptions(37, 21, axes=0))
    with pytest.raises(capi.CbaInvalidArgument):
        cal.patterns(StructuredLightOptions(37, 21, phase_steps=4, gray_skip_bits=3, phase_period=8))
    with pytest.raises(capi.CbaInvalidArgument):
        StructuredLightDecoder(StructuredLightOptions(37, 21), 0, 48)
    with pytest.raises(capi.CbaInvalidArgument):
        StructuredLightDecoder(StructuredLightOptions(37, 21, min_contrast=300), 64, 48)
    x = np.zeros((8, 8))
    with pytest.raises(ValueError):
        cal.projector_corners(x, np.zeros((8, 9)), np.zeros((1, 2)))
    with pytest.raises(ValueError):
        cal.projector_corners(x, x, np.zeros((1, 2)), radius=-1)
    # nothing to fit: no device is needed
    assert np.isnan(cal.projector_corners(np.full((8, 8), np.nan), x, np.array([[3.0, 3.0], [np.nan, 1.0]]))).all()
    assert cal.projector_corners(x[None], x[None], [np.zeros((0, 2))])[0].shape == (0, 2)


def test_driver_main_under_sanitizers():
    """the driver's own main (patterns, decode, every pixel back at its index) as a stand-alone program built under the
    address and undefined-behaviour sanitizers"""
    r = host_build.run_sanitized("sl_cpu")
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
