"""GPU tier of structured-light scanning (cba_sl_decoder): the kernels against the numpy restatement (tests/sl_ref.py) and against the
host build of the same header, at the sizes where the decode kernel changes path - widths that are and are not multiples of 16, a
row shorter than a lane's columns, exactly one wavefront of 16-column lanes and one lane more, odd image bases - the planted pixels at
the ends of rows and of lane groups, the argument errors that need a live handle, independence of the sequences of a batch, the points against calibration_amd.triangulate on the
decoded maps, and projector_corners."""
import numpy as np
import pytest

import calibration_amd as cal
from calibration_amd import capi
from calibration_amd.structured_light import StructuredLightDecoder, StructuredLightOptions
from calibration_amd.triangulate import triangulate
from tests import camera_ref as R
from tests import host_build
from tests import sl_ref as S
from tests import triangulate_ref as T

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (67, 37), (64, 64), (130, 33), (257, 5), (1024, 2), (1040, 3)]
# (n_sequences, projector, axes, s, N): every value of each at every size
CASES = [(1, (37, 21), 3, 0, 0), (3, (200, 120), 3, 3, 3), (3, (37, 21), 1, 0, 4), (1, (200, 120), 2, 3, 4), (3, (200, 120), 3, 0, 4),
         (1, (37, 21), 2, 3, 0), (3, (37, 21), 1, 3, 3)]

# Ground truth, measured on the restatement (tests/sl_ref.py decode, then tests/triangulate_ref.py), two-plane scene, 20 x 9 camera,
# 200 x 120 projector, (s, N, T) = (0, 4, 16), seed 5: the largest distance of a valid point to its plane is 0.001778 (pinhole) and
# 0.001452 (Scheimpflug) at depth 1 - a camera pixel is 1 / 24 of the depth there.  The bars are twice that.
PLANE_DISTANCE = {R.PINHOLE: 0.001778, R.SCHEIMPFLUG: 0.001452}
# ... and of projector_corners on the rendered plane (67 x 37 camera, seed 7, 12 corners, radius 8): the restatement path (sl_ref decode,
# numpy DLT) is within 0.003329 px of the renderer's exact projector positions.  The bar is twice that.
CORNER_ERROR_PX = 0.003329


@pytest.fixture(scope="module")
def host():
    return host_build.load("sl_cpu")


def _opts(o):
    return StructuredLightOptions(o.proj_width, o.proj_height, o.axes, o.s, o.N, o.T, o.min_contrast, o.min_bit_diff, o.min_modulation)


def _compare(got, ref, o):
    """the bars of the CPU tier: status and Gray-only coordinates bitwise, with phase 1e-9 px and 1e-12 relative, after the conditions"""
    assert ref["unwrap_margin"] >= 1e-6 and ref["mod_margin"] >= 1e-9, (ref["unwrap_margin"], ref["mod_margin"])
    assert np.array_equal(got["status"], ref["status"])
    assert S.same_nan(got["coord"], ref["coord"]) and S.same_nan(got["modulation"], ref["modulation"])
    if o.N == 0:
        assert np.array_equal(got["coord"], ref["coord"], equal_nan=True) and np.isnan(got["modulation"]).all()
    else:
        assert S.max_abs(got["coord"], ref["coord"]) <= 1e-9
        assert S.max_rel(got["modulation"], ref["modulation"]) <= 1e-12


# ---- 1. device against restatement and host build ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_device_matches_restatement_and_host_build(gpu_lib, host, size):
    W, H = size
    for n_seq, proj, axes, s, N in CASES:
        o = S.Options(proj[0], proj[1], axes, s, N, 16)
        sc = S.scene(R.PINHOLE, W, H, o, n_seq=n_seq, two_planes=W > 1, seed=W + n_seq)
        ref = S.decode_batch(o, sc["images"])
        with StructuredLightDecoder(_opts(o), W, H, max_sequences=n_seq + 1) as dec:
            got = dec.process(sc["images"])
        _compare(got, ref, o)
        hb = S.host_decode(host, o, sc["images"])
        assert np.array_equal(got["status"], hb["status"])
        if N == 0:
            assert np.array_equal(got["coord"], hb["coord"], equal_nan=True)
        else:
            assert S.max_abs(got["coord"], hb["coord"]) <= 1e-9 and S.max_rel(got["modulation"], hb["modulation"]) <= 1e-12


@pytest.mark.parametrize("size", [(64, 64), (67, 37)])
def test_each_output_null_in_turn(gpu_lib, size):
    W, H = size
    o = S.Options(200, 120, 3, 3, 3, 16)
    sc = S.scene(R.SCHEIMPFLUG, W, H, o, n_seq=2, two_planes=True, seed=1)
    names = ("coord", "modulation", "status", "xyz", "rms_px", "tri_status")
    with StructuredLightDecoder(_opts(o), W, H, max_sequences=2) as dec:
        dec.set_rig(sc["intr"][0], sc["intr"][1], sc["poses"])
        full = dec.process(sc["images"], **{k: True for k in names})
        _compare(full, S.decode_batch(o, sc["images"]), o)
        for skip in names:
            r = dec.process(sc["images"], **{k: k != skip for k in names})
            assert r[skip] is None
            for k in names:
                if k != skip:
                    assert np.array_equal(r[k], full[k], equal_nan=True), (skip, k)
        none = dec.process(sc["images"], **{k: False for k in names})
        assert all(v is None for v in none.values())


# ---- 2. planted pixels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 67])
def test_planted_pixels(gpu_lib, host, W):
    o = S.Options(**S.PLANT_OPTIONS)
    plants = S.plants()
    group_end = 15 if W % 16 == 0 else 3  # the last column of the first lane's group
    with StructuredLightDecoder(_opts(o), W, len(plants), max_sequences=1) as dec:
        for col in (0, W - 1, group_end, (W - 1) // (group_end + 1) * (group_end + 1) - 1):  # ... and of the last whole group
            img, want = S.planted_images(W, len(plants), [(i, col) for i in range(len(plants))])
            got = dec.process(img)
            for i, (name, _, st) in enumerate(plants):
                assert got["status"][0, i, col] == st, (name, col)
            assert np.array_equal(got["status"][0], want)
            ref = S.decode(o, img)
            _compare({k: got[k][0] for k in got if got[k] is not None}, ref, o)
            assert np.array_equal(S.host_decode(host, o, img[None])["status"][0], want)


@pytest.mark.parametrize("W", [64, 67])
def test_modulation_just_under_the_threshold(gpu_lib, W):
    """the threshold 1e-7 relative above the pixel's restated modulation marks the axis, 1e-7 below does not (sl_ref.modulation_plant)"""
    v, cases = S.modulation_plant()
    group_end = 15 if W % 16 == 0 else 3
    for min_modulation, st in cases:
        o = S.Options(**S.PLANT_OPTIONS, min_modulation=min_modulation)
        with StructuredLightDecoder(_opts(o), W, 3, max_sequences=1) as dec:
            for col in (0, W - 1, group_end):
                img, want = S.planted_images(W, 3, [(1, col)], [("modulation at the threshold", v, st)])
                ref = S.decode(o, img)
                assert 0.5 * S.MOD_STEP <= ref["mod_margin"] <= 2 * S.MOD_STEP
                got = dec.process(img)
                assert got["status"][0, 1, col] == st and np.array_equal(got["status"][0], want), (min_modulation, col)
                _compare({k: got[k][0] for k in got if got[k] is not None}, ref, o)


# ---- 2b. the argument errors that need a handle ---------------------------------------------------------------------------------------
def test_argument_errors_on_a_live_handle(gpu_lib):
    """n_sequences outside [0, max_sequences], NULL images, what cba_triangulate rejects in the rig, and n_sequences == 0 as no work:
    each on a decoder that decodes as before afterwards"""
    import ctypes as C
    import math

    lib, I, OK = gpu_lib, capi.CBA_ERR_INVALID_ARGUMENT, capi.CBA_OK
    W, H, n_max = 20, 9, 2
    o = S.Options(200, 120, 3, 0, 4, 16)
    sc = S.scene(R.PINHOLE, W, H, o, n_seq=3, two_planes=True, seed=5)
    img = sc["images"]
    none, none8, none32 = capi.dptr(None), capi.u8ptr(None), capi.i32ptr(None)
    with StructuredLightDecoder(_opts(o), W, H, max_sequences=n_max) as dec:
        h = dec._h
        before = dec.process(img[:2])

        def process(n, images, points=False):
            coord, status = np.full((max(n, 1), 2, H, W), -7.0), np.full((max(n, 1), H, W), 99, np.uint8)
            xyz = np.full((max(n, 1), H, W, 3), -7.0)
            st = lib.cba_sl_decoder_process(h, n, capi.u8ptr(images), capi.dptr(coord), none, capi.u8ptr(status),
                                            capi.dptr(xyz) if points else none, none, none32)
            assert (coord == -7.0).all() and (status == 99).all() and (xyz == -7.0).all()  # nothing was written
            return st

        def usable(points=False):
            again = dec.process(img[:2], xyz=points)
            assert all(S.bitwise(again[k], before[k]) for k in ("coord", "modulation", "status"))
            return again

        # n_sequences outside [0, max_sequences]
        assert process(-1, img) == I and process(n_max + 1, img) == I
        with pytest.raises(capi.CbaInvalidArgument):
            dec.process(img)  # 3 sequences > max_sequences
        # NULL images with work to do; no work with n_sequences == 0, whatever the pointers
        assert process(1, None) == I and process(n_max, None) == I
        assert process(0, None) == OK and process(0, img) == OK
        assert lib.cba_sl_decoder_process(h, 0, none8, none, none, none8, none, none, none32) == OK
        assert process(1, img, points=True) == I and process(0, None, points=True) == I  # points without a rig, before "no work"
        usable()

        # what cba_triangulate rejects in the rig
        intr, poses = np.ascontiguousarray(sc["intr"]), np.ascontiguousarray(sc["poses"])
        inv = np.zeros((2, 4))

        def set_rig(model=R.PINHOLE, intr=intr, n_inv=0, inv=None, poses=poses, opts=True, **fields):
            co = capi.CbaTriangulateOptions()
            lib.cba_triangulate_options_default(C.byref(co))
            for k, val in fields.items():
                setattr(co, k, val)
            return lib.cba_sl_decoder_set_rig(h, model, capi.dptr(intr), n_inv, capi.dptr(inv), capi.dptr(poses), C.byref(co) if opts else None)

        def with_zero(cam, k):
            z = intr.copy()
            z[cam, k] = 0.0
            return z

        rejected = [dict(model=2), dict(model=-1), dict(intr=None), dict(poses=None), dict(opts=False),
                    dict(intr=with_zero(0, 0)), dict(intr=with_zero(0, 1)), dict(intr=with_zero(1, 0)), dict(intr=with_zero(1, 1)),
                    dict(n_inv=1, inv=inv), dict(n_inv=17, inv=inv),
                    dict(max_iterations=-1), dict(step_tolerance=-1e-300), dict(step_tolerance=math.nan),
                    dict(max_reproj_px=0.0), dict(max_reproj_px=-1.0), dict(max_reproj_px=math.nan)]
        for bad in rejected:
            assert set_rig(**bad) == I, bad
            assert process(1, img, points=True) == I, bad  # a rejected rig is no rig
        usable()
        assert set_rig(n_inv=1) == OK  # a count without coefficients is not read, as in cba_triangulate
        pts = usable(points=True)
        for bad in rejected:  # ... and a rejected rig leaves the one that is set
            assert set_rig(**bad) == I, bad
        assert S.bitwise(usable(points=True)["xyz"], pts["xyz"]) and np.isfinite(pts["xyz"]).any()
        assert process(n_max + 1, img, points=True) == I and process(0, None, points=True) == OK


# ---- 3. independence and determinism -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (67, 37)])
def test_independence_and_determinism(gpu_lib, size):
    W, H = size
    o = S.Options(200, 120, 3, 0, 4, 16)
    a = S.scene(R.PINHOLE, W, H, o, n_seq=3, two_planes=True, seed=11)["images"]
    b = S.scene(R.PINHOLE, W, H, o, n_seq=2, seed=12)["images"]
    names = ("coord", "modulation", "status")

    def same(x, y):
        return all(S.bitwise(x[k], y[k]) for k in names)

    with StructuredLightDecoder(_opts(o), W, H, max_sequences=3) as dec:
        batch = dec.process(a)
        assert same(batch, dec.process(a))  # two runs
        for i in range(3):  # alone and inside the batch
            one = dec.process(a[i])
            assert all(S.bitwise(one[k][0], batch[k][i]) for k in names), i
        after = dec.process(b)  # other data, fewer sequences, on the same handle
    with StructuredLightDecoder(_opts(o), W, H, max_sequences=2) as fresh:
        assert same(after, fresh.process(b))
    _compare(after, S.decode_batch(o, b), o)


# ---- 4. points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [R.PINHOLE, R.SCHEIMPFLUG])
def test_points_are_triangulate_on_the_decoded_maps(gpu_lib, model):
    o = S.Options(200, 120, 3, 0, 4, 16)
    for (W, H), seed in (((20, 9), 5), ((64, 5), 6)):  # the 4-column and the 16-column path
        sc = S.scene(model, W, H, o, n_seq=2, two_planes=True, seed=seed)
        with StructuredLightDecoder(_opts(o), W, H, max_sequences=2) as dec:
            with pytest.raises(capi.CbaInvalidArgument):
                dec.decode(sc["images"], want_points=True)  # no rig yet
            dec.set_rig(sc["intr"][0], sc["intr"][1], sc["poses"])
            d = dec.decode(sc["images"], want_points=True)
        v, u = np.mgrid[0:H, 0:W]
        cam = np.tile(np.stack([u.ravel(), v.ravel()], axis=1).astype(float), (2, 1))
        uv = np.stack([cam, np.stack([d.x.ravel(), d.y.ravel()], axis=1)])
        t = triangulate(list(sc["intr"]), sc["poses"], uv)
        assert S.bitwise(d.xyz.reshape(-1, 3), t.xyz) and S.bitwise(d.rms_px.ravel(), t.rms_px) and np.array_equal(d.tri_status.ravel(), t.status)
        bad = (d.status != 0).ravel()
        assert bad.any() and (t.status[bad] == capi.TRI_TOO_FEW).all() and np.isnan(t.xyz[bad]).all() and np.isnan(t.rms_px[bad]).all()
        if (W, H) == (20, 9):  # the scene of the recorded ground truth: its first sequence
            ref = S.decode(o, sc["images"][0])
            n = W * H
            rt = T.triangulate(model, list(sc["intr"]), None, list(sc["poses"]), np.stack([cam[:n], np.stack([ref["coord"][0].ravel(), ref["coord"][1].ravel()], axis=1)]))
            ok = (rt["status"] == T.OK) & (ref["status"].ravel() == 0)
            which = sc["plane_of_pixel"].ravel()
            measured = S.plane_distance(rt["xyz"][ok], which[ok]).max()
            print(f"model {model}: restatement max plane distance {measured:.6f}")
            assert measured <= PLANE_DISTANCE[model] + 5e-7
            okd = ~bad[:n]
            assert S.plane_distance(t.xyz[:n][okd], which[okd]).max() <= 2 * PLANE_DISTANCE[model]
    with StructuredLightDecoder(_opts(S.Options(200, 120, 1)), 20, 9) as one_axis:
        one_axis.set_rig(sc["intr"][0], sc["intr"][1], sc["poses"])
        with pytest.raises(capi.CbaInvalidArgument):
            one_axis.process(np.zeros((one_axis.n_images, 9, 20), np.uint8), xyz=True)


# ---- 5. projector_corners -------------------------------------------------------------------------------------------------------------
def test_projector_corners_on_exact_maps(gpu_lib):
    W, H = 80, 60
    Hm = np.array([[2.1, 0.15, 30.0], [-0.08, 1.9, 12.0], [2e-4, -1e-4, 1.0]])
    v, u = np.mgrid[0:H, 0:W].astype(float)
    q = np.einsum("ij,jhw->ihw", Hm, np.stack([u, v, np.ones_like(u)]))
    x, y = q[0] / q[2], q[1] / q[2]
    rng = np.random.default_rng(2)
    hole = rng.random((H, W)) < 0.2
    x[hole] = np.nan
    y[rng.random((H, W)) < 0.1] = np.nan
    x[20:40, 60:80] = np.nan  # a region without any valid pixel
    corners = np.array([[20.3, 15.7], [40.49, 30.51], [0.2, 0.4], [79.4, 59.3], [3.6, 55.2], [70.0, 30.0], [np.nan, 5.0], [65.5, 41.8]])
    got = cal.projector_corners(x, y, corners)
    want = np.c_[corners, np.ones(len(corners))] @ Hm.T
    want = want[:, :2] / want[:, 2:3]
    solved = [0, 1, 2, 3, 4, 7]  # the border corners use the clipped window; [7] keeps the part of its window beside the hole
    assert np.isfinite(got[solved]).all() and np.isnan(got[[5, 6]]).all()
    assert (np.abs(got[solved] - want[solved]) / np.abs(want[solved])).max() <= 1e-9
    # fewer than min_valid valid neighbours: the corner at (0.2, 0.4) has at most 9 x 9 pixels in its clipped window
    assert np.isnan(cal.projector_corners(x, y, corners[[2]], min_valid=82)).all()
    many = cal.projector_corners(np.stack([x, x]), np.stack([y, y]), [corners[:3], corners[3:5]])
    assert np.array_equal(many[0], got[:3]) and np.array_equal(many[1], got[3:5])


def test_projector_corners_end_to_end(gpu_lib):
    o = S.Options(200, 120, 3, 0, 4, 16)
    W, H = 67, 37
    sc = S.scene(R.PINHOLE, W, H, o, seed=7)
    gu, gv = np.meshgrid(np.linspace(9, W - 11, 4), np.linspace(9, H - 10, 3))
    corners = np.stack([gu.ravel() + 0.37, gv.ravel() - 0.21], axis=1)
    exact, _ = S.projector_of(R.PINHOLE, sc["intr"], sc["poses"], corners, np.zeros(len(corners), int))
    ref = S.decode(o, sc["images"][0])
    measured = np.abs(S.projector_corners(ref["coord"][0], ref["coord"][1], corners) - exact).max()
    print(f"restatement path: max corner error {measured:.6f} px")
    assert measured <= CORNER_ERROR_PX + 5e-7
    with StructuredLightDecoder(_opts(o), W, H) as dec:
        d = dec.decode(sc["images"])
    got = cal.projector_corners(d.x[0], d.y[0], corners)
    assert np.abs(got - exact).max() <= 2 * CORNER_ERROR_PX
