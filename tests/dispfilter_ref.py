"""Independent numpy restatement of the disparity filters as calibba.h states them (cba_disparity_filter): reading, the windowed lower
median by a sort over the stacked window, and speckle removal by a flood fill over each map.  Also the wrappers of the host build
(tests/dispfilter_cpu), the result cache both tiers share, the option grid and the planted scenes.  Test infrastructure: the host build
and the device are checked against it."""
import numpy as np

from tests.stereo_ref import bitwise  # noqa: F401  (the comparison of every tier)

TW, TH = 32, 8  # DF_TW, DF_TH of disparity_filter_math.hpp: the component tile (test_dispfilter_cpu.py checks the two agree)
NAN = np.float32(np.nan)


class Options:  # cba_disparity_filter_options
    def __init__(self, median_half=1, speckle_max_size=100, speckle_max_diff=1.0):
        self.median_half, self.speckle_max_size, self.speckle_max_diff = median_half, speckle_max_size, speckle_max_diff

    def __repr__(self):
        return f"m{self.median_half}_S{self.speckle_max_size}_d{self.speckle_max_diff}"


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def read(img):
    """step 0: non-finite -> NaN, -0.0 -> +0.0"""
    a = np.array(img, dtype=np.float32)
    a[~np.isfinite(a)] = np.nan
    a[a == 0] = 0.0
    return a


def median(a, m):
    """step 1 on one map that went through read(): np.sort puts the NaNs last, so the k valid values lead"""
    if m == 0:
        return a.copy()
    H, W = a.shape
    P = np.full((H + 2 * m, W + 2 * m), np.nan, np.float32)
    P[m:m + H, m:m + W] = a
    win = np.stack([P[j:j + H, i:i + W] for j in range(2 * m + 1) for i in range(2 * m + 1)], axis=-1)
    k = np.isfinite(win).sum(-1)
    srt = np.sort(win, axis=-1)
    out = np.take_along_axis(srt, (np.maximum(k, 1) - 1)[..., None] // 2, axis=-1)[..., 0]
    return np.where(np.isnan(a), NAN, out).astype(np.float32)


def speckle(a, max_size, max_diff):
    """step 2 on one map: (filtered map, components removed, pixels removed), by a flood fill from every unvisited valid pixel"""
    H, W = a.shape
    out = a.copy()
    valid = ~np.isnan(a)
    seen = np.zeros((H, W), bool)
    d = a.astype(np.float64)
    comps = pixels = 0
    for y0, x0 in zip(*np.nonzero(valid)):
        if seen[y0, x0]:
            continue
        seen[y0, x0] = True
        comp = [(y0, x0)]
        k = 0
        while k < len(comp):
            y, x = comp[k]
            k += 1
            for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                if 0 <= yy < H and 0 <= xx < W and valid[yy, xx] and not seen[yy, xx] and abs(d[y, x] - d[yy, xx]) <= max_diff:
                    seen[yy, xx] = True
                    comp.append((yy, xx))
        if len(comp) <= max_size:
            comps += 1
            pixels += len(comp)
            for y, x in comp:
                out[y, x] = np.nan
    return out, comps, pixels


def filter_maps(maps, o):
    """maps [n][H][W] float32 -> (filtered [n][H][W] float32, stats int64 [n][3])"""
    maps = np.asarray(maps, np.float32)
    out, stats = np.empty_like(maps), np.zeros((maps.shape[0], 3), np.int64)
    for i, img in enumerate(maps):
        a = read(img)
        stats[i, 0] = np.isfinite(a).sum()
        a = median(a, o.median_half)
        if o.speckle_max_size > 0:
            a, stats[i, 1], stats[i, 2] = speckle(a, o.speckle_max_size, o.speckle_max_diff)
        out[i] = a
    return out, stats


_CACHE = {}


def filter_cached(key, maps, o):
    """filter_maps() computed once per key: the CPU and GPU tiers share the restatement's results"""
    if key not in _CACHE:
        _CACHE[key] = filter_maps(maps, o)
    return _CACHE[key]


def same(got, ref):
    """(maps, stats) pairs equal to the bit"""
    return bitwise(got[0], ref[0]) and bool(np.array_equal(got[1], ref[1]))


# ---- the host build of disparity_filter_math.hpp (tests/dispfilter_cpu) ---------------------------------------------------------------
def host_filter(Lb, maps, o, inplace=False):
    import ctypes as C

    maps = np.ascontiguousarray(maps, np.float32)
    n, H, W = maps.shape
    src = maps.copy()
    out = src if inplace else np.empty_like(maps)
    stats = np.zeros((n, 3), np.int64)
    Lb.dispfilter_run(C.c_int(W), C.c_int(H), C.c_int(n), C.c_int(o.median_half), C.c_int(o.speckle_max_size), C.c_double(o.speckle_max_diff),
                      src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p))
    return out, stats


# ---- the option grid of both tiers -------------------------------------------------------------------------------------------------------
# (1,1) (1,9) (7,1) (2,2), one below / at / above the tile's height and width, two tiles plus three pixels in each direction
SIZES = [(1, 1), (1, 9), (7, 1), (2, 2), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 3)]
GRID = [Options(m, S, d) for m in (0, 1, 2) for S in (0, 1, 5, 2**31 - 1) for d in (0.0, 0.5, 1.0)]


def random_maps(n, H, W, seed=0):
    """about 30 % NaN, the rest multiples of 0.25 in [0, 2]: equal and near-equal neighbours are common, so components of every small
    size occur at each speckle_max_diff of the grid"""
    rng = np.random.default_rng(seed + 1000 * H + W + 7 * n)
    a = (rng.integers(0, 9, (n, H, W)) / 4).astype(np.float32)
    a[rng.random((n, H, W)) < 0.3] = np.nan
    return a


def grid_cases(size):
    """[(key, maps, Options)] of one size: the whole option grid at n = 1 and n = 3"""
    H, W = size
    return [(f"grid_{H}x{W}_n{n}_{o}", random_maps(n, H, W), o) for n in (1, 3) for o in GRID]


# ---- planted scenes ------------------------------------------------------------------------------------------------------------------------
class Planted:
    """maps [n][H][W], options, and check(out, stats): the property the scene was planted for, asserted on any tier's result"""

    def __init__(self, name, maps, o, check):
        self.name, self.maps, self.o, self.check = name, np.ascontiguousarray(maps, np.float32), o, check


def _empty(H, W, n=1):
    return np.full((n, H, W), np.nan, np.float32)


def _serpentine():
    H, W = 3 * TH, 3 * TW
    a = _empty(H, W)
    for y in range(0, H, 2):
        a[0, y, :] = 3.0
        if y + 1 < H:
            a[0, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = 3.0
    return a, int(np.isfinite(a).sum())


def planted_cases():
    cases = []

    def add(name, maps, o, check):
        cases.append(Planted(name, maps, o, check))

    def kept(mask):  # the masked pixels all survive
        return lambda out, stats: bool(np.isfinite(out[mask]).all())

    def gone(mask, comps=None):  # the masked pixels are all removed (and so many components)
        return lambda out, stats: bool(np.isnan(out[mask]).all()) and (comps is None or int(stats[:, 1].sum()) == comps)

    # a one-pixel-wide serpentine through every tile of a 3 x 3-tile map: one component
    a, length = _serpentine()
    m = np.isfinite(a)
    add("serpentine_kept", a, Options(0, length - 1, 0.0), kept(m))
    add("serpentine_removed", a, Options(0, length, 0.0), gone(m, 1))
    add("serpentine_removed_max", a, Options(0, 2**31 - 1, 0.0), gone(m, 1))
    # a U whose arms lie in the tile (0, 0) and join only in the tile below
    a = _empty(2 * TH, TW)
    a[0, 0:TH + 3, 2] = 1.0
    a[0, 0:TH + 3, 6] = 1.0
    a[0, TH + 2, 2:7] = 1.0
    m = np.isfinite(a)
    size = int(m.sum())
    add("u_kept", a, Options(0, size - 1, 0.0), kept(m))
    add("u_removed", a, Options(0, size, 0.0), gone(m, 1))
    # two 2 x 2 blocks that touch diagonally at a tile corner: never joined
    a = _empty(2 * TH, 2 * TW)
    a[0, TH - 2:TH, TW - 2:TW] = 1.0
    a[0, TH:TH + 2, TW:TW + 2] = 1.0
    m = np.isfinite(a)
    add("diagonal_two_components", a, Options(0, 4, 0.0), gone(m, 2))
    add("diagonal_kept", a, Options(0, 3, 0.0), kept(m))
    # a checkerboard of valid / NaN pixels: every component has size 1
    yy, xx = np.indices((TH + 3, TW + 5))
    a = np.where((yy + xx) % 2 == 0, np.float32(2.0), NAN)[None]
    m = np.isfinite(a)
    add("checkerboard", a, Options(0, 1, 1.0), lambda out, stats, m=m: bool(np.isnan(out).all()) and stats[0].tolist() == [m.sum(), m.sum(), m.sum()])
    # components of exactly S and S + 1 pixels
    a = _empty(5, 12)
    a[0, 1, 2:7] = 1.0
    a[0, 3, 2:8] = 1.0
    add("size_S_and_S_plus_1", a, Options(0, 5, 0.0),
        lambda out, stats: bool(np.isnan(out[0, 1]).all() and np.isfinite(out[0, 3, 2:8]).all()) and stats[0].tolist() == [11, 1, 5])
    # a ramp whose neighbours differ by exactly speckle_max_diff (multiples of 0.5: every fp64 difference is exact): one component
    a = _empty(3, 2 * TW + 6)
    a[0, 1, :] = 0.5 * np.arange(2 * TW + 6)
    m = np.isfinite(a)
    add("ramp_kept", a, Options(0, 2 * TW + 5, 0.5), kept(m))
    add("ramp_removed", a, Options(0, 2 * TW + 6, 0.5), gone(m, 1))
    # the same with one step of diff + the next float32, at a tile border: it splits there.  8 .. 15.5 stay in one binade, so the steps
    # after the split are exact again
    a = _empty(3, 2 * TW)
    ramp = (8 + 0.5 * np.arange(16)).astype(np.float32)
    ramp[8:] = np.nextafter(ramp[8:], np.float32(np.inf))
    steps = np.diff(ramp.astype(np.float64))
    assert (np.delete(steps, 7) == 0.5).all() and steps[7] > 0.5
    a[0, 1, TW - 8:TW + 8] = ramp
    m = np.isfinite(a)
    add("ramp_split", a, Options(0, 8, 0.5), gone(m, 2))
    add("ramp_split_kept", a, Options(0, 7, 0.5), kept(m))
    # an island in the last row of map 0 above valid pixels in the first row of map 1: never joined
    a = _empty(TH + 1, TW + 1, n=2)
    a[0, TH, 3:6] = 2.0
    a[1, 0, :] = 2.0
    add("map_border", a, Options(0, 3, 0.0),
        lambda out, stats: bool(np.isnan(out[0]).all() and np.isfinite(out[1, 0]).all()) and stats.tolist() == [[3, 1, 3], [TW + 1, 0, 0]])
    # an island at the end of a row and one at the start of the next row: never joined
    a = _empty(6, TW + 1)
    a[0, 2, TW - 1:] = 2.0
    a[0, 3, :2] = 2.0
    m = np.isfinite(a)
    add("row_wrap_two_components", a, Options(0, 2, 0.0), gone(m, 2))
    add("row_wrap_kept", a, Options(0, 1, 0.0), kept(m))
    # +-inf and -0.0 on input
    a = np.array([[[np.inf, -np.inf, -0.0, 1.0, np.nan]]], np.float32)
    for mh in (0, 1):  # with the median, the window of the 1.0 holds {+0.0, 1.0}: the lower one
        bits = [0, int(np.float32(0.0 if mh else 1.0).view(np.int32))]
        add(f"inf_and_negative_zero_m{mh}", a, Options(mh, 0, 1.0),
            lambda out, stats, bits=bits: bool(np.isnan(out[0, 0, [0, 1, 4]]).all()) and out[0, 0, 2:4].view(np.int32).tolist() == bits
            and stats[0].tolist() == [2, 0, 0])
    # median: a window with all neighbours NaN
    a = _empty(5, 5)
    a[0, 2, 2] = 7.0
    add("median_lonely_pixel", a, Options(2, 0, 1.0), lambda out, stats: out[0, 2, 2] == 7.0 and int(np.isfinite(out).sum()) == 1)
    # median: even k takes the lower of the two middle values
    a = _empty(3, 4)
    a[0, 1, 1], a[0, 1, 2] = 5.0, 3.0
    add("median_even_k", a, Options(1, 0, 1.0), lambda out, stats: out[0, 1, 1] == 3.0 and out[0, 1, 2] == 3.0)
    # median: W and H smaller than the window
    a = np.array([[[4.0, 1.0], [3.0, 2.0]]], np.float32)
    add("median_small_map", a, Options(2, 0, 1.0), lambda out, stats: bool((out == 2.0).all()))
    add("median_one_pixel", np.array([[[9.0]]], np.float32), Options(2, 0, 1.0), lambda out, stats: out[0, 0, 0] == 9.0)
    # median: an image-border pixel (the corner's window has 4 values, the lower median is the second)
    a = (np.arange(20, dtype=np.float32).reshape(1, 4, 5) * 3) % 7
    add("median_border", a, Options(1, 0, 1.0), lambda out, stats, a=a: out[0, 0, 0] == np.sort(a[0, :2, :2].ravel())[1]
        and out[0, 3, 4] == np.sort(a[0, 2:, 3:].ravel())[1] and out[0, 0, 2] == np.sort(a[0, :2, 1:4].ravel())[2])
    return cases


# ---- the occluded strip of tests/test_sgm_gpu.py::test_occluded_strip ----------------------------------------------------------------------
STRIP = (slice(2, 22), slice(48, 56))       # left columns whose match lies in the replaced strip of the right image
ELSEWHERE = (slice(2, 22), slice(20, 40))
STRIP_FILTER = Options(1, 20, 1.0)


def strip_pair():
    from tests import stereo_ref as S

    L, R, _ = S.truth_pair(lambda x, y: 6.0, H=24, W=96)
    R = R.copy()
    R[:, 40:52] = S.truth_pair(lambda x, y: 6.0, H=24, W=96, seed=9)[1][:, 10:22]
    return L, R


def strip_shares(disp):
    """(finite share of the strip, wrong share of the strip: |d - 6| > 1 among all its pixels, finite share elsewhere)"""
    s = disp[STRIP]
    return float(np.isfinite(s).mean()), float((np.isfinite(s) & (np.abs(s - 6.0) > 1.0)).mean()), float(np.isfinite(disp[ELSEWHERE]).mean())
