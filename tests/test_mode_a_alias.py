"""Mode A holds the duplicated Jacobian entry (d v / d fy = d u / d skew) in one slot of its output and stores it once.

reproj_core (calibration_amd/csrc/reproj_math.hpp) assigns both entries the same expression, yd + m0y.  jac_alias() in that header
is the one statement of it; eval_row_slot() (eval_layout.hpp) resolves the v row's fy entry to the u row's skew slot, k_eval
stores the slot once, and every fetch hands back the full (2n, P) Jacobian with both entries present.

CPU tier: tests/mode_a_alias/check.cpp, a stand-alone program built here with the host compiler, pins jac_alias() against
reproj_point() and checks that eval_row_slot() is a layout (in range, no hole, exactly the named pair shares a slot, no constant
row shares one).  It runs once more built with -fsanitize=address,undefined.

GPU tier, through the C ABI only: what a shared, shifted slot can get wrong - a live row landing on a filled gap, a fetch reading
the old position, a stale slot after a second pass, a layout or scalar switch on a live handle, a batched transfer cut at the
wrong tile.  Bars of the parity suite (fp64: 1e-9 absolute on residuals, 1e-9 * max(1, |J|) on Jacobian entries; fp32: 3e-4 and
2e-4, the bars of test_gpu_parity.test_fp32_mode_a_error_vs_fp64_oracle); the aliased pair and the constants are compared bit for
bit through an integer view, at the positions the two check programs print from jac_alias() / jac_const() themselves.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from calibration_amd import optim
from tests import helpers, synth
from tests.test_gpu_parity import SCENES, _perturb_intr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "calibration_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "mode_a_alias", "check.cpp")
SRC_CONST = os.path.join(ROOT, "tests", "mode_a_const_rows", "check.cpp")


def _compile(src, exe, *flags):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wno-unknown-pragmas", *flags, "-I", CSRC, src, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mode_a_alias")
    return dict(alias=_compile(SRC, str(d / "check")), const=_compile(SRC_CONST, str(d / "check_const")), dir=d)


def _table(exe):
    out = subprocess.run([exe, "table"], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.split("\n"):
        if line.strip():
            chain, model, *entry = map(int, line.split())
            table.setdefault((chain, model), []).append(tuple(entry))
    return table


@pytest.fixture(scope="module")
def tables(programs):
    """({(chain, model): [(row, k, to_row, to_k)]} as jac_alias() marks them, {(chain, model): [(row, k, value)]} from jac_const())"""
    return _table(programs["alias"]), _table(programs["const"])


def test_alias_and_layout(programs):
    p = subprocess.run([programs["alias"]], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout


def test_alias_and_layout_under_sanitizers(programs):
    exe = _compile(SRC, str(programs["dir"] / "check_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout


def test_table_names_one_pair_per_chain_and_model(tables):
    alias, _ = tables
    assert sorted(alias) == [(c, m) for c in range(3) for m in range(2)]
    for (chain, _model), entries in alias.items():
        oi = 6 if chain == 0 else 12
        assert entries == [(1, oi + 1, 0, oi + 4)]  # v fy -> u skew


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------
def _set_skew(flat):
    intr = flat.intr.reshape(flat.n_cams, -1)
    intr[:, 4] = 0.7 + 0.2 * np.arange(flat.n_cams)


def _check(flat, tables, r1, J1, r0, J0, r_tol=1e-9, j_tol=1e-9):
    """r1, J1 (fetched) against the oracle's r0, J0 at the bars; the aliased pair bit-equal and not constant; the seven constants
    bit-exact at their positions."""
    alias, const = tables
    key = (int(flat.chain), int(flat.model))
    as_int = np.uint64 if J1.dtype == np.float64 else np.uint32
    assert np.abs(r0 - r1).max() <= r_tol
    assert (np.abs(J0 - J1) / np.maximum(1.0, np.abs(J0))).max() <= j_tol
    (row, k, to_row, to_k), = alias[key]
    a = np.ascontiguousarray(J1[row::2, k]).view(as_int)
    b = np.ascontiguousarray(J1[to_row::2, to_k]).view(as_int)
    assert np.array_equal(a, b)
    assert len(a) < 2 or len(np.unique(a)) > 1  # a live entry, not a fill value
    assert len(const[key]) == 7
    for row, k, val in const[key]:
        want = np.array([val], dtype=J1.dtype).view(as_int)[0]
        got = np.ascontiguousarray(J1[row::2, k]).view(as_int)
        assert (got == want).all(), (row, k, val)


def _ragged(counts, rows=17, cols=17):
    """An intrinsics problem whose view b keeps the first counts[b] points of its grid."""
    f = synth.scene_intrinsics(len(counts), rows=rows, cols=cols).flat
    views = []
    for b, n in enumerate(counts):
        lo = int(f.blk_offset[b])
        assert lo + n <= f.blk_offset[b + 1]
        views.append(np.stack([f.X[lo:lo + n], f.Y[lo:lo + n], f.u[lo:lo + n], f.v[lo:lo + n]], axis=1))
    nb = len(counts)
    flat = optim.FlatProblem(f.chain, f.model, views, np.zeros(nb, np.int32), np.arange(nb, dtype=np.int32), f.intr, None,
                             f.view_pose, None)
    _set_skew(flat)
    return flat


@pytest.mark.gpu
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("kind", ["intr", "ext", "bundle"])
def test_all_chains_and_models(gpu_lib, oracle, tables, kind, model):
    sc = SCENES[kind](model)
    _perturb_intr(sc)
    _set_skew(sc.flat)
    r0, J0 = helpers.oracle_eval(oracle, sc.flat)
    with optim.ReprojHandle(sc.flat) as h:
        h.eval()
        r1, J1 = h.eval_fetch()
    _check(sc.flat, tables, r1, J1, r0, J0)


@pytest.mark.gpu
def test_tile_edges(gpu_lib, oracle, tables):
    """Views of 1, 2, 127, 128, 129 and 257 observations on one handle: a full tile, one short of it, one past it (a second tile
    holding one padded pair), three tiles, odd and even pair tails.  Then a block range that starts and ends mid-problem."""
    counts = [1, 2, 127, 128, 129, 257]
    flat = _ragged(counts)
    r0, J0 = helpers.oracle_eval(oracle, flat)
    with optim.ReprojHandle(flat) as h:
        h.eval()
        assert h.n_obs == sum(counts)
        r1, J1 = h.eval_fetch()
        _check(flat, tables, r1, J1, r0, J0)
        for b0, b1 in ((2, 5), (1, 2), (4, 6)):
            rb, Jb = h.eval_fetch_blocks(b0, b1)
            lo, hi = int(flat.blk_offset[b0]), int(flat.blk_offset[b1])
            assert np.array_equal(rb.view(np.uint64), r1[2 * lo:2 * hi].view(np.uint64))
            assert np.array_equal(Jb.view(np.uint64), J1[2 * lo:2 * hi].view(np.uint64))


@pytest.mark.gpu
def test_two_evaluations_on_one_handle(gpu_lib, oracle, tables):
    """fy, skew and the distortion move between two passes: both logical entries follow (neither is served from a stale slot)."""
    sc = SCENES["ext"](1)
    _perturb_intr(sc)
    _set_skew(sc.flat)
    alias, _ = tables
    (row, k, to_row, to_k), = alias[(int(sc.flat.chain), int(sc.flat.model))]
    with optim.ReprojHandle(sc.flat) as h:
        h.eval()
        ra, Ja = h.eval_fetch()
        _check(sc.flat, tables, ra, Ja, *helpers.oracle_eval(oracle, sc.flat))
        intr = sc.flat.intr.reshape(sc.flat.n_cams, -1).copy()
        intr[:, 1] *= 1.03          # fy
        intr[:, 4] += 0.4           # skew
        intr[:, 5:10] *= 1.5        # k1 k2 k3 p1 p2
        h.set_params(intr=intr)
        r0, J0 = helpers.oracle_eval(oracle, sc.flat)  # set_params wrote the new values into sc.flat
        h.eval()
        rb, Jb = h.eval_fetch()
    _check(sc.flat, tables, rb, Jb, r0, J0)
    for rr, kk in ((row, k), (to_row, to_k)):
        assert np.abs(Ja[rr::2, kk] - Jb[rr::2, kk]).max() > 1e-6  # the entry did move


@pytest.mark.gpu
def test_layout_and_scalar_switch_on_a_live_handle(gpu_lib, oracle, tables, monkeypatch):
    """Blocked, whole-array columns, blocked again, then fp32 and back to fp64, on one handle: every layout goes through the one
    slot map, and no switch leaves an entry of the pair (or a constant) where the other layout had something else."""
    monkeypatch.delenv("CBA_EVAL_BLOCKED", raising=False)
    monkeypatch.delenv("CBA_EVAL_VARIANT", raising=False)
    sc = SCENES["ext"](0, noise_px=0.3)
    _perturb_intr(sc)
    _set_skew(sc.flat)
    r0, J0 = helpers.oracle_eval(oracle, sc.flat)
    with optim.ReprojHandle(sc.flat) as h:
        h.eval()
        _check(sc.flat, tables, *h.eval_fetch(), r0, J0)
        monkeypatch.setenv("CBA_EVAL_BLOCKED", "0")
        h.eval_timed(0, 1)
        _check(sc.flat, tables, *h.eval_fetch(), r0, J0)
        monkeypatch.setenv("CBA_EVAL_BLOCKED", "1")
        h.eval_timed(0, 1)
        _check(sc.flat, tables, *h.eval_fetch(), r0, J0)
        monkeypatch.delenv("CBA_EVAL_BLOCKED")
        h.set_scalar(1)
        h.eval()
        r1, J1 = h.eval_fetch_f32()
        assert J1.dtype == np.float32
        _check(sc.flat, tables, r1, J1, r0, J0, r_tol=3e-4, j_tol=2e-4)
        h.set_scalar(0)
        h.eval()
        _check(sc.flat, tables, *h.eval_fetch(), r0, J0)


@pytest.mark.gpu
def test_batched_fetch(gpu_lib, oracle, tables):
    """300 views of one observation pair = 300 tiles.  The fetch moves runs of tiles through a 4 MiB staging buffer: at P = 16 a
    tile is 33 * 128 * 8 = 33 792 B in fp64 (124 tiles per transfer: 124 + 124 + 52) and 16 896 B in fp32 (248 + 52), so both
    fetches take several transfers and end on a partial one.  The oracle is the tile-by-tile reference: row i of its output is
    observation i whatever transfer brought it."""
    flat = _ragged([2] * 300, rows=2, cols=2)
    r0, J0 = helpers.oracle_eval(oracle, flat)
    with optim.ReprojHandle(flat) as h:
        h.eval()
        r1, J1 = h.eval_fetch()
        _check(flat, tables, r1, J1, r0, J0)
        rb, Jb = h.eval_fetch_blocks(100, 290)  # starts inside the first transfer's range, ends inside the last one's
        assert np.array_equal(rb.view(np.uint64), r1[400:1160].view(np.uint64))
        assert np.array_equal(Jb.view(np.uint64), J1[400:1160].view(np.uint64))
        h.set_scalar(1)
        h.eval()
        r2, J2 = h.eval_fetch_f32()
    _check(flat, tables, r2, J2, r0, J0, r_tol=3e-4, j_tol=2e-4)
