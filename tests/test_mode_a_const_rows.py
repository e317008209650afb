"""Mode A writes the Jacobian's structural constants once per output buffer, not on every pass.

Seven of the 2 P Jacobian rows of an observation are literals in reproj_core (calibration_amd/csrc/reproj_math.hpp): +0.0 or 1.0
whatever the observation, the parameters, the chain, the camera model and the scalar type.  jac_const() in that header is the one
statement of which; k_eval skips those rows and a fill kernel writes them when the buffer is obtained.

CPU tier: tests/mode_a_const_rows/check.cpp, a stand-alone program built here with the host compiler, pins jac_const() against
reproj_point() (marked entries bit-equal to the fill values, live entries not constant, exactly seven marked).

GPU tier: what a pre-filled buffer can get wrong - a fill that is stale after a layout switch, a scalar switch, a reallocation or
on a block recycled from another handle.  Everything goes through the C ABI.  Live entries are held to the oracle at the parity
suite's bars (fp64: 1e-9 absolute on residuals, 1e-9 * max(1, |J|) on Jacobian entries; fp32: 3e-4 and 2e-4, the bars of
test_gpu_parity.test_fp32_mode_a_error_vs_fp64_oracle); constants are compared bit for bit through an integer view, at the
positions the program above prints from jac_const() itself.
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
SRC = os.path.join(ROOT, "tests", "mode_a_const_rows", "check.cpp")
CSRC = os.path.join(ROOT, "calibration_amd", "csrc")


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("const_rows") / "check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def const_table(check_program):
    """{(chain, model): [(row, column, value), ...]} as jac_const() marks them."""
    out = subprocess.run([check_program, "table"], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.split("\n"):
        if line.strip():
            chain, model, row, k, val = map(int, line.split())
            table.setdefault((chain, model), []).append((row, k, val))
    return table


def test_jac_const_matches_reproj_point(check_program):
    p = subprocess.run([check_program], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all ok" in p.stdout


def test_table_has_seven_entries_per_chain_and_model(const_table):
    assert sorted(const_table) == [(c, m) for c in range(3) for m in range(2)]
    assert all(len(v) == 7 for v in const_table.values())


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------
def _check(flat, const_table, r1, J1, r0, J0, r_tol=1e-9, j_tol=1e-9):
    """r1, J1 (fetched) against the oracle's r0, J0: constants bit-exact, everything else within the bars."""
    marked = const_table[(int(flat.chain), int(flat.model))]
    assert len(marked) == 7
    as_int = np.uint64 if J1.dtype == np.float64 else np.uint32
    live = np.ones(J1.shape, dtype=bool)
    for row, k, val in marked:
        want = np.array([val], dtype=J1.dtype).view(as_int)[0]  # +0.0 -> all bits clear, 1.0 -> 0x3FF0... / 0x3F80...
        got = np.ascontiguousarray(J1[row::2, k]).view(as_int)
        assert (got == want).all(), (row, k, val, J1[row::2, k][got != want][:4])
        assert (J0[row::2, k] == val).all()  # the oracle agrees that it is a constant
        live[row::2, k] = False
    assert np.abs(r0 - r1).max() <= r_tol
    err = np.abs(J0 - J1) / np.maximum(1.0, np.abs(J0))
    assert err[live].max() <= j_tol


@pytest.mark.gpu
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("kind", ["intr", "ext", "bundle"])
def test_all_chains_and_models(gpu_lib, oracle, const_table, kind, model):
    sc = SCENES[kind](model)
    _perturb_intr(sc)
    r0, J0 = helpers.oracle_eval(oracle, sc.flat)
    with optim.ReprojHandle(sc.flat) as h:
        h.eval()
        r1, J1 = h.eval_fetch()
    _check(sc.flat, const_table, r1, J1, r0, J0)


@pytest.mark.gpu
def test_ragged_views(gpu_lib, oracle, const_table):
    """views of 1, 2, 3, 127, 128, 129 and 257 points: a partial last tile, an odd count, a tile holding a single pair."""
    f = synth.scene_intrinsics(7, rows=17, cols=17).flat
    keep = [1, 2, 3, 127, 128, 129, 257]
    views = []
    for b, n in enumerate(keep):
        lo = f.blk_offset[b]
        views.append(np.stack([f.X[lo:lo + n], f.Y[lo:lo + n], f.u[lo:lo + n], f.v[lo:lo + n]], axis=1))
    flat = optim.FlatProblem(f.chain, f.model, views, np.zeros(7, np.int32), np.arange(7, dtype=np.int32), f.intr, None,
                             f.view_pose, None)
    r0, J0 = helpers.oracle_eval(oracle, flat)
    with optim.ReprojHandle(flat) as h:
        h.eval()
        r1, J1 = h.eval_fetch()
        assert h.n_obs == sum(keep)
    _check(flat, const_table, r1, J1, r0, J0)


@pytest.mark.gpu
def test_two_evaluations_on_one_handle(gpu_lib, oracle, const_table):
    sc = SCENES["ext"](0)
    _perturb_intr(sc)
    with optim.ReprojHandle(sc.flat) as h:
        h.eval()
        ra, Ja = h.eval_fetch()
        _check(sc.flat, const_table, ra, Ja, *helpers.oracle_eval(oracle, sc.flat))
        rng = np.random.default_rng(5)
        view_pose = np.array(sc.flat.view_pose, dtype=np.float64).reshape(-1, 7)
        view_pose[:, 4:] += 1e-2 * rng.uniform(-1, 1, (view_pose.shape[0], 3))
        h.set_params(intr=sc.flat.intr * (1 + 0.01 * rng.uniform(-1, 1, sc.flat.intr.shape)), view_pose=view_pose)
        r0, J0 = helpers.oracle_eval(oracle, sc.flat)  # set_params wrote the new values into sc.flat
        h.eval()
        rb, Jb = h.eval_fetch()
    _check(sc.flat, const_table, rb, Jb, r0, J0)
    assert np.abs(Ja - Jb).max() > 1e-3  # the live entries did follow the new parameters


@pytest.mark.gpu
def test_layout_switch_on_a_live_handle(gpu_lib, oracle, const_table, monkeypatch):
    """Blocked, then whole-array columns, then blocked again, on one handle.  15 tiles of 88 observations: the column layout needs
    44 * 1536 doubles and the blocked one 15 * 46 * 128 = 88 320, so the second layout keeps the first one's block and a fill that
    is not redone leaves live values of the other layout where the constants belong."""
    monkeypatch.delenv("CBA_EVAL_BLOCKED", raising=False)
    monkeypatch.delenv("CBA_EVAL_VARIANT", raising=False)
    sc = SCENES["ext"](0)
    _perturb_intr(sc)
    r0, J0 = helpers.oracle_eval(oracle, sc.flat)
    with optim.ReprojHandle(sc.flat) as h:
        h.eval()
        _check(sc.flat, const_table, *h.eval_fetch(), r0, J0)
        monkeypatch.setenv("CBA_EVAL_BLOCKED", "0")
        h.eval_timed(0, 1)
        _check(sc.flat, const_table, *h.eval_fetch(), r0, J0)
        monkeypatch.setenv("CBA_EVAL_BLOCKED", "1")
        h.eval_timed(0, 1)
        _check(sc.flat, const_table, *h.eval_fetch(), r0, J0)


@pytest.mark.gpu
def test_recycled_block(gpu_lib, oracle, const_table):
    """A handle's released output block goes to the next handle with its old contents.
    Extrinsic chain, P = 22: 15 blocks of 88 observations = 15 tiles of (2 + 44) * 128 * 8 = 47 104 B -> 706 560 B.
    Intrinsic chain, P = 16: 20 views of 88 = 20 tiles of (2 + 32) * 128 * 8 = 34 816 B -> 696 320 B.
    Both lie in (512 KiB, 1 MiB], the block cache's 1 MiB class, far below its 16 MiB limit; the first handle leaves live
    values of a 46-row tile where the second expects the constants of a 34-row one."""
    gpu_lib.cba_trim_cache()  # the only 1 MiB block the cache can hand out is the first handle's
    a = SCENES["ext"](0)
    with optim.ReprojHandle(a.flat) as h:
        h.eval()
        _check(a.flat, const_table, *h.eval_fetch(), *helpers.oracle_eval(oracle, a.flat))
    b = synth.scene_intrinsics(20)
    assert b.flat.n_obs == 20 * 88
    _perturb_intr(b)
    r0, J0 = helpers.oracle_eval(oracle, b.flat)
    with optim.ReprojHandle(b.flat) as h:
        h.eval()
        r1, J1 = h.eval_fetch()
    _check(b.flat, const_table, r1, J1, r0, J0)


@pytest.mark.gpu
def test_scalar_switch(gpu_lib, oracle, const_table):
    sc = SCENES["ext"](0, noise_px=0.3)
    _perturb_intr(sc)
    r0, J0 = helpers.oracle_eval(oracle, sc.flat)
    with optim.ReprojHandle(sc.flat) as h:
        h.set_scalar(1)
        h.eval()
        r1, J1 = h.eval_fetch_f32()
        assert J1.dtype == np.float32
        _check(sc.flat, const_table, r1, J1, r0, J0, r_tol=3e-4, j_tol=2e-4)
        h.set_scalar(0)
        h.eval()
        r2, J2 = h.eval_fetch()
        _check(sc.flat, const_table, r2, J2, r0, J0)


@pytest.mark.gpu
def test_block_range_fetch(gpu_lib, const_table):
    """273 observations per view = 3 tiles, the last one partial: a block's tiles are found by walking the ones before it."""
    sc = synth.scene_intrinsics(5, rows=13, cols=21, noise_px=0.3)
    f = sc.flat
    with optim.ReprojHandle(f) as h:
        h.eval()
        r, J = h.eval_fetch()
        for b in (0, 2, 4):
            rb, Jb = h.eval_fetch_blocks(b, b + 1)
            lo, hi = int(f.blk_offset[b]), int(f.blk_offset[b + 1])
            assert np.array_equal(rb.view(np.uint64), r[2 * lo:2 * hi].view(np.uint64))
            assert np.array_equal(Jb.view(np.uint64), J[2 * lo:2 * hi].view(np.uint64))
