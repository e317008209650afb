"""CPU tier: the scenes of tests/resident_scenes.py are what they claim to be, on the reference alone.

tests/test_resident_edges_gpu.py holds the resident LM kernel (resident_lm.hip) to the project's parity bars at the shapes where
its code changes path.  That says something only if (1) each scene really has the width, the number of effective columns, the
block, view and tile counts and the run of rejections it is there for, and (2) the two references the kernel is compared with - the
oracle's dense solver and the host-side form of the iteration - agree with each other far inside the bar at the very cap the
GPU case runs: a scene on which two correct solvers already sit a third of the bar apart is ill-conditioned and tests the
valley, not the kernel.  Both are asserted here for every (scene, cap); the pair figures are printed (pytest -s, "FIGURES ...")
and kept in resident_scenes.CPU_PAIR.
"""
import numpy as np
import pytest

from calibration_amd import capi
from tests import helpers
from tests import resident_scenes as rs


@pytest.mark.parametrize("name", [s.name for s in rs.SCENES])
def test_scene_has_the_structure_it_is_there_for(hostmath, name):
    sc = rs.BY_NAME[name]
    flat = sc.make()
    assert rs.shared_width(flat) == sc.nsh <= rs.RES_NSH_MAX
    eff = rs.effective_columns(hostmath, flat, sc.options(rs.NONE))
    assert int(eff.sum()) == sc.m, (int(eff.sum()), sc.m)
    assert (flat.n_blocks, flat.n_views) == (sc.n_blocks, sc.n_views)
    tiles = rs.tiles_per_block(flat)
    assert int(tiles.sum()) == sc.n_tiles
    if sc.blk_tiles is None:
        assert (tiles == 1).all()
    else:
        assert tuple(int(t) for t in tiles) == sc.blk_tiles
    print(f"\nFIGURES {name}: nsh={sc.nsh} m={sc.m} blocks={sc.n_blocks} views={sc.n_views} tiles={sc.n_tiles} "
          f"obs={flat.n_obs} eff={''.join('x' if e else '.' for e in eff)}")


def test_the_set_covers_every_edge(hostmath):
    ms = {s.m for s in rs.SCENES}
    assert 0 in ms and 64 in ms and any(0 < m <= 63 for m in ms) and any(m >= 65 for m in ms)
    assert any(s.nsh == rs.RES_NSH_MAX for s in rs.SCENES)
    tiles = {s.n_tiles for s in rs.SCENES}
    assert any(t < rs.RES_WAVES for t in tiles) and rs.RES_WAVES in tiles and rs.RES_WAVES + 1 in tiles
    multi = [s for s in rs.SCENES if s.blk_tiles]
    assert any(2 in s.blk_tiles and 1 in s.blk_tiles for s in multi)
    assert 1 in rs.INTR_MULTI  # a tile of one observation
    assert any(s.n_blocks > rs.RES_THREADS and s.n_views > rs.RES_THREADS for s in rs.SCENES)
    assert any(s.n_blocks > rs.RES_THREADS and s.n_views == 0 for s in rs.SCENES)
    assert any(s.rejections for s in rs.SCENES)
    # the ragged rig: an idle camera whose columns are a hole in the MIDDLE of the effective list, and views some cameras miss
    flat = rs.BY_NAME["rig5-ragged"].make()
    eff = rs.effective_columns(hostmath, flat, rs.BY_NAME["rig5-ragged"].options(rs.NONE))
    assert not eff[32:48].any() and eff[48:].any() and eff[:32].any() and flat.intr.shape[0] == 5
    per_view = np.bincount(flat.blk_view, minlength=flat.n_views)
    assert sorted(set(int(v) for v in per_view)) == [3, 4]
    # the shapes the kernel must decline are just past its width, or fp32
    widths = sorted(rs.shared_width(mk()) for mk, _o, _n, scalar in rs.INELIGIBLE.values() if not scalar)
    assert widths == [86, 90, 96] and min(widths) > rs.RES_NSH_MAX
    for mk, _o, nsh, _scalar in rs.INELIGIBLE.values():
        assert rs.shared_width(mk()) == nsh


@pytest.mark.parametrize("name,cap", rs.CASES, ids=rs.case_id)
def test_reference_pair_agrees_far_inside_the_bar(oracle, hostmath, name, cap):
    sc = rs.BY_NAME[name]
    sh, fh, xs = rs.hostside_reference(hostmath, name, cap)
    capped = cap is not rs.NONE
    term = capi.TERM_NO_CONVERGENCE if capped else capi.TERM_CONVERGENCE
    assert sh.termination == term, bytes(sh.report)
    if capped:
        assert sh.iterations == cap
    else:
        assert sh.successful_steps >= sc.min_accepted
    if cap in sc.rejections:
        assert xs[5] == sc.rejections[cap] and xs[6] == 0, xs  # rejected steps; no line search
        assert sh.successful_steps == cap - xs[5]
    if not sc.uses_oracle(cap):
        print(f"\nFIGURES {name} cap={rs.case_id(cap)}: no oracle at this cap; host-side form {rs.counts(sh)}")
        return
    so, fo = rs.oracle_reference(oracle, name, cap)
    assert so.termination == term, bytes(so.report)
    assert rs.counts(sh) == rs.counts(so), (bytes(sh.report), bytes(so.report))
    pair = helpers.param_diff(fh, fo)
    bar = rs.BARS[sc.cls]
    print(f"\nFIGURES {name} cap={rs.case_id(cap)}: pair={pair:.1e} (recorded {rs.CPU_PAIR.get((name, cap), float('nan')):.1e}) "
          f"bar/3={bar / 3:.1e} counts={rs.counts(so)} rejected={xs[5]}")
    assert pair <= bar / 3.0, (pair, bar)
