"""GPU tier: every form of the shared-rows Mode B kernel (kernels_modeb.hip k_ne_shared) at its group and tile edges.

The launcher picks one of three paths by the problem's tile table (capi.cpp, structure.hpp choose_mode_b_tile: tiles of 2048
observations for problems of this size; a group is 64 * NP observations, NP = the wavefronts of the form's workgroup):

  "one"    every tile <= 64 NP observations: the single-group instantiation (ONE = true);
  "multi"  the general kernel, one tile per block: rows go straight to blk_acc (direct forms) or blk_mom (moment forms);
  "split"  the general kernel with blocks of several tiles: rows go to `partial`, then k_tile_sum or k_mom_expand.

Each of chain {intrinsic, extrinsic, bundle} x model {pinhole + Brown-Conrady, Scheimpflug} x scalar {fp64, fp32} - plus, in fp64,
the per-part direct launches of the two-pose chains (CBA_MODEB_MOMENTS=0) - runs one problem per path.  Every problem draws its
blocks from ONE 65 x 65 board: a block of n points is the first n entries of a seeded random permutation of the board (the board is
generated row by row: its first n points would lie on one line), seen with 0.3 px noise through intrinsics 1 % off.

Reference: the oracle's Jet Jacobian (helpers.oracle_block_normal_eq).  Two measures:
  block-max   |d| / the block's largest entry (the project's bar, 1e-10 in fp64) - blind to the small entries: focal-length sums
              are many orders above those of k3, the tangential terms or the sensor tilt;
  scaled      |dH_ij| / sqrt(H_ii H_jj),  |dg_i| / (sqrt(H_ii) |r|),  |d|r|^2| / |r|^2  with H_ii, |r| from the oracle; where the
              oracle's H_ii is exactly 0 the difference must be exactly 0.

Bounds of the scaled measure come from the reference alone (FLOORS below, measured on the CPU by measure_floors()):
  fp64  floor = the scaled difference between the oracle at the inputs and the oracle at inputs whose every parameter and
        observation is multiplied by 1 +- 2^-52 (seeded random signs): what ONE rounding of the inputs does to a correct
        implementation.  The kernel gets 32 x: its analytic Jacobian rounds tens of times per entry and it sums up to 4097 terms
        in another order.
  fp32  floor = the same between the oracle at the fp64 inputs and at the inputs rounded to float32 and back.  The kernel gets
        8 x: it accumulates in fp64, only the per-observation roundings add to the rounding of the inputs.  The block-max measure
        and the cost have no fp32 bar in the project; they get 8 x their own floor, measured the same way.
A floor is the maximum over the three problems of a form.  Regenerate the table with

    python -m tests.test_mode_b_forms_gpu

(CPU only; it builds the oracle if needed and prints the FLOORS literal).  tests/test_mode_b_floors_cpu.py re-measures it on the
CPU tier.  A floor above 1e-6 (fp64) / 1e-2 (fp32) means the scene is too ill-conditioned to test anything: change the scene.

Every test prints its figures next to their bounds before it asserts (pytest -s, lines "FIGURES ...").  For scale: the host build
of the same device math (tests/cpu_backend, fp64, sequential sums) gives H <= 6.5e-15, g <= 2.5e-14, s <= 2.0e-14 on these
problems, against bounds of 3e-13 .. 9e-13, 1.3e-12 .. 6e-12 and 1.2e-12 .. 7e-12.
"""
import functools
import os
import re

import numpy as np
import pytest

from calibration_amd import capi, optim
from calibration_amd.geometry import inv, make_pose, pose_from_matrix
from tests import helpers, synth

pytestmark = pytest.mark.gpu

CHAINS = {"intr": capi.CHAIN_INTRINSIC, "ext": capi.CHAIN_EXTRINSIC, "bundle": capi.CHAIN_BUNDLE}
MODELS = {"pinhole": capi.CAMERA_PINHOLE_BC, "scheimpflug": capi.CAMERA_SCHEIMPFLUG}
PROBLEMS = ("one", "multi", "split")
DELTAS = (1.0, -1.0, 25.0)
BOARD = 65  # 65 x 65 = 4225 points >= the longest block (4097)
FP64_FACTOR, FP32_FACTOR = 32.0, 8.0
FP64_FLOOR_CAP, FP32_FLOOR_CAP = 1e-6, 1e-2

# wavefronts per workgroup of the form that runs by default: (direct | moment, model) -> NP
NP_TABLE = {("direct", "pinhole"): 2, ("direct", "scheimpflug"): 4, ("moment", "pinhole"): 4, ("moment", "scheimpflug"): 4}
# The moment form of the pinhole model ran 3 wavefronts before the 4-wavefront split became its default (the per-part launches
# still use 3 parts): its problems keep the group edges of 3 wavefronts as well, as further blocks.
NP_EXTRA = {("moment", "pinhole"): (3,)}

# scaled floors (H, g, s) and, for fp32, the floors of the block-max measure and of the relative cost error, by measure_floors()
FLOORS = {
    ("intr", "pinhole", "fp64"): dict(H=1.03e-14, g=5.07e-14, s=3.83e-14),
    ("intr", "pinhole", "fp32"): dict(H=6.42e-07, g=1.32e-05, s=2.01e-05, blockmax=1.95e-07, cost=1.76e-06),
    ("intr", "scheimpflug", "fp64"): dict(H=1.28e-14, g=3.91e-14, s=7.09e-14),
    ("intr", "scheimpflug", "fp32"): dict(H=7.36e-07, g=6.25e-06, s=8.66e-06, blockmax=1.01e-07, cost=3.60e-06),
    ("ext", "pinhole", "fp64"): dict(H=1.09e-14, g=9.56e-14, s=1.35e-13),
    ("ext", "pinhole", "fp32"): dict(H=7.08e-07, g=8.94e-06, s=1.68e-05, blockmax=1.43e-07, cost=2.18e-06),
    ("ext", "scheimpflug", "fp64"): dict(H=9.23e-15, g=1.56e-13, s=1.89e-13),
    ("ext", "scheimpflug", "fp32"): dict(H=7.82e-07, g=1.08e-05, s=1.44e-05, blockmax=9.73e-08, cost=1.13e-06),
    ("bundle", "pinhole", "fp64"): dict(H=1.88e-14, g=1.82e-13, s=2.31e-13),
    ("bundle", "pinhole", "fp32"): dict(H=8.04e-07, g=2.20e-05, s=4.09e-05, blockmax=1.32e-07, cost=3.00e-06),
    ("bundle", "scheimpflug", "fp64"): dict(H=2.75e-14, g=1.92e-13, s=1.48e-13),
    ("bundle", "scheimpflug", "fp32"): dict(H=3.66e-06, g=6.94e-05, s=2.37e-05, blockmax=1.38e-07, cost=5.44e-06),
}


def form_of(chain):
    return "direct" if chain == "intr" else "moment"


def documented_np():
    """NP per form as the launcher (kernels_modeb.hip launch_normal_eq_shared_rows) and the tile table (structure.hpp
    choose_mode_b_tile) document their defaults."""
    csrc = os.path.join(helpers.ROOT, "calibration_amd", "csrc")
    src = open(os.path.join(csrc, "kernels_modeb.hip")).read()
    d = re.search(r"dparts_env \? dparts_env : \(e\.model == CAM_SCHEIMPFLUG \? (\d) : (\d)\)", src)
    v = re.search(r'std::atoi\(cba_exp_env\("CBA_MODEB_VARIANT"\)\) : (\d+);', src)
    assert d and v, "the launcher's defaults are no longer where this test reads them"
    parts = int(v.group(1)) & 15
    out = {("direct", "scheimpflug"): int(d.group(1)), ("direct", "pinhole"): int(d.group(2)),
           ("moment", "pinhole"): parts if parts in (2, 4, 5) else 3, ("moment", "scheimpflug"): parts if parts in (3, 5) else 4}
    t = re.search(r"np_obs = two_wavefront_form \? (\d+) : (\d+)", open(os.path.join(csrc, "structure.hpp")).read())
    assert t, "structure.hpp no longer states the observations per group"
    return out, (int(t.group(1)), int(t.group(2)))


def block_sizes(chain, model, problem):
    """-> (sizes, dup): the block lengths of the problem; dup = indices of the two blocks that share one point list."""
    key = (form_of(chain), model)
    np_all = (NP_TABLE[key],) + NP_EXTRA.get(key, ())
    sizes, dup = [], ()
    if problem == "one":
        sizes = [1, 2, 63, 64, 65]
        for n in sorted(np_all):
            sizes += [64 * n - 1, 64 * n]  # the largest tile is exactly 64 NP of the form that runs: ONE = true
    elif problem == "multi":
        for n in np_all:
            sizes += [64 * n + 1, 128 * n - 1, 128 * n, 128 * n + 1, 192 * n + 65]
        sizes += [2047, 2048]
        odd = 128 * NP_TABLE[key] + 77  # three groups, the last one partly filled
        dup = (len(sizes), len(sizes) + 1)  # after a block of another length: xy_start and start differ inside the prefetching loop
        sizes += [odd, odd]
    else:
        sizes = [2049, 3000, 4096, 4097, 1, 65] + [64 * n for n in np_all]  # 4097 = 2048 + 2048 + 1
    return sizes, dup


def _grid():
    return synth.make_target_grid(BOARD, BOARD, 0.02)  # 1.28 m x 1.28 m


def _camera(model, rng):
    cam = synth.camera_gt(model, True)
    if model == capi.CAMERA_SCHEIMPFLUG:
        cam[10:12] = (0.2, -0.15)
    cam[0:2] *= 1 + 0.01 * rng.uniform(-1, 1, 2)
    return cam


@functools.lru_cache(maxsize=None)
def problem(chain, model, prob):
    """The FlatProblem of (chain, model, problem); shared by every test, never modified."""
    ch, md = CHAINS[chain], MODELS[model]
    sizes, dup = block_sizes(chain, model, prob)
    nb = len(sizes)
    rng = np.random.default_rng([11, ch, md, PROBLEMS.index(prob)])
    grid = _grid()
    picks = [grid[rng.permutation(len(grid))[:n]] for n in sizes]
    if dup:
        picks[dup[1]] = picks[dup[0]].copy()
    wide = dict(dist=2.0, max_tilt_deg=45.0, jitter=0.3, depth_spread=0.4)
    n_cams = 1 if chain == "intr" else 2
    cams = [_camera(md, rng) for _ in range(n_cams)]
    bcam = [b % n_cams for b in range(nb)]  # both cameras own blocks of different sizes
    n_grp = (nb + n_cams - 1) // n_cams     # views (extrinsic chain) or robot poses (bundle chain)
    near = lambda T: synth.perturb_pose(T, rng, 0.1, 0.001)
    if chain == "intr":
        poses = synth.random_view_poses(nb, rng, **wide)
        views = [synth.render_view(cams[0], poses[b], picks[b], 0.3, rng, cull=False) for b in range(nb)]
        flat = optim.FlatProblem(ch, md, views, bcam, np.arange(nb), np.stack(cams), None,
                                 np.stack([pose_from_matrix(near(T)) for T in poses]), None)
    elif chain == "ext":
        c_T_r = synth.ring_cameras(n_cams)
        r_T_t = synth.random_view_poses(n_grp, rng, **wide)
        bview = [b // n_cams for b in range(nb)]
        views = [synth.render_view(cams[bcam[b]], c_T_r[bcam[b]] @ r_T_t[bview[b]], picks[b], 0.3, rng, cull=False) for b in range(nb)]
        flat = optim.FlatProblem(ch, md, views, bcam, bview, np.stack(cams), np.stack([pose_from_matrix(near(T)) for T in c_T_r]),
                                 np.stack([pose_from_matrix(near(T)) for T in r_T_t]), None)
    else:
        g_T_c = [make_pose(np.array([0.03 + 0.05 * c, 0.01 * c, 0.12]), np.array([0.0, 1.0, 0.0]), np.deg2rad(8.0 - 3.0 * c)) for c in range(n_cams)]
        b_T_t = make_pose(np.array([0.5, -0.1, 0.8]), np.array([1.0, 0.0, 0.0]), np.deg2rad(14.0))
        b_T_g = [b_T_t @ inv(T) @ inv(g_T_c[0]) for T in synth.random_view_poses(n_grp, rng, **wide)]
        views, btg = [], []
        for b in range(nb):
            T = b_T_g[b // n_cams]
            views.append(synth.render_view(cams[bcam[b]], inv(g_T_c[bcam[b]]) @ inv(T) @ b_T_t, picks[b], 0.3, rng, cull=False))
            btg.append(np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]))
        flat = optim.FlatProblem(ch, md, views, bcam, None, np.stack(cams), np.stack([pose_from_matrix(near(T)) for T in g_T_c]), None,
                                 pose_from_matrix(near(b_T_t)), np.stack(btg))
    flat.intr[...] = flat.intr * (1 + 0.01 * np.random.default_rng(1).uniform(-1, 1, flat.intr.shape))  # as _perturb_intr
    assert [int(n) for n in np.diff(flat.blk_offset)] == sizes
    return flat


def only_block(flat, b):
    """Block b of `flat` as the only block of a problem: its camera, its poses, its observations."""
    lo, hi = int(flat.blk_offset[b]), int(flat.blk_offset[b + 1])
    view = np.stack([flat.X[lo:hi], flat.Y[lo:hi], flat.u[lo:hi], flat.v[lo:hi]], axis=1)
    c = int(flat.blk_cam[b])
    intr = flat.intr.reshape(flat.n_cams, -1)[[c]]
    if flat.chain == capi.CHAIN_INTRINSIC:
        return optim.FlatProblem(flat.chain, flat.model, [view], [0], [0], intr, None, flat.view_pose.reshape(-1, 7)[[int(flat.blk_view[b])]], None)
    cam = flat.cam_pose.reshape(-1, 7)[[c]]
    if flat.chain == capi.CHAIN_EXTRINSIC:
        return optim.FlatProblem(flat.chain, flat.model, [view], [0], [0], intr, cam, flat.view_pose.reshape(-1, 7)[[int(flat.blk_view[b])]], None)
    return optim.FlatProblem(flat.chain, flat.model, [view], [0], None, intr, cam, None, flat.target_pose, flat.blk_b_T_g.reshape(-1, 12)[[b]])


# ---- the reference and its own error -------------------------------------------------------------------------------------------
_INPUTS = ("X", "Y", "u", "v", "intr", "cam_pose", "view_pose", "target_pose", "blk_b_T_g")


def _changed_inputs(flat, change):
    f = helpers.clone(flat)
    for name in _INPUTS:
        a = getattr(f, name)
        if a is not None:
            a[...] = change(a)
    return f


_REFERENCE = {}


def _reference(orc, chain, model, prob):
    """(block rows, costs) of the oracle: computed once, shared by every test that needs it."""
    key = (chain, model, prob)
    if key not in _REFERENCE:
        flat = problem(chain, model, prob)
        _REFERENCE[key] = helpers.oracle_block_normal_eq(orc, flat), tuple(helpers.oracle_cost(orc, flat, d) for d in DELTAS)
    return _REFERENCE[key]


def _figures(flat, rows, costs, ref, ref_costs):
    """Every measure of one result against the reference: the scaled ones, block-max and the relative cost error."""
    out = helpers.scaled_normal_eq_diff(rows, ref, helpers.local_cols(flat))
    out["blockmax"] = float((np.abs(rows - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())
    out["cost"] = max(abs(c - c0) / max(1.0, abs(c0)) for c, c0 in zip(costs, ref_costs))
    return out


def measure_floors(orc):
    """CPU only: {(chain, model, scalar): floors} from the oracle alone (see the module docstring)."""
    floors = {}
    for chain in CHAINS:
        for model in MODELS:
            for scalar in ("fp64", "fp32"):
                worst = {}
                for k, prob in enumerate(PROBLEMS):
                    flat = problem(chain, model, prob)
                    ref, ref_costs = _reference(orc, chain, model, prob)
                    if scalar == "fp64":
                        rng = np.random.default_rng([52, CHAINS[chain], MODELS[model], k])
                        other = _changed_inputs(flat, lambda a: a * (1.0 + rng.choice([-1.0, 1.0], a.shape) * 2.0 ** -52))
                    else:
                        other = _changed_inputs(flat, lambda a: a.astype(np.float32).astype(np.float64))
                    rows = helpers.oracle_block_normal_eq(orc, other)
                    fig = _figures(flat, rows, [helpers.oracle_cost(orc, other, d) for d in DELTAS], ref, ref_costs)
                    assert fig.pop("zero") == 0.0 or scalar == "fp32"
                    for m, x in fig.items():
                        worst[m] = max(worst.get(m, 0.0), x)
                floors[(chain, model, scalar)] = worst if scalar == "fp32" else {m: worst[m] for m in ("H", "g", "s")}
    return floors


def bounds(chain, model, scalar):
    fl = FLOORS[(chain, model, scalar)]
    if scalar == "fp64":
        return dict(H=FP64_FACTOR * fl["H"], g=FP64_FACTOR * fl["g"], s=FP64_FACTOR * fl["s"], blockmax=1e-10, cost=1e-11)
    return {m: FP32_FACTOR * fl[m] for m in ("H", "g", "s", "blockmax", "cost")}


# ---- the tests -----------------------------------------------------------------------------------------------------------------
# (chain, model, scalar, CBA_MODEB_MOMENTS): the 12 forms, and the per-part direct launches of the two-pose chains in fp64
VARIANTS = [(c, m, s, None) for c in CHAINS for m in MODELS for s in ("fp64", "fp32")] + \
           [(c, m, "fp64", "0") for c in ("ext", "bundle") for m in MODELS]
_ids = lambda v: "-".join(x for x in v[:3]) + ("-moments0" if v[3] else "")


def _run(monkeypatch, flat, scalar, moments, with_cost=True):
    """-> (rows, rows of a second call, costs) of the HIP path.  The handle reads CBA_MODEB_MOMENTS when it is created."""
    if moments is None:
        monkeypatch.delenv("CBA_MODEB_MOMENTS", raising=False)
    else:
        monkeypatch.setenv("CBA_MODEB_MOMENTS", moments)
    with optim.ReprojHandle(flat) as h:
        if scalar == "fp32":
            h.set_scalar(1)
        a = h.block_normal_eq()
        b = h.block_normal_eq() if with_cost else None
        costs = [h.cost(d) for d in DELTAS] if with_cost else None
    return a, b, costs


def test_np_table_is_the_documented_default():
    doc, (two, other) = documented_np()
    assert doc == NP_TABLE
    assert two == 64 * NP_TABLE[("direct", "pinhole")] and all(other == 64 * n for k, n in NP_TABLE.items() if k != ("direct", "pinhole"))


def test_problems_select_the_three_launcher_paths():
    """The tile table the launcher decides by, restated: 2048-observation tiles (structure.hpp) for problems of this size."""
    for chain in CHAINS:
        for model in MODELS:
            n_p = NP_TABLE[(form_of(chain), model)]
            one, multi, split = (np.array(block_sizes(chain, model, p)[0]) for p in PROBLEMS)
            assert one.max() == 64 * n_p and {1, 2, 63, 64, 65, 64 * n_p - 1} <= set(one)
            assert multi.min() == 64 * min((n_p,) + NP_EXTRA.get((form_of(chain), model), ())) + 1
            assert multi.max() == 2048 and {64 * n_p + 1, 128 * n_p - 1, 128 * n_p, 128 * n_p + 1, 192 * n_p + 65, 2047} <= set(multi)
            assert {2049, 3000, 4096, 4097, 1, 65, 64 * n_p} <= set(split)
            for sizes in (one, multi, split):
                assert sizes.sum() // len(sizes) <= 2048  # the average block is at most one minimal tile: choose_mode_b_tile gives 2048
            dup = block_sizes(chain, model, "multi")[1]
            assert multi[dup[0]] == multi[dup[1]] and multi[dup[0]] % 2 == 1 and multi[dup[0] - 1] != multi[dup[0]]
            f = problem(chain, model, "multi")
            a, b = (slice(int(f.blk_offset[i]), int(f.blk_offset[i + 1])) for i in dup)
            assert np.array_equal(f.X[a], f.X[b]) and np.array_equal(f.Y[a], f.Y[b]) and not np.array_equal(f.u[a], f.u[b])
            if chain != "intr":
                assert len({tuple(sorted(np.diff(f.blk_offset)[f.blk_cam == c])) for c in range(2)}) == 2


@pytest.mark.parametrize("prob", PROBLEMS)
@pytest.mark.parametrize("variant", VARIANTS, ids=_ids)
def test_form_against_the_oracle(gpu_lib, oracle, monkeypatch, variant, prob):
    chain, model, scalar, moments = variant
    flat = problem(chain, model, prob)
    ref, ref_costs = _reference(oracle, chain, model, prob)
    rows, again, costs = _run(monkeypatch, flat, scalar, moments)
    fig = _figures(flat, rows, costs, ref, ref_costs)
    bnd = bounds(chain, model, scalar)
    print(f"\nFIGURES {_ids(variant)} {prob}: " + " ".join(f"{m}={fig[m]:.3e}/{bnd[m]:.3e}" for m in ("H", "g", "s", "blockmax", "cost"))
          + f" zero={fig['zero']:.3e}")
    assert rows.tobytes() == again.tobytes(), "a second block_normal_eq() call returned other bytes"
    assert np.isfinite(rows).all()
    assert fig["blockmax"] <= bnd["blockmax"]
    assert fig["cost"] <= bnd["cost"]
    assert fig["zero"] == 0.0, "an entry whose oracle scale is exactly 0 is not exactly 0"
    assert fig["H"] <= bnd["H"] and fig["g"] <= bnd["g"] and fig["s"] <= bnd["s"]


@pytest.mark.parametrize("prob", ["multi", "split"])
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v[2] == "fp64"], ids=_ids)
def test_block_rows_do_not_depend_on_the_other_blocks(gpu_lib, monkeypatch, variant, prob):
    """fp64: every block's row equals, bit for bit, the row of the problem that holds this block alone - no tile reads a neighbour's
    rows or the padding between blocks, whatever the tolerance."""
    chain, model, scalar, moments = variant
    flat = problem(chain, model, prob)
    rows, _, _ = _run(monkeypatch, flat, scalar, moments, with_cost=False)
    differ = []
    for b in range(flat.n_blocks):
        alone, _, _ = _run(monkeypatch, only_block(flat, b), scalar, moments, with_cost=False)
        if alone[0].tobytes() != rows[b].tobytes():
            differ.append((b, int(flat.blk_offset[b + 1] - flat.blk_offset[b]), float(np.abs(alone[0] - rows[b]).max() / np.abs(rows[b]).max())))
    assert not differ, f"(block, length, largest difference / largest entry): {differ}"


if __name__ == "__main__":
    import subprocess

    subprocess.run(["make", "-s", "-C", os.path.join(helpers.ROOT, "oracle")], check=True)
    print("FLOORS = {")
    for key, fl in measure_floors(helpers.load_oracle()).items():
        print(f"    {key!r}: dict(" + ", ".join(f"{m}={x:.2e}" for m, x in fl.items()) + "),")
    print("}")
