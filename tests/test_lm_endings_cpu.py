"""CPU tier: LM solves that END by the iteration cap or by the gradient tolerance, compared over every parameter block.

The controller form of the iteration (lm_ctl.hpp, the default LM path: LMDriver::solve_ctl) against the host-side form
(LMDriver::solve_host) and the oracle's dense solver, all three on the same scene.  test_controller_takes_the_decisions_of_the_host_side_form
covers solves that end by the function or parameter tolerance; there the controller ends the solve before any accept.  The endings
here come from the loop-top tests, which run right AFTER an accepted step: an accepted speculative step whose private poses were never
made current, or a loop-top test that does not fire, is visible only in the view poses, the termination reason and the cost at
the returned point.  So every solve is checked on all four of them.

Endings covered: the iteration cap (noisy scenes, max_iterations 0 .. 5), the gradient tolerance straight after an accepted step
(pixel-scaled scenes: synth.scale_pixels), and a rough start capped in the middle of a run of rejected steps.  Two endings are not
covered because no scene reaches them: the minimum trust-region radius (1e-32: from the initial 1e4 that takes more than 50
consecutive rejections with a growing decrease factor) and a line search that fails (the rough starts of helpers.rough_start_scene
search successfully).  Neither is faked here.
"""
import ctypes as C

import pytest

from calibration_amd import capi
from calibration_amd.capi import CbaSummary
from tests import helpers, synth
from tests.helpers import options

CHAINS = {
    "intr": lambda m: synth.scene_intrinsics(10, model=m, spacing=0.08, noise_px=0.2),
    "ext": lambda m: synth.scene_extrinsics(6, 3, model=m, spacing=0.08, noise_px=0.2),
    "bundle": lambda m: synth.scene_bundle(12, 2, model=m, spacing=0.04, noise_px=0.2),
}
# the pixel scale at which each scene ends by the gradient tolerance with epsilon 1e-9 (the narrow Scheimpflug intrinsics scene needs a
# smaller one); the Scheimpflug bundle is the well-conditioned one: on the narrow one the host-side form and the oracle end 1e-7 apart in
# its flat valley (test_host_logic.py test_scheimpflug_parity_gap_lies_in_the_flat_valley), which is not what this test is about
GRAD_SCENES = {("intr", 0): (CHAINS["intr"], 1e-5), ("ext", 0): (CHAINS["ext"], 1e-5), ("bundle", 0): (CHAINS["bundle"], 1e-5),
               ("intr", 1): (CHAINS["intr"], 1e-7), ("ext", 1): (CHAINS["ext"], 1e-5),
               ("bundle", 1): (lambda m: synth.scene_bundle_wide(12, model=m), 1e-5)}
MSG = {capi.TERM_NO_CONVERGENCE: b"Maximum number of iterations reached.", capi.TERM_CONVERGENCE: b"Gradient tolerance reached."}


def hm_solve_mode(hostmath, flat, o, controller, speculate):
    d = flat.struct()
    s = CbaSummary()
    xs = (C.c_int64 * 8)()
    st = hostmath.hm_reproj_solve_mode(C.byref(d), C.byref(o), capi.ALLREDUCE_FN(), None, 1, 0, speculate, controller, C.byref(s), xs)
    assert st == 0, hostmath.hm_last_error()
    return s, [int(v) for v in xs]


def three_forms(oracle, hostmath, mk, o, speculate):
    """controller form, host-side form, oracle: each on its own copy of the scene -> [(summary, flat)]"""
    c, h, r = mk(), mk(), mk()
    sc, _ = hm_solve_mode(hostmath, c.flat, o, 1, speculate)
    sh, xh = hm_solve_mode(hostmath, h.flat, o, 0, speculate)
    so = helpers.oracle_solve(oracle, r.flat, o)
    return [(sc, c.flat), (sh, h.flat), (so, r.flat)], xh


def check_endings(oracle, runs, term, msg, model, o, rough=False):
    """Every form ends as the case says, with the same decisions; all blocks agree; final_cost is the cost AT the returned point.
    The parameter bars are test_controller_takes_the_decisions_of_the_host_side_form's: a rough start stopped half-way carries the
    rounding of the path behind it (1e-8)."""
    bar = 1e-7 if model == 1 else 1e-8 if rough else 1e-9
    (sc, fc), (sh, fh), (so, fo) = runs
    for s, _f in runs:
        assert s.termination == term and msg in bytes(s.report), [bytes(r[0].report) for r in runs]
    assert (sc.iterations, sc.successful_steps) == (sh.iterations, sh.successful_steps) == (so.iterations, so.successful_steps), \
        [bytes(r[0].report) for r in runs]
    assert helpers.param_diff(fc, fh) <= bar, ("controller vs host-side form", helpers.param_diff(fc, fh))
    assert helpers.param_diff(fc, fo) <= bar, ("controller vs oracle", helpers.param_diff(fc, fo))
    assert helpers.param_diff(fh, fo) <= bar, ("host-side form vs oracle", helpers.param_diff(fh, fo))
    for s, f in runs:
        c = helpers.oracle_cost(oracle, f, o.huber_delta)
        assert abs(s.final_cost - c) <= 1e-12 * c, (bytes(s.report), s.final_cost, c)


def _okw(kind):
    return dict(optimize_intrinsics=1) if kind == "bundle" else {}


@pytest.mark.parametrize("speculate", [1, 0])
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("kind", ["intr", "ext", "bundle"])
@pytest.mark.parametrize("cap", [0, 1, 2, 3, 5])
def test_iteration_cap_ends_at_the_same_point_in_every_form(oracle, hostmath, cap, kind, model, speculate):
    """max_iterations reached, usually right after an accepted (speculative) step: the view poses returned are the accepted
    step's, as are the shared blocks and the cost."""
    o = options(epsilon=1e-12, max_iterations=cap, **_okw(kind))
    runs, _ = three_forms(oracle, hostmath, lambda: CHAINS[kind](model), o, speculate)
    check_endings(oracle, runs, capi.TERM_NO_CONVERGENCE, MSG[capi.TERM_NO_CONVERGENCE], model, o)
    assert runs[0][0].iterations == cap
    if cap == 0:
        assert runs[0][0].final_cost == runs[0][0].initial_cost


@pytest.mark.parametrize("speculate", [1, 0])
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("kind", ["intr", "ext", "bundle"])
def test_gradient_tolerance_after_an_accepted_step(oracle, hostmath, kind, model, speculate):
    """The pixel-scaled scene ends by the gradient tolerance: the loop-top test after the step that brought |g| below epsilon.
    (CBA_TERM_CONVERGENCE is 0: a loop-top test that returns the termination code as its "stop" flag never stops there.)"""
    mk, s = GRAD_SCENES[(kind, model)]
    o = options(epsilon=1e-9, **_okw(kind))
    runs, _ = three_forms(oracle, hostmath, lambda: synth.scale_pixels(mk(model), s), o, speculate)
    check_endings(oracle, runs, capi.TERM_CONVERGENCE, MSG[capi.TERM_CONVERGENCE], model, o)
    assert runs[0][0].iterations >= 1 and runs[0][0].successful_steps >= 1


@pytest.mark.parametrize("speculate", [1, 0])
@pytest.mark.parametrize("kind,seed,cap", [("intr", 19, 11), ("ext", 23, 17)])
def test_rough_start_capped_in_the_middle_of_its_rejections(oracle, hostmath, monkeypatch, kind, seed, cap, speculate):
    """A rough start with the line search off on both sides (its Armijo failures become plain rejections), capped while it rejects
    steps: the previous iteration and the last one are both rejected, so the returned point is the last ACCEPTED one, several
    exchanges back."""
    monkeypatch.setenv("CBA_LM_LINE_SEARCH", "0")
    monkeypatch.setenv("ORC_LINE_SEARCH", "0")
    o = options(epsilon=1e-10, max_iterations=cap)
    runs, xh = three_forms(oracle, hostmath, lambda: helpers.rough_start_scene(kind, 0, seed), o, speculate)
    check_endings(oracle, runs, capi.TERM_NO_CONVERGENCE, MSG[capi.TERM_NO_CONVERGENCE], 0, o, rough=True)
    sc = runs[0][0]
    assert xh[5] >= 2 and xh[6] == 0  # rejections, no line search
    # the cap falls inside a run of rejections: one iteration fewer accepts as many steps
    o1 = options(epsilon=1e-10, max_iterations=cap - 1)
    s1, _ = hm_solve_mode(hostmath, helpers.rough_start_scene(kind, 0, seed).flat, o1, 1, speculate)
    assert sc.successful_steps == s1.successful_steps < cap - 1
