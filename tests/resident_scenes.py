"""The scenes of the resident LM kernel's edge suite (resident_lm.hip), shared by tests/test_resident_edges_cpu.py (the scenes are
what they claim, on the reference alone) and tests/test_resident_edges_gpu.py (the kernel against the host-driven iteration and
the oracle).

One workgroup of RES_THREADS = 512 threads (RES_WAVES = 8 wavefronts) runs the whole solve; the reduced system of nsh <= 80
(RES_NSH_MAX) columns lives in LDS and is factorised by wavefront 0, lane r owning rows r and r + 64.  Each scene puts one of
the kernel's path changes on the table:

  m (effective columns) <= 63, == 64, >= 65, == 0, nsh == 80, holes in the middle of sh.idx    phase_solve_reduced
  one camera (2 * total <= 512: the dealt sums) against rigs and bundles (the strided sums)     grouped_sums
  3, 7, 8, 9 tiles on 8 wavefronts                                                             the w += RES_WAVES tile loops
  blocks of more than 2048 observations (n_tiles != n_blocks)                                  the `partial` path
  513 blocks with 513 views, and with none                                                     the += RES_THREADS loops
  a ragged 5-camera rig with an idle camera                                                    view_cam_blk < 0 in phase_schur
  a rough start capped inside a run of rejections                                              re_eliminate, the last phase_consts
  accepted steps whose gain ratio is below 0.937 (the next radius depends on it)               the model change (reversed loop)

CPU_PAIR holds, per (scene, cap), the param_diff between the two REFERENCE forms - the host-side form of the iteration in the
test-only host build (hm_reproj_solve_mode, controller = 0, speculate = 0) and the oracle's dense solver - as
tests/test_resident_edges_cpu.py printed it.  Neither is code under test; a scene is usable only while that figure stays below
a third of its bar.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from calibration_amd import capi, optim
from calibration_amd.capi import CbaSummary
from tests import helpers, synth

TILE = 2048  # structure.hpp choose_mode_b_tile: the Mode B tile of problems this size
RES_THREADS, RES_WAVES, RES_NSH_MAX = 512, 8, 80

# the project's parity bars (SURVEY.md §8d / test_lm_solve_matches_oracle; check_endings(rough=True); check_endings, the flat valley)
BARS = {"pinhole": 1e-9, "rough": 1e-8, "scheimpflug": 1e-7}
NONE = None  # "no cap": max_iterations stays at the default 1000
PINHOLE_CAPS = (0, 1, 2, NONE)
CAPPED = (0, 1, 2)


def cut_blocks(flat, keep, counts=None):
    """The blocks `keep` of an intrinsic- or extrinsic-chain problem, block i cut to its first counts[i] points (every camera and
    view stays, observed or not): the cut of test_mode_a_odd_and_tiny_views and test_unobserved_camera_on_gpu."""
    f = flat
    views = []
    for i, b in enumerate(keep):
        lo, hi = int(f.blk_offset[b]), int(f.blk_offset[b + 1])
        if counts is not None:
            assert lo + counts[i] <= hi, (b, counts[i], hi - lo)
            hi = lo + counts[i]
        views.append(np.stack([f.X[lo:hi], f.Y[lo:hi], f.u[lo:hi], f.v[lo:hi]], axis=1))
    keep = np.asarray(keep, dtype=np.int64)
    return optim.FlatProblem(f.chain, f.model, views, f.blk_cam[keep], f.blk_view[keep], f.intr, f.cam_pose, f.view_pose, None,
                             first_view_global=f.first_view_global)


def _ext(n_views, n_cams, **kw):
    return lambda: synth.scene_extrinsics(n_views, n_cams, spacing=0.08, noise_px=0.2, **kw).flat


def _bundle(n_poses, n_cams, **kw):
    return lambda: synth.scene_bundle(n_poses, n_cams, spacing=0.04, noise_px=0.2, **kw).flat


def _intr(n_views, **kw):
    return lambda: synth.scene_intrinsics(n_views, spacing=0.08, noise_px=0.2, **kw).flat


def _ragged_rig():
    """7 views of a 5-camera rig: camera 2 sees nothing (16 idle columns in the middle of the 80), camera 3 misses views 0 and 2,
    camera 1 misses view 4."""
    f = synth.scene_extrinsics(7, 5, spacing=0.08, noise_px=0.2).flat
    keep = [b for b in range(f.n_blocks) if f.blk_cam[b] != 2 and not (f.blk_cam[b] == 3 and f.blk_view[b] in (0, 2))
            and not (f.blk_cam[b] == 1 and f.blk_view[b] == 4)]
    return cut_blocks(f, keep)


INTR_MULTI = (2049, 2048, 2047, 88, 64, 65, 1, 2209, 300)  # 2, 1, 1, 1, 1, 1, 1, 2, 1 tiles; one tile of a single observation
EXT_MULTI = (2049, 88, 2048, 64, 65, 2209, 300, 129)


def _intr_multitile():
    f = synth.scene_intrinsics(9, rows=47, cols=47, spacing=0.012, noise_px=0.2).flat
    return cut_blocks(f, list(range(9)), INTR_MULTI)


def _ext_multitile():
    f = synth.scene_extrinsics(4, 2, rows=47, cols=47, spacing=0.012, noise_px=0.2).flat
    return cut_blocks(f, list(range(8)), EXT_MULTI)


def _rough_rig():
    """helpers.rough_start_scene's start (focal lengths 20 % short, no distortion, 0.5 px noise) on the widest eligible rig"""
    sc = synth.scene_extrinsics(6, 5, noise_px=0.5, seed=23)
    sc.flat.intr[:, 5:10] = 0.0
    sc.flat.intr[:, 0:2] *= 0.8
    return sc.flat


def _rough_intr():
    return helpers.rough_start_scene("intr", 0, 19).flat


LINE_SEARCH_OFF = {"CBA_LM_LINE_SEARCH": "0", "ORC_LINE_SEARCH": "0"}


@dataclass
class ResidentScene:
    name: str
    make: Callable[[], optim.FlatProblem]
    okw: Dict[str, int]
    caps: Tuple[Optional[int], ...]
    cls: str  # "pinhole" | "scheimpflug" | "rough": the bar (BARS)
    # the structure the scene must have (asserted by the CPU tier)
    nsh: int
    m: int  # effective columns of the reduced system: active (hm_reproj_masks) and observed
    n_blocks: int
    n_views: int
    n_tiles: int
    blk_tiles: Optional[Tuple[int, ...]] = None  # tiles per block where they are not all 1
    epsilon: float = 1e-12
    env: Dict[str, str] = field(default_factory=dict)
    oracle_caps: Optional[Tuple[Optional[int], ...]] = None  # caps at which the dense oracle is affordable (default: all)
    rejections: Dict[int, int] = field(default_factory=dict)  # cap -> rejected steps of the host-side form
    min_accepted: int = 3  # uncapped: accepted steps at least

    def options(self, cap):
        kw = dict(self.okw)
        if cap is not NONE:
            kw["max_iterations"] = cap
        return helpers.options(epsilon=self.epsilon, **kw)

    def uses_oracle(self, cap) -> bool:
        return self.oracle_caps is None or cap in self.oracle_caps


_BI = dict(optimize_intrinsics=1)
SCENES = [
    # ---- the reduced solve: m around 64, nsh at RES_NSH_MAX ---------------------------------------------------------------
    ResidentScene("rig5", _ext(6, 5), {}, PINHOLE_CAPS, "pinhole", 80, 69, 30, 6, 30),
    ResidentScene("rig5-skew", _ext(6, 5), dict(optimize_skew=1), PINHOLE_CAPS, "pinhole", 80, 74, 30, 6, 30),
    ResidentScene("rig4", _ext(6, 4), {}, PINHOLE_CAPS, "pinhole", 64, 54, 24, 6, 24),
    ResidentScene("rig4-scheimpflug", _ext(6, 4, model=1), {}, CAPPED, "scheimpflug", 72, 62, 24, 6, 24),
    ResidentScene("rig4-scheimpflug-skew", _ext(6, 4, model=1), dict(optimize_skew=1), CAPPED, "scheimpflug", 72, 66, 24, 6, 24),
    ResidentScene("bundle4-m60", _bundle(16, 4), dict(_BI, optimize_target_pose=0), PINHOLE_CAPS, "pinhole", 70, 60, 64, 0, 64),
    ResidentScene("bundle4-m64", _bundle(16, 4), dict(_BI, optimize_skew=1, optimize_target_pose=0), PINHOLE_CAPS, "pinhole", 70, 64, 64, 0, 64),
    ResidentScene("bundle4-m66", _bundle(16, 4), dict(_BI), PINHOLE_CAPS, "pinhole", 70, 66, 64, 0, 64),
    ResidentScene("bundle4-m70", _bundle(16, 4), dict(_BI, optimize_skew=1), PINHOLE_CAPS, "pinhole", 70, 70, 64, 0, 64),
    ResidentScene("bundle4-scheimpflug", _bundle(16, 4, model=1), dict(_BI), CAPPED, "scheimpflug", 78, 74, 64, 0, 64),
    ResidentScene("rig3-views-only", _ext(6, 3), dict(optimize_intrinsics=0, optimize_extrinsics=0), PINHOLE_CAPS, "pinhole", 48, 0, 18, 6, 18),
    ResidentScene("rig5-ragged", _ragged_rig, {}, PINHOLE_CAPS, "pinhole", 80, 54, 25, 7, 25),
    # ---- one camera: the dealt sums; tiles below, at and above the 8 wavefronts ------------------------------------------------
    ResidentScene("intr3", _intr(3), {}, PINHOLE_CAPS, "pinhole", 10, 9, 3, 3, 3),
    ResidentScene("intr7", _intr(7), {}, PINHOLE_CAPS, "pinhole", 10, 9, 7, 7, 7),
    ResidentScene("intr8", _intr(8), {}, PINHOLE_CAPS, "pinhole", 10, 9, 8, 8, 8),
    ResidentScene("intr9", _intr(9), {}, PINHOLE_CAPS, "pinhole", 10, 9, 9, 9, 9),
    # ---- blocks of several tiles: rows through `partial` ---------------------------------------------------------------------
    # (caps 9 and 12: the gain ratio of iterations 5, 7 and 8 is below 0.937, where the next radius depends on it - see intr-rough;
    #  at caps 5 to 8 the reference pair is itself 1.6e-10 to 5.4e-10 apart: not usable)
    ResidentScene("intr-multitile", _intr_multitile, {}, (0, 1, 2, 9, 12, NONE), "pinhole", 10, 9, 9, 9, 11, blk_tiles=(2, 1, 1, 1, 1, 1, 1, 2, 1)),
    ResidentScene("ext-multitile", _ext_multitile, {}, PINHOLE_CAPS, "pinhole", 32, 24, 8, 4, 10, blk_tiles=(2, 1, 1, 1, 1, 2, 1, 1)),
    # ---- past 512 blocks: with as many views, and with none ------------------------------------------------------------------
    # (the dense oracle needs 4 s for one iteration at 513 views and minutes for the whole solve: beyond cap 1 the references are
    #  the host-side form on the CPU and the host-driven form on the GPU)
    ResidentScene("intr513", _intr(513, rows=4, cols=5), {}, PINHOLE_CAPS, "pinhole", 10, 9, 513, 513, 513, oracle_caps=(0, 1)),
    ResidentScene("bundle513", _bundle(513, 1, rows=4, cols=5), dict(_BI), PINHOLE_CAPS, "pinhole", 22, 21, 513, 0, 513),
    # ---- a solve that ends inside a run of rejections, at full width ---------------------------------------------------------
    ResidentScene("rig5-rough", _rough_rig, {}, (13, 17), "rough", 80, 69, 30, 6, 30, epsilon=1e-10, env=LINE_SEARCH_OFF,
                  rejections={13: 1, 17: 3}),
    # The radius after an accepted step is radius / max(1/3, 1 - (2 rho - 1)^3), rho = cost change / model change: it simply triples
    # while rho > 0.937, which is every early step of the scenes above - there an error in the model change (the thread-reversed
    # loop over the shared columns) changes nothing.  helpers.rough_start_scene("intr", 0, 19) has rho = 0.913 at iteration 4,
    # 0.908 at 5: caps 5, 6 and 8 (from cap 9 on the reference pair is itself 7e-9 apart: not usable).
    ResidentScene("intr-rough", _rough_intr, {}, (5, 6, 8), "rough", 10, 9, 6, 6, 6, epsilon=1e-10, env=LINE_SEARCH_OFF,
                  rejections={5: 0, 6: 0, 8: 0}),
]
BY_NAME = {s.name: s for s in SCENES}
CASES = [(s.name, cap) for s in SCENES for cap in s.caps]


def case_id(val):
    return "nocap" if val is NONE else str(val)


# shapes the resident kernel must decline (resident_lm_eligible): three widths past RES_NSH_MAX, and an fp32 handle
INELIGIBLE = {
    "rig6-nsh96": (_ext(6, 6), {}, 96, 0),
    "bundle5-nsh86": (_bundle(16, 5), dict(_BI), 86, 0),
    "rig5-scheimpflug-nsh90": (_ext(6, 5, model=1), {}, 90, 0),
    "rig5-fp32": (_ext(6, 5), {}, 80, 1),
}

# param_diff of the reference pair (host-side form on the CPU vs the oracle), as tests/test_resident_edges_cpu.py printed it
CPU_PAIR = {
    ("rig5", 0): 0.0e+00, ("rig5", 1): 3.3e-11, ("rig5", 2): 2.9e-12, ("rig5", NONE): 8.1e-13,
    ("rig5-skew", 0): 0.0e+00, ("rig5-skew", 1): 2.7e-11, ("rig5-skew", 2): 2.5e-12, ("rig5-skew", NONE): 1.1e-12,
    ("rig4", 0): 0.0e+00, ("rig4", 1): 3.2e-11, ("rig4", 2): 1.2e-11, ("rig4", NONE): 3.5e-13,
    ("rig4-scheimpflug", 0): 0.0e+00, ("rig4-scheimpflug", 1): 2.4e-11, ("rig4-scheimpflug", 2): 1.9e-11, ("rig4-scheimpflug-skew", 0): 0.0e+00,
    ("rig4-scheimpflug-skew", 1): 2.3e-11, ("rig4-scheimpflug-skew", 2): 3.2e-11, ("bundle4-m60", 0): 0.0e+00, ("bundle4-m60", 1): 1.9e-11,
    ("bundle4-m60", 2): 7.2e-12, ("bundle4-m60", NONE): 8.0e-13, ("bundle4-m64", 0): 0.0e+00, ("bundle4-m64", 1): 2.2e-11,
    ("bundle4-m64", 2): 4.9e-12, ("bundle4-m64", NONE): 4.7e-13, ("bundle4-m66", 0): 0.0e+00, ("bundle4-m66", 1): 2.0e-11,
    ("bundle4-m66", 2): 4.6e-12, ("bundle4-m66", NONE): 7.7e-13, ("bundle4-m70", 0): 0.0e+00, ("bundle4-m70", 1): 2.0e-11,
    ("bundle4-m70", 2): 1.1e-11, ("bundle4-m70", NONE): 8.2e-13, ("bundle4-scheimpflug", 0): 0.0e+00, ("bundle4-scheimpflug", 1): 2.5e-11,
    ("bundle4-scheimpflug", 2): 8.7e-12, ("rig3-views-only", 0): 0.0e+00, ("rig3-views-only", 1): 1.2e-16, ("rig3-views-only", 2): 2.2e-16,
    ("rig3-views-only", NONE): 2.2e-16, ("rig5-ragged", 0): 0.0e+00, ("rig5-ragged", 1): 3.5e-11, ("rig5-ragged", 2): 1.6e-11,
    ("rig5-ragged", NONE): 6.4e-13, ("intr3", 0): 0.0e+00, ("intr3", 1): 2.3e-11, ("intr3", 2): 1.1e-11,
    ("intr3", NONE): 1.4e-12, ("intr7", 0): 0.0e+00, ("intr7", 1): 3.7e-12, ("intr7", 2): 4.0e-12,
    ("intr7", NONE): 4.5e-13, ("intr8", 0): 0.0e+00, ("intr8", 1): 5.9e-12, ("intr8", 2): 3.3e-12,
    ("intr8", NONE): 4.6e-13, ("intr9", 0): 0.0e+00, ("intr9", 1): 4.3e-11, ("intr9", 2): 1.9e-12,
    ("intr9", NONE): 2.2e-13, ("intr-multitile", 0): 0.0e+00, ("intr-multitile", 1): 2.2e-11, ("intr-multitile", 2): 2.8e-11,
    ("intr-multitile", NONE): 3.6e-12, ("ext-multitile", 0): 0.0e+00, ("ext-multitile", 1): 1.8e-10, ("ext-multitile", 2): 4.3e-11,
    ("ext-multitile", NONE): 6.9e-13, ("intr513", 0): 0.0e+00, ("intr513", 1): 1.1e-10, ("bundle513", 0): 0.0e+00,
    ("bundle513", 1): 7.0e-11, ("bundle513", 2): 1.4e-12, ("bundle513", NONE): 4.3e-14, ("rig5-rough", 13): 2.9e-09,
    ("rig5-rough", 17): 1.6e-09,
    ("intr-multitile", 9): 9.4e-11, ("intr-multitile", 12): 3.6e-12, ("intr-rough", 5): 5.5e-11, ("intr-rough", 6): 1.8e-10,
    ("intr-rough", 8): 7.3e-10,
}


# ---- structure of a problem, from the problem alone -----------------------------------------------------------------------------
def shared_width(flat) -> int:
    """nsh (structure.hpp): intrinsic chain = the camera; extrinsic = per camera pose + intrinsics; bundle = target pose + the same"""
    PI = flat.intr.shape[-1]
    if flat.chain == capi.CHAIN_INTRINSIC:
        return PI
    return (6 if flat.chain == capi.CHAIN_BUNDLE else 0) + flat.n_cams * (6 + PI)


def effective_columns(hostmath, flat, opts) -> np.ndarray:
    """The columns of the reduced system the solve works on: the ones the options leave variable (the product's own masks through
    the host build, as helpers.solution_gap_report reads them) that some block observes - an idle camera's columns have a zero
    diagonal and behave like constants (phase_assemble's sh.eff)."""
    nsh = shared_width(flat)
    active, cam_var, flags = np.zeros(nsh, np.int8), np.zeros(flat.n_cams, np.int8), np.zeros(3, np.int32)
    d = flat.struct()
    assert hostmath.hm_reproj_masks(C.byref(d), C.byref(opts), active.ctypes.data_as(C.POINTER(C.c_int8)),
                                    cam_var.ctypes.data_as(C.POINTER(C.c_int8)), flags.ctypes.data_as(C.POINTER(C.c_int32))) == 0, hostmath.hm_last_error()
    eff = active.astype(bool)
    if flat.chain != capi.CHAIN_INTRINSIC:
        PC = 6 + flat.intr.shape[-1]
        base = 6 if flat.chain == capi.CHAIN_BUNDLE else 0
        seen = np.bincount(flat.blk_cam, minlength=flat.n_cams) > 0
        for c in range(flat.n_cams):
            if not seen[c]:
                eff[base + c * PC:base + (c + 1) * PC] = False
    return eff


def tiles_per_block(flat) -> np.ndarray:
    return (np.diff(flat.blk_offset) + TILE - 1) // TILE


# ---- the references, computed once per (scene, cap) and shared -----------------------------------------------------------------
class scene_env:
    """the scene's environment switches (line search off on both sides) for the duration of a solve"""

    def __init__(self, scene):
        self.env, self.old = scene.env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_ORACLE, _HOSTSIDE = {}, {}


def oracle_reference(oracle, name, cap):
    """-> (summary, flat at the oracle's end point); callers must not change either"""
    key = (name, cap)
    if key not in _ORACLE:
        sc = BY_NAME[name]
        assert sc.uses_oracle(cap), key
        flat = sc.make()
        with scene_env(sc):
            s = helpers.oracle_solve(oracle, flat, sc.options(cap))
        _ORACLE[key] = (s, flat)
    return _ORACLE[key]


def hostside_reference(hostmath, name, cap):
    """The host-side form of the iteration in the host build (no controller, no speculation)
    -> (summary, flat at its end point, exchange counters); callers must not change any of them"""
    key = (name, cap)
    if key not in _HOSTSIDE:
        sc = BY_NAME[name]
        flat = sc.make()
        d = flat.struct()
        s = CbaSummary()
        xs = (C.c_int64 * 8)()
        o = sc.options(cap)
        with scene_env(sc):
            st = hostmath.hm_reproj_solve_mode(C.byref(d), C.byref(o), capi.ALLREDUCE_FN(), None, 1, 0, 0, 0, C.byref(s), xs)
        assert st == 0, hostmath.hm_last_error()
        _HOSTSIDE[key] = (s, flat, [int(v) for v in xs])
    return _HOSTSIDE[key]


def counts(s):
    return (int(s.termination), int(s.iterations), int(s.successful_steps))
