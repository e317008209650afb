"""CPU tier: the floors that bound tests/test_mode_b_forms_gpu.py are what the oracle gives today.

The floors are differences between two oracle runs at the rounding level; BLAS builds sum J^T J in different orders, so a re-measured
floor may differ from the committed one by a small factor, never by an order of magnitude."""
import numpy as np

from tests import test_mode_b_forms_gpu as forms


def test_committed_floors_are_reproduced_by_the_generator(oracle):
    measured = forms.measure_floors(oracle)
    assert set(measured) == set(forms.FLOORS)
    for key, fl in measured.items():
        cap = forms.FP64_FLOOR_CAP if key[2] == "fp64" else forms.FP32_FLOOR_CAP
        assert set(fl) == set(forms.FLOORS[key]), key
        for m, x in fl.items():
            c = forms.FLOORS[key][m]
            assert 0.0 < c <= cap, (key, m, c)  # above the cap the scene is too ill-conditioned to test anything
            assert c / 2.0 <= x <= 2.0 * c, (key, m, x, c)


def test_scaled_measure_sees_what_block_max_hides():
    """A small entry (H_kk of a weak column) wrong by half: invisible to the block-max measure, 0.5 in the scaled one."""
    from tests import helpers

    p = 3
    J = np.array([[1e3, 1.0, 1e-6], [2e3, -1.0, 2e-6], [5e2, 0.5, -1e-6], [1e3, 2.0, 3e-6]])
    r = np.array([1.0, -2.0, 0.5, 1.5])
    H = J.T @ J
    ref = np.concatenate([H[np.triu_indices(p)], J.T @ r, [r @ r]])[None, :]
    bad = ref.copy()
    bad[0, 5] *= 0.5  # H_22
    fig = helpers.scaled_normal_eq_diff(bad, ref, p)
    assert abs(fig["H"] - 0.5) < 1e-12 and fig["g"] == 0.0 and fig["s"] == 0.0 and fig["zero"] == 0.0
    assert np.abs(bad - ref).max() / np.abs(ref).max() < 1e-17
    zero = ref.copy()
    zero[0, [2, 4, 5, 8]] = 0.0  # a column the block does not see at all
    off = zero.copy()
    off[0, 4] = 1e-30
    assert helpers.scaled_normal_eq_diff(off, zero, p)["zero"] == 1e-30
