"""RunRecords.harmonicFit (blitzdg_amd/_records.py: harmonic_fit) on synthetic accumulators; no device.

500 series a0 + sum_j A_j cos(omega_j t - phi_j), A in [0.1, 3], sampled over [0, 2 T] at irregular steps of 210 .. 300 s,
T = 44 712 s (M2), accumulated by tests/fieldstats_ref.synthetic the way the device accumulates them. With the periods (T, T / 2)
the normal matrix has cond ~ 3, and the fit was measured at 6e-15 relative in the amplitude, 1e-14 in the phase and 3e-15 in
the mean; the bound of 1e-11 is about a thousand times that: room for another sample draw at cond ~ 3, and far below what a
wrong sign or convention gives."""
import numpy as np
import pytest

import fieldstats_ref as ref
from blitzdg_amd._records import harmonic_fit

T = 44712.0
BOUND = 1e-11


def test_fit_recovers_mean_amplitude_and_phase():
    stats, a0, A, phi = ref.synthetic((T, T / 2), 2 * T, seed=1)
    assert a0.size == 500 and A.min() >= 0.1 and A.max() <= 3.0
    assert np.all(np.diff(stats["t"]) >= 210.0 - 1e-9) and np.all(np.diff(stats["t"]) <= 300.0 + 1e-9)
    fit = harmonic_fit(stats)
    assert fit["mean"].shape == a0.shape and fit["amplitude"].shape == A.shape and fit["phase"].shape == phi.shape
    amp = (np.abs(fit["amplitude"] - A) / A).max()
    dphi = np.abs(np.angle(np.exp(1j * (fit["phase"] - phi)))).max()      # the difference taken on the circle
    mean = np.abs(fit["mean"] - a0).max()
    print(f"cond {fit['cond']:.3g}  amplitude {amp:.3g}  phase {dphi:.3g}  mean {mean:.3g}")
    assert 1.0 <= fit["cond"] < 10.0
    assert amp < BOUND
    assert dphi < BOUND
    assert mean < BOUND


def test_close_periods_return_their_condition_number():
    stats, _, _, _ = ref.synthetic((T, 43200.0), 2 * T, seed=2)
    fit = harmonic_fit(stats)
    print(f"cond {fit['cond']:.4g}")
    assert np.isfinite(fit["cond"]) and fit["cond"] > 100.0
    assert np.all(np.isfinite(fit["amplitude"])) and np.all(np.isfinite(fit["mean"]))


def test_two_identical_periods_are_refused():
    stats, _, _, _ = ref.synthetic((T, T), 2 * T, seed=3)
    with pytest.raises(ValueError):
        harmonic_fit(stats)


def test_no_periods_are_refused():
    stats, _, _, _ = ref.synthetic((), 2 * T, seed=4)
    assert "cos" not in stats
    with pytest.raises(ValueError, match="at least one period"):
        harmonic_fit(stats)
    with pytest.raises(ValueError, match="mean group"):
        full, _, _, _ = ref.synthetic((T,), 2 * T, seed=4)
        del full["sum"]
        harmonic_fit(full)
