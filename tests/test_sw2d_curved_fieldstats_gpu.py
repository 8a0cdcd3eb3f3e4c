"""Field statistics of the curved solver on the GPU: bdg_sw2d_curved_enable_field_stats and its field_stats_* group, the wiring
of FieldStatsState (csrc/hip/run_records.hpp) and sw2d_stats_kernel.hpp into the curved steppers.

The accumulators are compared bit for bit (NaNs by position) with the NumPy restatement tests/fieldstats_ref.py, fed with the
states the solver gives back after each sampled step and with the library's own sample log, as tests/test_sw2d_fieldstats_gpu.py
has it. The log is held to math.cos / math.sin of 2 pi t / T within 2^-52.

Shape: the shuffled K = 84 mesh at N = 4 (curved elements scattered; K is no multiple of 64), two periods, stride 2."""
import ctypes
import math

import numpy as np
import pytest

import curved_cases as cc
import fieldstats_ref as ref
from blitzdg_amd import _capi as C

pytestmark = pytest.mark.gpu

PERIODS = (0.9, 0.35)


def depth(c):
    return 0.8 + 0.1 * c.x - 0.05 * c.y * c.y


def assert_stats(got, want, what):
    keys = ("sum", "etaMax", "hMin", "speedMax", "cos", "sin")
    assert [k for k in keys if k in got] == [k for k in keys if k in want], f"{what}: keys {sorted(got)}"
    for k in keys:
        if k in want:
            assert ref.same(got[k], want[k]), f"{what}: {k} differs from the restatement"


@pytest.mark.parametrize("given", ["own-H", "driver-H"])
def test_accumulators_over_rk2_lserk4_and_adaptive_steps(given):
    c = cc.case("inst-N4")
    dt, H = cc.step_size(c), depth(c)
    s = cc.solver(c)
    s.enableDriver(c.ctx, H=H)
    s.setState(*c.q)
    s.time = 0.25
    s.enableFieldStats(H=H if given == "own-H" else None, periods=PERIODS, stride=2)
    states, times = [], []

    def step(call):
        call()
        states.append(s.getState())
        times.append(s.time)

    for _ in range(4):
        step(lambda: s.stepRK2(dt, 1, filter=True))
    for n in (3, 2, 5, 5):                                                  # three steps in uneven chunks of stages
        s.lserk4Stages(dt, n)
        if s.time != times[-1]:                                             # the chunk completed a step
            states.append(s.getState())
            times.append(s.time)
    tt, dd = s.time, None
    for _ in range(3):
        tt, dd, n = s.runAdaptive(0.5, 1e9, t=tt, dt=dd, maxSteps=1)
        assert n == 1
        states.append(s.getState())
        times.append(s.time)
    assert len(states) == 10
    got = s.fieldStats()
    sampled = slice(1, None, 2)                                             # every second completed step
    assert got["n"] == 5 and np.array_equal(got["t"], np.array(times)[sampled])
    for t, row in zip(got["t"], got["trig"]):
        for j, T in enumerate(PERIODS):
            assert abs(row[2 * j] - math.cos(2 * math.pi / T * t)) <= 2.0 ** -52
            assert abs(row[2 * j + 1] - math.sin(2 * math.pi / T * t)) <= 2.0 ** -52
    assert_stats(got, ref.accumulate(states[sampled], H, got["trig"]), given)
    assert np.abs(got["sum"][1]).max() > 0 and (got["etaMax"] > -np.inf).all()
    fit = s.harmonicFit(got)
    assert fit["mean"].shape == (3, s.Np, s.K) and fit["amplitude"].shape == (2, 3, s.Np, s.K) and np.isfinite(fit["cond"])
    # one sample by hand, the timing call (which leaves the accumulators alone) and the reset
    s.sampleFieldStats()
    again = s.fieldStats()
    assert again["n"] == 6 and s.timeFieldStats(2) > 0
    assert_stats(s.fieldStats(), {k: v for k, v in again.items() if k not in ("n", "t", "trig")}, "after timeFieldStats")
    s.resetFieldStats()
    empty = s.fieldStats()
    assert empty["n"] == 0 and not empty["sum"].any() and (empty["hMin"] == np.inf).all()
    s.close()


def test_refusals_and_an_undisturbed_run():
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    c = cc.case("small-N4")
    dt = cc.step_size(c)
    finals = []
    for on in (True, False):
        s = cc.solver(c)
        n, m = ctypes.c_int(), ctypes.c_int()
        if on:
            assert lib.bdg_sw2d_curved_field_stats_sample(s._h) == E and b"not enabled" in lib.bdg_last_error()
            assert lib.bdg_sw2d_curved_field_stats_count(s._h, ctypes.byref(n), ctypes.byref(m)) == E
            before = s.deviceBytes
            with pytest.raises(C.BdgError, match="stride"):
                s.enableFieldStats(periods=(1.0,), stride=0)
            with pytest.raises(C.BdgError, match="nothing to accumulate"):
                s.enableFieldStats(mean=False, envelope=False)
            assert s.deviceBytes == before
            s.enableFieldStats(periods=(1.0,))                                # no H anywhere: eta = h
            with pytest.raises(C.BdgError, match="already enabled"):
                s.enableFieldStats(periods=(1.0,))
        s.setState(*c.q)
        s.stepRK2(dt, 3, filter=True)
        s.lserk4Stages(dt, 5)
        finals.append(s.getState())
        if on:
            got = s.fieldStats()
            assert got["n"] == 4
            assert ref.same(got["hMin"], np.minimum.reduce([got["hMin"], finals[0][0]]))
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*finals))
