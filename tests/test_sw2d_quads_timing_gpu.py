"""The timing entry points of the quadrilateral solver that only profiles/ scripts call: Sw2dQuadSolver.timeHeun
(bdg_sw2dq_time, kind 2), timeSpeedPass (bdg_sw2dq_time_speed) and timeDrifters (bdg_sw2dq_drifters_time).

Each launches the kernels of a call the suite pins elsewhere (stepSSPRK2, the speed pass of computeRHS, advanceDrifters)
between two events, so each is compared with a twin solver, created with the same arguments, that makes that call: the kernel
sequences are the same and the comparison is bit for bit. The smallest cases the suite builds: order 2 in the variant-B set-up of
test_sw2d_quadsB_gpu.py (K = 143, parallelogram form), and the order-1 frozen rotation with 63 drifters of
test_sw2d_quads_drifters_gpu.py."""
import math

import numpy as np
import pytest

import quaddrift_ref as D
import test_sw2d_quadsB_gpu as vb3
from test_sw2d_quads_drifters_gpu import plain_solver

pytestmark = pytest.mark.gpu

ORDER, FORM = 2, "shear-auto"


def twins_b():
    """(timed solver, twin, state, dt): two variant-B solvers with the same resident state and model time."""
    q, dt = vb3.problem(vb3.FORMS[FORM][0], ORDER)[4:6]
    pair = [vb3.solver(ORDER, FORM) for _ in range(2)]
    for s in pair:
        s.setTime(vb3.T0)
        s.setState(*q)
    return pair[0], pair[1], q, dt


def assert_same_state(a, b):
    for name, x, y in zip(("h", "hu", "hv"), a, b):
        assert np.array_equal(x, y), f"{name} differs in {int((x != y).sum())} entries"


def test_time_heun_is_two_unfiltered_heun_steps():
    s, twin, _, dt = twins_b()
    ms = s.timeHeun(dt, 2)
    twin.stepSSPRK2(dt, 2, filter=False, sponge=0.0)
    print(f"timeHeun: {ms:.4f} ms per step")
    assert math.isfinite(ms) and ms > 0
    assert_same_state(s.getState(), twin.getState())
    assert s.getTime() == twin.getTime() and s.getTime() > vb3.T0
    s.close()
    twin.close()


def test_time_speed_pass_leaves_the_speed_of_the_resident_state():
    s, twin, q, _ = twins_b()
    ms = s.timeSpeedPass(3)
    twin.computeRHS(*twin.getState())
    print(f"timeSpeedPass: {ms:.4f} ms, speed {s.globalSpeed():.17g}")
    assert math.isfinite(ms) and ms > 0
    assert s.globalSpeed() == twin.globalSpeed() and s.globalSpeed() > 0
    assert_same_state(s.getState(), q)
    assert s.getTime() == vb3.T0
    s.close()
    twin.close()


def test_time_drifters_advances_without_a_record():
    name, order, n = D.ROTATION_CASES[0]
    nodes, _, _, _, q, pts, _, dt, _, _ = D.rotation_problem(name, order, n)
    pair = [plain_solver(nodes, q) for _ in range(2)]
    for s in pair:
        s.enableDrifters(nodes, pts, capacity=8)
    s, twin = pair
    before = s.drifterState()
    ms = s.timeDrifters(dt, 3)
    twin.advanceDrifters(dt, 3)
    print(f"timeDrifters: {ms:.4f} ms per advance of {n} drifters")
    assert math.isfinite(ms) and ms > 0
    got, ref = s.drifterState(), twin.drifterState()
    assert sorted(got) == sorted(ref)
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key
    assert not np.array_equal(got["xy"], before["xy"])                      # they moved
    assert [len(a) for a in s.drifterTracks()] == [0, 0, 0]                 # ... and no record was taken
    assert [len(a) for a in twin.drifterTracks()] == [3, 3, 3]
    s.close()
    twin.close()
