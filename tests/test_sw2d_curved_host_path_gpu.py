"""The host path of the curved / over-integrated sw2d solver (sw2d_curved_device.hip): the calls whose results no other module pins.

Everything here but the last test compares the solver with itself, bit for bit: n steps in one call with n calls of one step, a
step with its two phases, a timed run with the plain run, stages in two calls with stages in one. The arithmetic of the kernels
is held to the oracle elsewhere (test_sw2d_curved_gpu.py, test_sw2d_curved_instances_gpu.py); these tests hold what the host
code around the launches carries from call to call -- the stage counter, the residual, the roles of the two state buffers, which
the nodal-trace form swaps at every stage -- and the text of its refusals.

The mesh is a 3 x 3 box: K = 18 triangles, one full 16-element tile and a ragged one. The two triangles of the middle cell are
deformed and listed, so the fix-up kernel and the side buffer run; the others are straight-sided and held compressed. Both
kernel forms.
"""
import types
from ctypes import POINTER, c_double

import numpy as np
import pytest

import curved_cases
from blitzdg_amd import _capi as C
from blitzdg_amd.sw2d_curved import Sw2dCurvedSolver

pytestmark = pytest.mark.gpu

ORDERS = (3, 6)
NO_FILTER = "filter requested but the solver was created without a Filter matrix"

_CASES = {}


@pytest.fixture(params=["nodal-trace", "general"], autouse=True)
def form(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("BDG_SW2D_CURVED_GENERAL", "1")
    else:
        monkeypatch.delenv("BDG_SW2D_CURVED_GENERAL", raising=False)
    return request.param


def _case(order):
    if order not in _CASES:
        c = curved_cases.problem(order, 3, 3, deformation=curved_cases.bump, odd_curved=False)
        assert c.K == 18 and len(c.curvedEls) == 2 and np.array_equal(c.curvedEls, c.deformed)
        _CASES[order] = (c, curved_cases.step_size(c))
    return _CASES[order]


def _make(order, form, with_filter=True):
    """A solver of the case with its state set, the state, and a stable dt."""
    c, dt = _case(order)
    ctx = c.ctx if with_filter else types.SimpleNamespace(numLocalPoints=c.ctx.numLocalPoints, numElements=c.K, V=c.ctx.V, filter=None)
    s = Sw2dCurvedSolver(ctx, c.cub, c.gauss, c.curvedEls, c.J, c.gmapM, c.gmapP, g=c.ph["g"], zx=c.ph["zx"], zy=c.ph["zy"],
                         f=c.ph["f"], CD=c.ph["CD"])
    assert s.usesNodalTraces == (form == "nodal-trace") and s.hasFilter == with_filter
    s.setState(*c.q)
    return s, c.q, dt


def _assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), f"{what}: field {c} differs by {np.abs(u - v).max():.3e}"


@pytest.mark.parametrize("filt", [True, False], ids=["filter", "nofilter"])
@pytest.mark.parametrize("order", ORDERS)
def test_rk2_steps_in_one_call_equal_single_steps(order, filt, form):
    a, q, dt = _make(order, form)
    b = _make(order, form)[0]
    a.stepRK2(dt, 3, filter=filt)
    for _ in range(3):
        b.stepRK2(dt, 1, filter=filt)
    got = a.getState()
    _assert_same_bits(got, b.getState(), "three RK2 steps")
    assert not np.array_equal(got[1], q[1])                        # the state moved
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_an_rk2_step_equals_its_two_phases(order, form):
    a, q, dt = _make(order, form)
    b = _make(order, form)[0]
    a.stepRK2(dt, 1)
    b.rk2Phase(dt, 0)
    b.rk2Phase(dt, 1)
    _assert_same_bits(a.getState(), b.getState(), "predictor + corrector")
    assert not np.array_equal(a.getState()[1], q[1])
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_timed_steps_leave_what_plain_steps_leave(order, form):
    a, _, dt = _make(order, form)
    b = _make(order, form)[0]
    ms = a.timeRK2(dt, 3)
    b.stepRK2(dt, 3)
    assert np.isfinite(ms) and ms > 0
    _assert_same_bits(a.getState(), b.getState(), "three timed steps")
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_lserk_stages_carry_over_calls(order, form):
    """Seven stages, then three: an odd count first, after which the nodal-trace form has swapped its two state buffers and the
    stage counter stands two stages into the second step."""
    a, q, dt = _make(order, form)
    b = _make(order, form)[0]
    a.lserk4Stages(dt, 7)
    a.lserk4Stages(dt, 3)
    b.lserk4Stages(dt, 10)
    got = a.getState()
    _assert_same_bits(got, b.getState(), "7 + 3 stages")
    assert not np.array_equal(got[1], q[1])
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_set_state_resets_the_stage_count_and_the_residual(order, form):
    a, q, dt = _make(order, form)
    b = _make(order, form)[0]
    a.lserk4Stages(dt, 7)
    a.setState(*q)
    a.lserk4Stages(dt, 5)
    b.lserk4Stages(dt, 5)
    _assert_same_bits(a.getState(), b.getState(), "a step after setState")
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_an_rhs_evaluation_leaves_the_solver_alone(order, form):
    a, q, dt = _make(order, form)
    b = _make(order, form)[0]
    q1 = curved_cases.second_state(_case(order)[0])
    a.lserk4Stages(dt, 7)
    before = a.getState()
    got = a.computeRHS(*q1)
    _assert_same_bits(a.getState(), before, "state across computeRHS")
    _assert_same_bits(got, b.computeRHS(*q1), "RHS after seven stages against a fresh solver's")
    _assert_same_bits(b.getState(), q, "fresh state across computeRHS")
    a.lserk4Stages(dt, 3)                                           # and the stages go on from where they were
    b.lserk4Stages(dt, 10)
    _assert_same_bits(a.getState(), b.getState(), "7 stages, an RHS, 3 stages")
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_element_columns_round_trip_on_both_buffers(order, form):
    s, q, dt = _make(order, form)
    s.rk2Phase(dt, 0)                                               # the intermediate buffer holds a predictor
    Np = s.Np
    for intermediate in (False, True):
        whole = s.getElements(0, s.K, intermediate)
        assert whole.shape == (4 * Np, s.K)
        if not intermediate:
            _assert_same_bits([whole[c * Np:(c + 1) * Np] for c in range(4)], q, "getElements against the state")
        else:
            assert not np.array_equal(whole[Np:2 * Np], q[1])
        for first, n in ((0, s.K), (5, 9), (17, 1), (3, 0)):
            cols = s.getElements(first, n, intermediate)
            assert np.array_equal(cols, whole[:, first:first + n])
            s.setElements(first, cols, intermediate)
            assert np.array_equal(s.getElements(0, s.K, intermediate), whole)
        other = whole[:, ::-1][:, 4:11].copy()
        s.setElements(2, other, intermediate)                       # columns that differ do land, and only there
        now = s.getElements(0, s.K, intermediate)
        assert np.array_equal(now[:, 2:9], other) and np.array_equal(now[:, :2], whole[:, :2]) and np.array_equal(now[:, 9:], whole[:, 9:])
        s.setElements(0, whole, intermediate)
    _assert_same_bits(s.getState(), q, "state after the round trips")
    s.close()


def test_element_ranges_and_buffers_out_of_bounds_are_refused(form):
    s, q, _ = _make(3, form)
    buf = np.zeros((4 * s.Np, s.K + 1))
    ptr = buf.ctypes.data_as(POINTER(c_double))
    for name in ("get", "set"):
        fn = getattr(C.lib, f"bdg_sw2d_curved_{name}_elements")
        for first, n in ((-1, 2), (0, s.K + 1), (s.K, 1), (3, -1)):
            with pytest.raises(C.BdgError) as err:
                C.check(fn(s._h, 0, first, n, ptr))
            assert f"bdg_sw2d_curved_{name}_elements: element range out of bounds" in str(err.value)
        for which in (-1, 2):
            with pytest.raises(C.BdgError) as err:
                C.check(fn(s._h, which, 0, 1, ptr))
            assert f"bdg_sw2d_curved_{name}_elements: which must be 0 (state) or 1 (intermediate)" in str(err.value)
        with pytest.raises(C.BdgError) as err:
            C.check(fn(s._h, 0, 0, 1, None))
        assert f"bdg_sw2d_curved_{name}_elements: NULL buffer" in str(err.value)
    _assert_same_bits(s.getState(), q, "state after the refusals")
    s.close()


@pytest.mark.parametrize("order", ORDERS)
def test_filtered_calls_without_a_filter_are_refused(order, form):
    s, q, dt = _make(order, form, with_filter=False)
    for call in (lambda: s.stepRK2(dt, 1, filter=True), lambda: s.rk2Phase(dt, 0, filter=True), lambda: s.rk2Phase(dt, 1, filter=True),
                 lambda: s.computeRHS(*q, filter=True), lambda: s.kernelInfo(filter=True), lambda: s.timeRK2(dt, 1, filter=True)):
        with pytest.raises(C.BdgError, match=NO_FILTER):
            call()
    _assert_same_bits(s.getState(), q, "state after the refusals")   # nothing was launched before the refusal
    assert s.kernelInfo(filter=False)["form"] == (1 if form == "nodal-trace" else 0)
    s.stepRK2(dt, 1, filter=False)                                   # and the solver goes on
    assert not np.array_equal(s.getState()[1], q[1])
    s.close()


def test_straight_elements_use_the_weights_their_ratios_refer_to(form):
    """curved_cases.kref_case: elements 0 and 1 are straight-sided and listed, so the general form takes its reference cubature
    weights from element 0 and the nodal-trace form, which skips listed elements, from element 2, whose area is 27 % larger.
    The nodal-trace form's straight elements hold ratios to the weights of element 2: with element 0's weights in their place
    every straight element's volume term is off by that ratio. Against the oracle, to the tolerance of
    test_sw2d_curved_gpu.test_curved_rhs_matches_the_oracle_on_ragged_meshes."""
    from test_sw2d_curved_gpu import RHS_TOL, rel_field_err
    c = curved_cases.kref_case()
    s = curved_cases.solver(c)
    assert s.usesNodalTraces == (form == "nodal-trace")
    err = rel_field_err(s.computeRHS(*c.q), curved_cases.rhs(c, c.q))
    print(f"kref case, {form}: RHS error {err:.3e}")
    assert err < RHS_TOL
    s.close()
