"""The host path of the straight-element sw2d solver (sw2d_device.hip): the calls whose results no other module pins.

Everything here compares the solver with itself, bit for bit: a timed run with the plain run, a probed solver with a twin that
never probed, n steps in one call with n calls of one step. The arithmetic of the kernels is held to the oracle elsewhere
(test_stepper_families_gpu.py, test_sw2d_gpu.py); these tests hold what the host code around the launches carries from call to
call -- the stage counter, the frozen tide time, the buffer roles, the accumulated speed of variant B -- and the text of its refusals.

The mesh is a 3 x 3 box: K = 18 triangles, one full 16-element matrix-core tile and a ragged one. Order 3 takes the unrolled
(fastSources) branch of launchStage's ladder, order 6 the matrix-core (mfmaSources) branch.
"""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2d
from conftest import seeded_fields, tables_from_nodes, variant_b_setup

pytestmark = pytest.mark.gpu

ORDERS = (3, 6)
CFL = 0.65
SPONGE = 0.05
NO_FILTER = "filter requested but the solver was created without a Filter matrix"

_CASES = {}


def _case(order):
    """Mesh, nodes, tables and the variant-B problem (conftest.variant_b_setup: open left edge, sloping bed) at `order`, built once."""
    if order not in _CASES:
        m = dg.MeshManager()
        m.buildBoxMesh(3, 3)
        nodes = dg.TriangleNodesProvisioner(order, m)
        nodes.buildFilter(0.9 * order, order)
        t = tables_from_nodes(nodes)
        K = t["rx"].shape[1]
        assert K == 18 and K > 16 and K % 16 != 0
        bnodes, bt, e = variant_b_setup(order, m)
        e["Hx"], e["Hy"] = bnodes.bedSlopes(e["H"])
        e["sponge"] = bnodes.buildSpongeCoeff(e["mapO"], 2.0, 0.7)
        _CASES[order] = (nodes, t, bnodes, e)
    return _CASES[order]


def _make(order, kind):
    """A solver of `kind` with its state set, its set/get calls, and a stable dt. A: three fields; B: tide, sponge field and a
    non-zero model time; D: four fields with bed slope, Coriolis array and drag."""
    nodes, t, bnodes, e = _case(order)
    x, y = t["x"], t["y"]
    if kind == "A":
        s = sw2d.Sw2dSolver(nodes=nodes)
        q = seeded_fields(x, y, seed=order)
    elif kind == "B":
        s = sw2d.Sw2dSolver(nodes=bnodes)
        s.enableVariantB(e["H"], e["Hx"], e["Hy"], mapO=e["mapO"], CD=e["CD"], f=e["f"], sponge=e["sponge"])
        s.time = e["time"]
        q = (e["h"], e["hu"], e["hv"])
    else:
        src = {"zx": 0.2 * np.cos(2 * x) * np.sin(y + 0.3), "zy": -0.15 * np.sin(3 * y) * np.cos(x), "f": 0.3 * (1.0 + 0.5 * y),
               "CD": 2.5e-3}
        s = sw2d.Sw2dSolver(tables=t, fields=4, sources=src)
        h, hu, hv = seeded_fields(x, y, seed=order + 200)
        q = (h, hu, hv, h * (0.5 + 0.3 * np.sin(2 * x + 0.5) * np.cos(3 * y)))
    setq, getq = (s.setState4, s.getState4) if kind == "D" else (s.setState, s.getState)
    setq(*q)
    dt = 0.25 * s.computeDt(CFL)[0]
    return s, q, setq, getq, dt


def _assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v), f"{what}: field {c} differs by {np.abs(u - v).max():.3e}"


@pytest.mark.parametrize("kind", ["A", "B", "D"])
@pytest.mark.parametrize("order", ORDERS)
def test_timed_stages_leave_what_plain_stages_leave(order, kind):
    """timeLSERK4Stages(dt, 7) against lserk4Stages(dt, 7) on a twin, then three more plain stages on both: seven stages end two
    stages into the second step, so the stage counter and (variant B) the tide time frozen over a step have to carry over."""
    a, q, _, geta, dt = _make(order, kind)
    b, _, _, getb, _ = _make(order, kind)
    t0 = a.time
    ms = a.timeLSERK4Stages(dt, 7)
    b.lserk4Stages(dt, 7)
    assert np.isfinite(ms) and ms > 0
    got = geta()
    _assert_same_bits(got, getb(), "7 stages")
    assert not np.array_equal(got[1], q[1])            # the state moved
    assert a.time == b.time == t0 + dt                  # one step complete
    a.lserk4Stages(dt, 3)
    b.lserk4Stages(dt, 3)
    _assert_same_bits(geta(), getb(), "7 + 3 stages")
    assert a.time == b.time == t0 + dt + dt
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_traffic_probe_leaves_the_solver_alone(order):
    a, q, _, _, dt = _make(order, "A")
    b = _make(order, "A")[0]
    assert a.usesAffineGeometry
    before = a.getState()
    ms = a.probeStageTraffic(5)
    assert np.isfinite(ms) and ms > 0
    _assert_same_bits(a.getState(), before, "state across the probe")
    _assert_same_bits(before, q, "state as set")
    a.lserk4Stages(dt, 5)
    b.lserk4Stages(dt, 5)
    _assert_same_bits(a.getState(), b.getState(), "a step after the probe")
    a.close()
    b.close()
    n = sw2d.Sw2dSolver(nodes=_case(order)[0], flags=sw2d.NODAL_GEOMETRY)
    assert not n.usesAffineGeometry
    with pytest.raises(C.BdgError, match="bdg_sw2d_probe_stage_traffic: affine geometry only"):
        n.probeStageTraffic(5)
    n.close()


def test_field_calls_of_the_other_arity_are_refused():
    s3, q3, _, _, _ = _make(3, "A")
    s4, q4, _, _, _ = _make(3, "D")
    refusals = [
        (lambda: s3.setState4(*q4), "bdg_sw2d_set_state4: the solver was created with 3 fields"),
        (lambda: s3.getState4(), "bdg_sw2d_get_state4: the solver was created with 3 fields"),
        (lambda: s3.computeRHS4(*q4), "bdg_sw2d_rhs4: the solver was created with 3 fields"),
        (lambda: s4.setState(*q3), "bdg_sw2d_set_state: this solver has 4 fields, use bdg_sw2d_set_state4"),
        (lambda: s4.getState(), "bdg_sw2d_get_state: this solver has 4 fields, use bdg_sw2d_get_state4"),
        (lambda: s4.computeRHS(*q3), "bdg_sw2d_rhs: this solver has 4 fields, use bdg_sw2d_rhs4"),
    ]
    for call, text in refusals:
        with pytest.raises(C.BdgError) as err:
            call()
        assert text in str(err.value)
    _assert_same_bits(s3.getState(), q3, "three-field state after the refusals")
    _assert_same_bits(s4.getState4(), q4, "four-field state after the refusals")
    s3.close()
    s4.close()


@pytest.mark.parametrize("kind", ["A", "D"])
@pytest.mark.parametrize("order", ORDERS)
def test_set_state_resets_the_stage_count(order, kind):
    """Seven stages leave a step part-way (stepLSERK4 refuses to go on); setting the state starts over: stage 0, residual zero."""
    a, q, seta, geta, dt = _make(order, kind)
    b, _, _, getb, _ = _make(order, kind)
    a.lserk4Stages(dt, 7)
    with pytest.raises(C.BdgError, match="a previous step was left part-way through its stages"):
        a.stepLSERK4(dt, 1)
    seta(*q)
    a.stepLSERK4(dt, 1)
    b.stepLSERK4(dt, 1)
    _assert_same_bits(geta(), getb(), "a step after setState")
    a.close()
    b.close()


@pytest.mark.parametrize("filt", [True, False], ids=["filter", "nofilter"])
@pytest.mark.parametrize("kind", ["A", "B", "D"])
@pytest.mark.parametrize("order", ORDERS)
def test_rk2_steps_in_one_call_equal_single_steps(order, kind, filt):
    a, q, _, geta, dt = _make(order, kind)
    b, _, _, getb, _ = _make(order, kind)
    a.stepRK2(dt, 3, filter=filt)
    for _ in range(3):
        b.stepRK2(dt, 1, filter=filt)
    got = geta()
    _assert_same_bits(got, getb(), "three RK2 steps")
    assert not np.array_equal(got[1], q[1])
    assert a.time == b.time
    a.close()
    b.close()


@pytest.mark.parametrize("sponge", [0.0, SPONGE], ids=["nosponge", "sponge"])
@pytest.mark.parametrize("filt", [True, False], ids=["filter", "nofilter"])
@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("order", ORDERS)
def test_ssprk2_steps_in_one_call_equal_single_steps(order, kind, filt, sponge):
    a, q, _, geta, dt = _make(order, kind)
    b, _, _, getb, _ = _make(order, kind)
    a.stepSSPRK2(dt, 3, filter=filt, sponge=sponge)
    for _ in range(3):
        b.stepSSPRK2(dt, 1, filter=filt, sponge=sponge)
    got = geta()
    _assert_same_bits(got, getb(), "three SSP-RK2 steps")
    assert not np.array_equal(got[1], q[1])
    assert a.time == b.time
    a.close()
    b.close()


@pytest.mark.parametrize("order", ORDERS)
def test_filtered_steps_without_a_filter_are_refused(order):
    t = dict(_case(order)[1])
    t["Filter"] = None
    s = sw2d.Sw2dSolver(tables=t)
    q = seeded_fields(t["x"], t["y"], seed=order)
    s.setState(*q)
    dt = 0.25 * s.computeDt(CFL)[0]
    for call in (lambda: s.stepSSPRK2(dt, 1, filter=True), lambda: s.stepSSPRK2(dt, 1, filter=True, sponge=SPONGE),
                 lambda: s.stepRK2(dt, 1, filter=True), lambda: s.computeRHS(*q, filter=True)):
        with pytest.raises(C.BdgError, match=NO_FILTER):
            call()
    _assert_same_bits(s.getState(), q, "state after the refusals")   # nothing was launched before the refusal
    s.stepSSPRK2(dt, 1, filter=False)                                # and the solver goes on
    assert not np.array_equal(s.getState()[1], q[1])
    s.close()
