"""The four-field quadrilateral sw2d path on the GPU (bdg_sw2dq_*4, csrc/hip/sw2d_quad4_kernel.hpp: tracer, Coriolis, drag,
bed slope) against
  (a) the reference's own swhelpers.rhs.sw2dComputeRHS on this repository's quadrilateral tables
      (tests/golden/sw2dq_rhs4_*.npz), in both geometry forms, unfiltered and filtered, through computeRHS4 and through the
      13-argument drop-in blitzdg_amd.swhelpers.rhs.sw2dComputeRHS with a quadrilateral context;
  (b) NumPy loops of the same function (tests/quadref4.py, pinned to the fixtures by test_quad4_setup.py) for midpoint-RK2 +
      filter steps and LSERK4 stages;
  (c) properties: the tracer of hN = c h, agreement with the three-field solver, rest under rotation, water and tracer mass,
      computeDt, refusals.
Tolerances as tests/test_sw2d_quads_gpu.py: one RHS 1e-12 of max|RHS| per field, multi-step states 1e-11."""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2dquads
from blitzdg_amd._capi import BdgError, NumericalInstability
from blitzdg_amd.swhelpers.rhs import sw2dComputeRHS
from quadref import quad_box
from quadref4 import (FIXTURES4, PARALLELOGRAM4, compute_dt, gll_weights, load_fixture4, reference, rhs4, sources, state,
                      tables)
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11


def flags(general):
    return sw2dquads.GENERAL_GEOMETRY if general else 0


@pytest.mark.parametrize("name", FIXTURES4)
@pytest.mark.parametrize("general", [False, True])
def test_rhs4_matches_reference_fixture(name, general):
    d, _, nodes, ctx = load_fixture4(name)
    t = tables(ctx)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=float(d["g"]), flags=flags(general), fields=4, sources=sources(d))
    assert s.usesParallelogramGeometry == (not general and name in PARALLELOGRAM4)
    ref = reference(d)
    assert_fields_close(s.computeRHS4(*state(d)), ref, RHS_TOL, what=name)
    assert_fields_close(s.computeRHS4(*state(d), filter=True), [t["Filter"] @ r for r in ref], RHS_TOL,
                        what=name + " filtered")
    # the provisioner route builds the same solver
    s2 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]), flags=flags(general), fields=4, sources=sources(d))
    assert_fields_close(s2.computeRHS4(*state(d)), ref, RHS_TOL, what=name + " from nodes")


@pytest.mark.parametrize("name", FIXTURES4)
def test_thirteen_argument_drop_in_on_a_quadrilateral_context(name):
    d, _, _, ctx = load_fixture4(name)
    src = sources(d)
    H = 10.0 * np.ones_like(d["h"])
    vmapM, vmapP = ctx.vmapM, ctx.vmapP
    r = sw2dComputeRHS(d["h"], d["hu"], d["hv"], d["hN"], src["zx"], src["zy"], float(d["g"]), H, src["f"], src["CD"], ctx,
                       vmapM, vmapP)
    assert_fields_close(r, reference(d), RHS_TOL, what=name)
    # the cached solver serves a second state
    r = sw2dComputeRHS(d["h"], 2 * d["hu"], d["hv"], d["hN"], src["zx"], src["zy"], float(d["g"]), H, src["f"], src["CD"], ctx,
                       vmapM, vmapP)
    want = rhs4(d["h"], 2 * d["hu"], d["hv"], d["hN"], float(d["g"]), tables(ctx), **src)
    assert_fields_close(r, want, RHS_TOL, what=name + " second state")


@pytest.mark.parametrize("name", ["coarse_box_quads_fine_N4", "jitter_box5x4_N5", "box6x5_shuffled_N7",
                                  "scalarf_jitter_box5x4_N4"])
def test_rk2_filter_steps_match_numpy(name):
    d, _, _, ctx = load_fixture4(name)
    t = tables(ctx)
    g, dt, F, src = float(d["g"]), 2e-4, t["Filter"], sources(d)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=g, fields=4, sources=src)
    q = state(d)
    s.setState4(*q)
    s.stepRK2(dt, 20, filter=True)
    for _ in range(20):
        r = [F @ x for x in rhs4(*q, g, t, **src)]
        q1 = [a + 0.5 * dt * b for a, b in zip(q, r)]
        r = [F @ x for x in rhs4(*q1, g, t, **src)]
        q = [a + dt * b for a, b in zip(q, r)]
    assert_fields_close(s.getState4(), q, STATE_TOL, what=name)


@pytest.mark.parametrize("name", ["coarse_box_quads_fine_N3", "jitter_box5x4_N8", "box6x5_shuffled_N4",
                                  "nosrc_box6x5_shuffled_N5"])
def test_lserk4_stages_match_numpy(name):
    d, _, _, ctx = load_fixture4(name)
    t = tables(ctx)
    g, dt, src = float(d["g"]), 2e-4, sources(d)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=g, fields=4, sources=src)
    q = state(d)
    s.setState4(*q)
    s.lserk4Stages(dt, 10)
    res = [np.zeros_like(x) for x in q]
    for i in range(10):
        a, b = dg.LSERK4.rk4a[i % 5], dg.LSERK4.rk4b[i % 5]
        r = rhs4(*q, g, t, **src)
        res = [a * x + dt * y for x, y in zip(res, r)]
        q = [x + b * y for x, y in zip(q, res)]
    assert_fields_close(s.getState4(), q, STATE_TOL, what=name)


@pytest.mark.parametrize("name", ["jitter_box5x4_N5", "box6x5_shuffled_N7", "coarse_box_quads_fine_N2"])
@pytest.mark.parametrize("with_zero_sources", [False, True])
def test_zero_sources_tracer_proportional_to_depth_and_three_field_agreement(name, with_zero_sources):
    d, _, nodes, _ = load_fixture4(name)
    z = np.zeros_like(d["h"])
    src = {"zx": z, "zy": z, "f": 0.0, "CD": 0.0} if with_zero_sources else None
    s4 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]), fields=4, sources=src)
    s3 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]))
    c = 0.37
    r4 = s4.computeRHS4(d["h"], d["hu"], d["hv"], c * d["h"])
    assert_fields_close([r4[3]], [c * r4[0]], RHS_TOL, what=name + " tracer")
    assert_fields_close(r4[:3], s3.computeRHS(d["h"], d["hu"], d["hv"]), RHS_TOL, what=name + " against three fields")


@pytest.mark.parametrize("general", [False, True])
def test_fluid_at_rest_under_rotation_stays_at_rest(general):
    """Flat bed, f != 0 (array), drag on, fluid at rest: nothing moves, to the bounds of test_sw2d_quads_gpu.test_lake_at_rest."""
    d, _, nodes, ctx = load_fixture4("jitter_box5x4_N5") if general else load_fixture4("box6x5_shuffled_N7")
    z = np.zeros_like(d["h"])
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=flags(general), fields=4,
                                 sources={"zx": z, "zy": z, "f": 0.1 * (1 + 0.5 * ctx.y), "CD": 2.5e-2})
    h = 10.0 * np.ones_like(d["h"])
    r = s.computeRHS4(h, z, z, 0.5 * h)
    assert max(np.abs(x).max() for x in r) < 1e-12 * 9.81 * 100
    s.setState4(h, z, z, 0.5 * h)
    s.stepRK2(1e-3, 50, filter=True)
    q = s.getState4()
    assert np.abs(q[0] - 10.0).max() < 1e-12 and max(np.abs(q[1]).max(), np.abs(q[2]).max()) < 1e-11
    assert np.abs(q[3] - 5.0).max() < 1e-12


def test_water_and_tracer_mass_conserved_with_sources():
    """Drag, Coriolis and bed slope do not enter equations 1 and 4: with walls on every side, sum w J h and sum w J hN stay
    within 1e-12 relative over 100 unfiltered steps (the bound of test_mass_conserved_on_large_box)."""
    E, V = quad_box(400)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    nodes = dg.QuadNodesProvisioner(4, mesh)
    ctx = nodes.dgContext()
    x, y, J = ctx.x, ctx.y, ctx.J
    w = gll_weights(ctx, 4)
    h = 10.0 + np.exp(-40 * (x - 0.1) ** 2 - 40 * y ** 2)
    hu = 0.2 * np.exp(-40 * x ** 2 - 40 * (y + 0.2) ** 2)
    hv = np.zeros_like(h)
    hN = h * np.exp(-20 * (x + 0.2) ** 2 - 20 * (y - 0.1) ** 2)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, fields=4,
                                 sources={"zx": -0.05 + 0 * x, "zy": 0.05 * y, "f": 0.1 * (1 + 0.5 * y), "CD": 2.5e-2})
    assert s.usesParallelogramGeometry
    s.setState4(h, hu, hv, hN)
    m0, n0 = (w * J * h).sum(), (w * J * hN).sum()
    s.stepRK2(1e-5, 100, filter=False)
    q = s.getState4()
    m1, n1 = (w * J * q[0]).sum(), (w * J * q[3]).sum()
    assert np.abs(q[1] - hu).max() > 1e-6                    # the sources did act
    assert abs(m1 - m0) <= 1e-12 * abs(m0)
    assert abs(n1 - n0) <= 1e-12 * abs(n0)


@pytest.mark.parametrize("name", FIXTURES4)
@pytest.mark.parametrize("fields", [3, 4])
def test_compute_dt_matches_numpy_formula(name, fields):
    """The device forms the speed with the same IEEE-exact operations as NumPy (division, square root, no contraction) and a
    maximum, which is order-independent: equal to 1 ulp (the final division of dt happens on the host in both)."""
    d, _, _, ctx = load_fixture4(name)
    t = tables(ctx)
    g = float(d["g"])
    for general in (False, True):
        s = sw2dquads.Sw2dQuadSolver(tables=t, g=g, flags=flags(general), fields=fields)
        if fields == 4:
            s.setState4(*state(d))
        else:
            s.setState(*state(d)[:3])
        dt, speed = s.computeDt(0.5)
        want_dt, want_speed = compute_dt(d["h"], d["hu"], d["hv"], g, t, 0.5)
        if general:  # the tables themselves; the parallelogram form holds a per-face mean of Fscale (1e-10 relative at creation)
            assert abs(speed - want_speed) <= np.spacing(want_speed) and abs(dt - want_dt) <= np.spacing(want_dt)
        else:
            assert abs(speed - want_speed) <= (1e-10 if s.usesParallelogramGeometry else 0) * want_speed + np.spacing(want_speed)
    h = d["h"].copy()
    h[0, 0] = np.nan
    s.setState4(h, d["hu"], d["hv"], d["hN"]) if fields == 4 else s.setState(h, d["hu"], d["hv"])
    with pytest.raises(NumericalInstability):
        s.computeDt(0.5)


def test_blow_up_raises_on_a_four_field_solver():
    d, _, nodes, _ = load_fixture4("coarse_box_quads_fine_N3")
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, fields=4, sources=sources(d))
    h = d["h"].copy()
    h[0, 0] = np.nan
    s.setState4(h, d["hu"], d["hv"], d["hN"])
    with pytest.raises(NumericalInstability, match="numerical instability"):
        s.stepRK2(1e-4, 1, filter=True)


def test_refusals_leave_the_solver_usable():
    d, _, nodes, ctx = load_fixture4("coarse_box_quads_fine_N3")
    t = tables(ctx)
    src = sources(d)
    q = state(d)
    # sources of a wrong shape, a non-scalar drag, sources without the fourth field
    for bad in ({"zx": src["zx"][:-1]}, {"zy": src["zy"].T[:3]}, {"f": src["f"][:, :-1]}, {"CD": np.ones(3)}):
        with pytest.raises(ValueError):
            sw2dquads.Sw2dQuadSolver(tables=t, fields=4, sources={**src, **bad})
    with pytest.raises(ValueError):
        sw2dquads.Sw2dQuadSolver(tables=t, fields=3, sources=src)
    with pytest.raises(ValueError):
        sw2dquads.Sw2dQuadSolver(tables=t, fields=5)
    # three-field calls on a four-field solver
    s4 = sw2dquads.Sw2dQuadSolver(tables=t, g=float(d["g"]), fields=4, sources=src)
    for call in (lambda: s4.setState(*q[:3]), s4.getState, lambda: s4.computeRHS(*q[:3])):
        with pytest.raises(BdgError, match="4 fields"):
            call()
    with pytest.raises(ValueError):
        s4.setState4(q[0], q[1], q[2], q[3][:-1])
    assert_fields_close(s4.computeRHS4(*q), reference(d), RHS_TOL)
    # sources after the first evaluation
    with pytest.raises(BdgError, match="before the first evaluation"):
        s4.setSources(**src)
    assert_fields_close(s4.computeRHS4(*q), reference(d), RHS_TOL)
    s4.setState4(*q)
    s4.lserk4Stages(1e-4, 5)
    assert all(np.isfinite(a).all() for a in s4.getState4())
    # four-field calls and sources on a three-field solver
    s3 = sw2dquads.Sw2dQuadSolver(tables=t, g=float(d["g"]))
    for call in (lambda: s3.setState4(*q), s3.getState4, lambda: s3.computeRHS4(*q), lambda: s3.setSources(**src)):
        with pytest.raises(BdgError, match="3 fields"):
            call()
    s3.setState(*q[:3])
    s3.stepRK2(1e-4, 2, filter=True)
    assert all(np.isfinite(a).all() for a in s3.getState())
