"""The quadrilateral sw2d path on the GPU (bdg_sw2dq_*, csrc/hip/sw2d_quad_kernel.hpp) against
  (a) the reference script's sw2dComputeRHS on this repository's tables (tests/golden/sw2dq_rhs_*.npz), in both
      geometry forms, unfiltered and filtered;
  (b) NumPy loops of the same function (tests/quadref.py, pinned to the fixtures by test_quad_setup.py) for the
      script's midpoint-RK2 + filter steps and for LSERK4 stages;
  (c) properties: lake at rest, mass conservation on a 400 x 400 box, mirror symmetry, blow-up report, refusals.
Tolerances as tests/test_sw2d_gpu.py: one RHS 1e-12 of max|RHS| per field, multi-step states 1e-11."""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2dquads
from blitzdg_amd._capi import BdgError, NumericalInstability
from quadref import FIXTURES, load_fixture, quad_box, rhs, tables
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
PARALLELOGRAM = {"box6x5_shuffled_N4", "box6x5_shuffled_N7", "shear_box6x5_N3", "shear_box6x5_N8"}


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("general", [False, True])
def test_rhs_matches_reference_fixture(name, general):
    d, _, nodes, ctx = load_fixture(name)
    t = tables(ctx)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=float(d["g"]), flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    assert s.usesParallelogramGeometry == (not general and name in PARALLELOGRAM)
    ref = [d[f"rhs{i}"] for i in (1, 2, 3)]
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), ref, RHS_TOL, what=name)
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"], filter=True), [t["Filter"] @ r for r in ref], RHS_TOL,
                        what=name + " filtered")
    # the provisioner route builds the same solver
    s2 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]), flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    assert_fields_close(s2.computeRHS(d["h"], d["hu"], d["hv"]), ref, RHS_TOL, what=name + " from nodes")


def test_drop_in_signature():
    d, _, _, ctx = load_fixture("coarse_box_quads_fine_N4")
    H = 10.0 * np.ones_like(d["h"])
    r = sw2dquads.sw2dComputeRHS(d["h"], d["hu"], d["hv"], 9.81, H, ctx)
    assert_fields_close(r, [d[f"rhs{i}"] for i in (1, 2, 3)], RHS_TOL)


@pytest.mark.parametrize("name", ["coarse_box_quads_fine_N4", "jitter_box5x4_N5", "box6x5_shuffled_N7"])
def test_rk2_filter_steps_match_numpy(name):
    d, _, _, ctx = load_fixture(name)
    t = tables(ctx)
    g, dt, F = 9.81, 2e-4, t["Filter"]
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=g)
    q = [d["h"].copy(), d["hu"].copy(), d["hv"].copy()]
    s.setState(*q)
    s.stepRK2(dt, 20, filter=True)
    for _ in range(20):  # the script's loop body, sw2dquads.py:183-207
        r = [F @ x for x in rhs(*q, g, t)]
        q1 = [a + 0.5 * dt * b for a, b in zip(q, r)]
        r = [F @ x for x in rhs(*q1, g, t)]
        q = [a + dt * b for a, b in zip(q, r)]
    assert_fields_close(s.getState(), q, STATE_TOL, what=name)


@pytest.mark.parametrize("name", ["coarse_box_quads_fine_N3", "jitter_box5x4_N8", "box6x5_shuffled_N4"])
def test_lserk4_stages_match_numpy(name):
    d, _, _, ctx = load_fixture(name)
    t = tables(ctx)
    g, dt = 9.81, 2e-4
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=g)
    q = [d["h"].copy(), d["hu"].copy(), d["hv"].copy()]
    s.setState(*q)
    s.lserk4Stages(dt, 10)
    res = [np.zeros_like(x) for x in q]
    for i in range(10):
        a, b = dg.LSERK4.rk4a[i % 5], dg.LSERK4.rk4b[i % 5]
        r = rhs(*q, g, t)
        res = [a * x + dt * y for x, y in zip(res, r)]
        q = [x + b * y for x, y in zip(q, res)]
    assert_fields_close(s.getState(), q, STATE_TOL, what=name)


@pytest.mark.parametrize("general", [False, True])
def test_lake_at_rest(general):
    d, _, nodes, ctx = load_fixture("jitter_box5x4_N5") if general else load_fixture("box6x5_shuffled_N7")
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    h = 10.0 * np.ones_like(d["h"])
    z = np.zeros_like(h)
    r = s.computeRHS(h, z, z)
    assert max(np.abs(x).max() for x in r) < 1e-12 * 9.81 * 100
    s.setState(h, z, z)
    s.stepRK2(1e-3, 50, filter=True)
    q = s.getState()
    assert np.abs(q[0] - 10.0).max() < 1e-12 and max(np.abs(q[1]).max(), np.abs(q[2]).max()) < 1e-11


def test_mass_conserved_on_large_box():
    E, V = quad_box(400)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    nodes = dg.QuadNodesProvisioner(4, mesh)
    nodes.buildFilter(0.99 * 4, 4)
    ctx = nodes.dgContext()
    x, y, J = ctx.x, ctx.y, ctx.J
    V1 = dg.VandermondeBuilder().buildVandermondeMatrix(ctx.s[:5])[0]
    w1 = np.linalg.inv(V1 @ V1.T).sum(axis=1)               # 1-D Gauss-Lobatto mass-matrix row sums = weights
    w = np.outer(w1, w1).ravel()[:, None]                   # node (N+1) j + i: w1[j] w1[i]
    h = 10.0 + np.exp(-40 * (x - 0.1) ** 2 - 40 * y ** 2)
    hu = 0.2 * np.exp(-40 * x ** 2 - 40 * (y + 0.2) ** 2)
    hv = np.zeros_like(h)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes)
    assert s.usesParallelogramGeometry
    s.setState(h, hu, hv)
    m0 = (w * J * h).sum()
    s.stepRK2(1e-5, 100, filter=False)
    m1 = (w * J * s.getState()[0]).sum()
    assert abs(m1 - m0) <= 1e-12 * abs(m0)


def test_symmetric_gaussian_stays_symmetric():
    E, V = quad_box(12)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    nodes = dg.QuadNodesProvisioner(5, mesh)
    nodes.buildFilter(0.99 * 5, 4)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes)
    s.setState(h, np.zeros_like(h), np.zeros_like(h))
    s.stepRK2(2e-4, 40, filter=True)
    hh, hu, hv = s.getState()
    # x -> -x maps element (i, j) of the box to (n-1-i, j) and node (N+1) jr + is to (N+1) (N-jr) + is (r runs along x)
    n, N = 12, 5
    el = np.arange(n * n).reshape(n, n)[:, ::-1].ravel()
    nd = np.arange((N + 1) ** 2).reshape(N + 1, N + 1)[::-1, :].ravel()
    assert np.abs(x[np.ix_(nd, el)] + x).max() < 1e-14 and np.abs(y[np.ix_(nd, el)] - y).max() < 1e-14
    scale = np.abs(hh - 10.0).max()
    assert np.abs(hh[np.ix_(nd, el)] - hh).max() < 1e-12 * scale
    assert np.abs(hu[np.ix_(nd, el)] + hu).max() < 1e-12 * np.abs(hu).max()
    assert np.abs(hv[np.ix_(nd, el)] - hv).max() < 1e-12 * np.abs(hv).max()


def test_blow_up_raises():
    d, _, nodes, _ = load_fixture("coarse_box_quads_fine_N3")
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes)
    h = d["h"].copy()
    h[0, 0] = np.nan
    s.setState(h, d["hu"], d["hv"])
    with pytest.raises(NumericalInstability, match="numerical instability"):
        s.stepRK2(1e-4, 1, filter=True)
    s.setState(d["h"] * 1e9, d["hu"], d["hv"])
    with pytest.raises(NumericalInstability):
        s.lserk4Stages(1e-12, 1)


def test_create_refusals():
    d, _, _, ctx = load_fixture("coarse_box_quads_fine_N3")
    t = tables(ctx)
    bad = dict(t)
    bad["Dr"] = t["Dr"] + 1e-6 * np.random.default_rng(0).standard_normal(t["Dr"].shape)
    with pytest.raises(BdgError, match="tensor"):
        sw2dquads.Sw2dQuadSolver(tables=bad)
    bad = dict(t)
    bad["Lift"] = t["Lift"].copy()
    bad["Lift"][3, 1] += 0.5
    with pytest.raises(BdgError, match="Lift"):
        sw2dquads.Sw2dQuadSolver(tables=bad)
    for order in (0, 9):
        mesh = dg.MeshManager()
        mesh.buildMesh(*quad_box(2))
        Np = (order + 1) ** 2
        nfn = 4 * (order + 1)
        fake = {"order": order, "Dr": np.zeros((Np, Np)), "Ds": np.zeros((Np, Np)), "Lift": np.zeros((Np, nfn)),
                **{k: np.ones((Np, 4)) for k in ("rx", "sx", "ry", "sy")},
                **{k: np.ones((nfn, 4)) for k in ("nx", "ny", "Fscale")}, "vmapP": np.zeros(nfn * 4, np.int32)}
        with pytest.raises(BdgError, match="order"):
            sw2dquads.Sw2dQuadSolver(tables=fake)
    with pytest.raises(BdgError):
        dg.QuadNodesProvisioner(0, mesh)
    # filtered modes need a Filter
    t2 = dict(t)
    t2["Filter"] = None
    s = sw2dquads.Sw2dQuadSolver(tables=t2)
    with pytest.raises(BdgError, match="Filter"):
        s.computeRHS(d["h"], d["hu"], d["hv"], filter=True)
