"""blitzdg_amd.poisson2d on the device (the two passes of csrc/hip/poisson2d_kernel.hpp and the conjugate-gradient loop of
csrc/hip/poisson2d_device.hip) against tests/poisson_ref.py.

The mesh is buildBoxMesh(13, 11) with a shuffled element order (poisson_ref.nodes_tables: K = 286, four full waves and a tail; the
solver renumbers it on the device), the operator's input jumps at every face.

  test_apply            A u at N = 1..8 for Dirichlet, Neumann and mixed mapD, with and without g / qn, with and without sigma,
                        scalar and per-element kappa: within APPLY_TOL = 1e-12 of max|A u| of the float64 reference (licensed by
                        tests/test_poisson_reference.py: float64 is within 2.5e-13 of longdouble); massDot within 1e-13 relative
  test_solve            N = 1, 4, 8, the three analytic problems plus one backward-Euler step, relTol 1e-10, checkEvery 8:
                        converged; the TRUE residual of the returned u, evaluated by poisson_ref in float64, over relTol is at
                        most 4 times what poisson_ref.cg attains on the same input; the iteration count is at most the NumPy
                        count plus 25 %, rounded up to a multiple of checkEvery
  then the mean of the singular case's solution, determinism bit for bit, the zero right-hand side, a renumbered against a
  KEEP_ORDER solver, backward Euler against explicit steps, and the refusals that need a device.

Measured by poisson_ref.cg (tests/test_poisson_reference.py prints them): iterations / true residual over relTol
  N   sin            cos            harmonic        euler
  1   112 / 0.524    144 / 0.230    192 / 0.307      48 / 0.110
  4   288 / 0.648    296 / 0.482    632 / 0.576     200 / 0.716
  8    32 / 0.620     32 / 0.632   1776 / 0.869     568 / 0.706
and the ratio of its true to its recursive residual lies in [0.9998, 1.0009].

Measured on one MI355X: the operator within 1.2e-13 of max|A u| (N = 8; 2.2e-14 at N = 4, 2.2e-16 at N = 1); the loop takes the
NumPy loop's iteration count on all twelve inputs, its true residual over relTol differs from NumPy's by at most 0.009 (N = 8,
harmonic: 0.878 against 0.869); mean of the singular solution 3.9e-18; renumbered against KEEP_ORDER 1.1e-13; backward Euler
1.230e-02 from the explicit steps (bound 1.2296e-02) and 2.2e-12 from the dense backward Euler; 29 tests in 2.7 s."""
import os
import sys

import numpy as np
import pytest

import poisson_ref as P
from blitzdg_amd import _capi as C
from blitzdg_amd import poisson2d

pytestmark = pytest.mark.gpu

APPLY_TOL = 1e-12
ORDERS = tuple(range(1, 9))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_solver(order, case, **kw):
    _, t = P.nodes_tables(order)
    return poisson2d.Poisson2dSolver(tables=t, mapD=case["mapD"], kappa=case["kappa"], shift=case["sigma"], **kw)


@pytest.mark.parametrize("order", ORDERS)
def test_apply(order):
    _, t = P.nodes_tables(order)
    u = P.jumping_field(t)
    interior = ~P.boundary_nodes(t)
    uC = u.flatten("F")
    assert np.abs(uC[t["vmapM"]] - uC[t["vmapP"]])[interior].min() > 0          # u jumps at every face
    v = P.jumping_field(t, seed=9)
    for name, case in P.operator_cases(order).items():
        s = make_solver(order, case)
        data = case["g"] is not None or case["qn"] is not None
        if data:
            s.setBoundaryData(case["g"], case["qn"])
        got = s.apply(u, withData=data)
        ref = P.apply(u, t, **case)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"N{order} {name}: |A u - ref| {err:.2e} of max|A u|")
        assert err <= APPLY_TOL, name
        if data:   # ... and the homogeneous operator is still there beside the data
            hom = dict(case, g=None, qn=None)
            ref0 = P.apply(u, t, **hom)
            assert np.abs(s.apply(u) - ref0).max() <= APPLY_TOL * np.abs(ref0).max(), name
        md, want = s.massDot(u, v), P.mass_dot(u, v, t)
        assert abs(md - want) <= 1e-13 * abs(want), (name, md, want)
        s.close()


@pytest.mark.parametrize("name", P.PROBLEMS)
@pytest.mark.parametrize("order", P.SOLVE_ORDERS)
def test_solve(order, name):
    _, t = P.nodes_tables(order)
    p = P.solve_problem(name, order)
    _, ref = P.reference_solve(name, order)
    assert ref["converged"]
    s = make_solver(order, p)
    s.setBoundaryData(p["g"], p["qn"])
    u, info = s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY)
    s.close()
    true = P.true_residual(u, p, t)
    limit = -(-int(np.ceil(1.25 * ref["iterations"])) // P.CHECK_EVERY) * P.CHECK_EVERY
    print(f"N{order} {name}: {info.iterations} iterations (NumPy {ref['iterations']}, limit {limit}), true residual / relTol "
          f"{true / P.REL_TOL:.3f} (NumPy {ref['trueres'] / P.REL_TOL:.3f}), recursive {info.relativeResidual / P.REL_TOL:.3f}")
    assert info.converged
    assert info.projected == (name == "cos")
    # the NumPy loop's own ratio of true residual to relTol is between 0.110 and 0.869 on these inputs (the docstring's table)
    assert true / P.REL_TOL <= 4 * ref["trueres"] / P.REL_TOL
    assert info.iterations <= limit
    if p["exact"] is not None and order == 8:
        ex = p["exact"] - (P.mass_mean(p["exact"], t) if info.projected else 0.0)
        assert np.abs(u - ex).max() <= 1e-6


def test_the_singular_solution_is_mean_free():
    _, t = P.nodes_tables(4)
    p = P.solve_problem("cos", 4)
    s = make_solver(4, p)
    u, info = s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY)
    s.close()
    assert info.projected and info.converged
    mean = P.mass_mean(u, t)
    print(f"mass-weighted mean {mean:.2e}, max|u| {np.abs(u).max():.3f}")
    assert abs(mean) <= 1e-12 * np.abs(u).max()


def test_two_solves_give_the_same_bits():
    p = P.solve_problem("euler", 4)
    out = []
    for _ in range(2):
        s = make_solver(4, p)
        s.setBoundaryData(p["g"], p["qn"])
        out.append(s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY))
        s.close()
    assert out[0][1] == out[1][1]
    assert np.array_equal(out[0][0], out[1][0])
    s = make_solver(4, p)
    s.setBoundaryData(p["g"], p["qn"])
    again = [s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY)[0] for _ in range(2)]   # ... and on one solver
    s.close()
    assert np.array_equal(again[0], again[1]) and np.array_equal(again[0], out[0][0])


@pytest.mark.parametrize("name", ("sin", "cos"))
def test_a_zero_right_hand_side_returns_zero_in_zero_iterations(name):
    p = P.solve_problem(name, 3)
    s = make_solver(3, p)
    u, info = s.solve(np.zeros_like(p["f"]), x0=np.ones_like(p["f"]))
    s.close()
    assert info.iterations == 0 and info.converged
    assert not u.any()


def test_a_renumbered_and_a_keep_order_solver_agree():
    _, t = P.nodes_tables(4)
    p = P.solve_problem("harmonic", 4)
    got = {}
    for label, flags in (("renumbered", poisson2d.REORDER), ("kept", poisson2d.KEEP_ORDER)):
        s = make_solver(4, p, flags=flags)
        s.setBoundaryData(p["g"], p["qn"])
        got[label] = s.solve(p["f"], relTol=1e-12, checkEvery=P.CHECK_EVERY)[0]
        s.close()
    err = np.abs(got["renumbered"] - got["kept"]).max() / np.abs(got["kept"]).max()
    print(f"renumbered against KEEP_ORDER: {err:.2e}")
    assert err <= 1e-11


def test_a_start_vector_is_used():
    """From the reference solution the first residual is already below the tolerance."""
    p = P.solve_problem("euler", 4)
    u0, _ = P.reference_solve("euler", 4)
    s = make_solver(4, p)
    s.setBoundaryData(p["g"], p["qn"])
    u, info = s.solve(p["f"], x0=u0, relTol=2e-10, checkEvery=P.CHECK_EVERY)
    s.close()
    assert info.iterations == 0 and info.converged and np.array_equal(u, u0)


def test_backward_euler_stays_within_the_first_order_error_of_explicit_steps():
    """Ten steps of examples/heat2d.py's loop at dt = 50 diffusionDt against 500 forward-Euler steps of the same operator in NumPy
    (poisson_ref.heat_reference, which also measures the bound with the dense operator: the sum of both schemes' errors against
    the exact exponential, tests/test_poisson_reference.py prints and records it)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import heat2d
    finally:
        sys.path.pop(0)
    h = P.heat_reference()
    t, p = h["tables"], h["problem"]
    s = poisson2d.Poisson2dSolver(tables=t, mapD=p["mapD"], kappa=p["kappa"], shift=0.0)
    s.setBoundaryData(p["g"], p["qn"])
    u, iters = heat2d.backward_euler_steps(s, h["start"], h["dt"], P.HEAT_STEPS, relTol=P.HEAT_REL_TOL)
    s.close()
    assert np.all(np.isfinite(u)) and np.abs(u).max() <= 1.5 * max(np.abs(h["start"]).max(), np.abs(p["g"]).max())   # bounded
    err = np.abs(u - h["explicit"]).max()
    print(f"backward Euler against 500 explicit steps: {err:.3e} (bound {h['bound']:.3e}), against the dense backward Euler "
          f"{np.abs(u - h['implicit']).max():.2e}; {sum(iters)} iterations")
    assert err <= h["bound"]


def test_refusals():
    _, t = P.nodes_tables(2)
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dSolver(tables=t, mapD=np.nonzero(~P.boundary_nodes(t))[0][:1])   # an interior face node
    assert e.value.code == C.BDG_ERR_ARGUMENT
    with pytest.raises(ValueError):
        poisson2d.Poisson2dSolver(tables=t, kappa=np.ones_like(t["x"]))
    for bad in (dict(kappa=-1.0), dict(kappa=np.zeros(t["x"].shape[1])), dict(shift=-0.1), dict(flags=poisson2d.NODAL_GEOMETRY)):
        with pytest.raises(C.BdgError) as e:
            poisson2d.Poisson2dSolver(tables=t, **bad)
        assert e.value.code == C.BDG_ERR_ARGUMENT
    s = poisson2d.Poisson2dSolver(tables=t, mapD=P.all_boundary(t))
    before = s.deviceBytes()
    assert before > 0
    with pytest.raises(C.BdgError):
        s.setShift(-1.0)
    with pytest.raises(C.BdgError):
        s.solve(np.ones_like(t["x"]), relTol=0.0)
    s.setBoundaryData(*P.face_data(t))
    assert s.deviceBytes() == before + 2 * 8 * 9 * 64 * ((t["x"].shape[1] + 63) // 64)
    s.close()


def test_default_dirichlet_nodes_from_a_provisioner_are_the_walls():
    nodes, t = P.nodes_tables(3)
    p = P.solve_problem("sin", 3)
    a = poisson2d.Poisson2dSolver(nodes=nodes)
    b = poisson2d.Poisson2dSolver(tables=t, mapD=P.all_boundary(t))
    u = P.jumping_field(t)
    assert sorted(t["BCmap"][3]) == sorted(P.all_boundary(t))
    assert np.array_equal(a.apply(u), b.apply(u))
    assert np.abs(a.apply(u) - P.apply(u, t, p["mapD"])).max() <= APPLY_TOL * np.abs(a.apply(u)).max()
    a.close()
    b.close()
