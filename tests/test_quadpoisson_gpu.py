"""blitzdg_amd.poisson2d.Poisson2dQuadSolver on the device (the passes of csrc/hip/poisson2d_quad_kernel.hpp behind the
conjugate-gradient loop of csrc/hip/poisson2d_device.hip) against tests/poisson_ref.py on the quadrilateral tables of
tests/quadpoisson_ref.py.

The mesh is quadref_ld's shear mesh: the 13 x 11 box, shuffled, every element's vertex order rotated, sheared so that all four
metric terms are nonzero; K = 143 is tiles of 64, 32, 16 and 8 elements plus a tail. The operator's input jumps at every face.

  test_apply            A u at N = 1..12 for the six cases of poisson_ref.operator_cases (Dirichlet, Neumann and mixed mapD, with
                        and without g / qn, with and without sigma, scalar and per-element kappa): within
                        quadpoisson_ref.apply_tolerance(N) = max(1e-12, 8 x the distance of float64 NumPy from np.longdouble) of
                        max|A u| -- 1e-12 at every order, tests/test_quadpoisson_reference.py records the distances --; the
                        homogeneous operator intact beside the data; massDot within 1e-13 relative
  test_solve            N = 1, 4, 8, 12, relTol 1e-10, checkEvery 8: harmonic and euler on the shear mesh with data, sin and cos
                        (singular, projected) on the box of rectangles; at N = 12 the meshes are 6 x 5 (K = 30), because
                        poisson_ref.cg needs more than ten seconds on 13 x 11 there. Converged; the TRUE residual of the returned
                        u over relTol at most 4 times what poisson_ref.cg attains; iterations at most NumPy's plus 25 %, rounded
                        up to a multiple of checkEvery
  then the mean of the singular solution, determinism bit for bit, the zero right-hand side, a REORDER against a KEEP_ORDER
  solver, backward Euler against explicit steps (quadpoisson_ref.heat_reference), and the refusals.

Measured by poisson_ref.cg (tests/test_quadpoisson_reference.py prints them): iterations / true residual over relTol
  N    sin             cos             harmonic        euler
  1      8 / 3.0e-05     8 / 3.0e-05    160 / 0.535      40 / 0.360
  4     16 / 0.140      16 / 0.141      848 / 0.742     216 / 0.498
  8      8 / 0.035       8 / 0.033     2488 / 0.831     624 / 0.702
  12     8 / 2.9e-03     8 / 2.6e-03   2192 / 0.819     560 / 0.683      (6 x 5 meshes)

Measured on one MI355X: the operator within 2.1e-13 of max|A u| (N = 12; 1.5e-13 at N = 8, 1.9e-14 at N = 4, 8.3e-16 at N = 1);
massDot within 2.3e-14; the loop takes the NumPy loop's iteration count on fourteen of the sixteen inputs and 8 fewer at N = 12
(harmonic 2184, euler 552), its true residual over relTol is 0.93 to 2.73 times NumPy's (the largest: N = 12 cos, 6.98e-03
against 2.56e-03; N = 12 euler 0.912 against 0.683); mean of the singular solution 1.1e-16; REORDER against KEEP_ORDER 5.1e-13;
backward Euler 1.327e-02 from the explicit steps (bound 1.327e-02) and 7.4e-13 from the dense backward Euler; 37 tests in 6.0 s."""
import os
import sys

import numpy as np
import pytest

import poisson_ref as P
import quadpoisson_ref as Q
from blitzdg_amd import _capi as C
from blitzdg_amd import poisson2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_solver(t, case, **kw):
    return poisson2d.Poisson2dQuadSolver(tables=t, mapD=case["mapD"], kappa=case["kappa"], shift=case["sigma"], **kw)


@pytest.mark.parametrize("order", Q.ORDERS)
def test_apply(order):
    t = Q.mesh_tables("shear", order)[1]
    tol = Q.apply_tolerance(order)
    u = P.jumping_field(t)
    interior = ~P.boundary_nodes(t)
    uC = u.flatten("F")
    assert np.abs(uC[t["vmapM"]] - uC[t["vmapP"]])[interior].min() > 0          # u jumps at every face
    assert min(np.abs(t[k]).min() for k in ("rx", "sx", "ry", "sy")) > 0.1      # all four metric terms count
    v = P.jumping_field(t, seed=9)
    for name, case in Q.operator_cases(t).items():
        s = make_solver(t, case)
        data = case["g"] is not None or case["qn"] is not None
        if data:
            s.setBoundaryData(case["g"], case["qn"])
        got = s.apply(u, withData=data)
        ref = P.apply(u, t, **case)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"N{order} {name}: |A u - ref| {err:.2e} of max|A u| (tolerance {tol:.1e})")
        assert err <= tol, name
        if data:   # ... and the homogeneous operator is still there beside the data
            ref0 = P.apply(u, t, **dict(case, g=None, qn=None))
            assert np.abs(s.apply(u) - ref0).max() <= tol * np.abs(ref0).max(), name
        md, want = s.massDot(u, v), P.mass_dot(u, v, t)
        print(f"N{order} {name}: massDot off by {abs(md - want) / abs(want):.2e}")
        assert abs(md - want) <= 1e-13 * abs(want), (name, md, want)
        s.close()


@pytest.mark.parametrize("name", P.PROBLEMS)
@pytest.mark.parametrize("order", Q.SOLVE_ORDERS)
def test_solve(order, name):
    t = Q.solve_mesh(name, order)
    p, _, ref = Q.reference_solve(name, order)
    assert ref["converged"]
    s = make_solver(t, p)
    s.setBoundaryData(p["g"], p["qn"])
    u, info = s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY)
    s.close()
    true = P.true_residual(u, p, t)
    limit = -(-int(np.ceil(1.25 * ref["iterations"])) // P.CHECK_EVERY) * P.CHECK_EVERY
    print(f"N{order} {name}: {info.iterations} iterations (NumPy {ref['iterations']}, limit {limit}), true residual / relTol "
          f"{true / P.REL_TOL:.3e} (NumPy {ref['trueres'] / P.REL_TOL:.3e}), recursive {info.relativeResidual / P.REL_TOL:.3e}")
    assert info.converged
    assert info.projected == (name == "cos")
    assert true / P.REL_TOL <= 4 * ref["trueres"] / P.REL_TOL
    assert info.iterations <= limit
    if p["exact"] is not None and order >= 8:
        ex = p["exact"] - (P.mass_mean(p["exact"], t) if info.projected else 0.0)
        assert np.abs(u - ex).max() <= 1e-6


def test_the_singular_solution_is_mean_free():
    t = Q.solve_mesh("cos", 4)
    p = Q.reference_solve("cos", 4)[0]
    s = make_solver(t, p)
    u, info = s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY)
    s.close()
    assert info.projected and info.converged
    mean = P.mass_mean(u, t)
    print(f"mass-weighted mean {mean:.2e}, max|u| {np.abs(u).max():.3f}")
    assert abs(mean) <= 1e-12 * np.abs(u).max()


def test_two_solves_give_the_same_bits():
    t = Q.solve_mesh("euler", 4)
    p = Q.reference_solve("euler", 4)[0]
    out = []
    for _ in range(2):
        s = make_solver(t, p)
        s.setBoundaryData(p["g"], p["qn"])
        out.append(s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY))
        s.close()
    assert out[0][1] == out[1][1]
    assert np.array_equal(out[0][0], out[1][0])
    s = make_solver(t, p)
    s.setBoundaryData(p["g"], p["qn"])
    again = [s.solve(p["f"], relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY)[0] for _ in range(2)]   # ... and on one solver
    s.close()
    assert np.array_equal(again[0], again[1]) and np.array_equal(again[0], out[0][0])


@pytest.mark.parametrize("name", ("sin", "cos"))
def test_a_zero_right_hand_side_returns_zero_in_zero_iterations(name):
    t = Q.mesh_tables("rect", 3)[1]
    p = Q.analytic_problem(name, t)
    s = make_solver(t, p)
    u, info = s.solve(np.zeros_like(p["f"]), x0=np.ones_like(p["f"]))
    s.close()
    assert info.iterations == 0 and info.converged
    assert not u.any()


def test_a_reorder_and_a_keep_order_solver_agree():
    """As on triangles: both solved to 1e-12, so they differ by the operator's rounding (1e-12 of max|A u|) times the conditioning
    the solve to 1e-12 already has to overcome: 1e-11 of max|u|."""
    t = Q.solve_mesh("harmonic", 4)
    p = Q.reference_solve("harmonic", 4)[0]
    got = {}
    for label, flags in (("renumbered", poisson2d.REORDER), ("kept", poisson2d.KEEP_ORDER)):
        s = make_solver(t, p, flags=flags)
        s.setBoundaryData(p["g"], p["qn"])
        got[label] = s.solve(p["f"], relTol=1e-12, checkEvery=P.CHECK_EVERY)[0]
        s.close()
    err = np.abs(got["renumbered"] - got["kept"]).max() / np.abs(got["kept"]).max()
    print(f"REORDER against KEEP_ORDER: {err:.2e}")
    assert err <= 1e-11
    s = make_solver(t, p)                                                  # the default keeps the caller's order
    s.setBoundaryData(p["g"], p["qn"])
    assert np.array_equal(s.solve(p["f"], relTol=1e-12, checkEvery=P.CHECK_EVERY)[0], got["kept"])
    s.close()


def test_backward_euler_stays_within_the_first_order_error_of_explicit_steps():
    """Ten steps of examples/heat2d.py's loop at dt = 50 explicit steps against 500 forward-Euler steps of the same operator in
    NumPy (quadpoisson_ref.heat_reference: poisson_ref.heat_reference's bound rebuilt on the 5 x 4 sheared box at N = 3)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import heat2d
    finally:
        sys.path.pop(0)
    h = Q.heat_reference()
    t, p = h["tables"], h["problem"]
    s = poisson2d.Poisson2dQuadSolver(tables=t, mapD=p["mapD"], kappa=p["kappa"], shift=0.0)
    s.setBoundaryData(p["g"], p["qn"])
    u, iters = heat2d.backward_euler_steps(s, h["start"], h["dt"], P.HEAT_STEPS, relTol=P.HEAT_REL_TOL)
    s.close()
    assert np.all(np.isfinite(u)) and np.abs(u).max() <= 1.5 * max(np.abs(h["start"]).max(), np.abs(p["g"]).max())   # bounded
    err = np.abs(u - h["explicit"]).max()
    print(f"backward Euler against 500 explicit steps: {err:.3e} (bound {h['bound']:.3e}), against the dense backward Euler "
          f"{np.abs(u - h['implicit']).max():.2e}; {sum(iters)} iterations")
    assert err <= h["bound"]


def test_refusals():
    tj = Q.mesh_tables("jitter", 2)[1]
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(tables=tj, mapD=P.all_boundary(tj))                       # general bilinear elements
    assert e.value.code == C.BDG_ERR_ARGUMENT and "parallelogram" in str(e.value)
    nodes, t = Q.mesh_tables("shear", 2)
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(tables=t, mapD=np.nonzero(~P.boundary_nodes(t))[0][:1])   # an interior face node
    assert e.value.code == C.BDG_ERR_ARGUMENT
    with pytest.raises(ValueError):
        poisson2d.Poisson2dQuadSolver(tables=t, kappa=np.ones_like(t["x"]))                     # a nodal kappa
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(nodes=Q.mesh_tables("shear", 13, 3, 2)[0])                # order 13
    assert e.value.code == C.BDG_ERR_ARGUMENT
    for bad in (dict(kappa=-1.0), dict(kappa=np.zeros(t["x"].shape[1])), dict(shift=-0.1), dict(flags=poisson2d.NODAL_GEOMETRY)):
        with pytest.raises(C.BdgError) as e:
            poisson2d.Poisson2dQuadSolver(tables=t, **bad)
        assert e.value.code == C.BDG_ERR_ARGUMENT
    s = poisson2d.Poisson2dQuadSolver(tables=t, mapD=P.all_boundary(t))
    before = s.deviceBytes()
    assert before > 0
    with pytest.raises(C.BdgError):
        s.setShift(-1.0)
    with pytest.raises(C.BdgError):
        s.solve(np.ones_like(t["x"]), relTol=0.0)
    s.setBoundaryData(*P.face_data(t))
    assert s.deviceBytes() == before + 2 * 8 * 12 * 64 * ((t["x"].shape[1] + 63) // 64)       # two (4 Nfp, ld) planes
    s.close()


def test_default_dirichlet_nodes_from_a_provisioner_are_the_walls():
    nodes, t = Q.mesh_tables("shear", 3)
    a = poisson2d.Poisson2dQuadSolver(nodes=nodes)
    b = poisson2d.Poisson2dQuadSolver(tables=t, mapD=P.all_boundary(t))
    u = P.jumping_field(t)
    assert sorted(t["BCmap"][3]) == sorted(P.all_boundary(t))
    assert np.array_equal(a.apply(u), b.apply(u))
    assert np.abs(a.apply(u) - P.apply(u, t, P.all_boundary(t))).max() <= Q.apply_tolerance(3) * np.abs(a.apply(u)).max()
    a.close()
    b.close()


def test_the_triangle_solver_is_unchanged_beside_a_quadrilateral_one():
    """Both families live behind one handle type: a triangle solver created and used between quadrilateral ones gives the bits
    it gives alone."""
    _, tt = P.nodes_tables(3)
    ut = P.jumping_field(tt)
    alone = poisson2d.Poisson2dSolver(tables=tt, mapD=P.all_boundary(tt))
    want = alone.apply(ut)
    alone.close()
    t = Q.mesh_tables("shear", 3)[1]
    q = poisson2d.Poisson2dQuadSolver(tables=t, mapD=P.all_boundary(t))
    tri = poisson2d.Poisson2dSolver(tables=tt, mapD=P.all_boundary(tt))
    q.apply(P.jumping_field(t))
    assert np.array_equal(tri.apply(ut), want)
    q.close()
    tri.close()
