"""tests/triviscosity_ref.py, the definition of the eddy viscosity on triangles, held to its own properties in float64 and
np.longdouble. No GPU.

  * uniform flow over a varying depth: T_u = T_v = 0 to the rounding bound of the tracer's uniform-concentration test;
  * u = y^2, v = 0 with h and nu0 constant, Cs = 0, order >= 2: T_u = 2 nu0 h in every element without a boundary face, to 1e-10
    relative in the longdouble evaluation;
  * rigid rotation (u, v) = (-y, x): nu = nu0; pure strain (u, v) = (x, -y): nu = nu0 + 2 Cs^2 D^2 in every element without a
    boundary face, to 1e-10 relative in longdouble;
  * momentum conservation: for a velocity that jumps at every face, Smagorinsky on, sum(w T_u) = sum(w T_v) = 0 to 1e-12 of
    sum(w |T|), on buildBoxMesh(13, 11) and on a shuffled copy;
  * dissipation: with h = 1 and a fixed positive (smooth) nu field <u, T_u> + <v, T_v> <= 1e-9 rho |u|^2 in the mass inner
    product (sym(M A) has no eigenvalue above 1e-9 rho against M), N = 1..8, on the 24-element box and on its distorted copy;
  * the constant c of dt_visc = c / (nu_max (N+1)^4 max(Fscale)^2): with nu frozen at the Smagorinsky field of the GPU test's
    velocity, dt_visc rho <= 2 at every order on both meshes;
  * float64 against longdouble on the GPU test's inputs stays within LD_TOL = 2.5e-13 of the field's maximum (T_u, T_v, nu),
    which licenses holding the GPU to the project's 1e-12 / 1e-11.

Measured with the nodal nu (rho of the dense operator on the 4 x 3 box / its distorted copy, and the largest c that would still
satisfy the inequality, 2 / (rho dt_visc(c = 1))):
  N    rho box    rho distorted   c <= (box)   c <= (distorted)
  1   5.782e+01    1.078e+02        6.27          19.61
  2   1.323e+02    2.951e+02       12.61          34.21
  3   3.533e+02    9.678e+02       14.71          30.67
  4   7.938e+02    1.959e+03       17.63          39.12
  5   1.742e+03    3.035e+03       16.94          53.41
  6   3.155e+03    5.546e+03       17.17          54.32
  7   4.514e+03    8.892e+03       20.83          60.39
  8   7.401e+03    1.716e+04       27.26          61.90
so the tracer's c = 4 holds for a nodal viscosity as well (triviscosity_ref.DT_CONSTANT, bdg_sw2d::kViscosityDtConstant): nu
reaches its maximum at a few nodes only, which lowers rho against the constant-nu operator. With the smooth field the largest
<u, T_u> / |u|^2 found is 7.4e-14 (rho 7.1e+02). With the Smagorinsky field of a velocity that is noise at every node the
collocated product nu q is no longer dissipative in the mass norm at N = 8 (3.6e+01 against rho 7.4e+03 on the box): the
dissipation test takes the smooth field, and the step-size bound, which is about rho alone, takes the noisy one. float64 against
longdouble: at most 1.0e-15 of the field's maximum (N = 8). The other measured figures are printed by the tests and recorded
in DESIGN.md 3.7."""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import tridiff_ref as R
import triviscosity_ref as V
from conftest import tables_from_nodes
from quadref_ld import require_extended_precision
from test_quadB_reference import LD_TOL

ORDERS = tuple(range(1, 9))
EPS = np.finfo(np.float64).eps


def tables(order, mesh, filt=True):
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    if filt:
        nodes.buildFilter(0.9 * order, order)
    return nodes, tables_from_nodes(nodes)


def depth(t):
    return 11.0 + 1.5 * t["x"] - 0.8 * t["y"] ** 2


def inner_elements(t):
    bnd = R.boundary_nodes(t).reshape(t["nx"].shape, order="F").any(axis=0)
    assert 0 < bnd.sum() < bnd.size
    return ~bnd


@pytest.mark.parametrize("order", (1, 3, 6, 8))
def test_the_jacobian_of_the_definition_is_the_provisioners(order):
    nodes, t = tables(order, R.distorted_box(4, 3))
    J = nodes.dgContext().J
    assert np.abs(V.jacobian(t) - J).max() <= 1e-13 * np.abs(J).max()


@pytest.mark.parametrize("order", (1, 3, 6, 8))
def test_uniform_flow_has_no_viscous_term(order):
    """The gradient of a constant is rounding: two differentiations amplify eps c by at most |D|^2 ~ ((N+1)^2 max Fscale)^2, so
    |T| <= 64 eps nu h c (N+1)^4 max(Fscale)^2 (the bound of test_a_uniform_concentration...), with nu the largest nodal value."""
    _, t = tables(order, R.box(5, 4))
    h, cu, cv = depth(t), 0.37, -0.21
    nu0 = V.nu_field(t)
    nu = V.eddy_viscosity(h, cu * h, cv * h, nu0, V.SMAGORINSKY, t)
    Tu, Tv = V.viscous_terms(h, cu * h, cv * h, nu0, V.SMAGORINSKY, t)
    for T, c in ((Tu, cu), (Tv, cv)):
        bound = 64 * EPS * nu.max() * h.max() * abs(c) * (order + 1) ** 4 * np.abs(t["Fscale"]).max() ** 2
        err = np.abs(T).max()
        print(f"N{order}: |T| {err:.2e} (bound {bound:.2e})")
        assert err <= bound


@pytest.mark.parametrize("order", range(2, 9))
def test_quadratic_flow_has_a_constant_term(order):
    require_extended_precision()
    _, t = tables(order, R.box(5, 4))
    tl = R.to_ld(t)
    y = tl["y"]
    h0, nu0 = R.LD(7.5), R.LD(0.03)
    h = np.full(y.shape, h0)
    Tu, Tv = V.viscous_terms(h, h * y * y, np.zeros_like(h), nu0, 0.0, tl)
    inner = inner_elements(t)
    want = 2 * nu0 * h0
    err = float(np.abs(Tu[:, inner] - want).max() / want)
    print(f"N{order}: |T_u - 2 nu0 h| / (2 nu0 h) {err:.2e} in {int(inner.sum())} elements without a boundary face")
    assert err <= 1e-10 and np.abs(Tv).max() == 0
    assert np.abs(Tu[:, ~inner] - want).max() > 1e-3 * want       # ... and the zero stress shows in the others


@pytest.mark.parametrize("order", ORDERS)
def test_rotation_has_no_strain_and_pure_strain_has_two(order):
    require_extended_precision()
    _, t = tables(order, R.distorted_box(5, 4))
    tl = R.to_ld(t)
    x, y = tl["x"], tl["y"]
    h = depth(tl)
    nu0, cs = R.LD(0.03), R.LD(0.7)
    inner = inner_elements(t)
    rot = V.eddy_viscosity(h, -y * h, x * h, nu0, cs, tl)
    assert float(np.abs(rot[:, inner] - nu0).max() / nu0) <= 1e-10
    strain = V.eddy_viscosity(h, x * h, -y * h, nu0, cs, tl)
    want = nu0 + 2 * cs * cs * 2 * V.jacobian(tl) / R.LD(order + 1) ** 2
    err = float(np.abs(strain / want - 1)[:, inner].max())
    print(f"N{order}: |nu / (nu0 + 2 Cs^2 D^2) - 1| {err:.2e}; the term is {float((want / nu0 - 1).max()):.2e} of nu0")
    assert err <= 1e-10 and float((want - nu0).min()) > 1e-3 * float(nu0)


@pytest.mark.parametrize("seed", (0, 11), ids=("box13x11", "shuffled"))
@pytest.mark.parametrize("order", (1, 4, 8))
def test_momentum_is_conserved(order, seed):
    nodes, t, _, q, _, d = V.inputs(order, seed=seed)
    w = np.asarray(nodes.quadratureWeights())
    h = q[0]
    u, v = V.jumping_velocity(t)
    interior = ~R.boundary_nodes(t)
    for a in (u, v):
        aC = a.flatten("F")
        assert np.abs(aC[t["vmapM"]] - aC[t["vmapP"]])[interior].min() > 0          # the velocity jumps at every face
    nu = V.eddy_viscosity(h, h * u, h * v, d["nu_field"], d["smagorinsky"], t)
    assert (nu - d["nu_field"]).max() > 0.1 * d["nu_field"].max()                   # Smagorinsky is on and shows
    for T in V.viscous_terms(h, h * u, h * v, d["nu_field"], d["smagorinsky"], t):
        got, scale = (w * T).sum(), (w * np.abs(T)).sum()
        print(f"N{order} seed {seed}: sum(w T) = {abs(got) / scale:.2e} of sum(w |T|)")
        assert abs(got) <= 1e-12 * scale


def frozen_problem(order, mesh):
    """(nodes, tables, nu): the GPU test's state (trirefB4.problem, as tridiff_ref.inputs builds it) on the 4 x 3 box or its
    distorted copy, and its Smagorinsky field."""
    import trirefB4
    nodes, t, _, q, _ = trirefB4.problem(order, R.box(4, 3) if mesh == "box" else R.distorted_box(4, 3), seed=order)
    return nodes, t, V.eddy_viscosity(*q[:3], V.nu_field(t), V.SMAGORINSKY, t)


@pytest.mark.parametrize("mesh", ("box", "distorted"))
@pytest.mark.parametrize("order", ORDERS)
def test_the_operator_dissipates(order, mesh):
    """h = 1 and the fixed positive field nu_field: <u, T_u> = u^T M A u = u^T sym(M A) u <= lambda |u|_M^2 with lambda the largest
    eigenvalue of sym(M A) against M -- with M = L L^T that of L^-1 sym(M A) L^-T. T_v has the same operator."""
    nodes, t = tables(order, R.box(4, 3) if mesh == "box" else R.distorted_box(4, 3), filt=False)
    assert t["rx"].shape[1] == 24
    nu = V.nu_field(t)
    assert nu.min() > 0 and np.ptp(nu) > 0.5 * nu.min()
    A = V.dense_operator(t, nu)
    M = R.mass_matrix(nodes)
    MA = M @ A
    rho = np.abs(np.linalg.eigvals(A)).max()
    Linv = np.linalg.inv(np.linalg.cholesky(M))
    top = np.linalg.eigvalsh(Linv @ (0.5 * (MA + MA.T)) @ Linv.T).max()
    print(f"N{order} {mesh}: rho {rho:.4e}, largest <u, T_u> / |u|^2 {top:.2e}")
    assert top <= 1e-9 * rho


@pytest.mark.parametrize("mesh", ("box", "distorted"))
@pytest.mark.parametrize("order", ORDERS)
def test_the_dt_constant_holds_for_a_nodal_viscosity(order, mesh):
    nodes, t, nu = frozen_problem(order, mesh)
    assert t["rx"].shape[1] == 24
    assert nu.min() > 0 and nu.max() > 2 * nu.min()                                  # a nodal field, far from constant
    rho = np.abs(np.linalg.eigvals(V.dense_operator(t, nu))).max()
    dt1 = V.viscosity_dt(nu.max(), order, t, c=1.0)
    print(f"N{order} {mesh}: rho {rho:.4e}, max nu {nu.max():.3e}, largest admissible constant {2.0 / (rho * dt1):.2f}")
    assert V.viscosity_dt(nu.max(), order, t) * rho <= 2.0


@pytest.mark.parametrize("order", ORDERS)
def test_float64_is_within_a_quarter_of_the_gpu_tolerance(order):
    require_extended_precision()
    _, t, _, q, _, d = V.inputs(order)
    h, hu, hv = q[:3]
    worst = 0.0
    for nu0, cs in ((d["nu"], 0.0), (d["nu_field"], 0.0), (d["nu_field"], d["smagorinsky"])):
        got = [V.eddy_viscosity(h, hu, hv, nu0, cs, t)]
        ref = [V.eddy_viscosity_ld(h, hu, hv, nu0, cs, t)]
        for filt in (False, True):
            got += V.viscous_terms(h, hu, hv, nu0, cs, t, filt)
            ref += V.viscous_terms_ld(h, hu, hv, nu0, cs, t, filt)
        for a, b in zip(got, ref):
            assert b.dtype == R.LD and np.all(np.isfinite(a))
            worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    print(f"N{order}: float64 against longdouble {worst:.2e} of the field's maximum")
    assert worst <= LD_TOL


def test_smagorinsky_shows_on_the_gpu_tests_input():
    for order in ORDERS:
        _, t, _, q, _, d = V.inputs(order)
        nu = V.eddy_viscosity(*q[:3], d["nu_field"], d["smagorinsky"], t)
        assert (nu - d["nu_field"]).max() >= d["nu_field"].max()


def test_null_handles_are_refused_without_a_gpu():
    from blitzdg_amd import _capi as C
    d = C.Sw2dViscosityDesc(0.1, None, 0.0)
    assert C.lib.bdg_sw2d_enable_viscosity(None, ctypes.byref(d)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2d_enable_viscosity(None, None) == C.BDG_ERR_ARGUMENT
    v = ctypes.c_double()
    assert C.lib.bdg_sw2d_viscosity_dt(None, ctypes.byref(v)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2d_eddy_viscosity(None, None) == C.BDG_ERR_ARGUMENT
