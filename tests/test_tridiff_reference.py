"""tests/tridiff_ref.py, the definition of the tracer's diffusion, source and decay on triangles, held to its own properties in
float64 and np.longdouble. No GPU.

  * a uniform concentration: T = S - k hN to rounding;
  * N = x^2 with h and kappa constant, order >= 2: the gradient is exact everywhere and T = 2 kappa h in every element without a
    boundary face, to 1e-10 relative in the longdouble evaluation;
  * conservation: for a tracer that jumps at every face sum(w T) = sum(w (S - k hN)) to 1e-12 of sum(w |T|), on
    buildBoxMesh(13, 11) and on a shuffled copy;
  * with h = 1 and S = k = 0 the dense operator on a 24-element box is symmetric negative semi-definite in the mass inner
    product at N = 1..8 (eigenvalues <= 1e-9 rho), on the box and on a distorted copy of it;
  * the constant c of dt_diff = c / (kappa (N+1)^4 max(Fscale)^2) keeps dt_diff <= 2 / rho at every order on both;
  * float64 against longdouble on the GPU test's inputs stays within LD_TOL = 2.5e-13 of max|T|, which licenses holding the GPU
    to 1e-12 against the float64 evaluation;
  * cos(pi (x + 1) / 2) in the closed box against its analytic Laplacian: the error of T decreases strictly over N = 2, 4, 6.

Measured (rho on the 4 x 3 box / its distorted copy, and the largest c that would still satisfy the inequality):
  N    rho box    rho distorted   c <= (box)   c <= (distorted)
  1   1.858e+02    3.908e+02        4.30          10.78
  2   6.066e+02    1.430e+03        6.68          14.91
  3   1.456e+03    3.556e+03        8.79          18.95
  4   3.021e+03    7.414e+03       10.34          22.19
  5   5.615e+03    1.381e+04       11.54          24.70
  6   9.620e+03    2.383e+04       12.48          26.52
  7   1.551e+04    3.851e+04       13.20          28.00
  8   2.375e+04    5.940e+04       13.81          29.08
so c = 4 (tridiff_ref.DT_CONSTANT, bdg_sw2d::kDiffusionDtConstant); the largest eigenvalue found is 2.5e-11 (rho 3.9e+04), the
largest asymmetry of M A 2.3e-14 of max|M A|. The other measured figures are printed by the tests and recorded in DESIGN.md 3.7."""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import tridiff_ref as R
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


@pytest.mark.parametrize("order", (1, 3, 6, 8))
def test_a_uniform_concentration_leaves_source_and_decay(order):
    """The gradient of a constant is rounding: two differentiations amplify eps c by at most |D|^2 ~ ((N+1)^2 max Fscale)^2, so
    |T - (S - k hN)| <= 64 eps kappa h c (N+1)^4 max(Fscale)^2."""
    _, t = tables(order, R.box(5, 4))
    h, c = depth(t), 0.37
    kap, S = R.kappa_field(t), R.source_field(t)
    T = R.diffusion_term(h, c * h, kap, t, S, R.DECAY)
    bound = 64 * EPS * kap.max() * h.max() * c * (order + 1) ** 4 * np.abs(t["Fscale"]).max() ** 2
    err = np.abs(T - (S - R.DECAY * c * h)).max()
    print(f"N{order}: |T - (S - k hN)| {err:.2e} (bound {bound:.2e})")
    assert err <= bound


@pytest.mark.parametrize("order", range(2, 9))
def test_quadratic_tracer_has_an_exact_gradient_and_a_constant_term(order):
    require_extended_precision()
    _, t = tables(order, R.box(5, 4))
    tl = R.to_ld(t)
    x = tl["x"]
    h0, kap = R.LD(7.5), R.LD(0.03)
    h = np.full(x.shape, h0)
    fx, fy = R.gradient_flux(h, h * x * x, kap, tl)
    scale = float(kap * h0 * 2)
    assert np.abs(fx - kap * h0 * 2 * x).max() <= 1e-10 * scale and np.abs(fy).max() <= 1e-10 * scale     # q is exact everywhere
    T = R.diffusion_term(h, h * x * x, kap, tl)
    bnd = R.boundary_nodes(t).reshape(t["nx"].shape, order="F").any(axis=0)
    assert 0 < bnd.sum() < bnd.size
    want = 2 * kap * h0
    err = float(np.abs(T[:, ~bnd] - want).max() / want)
    print(f"N{order}: |T - 2 kappa h| / (2 kappa h) {err:.2e} in {int((~bnd).sum())} elements without a boundary face")
    assert err <= 1e-10
    assert np.abs(T[:, bnd] - want).max() > 1e-3 * want          # ... and the zero normal flux shows in the others


@pytest.mark.parametrize("seed", (0, 11), ids=("box13x11", "shuffled"))
@pytest.mark.parametrize("order", (1, 4, 8))
def test_the_operator_is_conservative(order, seed):
    nodes, t, _, q, _, d = R.inputs(order, seed=seed)
    w = np.asarray(nodes.quadratureWeights())
    h, hN = q[0], q[3]
    N = (hN / h).flatten("F")
    interior = ~R.boundary_nodes(t)
    assert np.abs(N[t["vmapM"]] - N[t["vmapP"]])[interior].min() > 0             # the tracer jumps at every face
    for kap in (d["kappa_field"], d["kappa"]):
        T = R.diffusion_term(h, hN, kap, t, d["source"], d["decay"])
        got, want = (w * T).sum(), (w * (d["source"] - d["decay"] * hN)).sum()
        scale = (w * np.abs(T)).sum()
        print(f"N{order} seed {seed}: sum(w T) - sum(w (S - k hN)) = {abs(got - want) / scale:.2e} of sum(w |T|)")
        assert abs(got - want) <= 1e-12 * scale


@pytest.mark.parametrize("mesh", ("box", "distorted"))
@pytest.mark.parametrize("order", ORDERS)
def test_the_operator_is_negative_semi_definite_and_the_dt_constant_holds(order, mesh):
    nodes, t = tables(order, R.box(4, 3) if mesh == "box" else R.distorted_box(4, 3), filt=False)
    assert t["rx"].shape[1] == 24
    if mesh == "distorted":
        assert np.ptp(np.abs(t["Fscale"])) > 0.5 * np.abs(t["Fscale"]).min()
    A = R.dense_operator(t)
    MA = R.mass_matrix(nodes) @ A
    asym = np.abs(MA - MA.T).max() / np.abs(MA).max()
    ev = np.linalg.eigvals(A)
    rho = np.abs(ev).max()
    dt = R.diffusion_dt(R.DT_CONSTANT, 1.0, order, t)
    print(f"N{order} {mesh}: rho {rho:.4e}, largest eigenvalue {ev.real.max():.2e}, asymmetry {asym:.1e}, dt_diff rho / 2 = {dt * rho / 2:.3f}")
    assert asym <= 1e-12
    assert np.abs(ev.imag).max() <= 1e-9 * rho and ev.real.max() <= 1e-9 * rho
    assert dt <= 2.0 / rho


@pytest.mark.parametrize("order", ORDERS)
def test_float64_is_within_a_quarter_of_the_gpu_tolerance(order):
    require_extended_precision()
    _, t, _, q, _, d = R.inputs(order)
    h, hN = q[0], q[3]
    worst = 0.0
    for kap in (d["kappa_field"], d["kappa"]):
        for filt in (False, True):
            got = R.diffusion_term(h, hN, kap, t, d["source"], d["decay"], filt)
            ref = R.diffusion_term_ld(h, hN, kap, t, d["source"], d["decay"], filt)
            assert ref.dtype == R.LD and np.all(np.isfinite(got))
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"N{order}: float64 against longdouble {worst:.2e} of max|T|")
    assert worst <= LD_TOL


def test_the_error_against_the_analytic_laplacian_decreases_with_the_order():
    """N = cos(pi (x + 1) / 2) has zero normal derivative on all four sides of [-1, 1]^2; h = 1, kappa = 1."""
    errs = {}
    for order in (2, 4, 6):
        _, t = tables(order, R.box(4, 3), filt=False)
        N = np.cos(np.pi * (t["x"] + 1) / 2)
        T = R.diffusion_term(np.ones_like(N), N, 1.0, t)
        errs[order] = np.abs(T + (np.pi / 2) ** 2 * N).max()
    print("max|T - laplacian|: " + ", ".join(f"N{n} {e:.3e}" for n, e in errs.items()))
    assert errs[2] > errs[4] > errs[6]


def test_null_handles_are_refused_without_a_gpu():
    from blitzdg_amd import _capi as C
    d = C.Sw2dDiffusionDesc(0.1, None, None, 0.0)
    assert C.lib.bdg_sw2d_enable_tracer_diffusion(None, ctypes.byref(d)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2d_enable_tracer_diffusion(None, None) == C.BDG_ERR_ARGUMENT
    v = ctypes.c_double()
    assert C.lib.bdg_sw2d_diffusion_dt(None, ctypes.byref(v)) == C.BDG_ERR_ARGUMENT
