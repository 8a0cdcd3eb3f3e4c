"""tests/poisson_ref.py, the definition of the elliptic operator A u = sigma u - div(kappa grad u) and of the conjugate-gradient
loop of blitzdg_amd.poisson2d, held to its own properties in float64 and np.longdouble. No GPU.

  * the dense operator on the 24-element box buildBoxMesh(4, 3) and on its distorted copy, N = 1..8, for Dirichlet, mixed, Neumann
    with sigma > 0 and Neumann with sigma = 0: the asymmetry of M A stays within 1e-12 of max|M A|; the smallest eigenvalue is
    positive, except that the Neumann sigma = 0 operator has exactly one eigenvalue at rounding (<= 1e-9 rho) whose eigenvector
    is the constant;
  * the same symmetry with a kappa that differs from element to element;
  * u = x^2, constant kappa, N >= 2: A u = -2 kappa in every element without a boundary face to 1e-10 in longdouble (Neumann
    kind, no data), and in EVERY element once g = x^2 and qn = 2 kappa x nx are given;
  * solving with numpy.linalg.solve of the dense operator on a 6 x 5 box, the error against sin(pi x) sin(pi y) (Dirichlet),
    cos(pi x) cos(pi y) (Neumann, mean removed) and the harmonic exp(x) cos(y) (Dirichlet data left and right, Neumann data top
    and bottom) decreases strictly over N = 2, 4, 6;
  * poisson_ref.cg reaches relTol = 1e-10 on the GPU tests' inputs; its iteration count and the ratio of its true to its
    recursive residual are what tests/test_poisson2d_gpu.py holds the device to;
  * float64 against longdouble on the GPU test's operator inputs stays within LD_TOL = 2.5e-13 of max|A u|, which licenses
    holding the GPU to 1e-12 against the float64 evaluation;
  * the explicit steps of the backward-Euler comparison are stable, and the first-order bound between the two schemes;
  * the refusals of the C ABI that need no GPU.

Measured with kappa = 0.7 (sigma = 2.5 where it is not 0), box / distorted copy:
  N   rho (Dirichlet)          lambda_min Dirichlet   mixed           Neumann: zero eigenvalue     second
  1   1.985e+02 / 5.700e+02    3.783 / 3.981          0.879 / 0.887   -2.9e-14 / 7.1e-14           1.776 / 1.794
  2   7.054e+02 / 2.088e+03    3.464 / 3.469          0.864 / 0.864    8.6e-14 / -2.5e-14          1.727 / 1.728
  3   1.814e+03 / 5.470e+03    3.455 / 3.455          0.864 / 0.864   -3.4e-14 / 3.8e-14           1.727 / 1.727
  4   3.956e+03 / 1.202e+04    3.454 / 3.454          0.864 / 0.864    5.1e-13 / 6.8e-13           1.727 / 1.727
  5   7.522e+03 / 2.309e+04    3.454 / 3.454          0.864 / 0.864   -1.3e-13 / 2.0e-13           1.727 / 1.727
  6   1.322e+04 / 4.071e+04    3.454 / 3.454          0.864 / 0.864   -4.8e-13 / 2.6e-14           1.727 / 1.727
  7   2.152e+04 / 6.674e+04    3.454 / 3.454          0.864 / 0.864    2.1e-13 / 1.1e-12           1.727 / 1.727
  8   3.347e+04 / 1.039e+05    3.454 / 3.454          0.864 / 0.864    2.6e-13 / -2.3e-12          1.727 / 1.727
(kappa pi^2 / 2 = 3.454 is the continuous Dirichlet eigenvalue on [-1, 1]^2, kappa pi^2 / 4 = 1.727 the first nonzero Neumann
one, kappa pi^2 / 8 = 0.864 the mixed one; with sigma the Neumann operator's smallest eigenvalue is 2.500.) The largest
asymmetry found is 2.6e-14 of max|M A| (3.2e-14 with a kappa per element), the zero eigenvalue at most 2.2e-17 rho in size.
u = x^2: at most 7.4e-12 (N = 8). The loop's figures are in the docstring of tests/test_poisson2d_gpu.py; float64 against
longdouble is at most 5.0e-16 of max|A u|; the backward-Euler bound is 1.2296e-02 (backward Euler against the exponential
1.207e-02, forward Euler 2.29e-04, allowance 1.5e-09) with dt_diff rho = 1.622. Dense solves on the 6 x 5 box, max|u - exact| at
N = 2, 4, 6: the test prints them (harmonic: 2.6e-03, 1.5e-06, 5.7e-10)."""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import poisson_ref as P
from quadref_ld import require_extended_precision
from test_quadB_reference import LD_TOL

ORDERS = tuple(range(1, 9))
KAPPA, SIGMA = P.KAPPA_SCALAR, P.SIGMA


def small_tables(order, mesh):
    return P.tables(dg.TriangleNodesProvisioner(order, P.box(4, 3) if mesh == "box" else P.distorted_box(4, 3)))


def symmetric_spectrum(A, t):
    """(asymmetry of M A over max|M A|, eigenvalues ascending, eigenvectors of A as columns): M A y = lambda M y."""
    M = P.mass_matrix(t)
    MA = M @ A
    asym = np.abs(MA - MA.T).max() / np.abs(MA).max()
    L = np.linalg.cholesky(M)
    Linv = np.linalg.inv(L)
    S = Linv @ (0.5 * (MA + MA.T)) @ Linv.T
    lam, Y = np.linalg.eigh(S)
    return asym, lam, Linv.T @ Y


@pytest.mark.parametrize("mesh", ("box", "distorted"))
@pytest.mark.parametrize("order", ORDERS)
def test_the_operator_is_symmetric_and_positive_in_the_mass_inner_product(order, mesh):
    t = small_tables(order, mesh)
    assert t["rx"].shape[1] == 24
    if mesh == "distorted":
        assert np.ptp(np.abs(t["Fscale"])) > 0.5 * np.abs(t["Fscale"]).min()
    n = t["rx"].size
    line = [f"N{order} {mesh}:"]
    for name, mapD in (("dirichlet", P.all_boundary(t)), ("mixed", P.side_nodes(t, "lb")), ("neumann", np.zeros(0, dtype=np.int32))):
        A = P.dense_operator(t, mapD, KAPPA, 0.0)
        for sigma in ((0.0,) if name != "neumann" else (SIGMA, 0.0)):
            asym, lam, Y = symmetric_spectrum(A + sigma * np.eye(n), t)
            rho = np.abs(lam).max()
            line.append(f"{name} sigma {sigma:g}: rho {rho:.4e} lambda_min {lam[0]:.3e} second {lam[1]:.3e} asymmetry {asym:.1e};")
            assert asym <= 1e-12, (name, sigma)
            if name == "neumann" and sigma == 0.0:
                assert abs(lam[0]) <= 1e-9 * rho and lam[1] > 1e-6 * rho        # exactly one eigenvalue at rounding ...
                y = Y[:, 0] / Y[np.abs(Y[:, 0]).argmax(), 0]
                assert np.abs(y - 1.0).max() <= 1e-7                            # ... and its eigenvector is the constant
            else:
                assert lam[0] > 1e-6 * rho, (name, sigma)
            if sigma:
                assert lam[0] >= sigma * (1 - 1e-9)
    print(" ".join(line))


@pytest.mark.parametrize("order", (1, 4, 8))
def test_symmetry_holds_with_a_kappa_per_element(order):
    t = small_tables(order, "distorted")
    kap = P.kappa_elements(t)
    assert np.ptp(kap) > 0.3
    for mapD in (P.side_nodes(t, "lb"), np.zeros(0, dtype=np.int32)):
        asym, lam, _ = symmetric_spectrum(P.dense_operator(t, mapD, kap, 0.0), t)
        print(f"N{order}: kappa per element, {len(mapD)} Dirichlet nodes: asymmetry {asym:.1e}, lambda_min {lam[0]:.3e}")
        assert asym <= 1e-12 and lam[0] >= -1e-9 * np.abs(lam).max()


def test_a_nodal_kappa_field_is_refused():
    t = small_tables(2, "box")
    with pytest.raises(ValueError):
        P.apply(t["x"], t, [], np.ones_like(t["x"]))
    with pytest.raises(ValueError):
        P.apply(t["x"], t, np.nonzero(~P.boundary_nodes(t))[0][:1])              # a mapD entry that is not a boundary node


@pytest.mark.parametrize("order", range(2, 9))
def test_a_quadratic_has_a_constant_image_away_from_the_boundary(order):
    require_extended_precision()
    t = P.tables(dg.TriangleNodesProvisioner(order, P.box(5, 4)))
    tl = P.to_ld(t)
    x = tl["x"]
    kap = P.LD(0.03)
    none = np.zeros(0, dtype=np.int32)
    Au = P.apply(x * x, tl, none, kap, P.LD(0), P.LD(P.penalty(t, 0.03)))
    bnd = P.boundary_nodes(t).reshape(t["nx"].shape, order="F").any(axis=0)
    assert 0 < bnd.sum() < bnd.size
    want = -2 * kap
    err = float(np.abs(Au[:, ~bnd] - want).max() / abs(want))
    print(f"N{order}: |A u + 2 kappa| / (2 kappa) {err:.2e} in {int((~bnd).sum())} elements without a boundary face")
    assert err <= 1e-10
    assert np.abs(Au[:, bnd] - want).max() > 1e-3 * abs(want)                    # ... and the zero normal flux shows in the others
    # with the data of u itself the image is constant everywhere, whatever the kinds
    g = P.face_values(lambda x, y, nx, ny: x * x, t).astype(P.LD)
    qn = P.face_values(lambda x, y, nx, ny: 2 * 0.03 * x * nx, t).astype(P.LD)
    for mapD in (P.all_boundary(t), P.side_nodes(t, "lt"), none):
        full = P.apply(x * x, tl, mapD, kap, P.LD(0), P.LD(P.penalty(t, 0.03)), g, qn)
        assert float(np.abs(full - want).max() / abs(want)) <= 1e-10


def test_the_error_against_three_analytic_solutions_decreases_with_the_order():
    errs = {}
    for order in (2, 4, 6):
        t = P.tables(dg.TriangleNodesProvisioner(order, P.box(6, 5)))
        for name in ("sin", "cos", "harmonic"):
            p = P.analytic_problem(name, t)
            A = P.dense_operator(t, p["mapD"], p["kappa"], p["sigma"])
            b = P.right_hand_side(p["f"], t, **P.operator_args(p)).flatten("F")
            exact = p["exact"]
            if name == "cos":       # the singular system, bordered with the mass-weighted constant to pin the mean
                w = P.mass_apply(np.ones_like(exact), t).flatten("F")
                A = np.block([[A, np.ones((A.shape[0], 1))], [w[None, :], np.zeros((1, 1))]])
                b = np.append(b, 0.0)
                exact = exact - P.mass_mean(exact, t)
            u = np.linalg.solve(A, b)[:exact.size].reshape(exact.shape, order="F")
            errs[name, order] = np.abs(u - exact).max()
    for name in ("sin", "cos", "harmonic"):
        print(f"{name}: max|u - exact| " + ", ".join(f"N{n} {errs[name, n]:.3e}" for n in (2, 4, 6)))
        assert errs[name, 2] > errs[name, 4] > errs[name, 6]


@pytest.mark.parametrize("name", P.PROBLEMS)
@pytest.mark.parametrize("order", P.SOLVE_ORDERS)
def test_the_reference_loop_reaches_the_tolerance_on_the_gpu_tests_inputs(order, name):
    u, info = P.reference_solve(name, order)
    p = P.solve_problem(name, order)
    t = P.nodes_tables(order)[1]
    ratio = info["trueres"] / info["relres"]
    print(f"N{order} {name}: {info['iterations']} iterations, recursive residual / relTol {info['relres'] / P.REL_TOL:.3f}, "
          f"true / relTol {info['trueres'] / P.REL_TOL:.3f}, true / recursive {ratio:.4f}")
    assert info["converged"] and info["relres"] <= P.REL_TOL
    assert info["iterations"] % P.CHECK_EVERY == 0
    assert info["projected"] == (name == "cos")
    assert 0.5 <= ratio <= 2.0
    assert abs(P.true_residual(u, p, t) - info["trueres"]) <= 1e-3 * info["trueres"]
    if name == "cos":
        assert abs(P.mass_mean(u, t)) <= 1e-12 * np.abs(u).max()


def test_the_reference_loop_returns_zero_for_a_zero_right_hand_side():
    p = P.solve_problem("sin", 1)
    u, info = P.cg(np.zeros_like(p["f"]), P.nodes_tables(1)[1], mapD=p["mapD"], x0=np.ones_like(p["f"]))
    assert info["iterations"] == 0 and info["converged"] and not u.any()


@pytest.mark.parametrize("order", ORDERS)
def test_float64_is_within_a_quarter_of_the_gpu_tolerance(order):
    require_extended_precision()
    _, t = P.nodes_tables(order)
    u = P.jumping_field(t)
    worst = 0.0
    for name, case in P.operator_cases(order).items():
        got = P.apply(u, t, **case)
        ref = P.apply_ld(u, t, **case)
        assert ref.dtype == P.LD and np.all(np.isfinite(got))
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"N{order}: float64 against longdouble {worst:.2e} of max|A u|")
    assert worst <= LD_TOL


def test_the_operator_cases_cover_what_the_gpu_test_promises():
    _, t = P.nodes_tables(2)
    assert t["rx"].shape[1] == 286
    cases = P.operator_cases(2)
    nb = P.all_boundary(t).size
    assert {len(c["mapD"]) for c in cases.values()} >= {0, nb} and any(0 < len(c["mapD"]) < nb for c in cases.values())
    assert any(c["g"] is not None for c in cases.values()) and any(c["qn"] is not None for c in cases.values())
    assert any(c["g"] is None and c["qn"] is None for c in cases.values())
    assert {c["sigma"] for c in cases.values()} == {0.0, P.SIGMA}
    assert any(np.ndim(c["kappa"]) == 1 for c in cases.values()) and any(np.ndim(c["kappa"]) == 0 for c in cases.values())


def test_the_explicit_steps_are_stable_and_the_first_order_bound():
    h = P.heat_reference()
    be, fe = np.abs(h["implicit"] - h["exact"]).max(), np.abs(h["explicit"] - h["exact"]).max()
    print(f"dt_diff rho {h['rho_dt']:.3f}; backward Euler against the exponential {be:.3e}, forward Euler {fe:.3e}, allowance "
          f"{h['allowance']:.2e}, bound {h['bound']:.4e}; |implicit - explicit| {np.abs(h['implicit'] - h['explicit']).max():.4e}")
    assert h["rho_dt"] < 2.0
    assert fe < be < 0.05 * np.abs(h["start"]).max()
    assert np.abs(h["implicit"] - h["explicit"]).max() <= h["bound"]


def test_refusals_without_a_gpu():
    from blitzdg_amd import _capi as C
    h = ctypes.c_void_p()

    def create(**kw):
        d = C.Poisson2dDesc()
        d.order, d.num_elements, d.kappa, d.tau_scale = 2, 4, 1.0, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        rc = C.lib.bdg_poisson2d_create(ctypes.byref(d), ctypes.byref(h))
        assert not h.value
        return rc

    assert create(order=99) == C.BDG_ERR_ARGUMENT
    assert create(order=0) == C.BDG_ERR_ARGUMENT
    assert create(kappa=0.0) == C.BDG_ERR_ARGUMENT
    assert create(kappa=-1.0) == C.BDG_ERR_ARGUMENT
    assert create(sigma=-0.5) == C.BDG_ERR_ARGUMENT
    assert create(flags=C.BDG_SW2D_NODAL_GEOMETRY) == C.BDG_ERR_ARGUMENT
    assert create() == C.BDG_ERR_ARGUMENT                                          # no tables
    assert C.lib.bdg_poisson2d_create(None, ctypes.byref(h)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_create_from_nodes(None, None, -1, 1.0, None, 0.0, 1.0, 0, 0, ctypes.byref(h)) == C.BDG_ERR_ARGUMENT
    # NULL handles are reported, not dereferenced
    v, ms, res = ctypes.c_double(), ctypes.c_float(), C.Poisson2dResult()
    assert C.lib.bdg_poisson2d_set_shift(None, 1.0) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_set_boundary_data(None, None, None) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_apply(None, None, None, 0) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_mass_dot(None, None, None, ctypes.byref(v)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_solve(None, None, None, 1e-8, 0, 8, ctypes.byref(res)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_time_apply(None, 1, ctypes.byref(ms)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_time_iterations(None, 1, ctypes.byref(ms)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_poisson2d_device_bytes(None) == 0
    C.lib.bdg_poisson2d_destroy(None)


def test_a_mapD_entry_off_the_boundary_is_refused_without_a_gpu():
    """The tables of a real mesh with one interior face node in mapD: refused on the host, before a device is looked for."""
    from blitzdg_amd import _capi as C
    t = small_tables(2, "box")
    Np, K = t["rx"].shape
    keep = {k: C.as_f64(t[k]) for k in ("Dr", "Ds", "Lift", "Vinv", "rx", "sx", "ry", "sy", "J", "nx", "ny", "Fscale")}
    vM, vP = C.as_i32(t["vmapM"]).reshape(-1), C.as_i32(t["vmapP"]).reshape(-1)
    bad = C.as_i32(np.nonzero(~P.boundary_nodes(t))[0][:1])
    d = C.Poisson2dDesc(2, K, *[C.ptr(keep[k]) for k in ("Dr", "Ds", "Lift", "Vinv", "rx", "sx", "ry", "sy", "J", "nx", "ny", "Fscale")],
                        C.ptr(vM), C.ptr(vP), C.ptr(bad), 1, 1.0, None, 0.0, 1.0, 0, 0)
    h = ctypes.c_void_p()
    assert C.lib.bdg_poisson2d_create(ctypes.byref(d), ctypes.byref(h)) == C.BDG_ERR_ARGUMENT and not h.value
    assert b"boundary" in C.lib.bdg_last_error()


def test_curved_triangles_and_bad_arguments_are_refused_on_the_host():
    """The twin of test_quadpoisson_reference's quadrilateral refusals: these come before a device is looked for."""
    from blitzdg_amd import _capi as C
    from blitzdg_amd import poisson2d
    t = small_tables(2, "box")
    K = t["rx"].shape[1]

    def refused(tables=t, **kw):
        with pytest.raises(C.BdgError) as e:
            poisson2d.Poisson2dSolver(tables=tables, **kw)
        assert e.value.code == C.BDG_ERR_ARGUMENT
        return str(e.value)

    bent = dict(t, rx=t["rx"].copy())    # one node's rx off by 1e-6 of the element's metric terms: no longer affine at 1e-8
    bent["rx"][1, 0] += 1e-6 * sum(abs(t[k][0, 0]) for k in ("rx", "sx", "ry", "sy"))
    assert "straight-sided" in refused(bent, mapD=P.all_boundary(t))
    assert "boundary face node" in refused(mapD=np.nonzero(~P.boundary_nodes(t))[0][:1])
    assert "order" in refused(P.tables(dg.TriangleNodesProvisioner(9, P.box(4, 3))))
    assert "per-node geometry" in refused(flags=poisson2d.NODAL_GEOMETRY)
    for kappa in (0.0, -1.0, np.zeros(K)):
        assert "kappa" in refused(kappa=kappa)
    assert "sigma" in refused(shift=-0.1)
