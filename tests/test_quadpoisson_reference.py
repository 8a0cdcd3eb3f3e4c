"""What licenses conjugate gradients on quadrilaterals, and what the device solver is held to: the definition of
tests/poisson_ref.py on the quadrilateral tables of tests/quadpoisson_ref.py, in NumPy, no GPU. The library's host part builds
the tables.

  * parallelograms: the asymmetry of M A (dense, on the 3 x 2 sheared box: at N = 12 the matrix of the 143-element mesh would
    take 4.7 GB) with a kappa per element, Dirichlet and Neumann walls, N = 1..12, asserted at ASYM_BOUND = 10 x the largest
    measured value; the same asymmetry without a matrix, |<v, A u> - <u, A v>| for random fields, on the 13 x 11 shear mesh
  * the two smallest Dirichlet eigenvalues on the 3 x 2 box of rectangles against pi^2 / 2 and 5 pi^2 / 4 of [-1, 1]^2 (the
    sheared domain has no closed form)
  * the Neumann operator's single zero eigenvalue, the constant its eigenvector
  * u = x^2 on the shear mesh with Dirichlet data left and bottom and Neumann data right and top: A(u; g, qn) = -2 kappa
  * general bilinear elements (quadref_ld's jitter map): asymmetry >= 1e-3 -- why the solver refuses them -- and the refusal
    itself, which needs no device
  * the distance of float64 apply from its np.longdouble evaluation at every order and case: the device operator's tolerance is
    quadpoisson_ref.apply_tolerance(N) = max(1e-12, 8 x that distance)
  * poisson_ref.cg's iteration counts and true residuals on the GPU solve test's inputs

Measured here (python -m pytest tests/test_quadpoisson_reference.py -s prints them):
  N                       1        2        3        4        5        6        7        8        9        10       11       12
  asymmetry, Dirichlet    1.5e-16  3.3e-16  9.2e-16  2.3e-15  2.8e-15  3.6e-15  8.9e-15  7.5e-15  5.6e-15  2.3e-14  1.1e-14  3.7e-14
  asymmetry, Neumann      2.8e-16  6.4e-16  1.6e-15  4.0e-15  4.8e-15  6.0e-15  1.5e-14  1.3e-14  1.3e-14  3.8e-14  1.9e-14  6.1e-14
  bilinear, 143 elements  2.6e-17  4.5e-17  1.7e-16  1.6e-16  5.7e-16  2.1e-16  1.4e-16  4.0e-16  3.6e-16  2.3e-15  8.9e-16  1.2e-15
  asymmetry, jitter       1.0e-01  1.0e-01  1.3e-01  1.1e-01  1.2e-01  1.1e-01  1.1e-01  1.1e-01  1.1e-01  1.1e-01  1.1e-01  1.1e-01
  (on the jitter mesh max|Im lambda| / max|lambda| reaches 4.2e-03: the spectrum is complex at some orders)
  float64 - longdouble    2.2e-16  2.2e-16  2.7e-16  2.0e-16  2.9e-16  3.0e-16  2.4e-16  3.0e-16  2.8e-16  2.2e-16  2.6e-16  2.8e-16
  (the largest of the six cases; 8 x that is below 1e-12 at every order, so the device tolerance is 1e-12 throughout)
Eigenvalues on the square, relative error of the first: 1.3e-01, 2.8e-03, 6.2e-05, 5.5e-07, 3.8e-09, 1.6e-11, then below 1e-12.
u = x^2: |A(u; g, qn) + 2 kappa| at most 1.3e-16 of max|A u|. Heat reference: rho dt = 1.45 with the explicit step dt_diff / 2.
  cg iterations / true residual over relTol: the docstring of tests/test_quadpoisson_gpu.py"""
import numpy as np
import pytest

import poisson_ref as P
import quadpoisson_ref as Q
from blitzdg_amd import _capi as C
from blitzdg_amd import poisson2d

ASYM_BOUND = 6.1e-13      # 10 x 6.1e-14, the largest measured asymmetry of M A on parallelograms (N = 12, Neumann walls)
# largest max|apply - apply_ld| / max|apply_ld| over the orders and the six cases on the 13 x 11 shear mesh, measured here: between
# 1.0e-16 and 3.0e-16 at every order (max|A u| is the penalty term's, which both evaluations round alike)
APPLY_DISTANCE = 3.0e-16
NONE = np.zeros(0, dtype=np.int32)


@pytest.mark.parametrize("order", Q.ORDERS)
def test_M_A_is_symmetric_on_parallelograms(order):
    t = Q.mesh_tables("shear", order, 3, 2)[1]
    ke = P.kappa_elements(t)
    asymD, A, _ = Q.asymmetry(t, P.all_boundary(t), ke)
    asymN, An, _ = Q.asymmetry(t, NONE, ke)
    ts = Q.mesh_tables("shear", order)[1]
    bil = max(Q.bilinear_asymmetry(ts, Q.side_nodes(ts, "lb"), P.kappa_elements(ts)), Q.bilinear_asymmetry(ts, NONE, P.KAPPA_SCALAR, P.SIGMA))
    ev, evN = np.linalg.eigvals(A), np.linalg.eigvals(An)
    print(f"N{order}: asymmetry of M A Dirichlet {asymD:.1e} Neumann {asymN:.1e}, of the bilinear form on 143 elements {bil:.1e}; "
          f"max|Im lambda| {max(np.abs(ev.imag).max(), np.abs(evN.imag).max()):.1e}, min Re lambda Dirichlet {ev.real.min():.3f}")
    assert max(asymD, asymN, bil) <= ASYM_BOUND
    assert np.abs(ev.imag).max() <= 1e-9 * np.abs(ev).max() and np.abs(evN.imag).max() <= 1e-9 * np.abs(evN).max()   # a real spectrum
    assert ev.real.min() > 0                                                                                            # positive definite
    # Neumann walls: one zero eigenvalue, the constant its eigenvector
    one = np.ones(An.shape[0])
    assert np.abs(An @ one).max() <= 1e-12 * np.abs(An).sum(axis=1).max()
    low = np.sort(evN.real)
    assert abs(low[0]) <= 1e-9 * np.abs(evN).max() and low[1] > 1e-3 * np.abs(evN).max() / (order + 1) ** 4, low[:2]


@pytest.mark.parametrize("order", Q.ORDERS)
def test_smallest_eigenvalues_on_the_square(order):
    """-lap on [-1, 1]^2 with u = 0 on the boundary has the eigenvalues (pi / 2)^2 (m^2 + n^2): pi^2 / 2, then 5 pi^2 / 4 twice.
    Three by two elements resolve the first to 13 % at N = 1 and 0.3 % at N = 2 and converge spectrally from there (5.5e-7 at
    N = 4, below 1e-9 from N = 6 on); the bounds leave a factor of 1.5 to 20."""
    t = Q.mesh_tables("rect", order, 3, 2)[1]
    ev = np.sort(np.linalg.eigvals(P.dense_operator(t, P.all_boundary(t), 1.0)).real)
    err = [abs(ev[0] / (np.pi ** 2 / 2) - 1), abs(ev[1] / (5 * np.pi ** 2 / 4) - 1), abs(ev[2] / (5 * np.pi ** 2 / 4) - 1)]
    print(f"N{order}: lambda {ev[0]:.10f} {ev[1]:.10f} {ev[2]:.10f}, relative errors {err[0]:.1e} {err[1]:.1e} {err[2]:.1e}")
    first = {1: 0.2, 2: 5e-3, 3: 1e-3}.get(order, 1e-5 if order < 6 else 1e-8)
    assert err[0] <= first
    if order >= 4:
        assert max(err[1:]) <= 10 * first


@pytest.mark.parametrize("order", Q.ORDERS[1:])
def test_a_quadratic_is_reproduced_with_data(order):
    """u = x^2 is in the space from N = 2 on (the map is affine), its jumps vanish and the data are exact: -div(kappa grad u) =
    -2 kappa up to rounding, which the penalty term scales: measured against max|A u| of the homogeneous operator on u."""
    t = Q.mesh_tables("shear", order)[1]
    kappa = P.KAPPA_SCALAR
    u = t["x"] ** 2
    g = P.face_values(lambda x, y, nx, ny: x * x, t)
    qn = P.face_values(lambda x, y, nx, ny: kappa * 2 * x * nx, t)
    mapD = Q.side_nodes(t, "lb")
    got = P.apply(u, t, mapD, kappa, 0.0, None, g, qn)
    scale = np.abs(P.apply(u, t, mapD, kappa)).max()
    err = np.abs(got + 2 * kappa).max() / scale
    print(f"N{order}: |A(x^2; g, qn) + 2 kappa| {err:.1e} of max|A x^2| = {scale:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("order", Q.ORDERS)
def test_M_A_is_not_symmetric_on_general_quadrilaterals(order):
    t = Q.mesh_tables("jitter", order, 3, 2)[1]
    asym, A, _ = Q.asymmetry(t, P.all_boundary(t), P.kappa_elements(t))
    print(f"N{order}: asymmetry of M A on the jitter mesh {asym:.1e}, max|Im lambda| / max|lambda| "
          f"{np.abs(np.linalg.eigvals(A).imag).max() / np.abs(np.linalg.eigvals(A)).max():.1e}")
    assert asym >= 1e-3


def test_general_quadrilaterals_and_bad_arguments_are_refused_on_the_host():
    """These refusals come before a device is looked for."""
    t = Q.mesh_tables("jitter", 3, 3, 2)[1]
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(tables=t, mapD=P.all_boundary(t))
    assert e.value.code == C.BDG_ERR_ARGUMENT and "parallelogram" in str(e.value)
    nodes, t = Q.mesh_tables("shear", 2, 3, 2)
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(tables=t, mapD=np.nonzero(~P.boundary_nodes(t))[0][:1])    # an interior face node
    assert e.value.code == C.BDG_ERR_ARGUMENT and "boundary face node" in str(e.value)
    with pytest.raises(ValueError):
        poisson2d.Poisson2dQuadSolver(tables=t, kappa=np.ones_like(t["x"]))
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(tables=Q.mesh_tables("shear", 13, 3, 2)[1])
    assert e.value.code == C.BDG_ERR_ARGUMENT and "order" in str(e.value)
    with pytest.raises(C.BdgError) as e:
        poisson2d.Poisson2dQuadSolver(tables=t, flags=poisson2d.NODAL_GEOMETRY)
    assert e.value.code == C.BDG_ERR_ARGUMENT


@pytest.mark.parametrize("order", Q.ORDERS)
def test_float64_is_close_to_longdouble(order):
    d = Q.apply_distance(order)
    print(f"N{order}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()) + f"; device tolerance {Q.apply_tolerance(order):.1e}")
    # the recorded table stays an honest description: within a factor of 2 of what this platform measures
    assert max(d.values()) <= 2 * APPLY_DISTANCE
    assert Q.apply_tolerance(order) <= 1e-12          # 8 x the distance stays below the floor at every order: the tolerance is 1e-12


@pytest.mark.parametrize("name", P.PROBLEMS)
@pytest.mark.parametrize("order", Q.SOLVE_ORDERS)
def test_cg_converges_on_the_solve_inputs(order, name):
    p, u, info = Q.reference_solve(name, order)
    t = Q.solve_mesh(name, order)
    print(f"N{order} {name}: {info['iterations']} iterations, true residual / relTol {info['trueres'] / P.REL_TOL:.3e}, "
          f"recursive {info['relres'] / P.REL_TOL:.3e}, K = {t['x'].shape[1]}")
    assert info["converged"] and info["projected"] == (name == "cos")
    assert info["trueres"] <= 1.5 * P.REL_TOL
    if p["exact"] is not None and order >= 8:
        ex = p["exact"] - (P.mass_mean(p["exact"], t) if info["projected"] else 0.0)
        assert np.abs(u - ex).max() <= 1e-6


def test_the_heat_reference_is_stable_and_first_order():
    h = Q.heat_reference()
    print(f"rho dt {h['rho_dt']:.3f}, |implicit - exact| {np.abs(h['implicit'] - h['exact']).max():.3e}, |explicit - exact| "
          f"{np.abs(h['explicit'] - h['exact']).max():.3e}, allowance {h['allowance']:.1e}, bound {h['bound']:.4e}")
    assert h["rho_dt"] < 2
    assert np.abs(h["explicit"] - h["implicit"]).max() <= h["bound"]


SHARED_REFUSALS = {
    "kappa": lambda t: dict(kappa=0.0),
    "kappa-per-element": lambda t: dict(kappa=np.zeros(t["x"].shape[1])),
    "shift": lambda t: dict(shift=-0.1),
    "tau-scale": lambda t: dict(tauScale=-1.0),
    "mapD-interior": lambda t: dict(mapD=np.nonzero(~P.boundary_nodes(t))[0][:1]),
    "mapD-range": lambda t: dict(mapD=[np.asarray(t["vmapM"]).size]),
    "vmapP-range": lambda t: dict(tables=dict(t, vmapP=np.where(np.arange(np.asarray(t["vmapP"]).size) == 5, t["x"].size,
                                                                np.asarray(t["vmapP"]).reshape(-1)))),
    "J": lambda t: dict(tables=dict(t, J=-t["J"])),
}


@pytest.mark.parametrize("name", sorted(SHARED_REFUSALS))
def test_both_families_refuse_a_shared_bad_argument_in_the_same_words(name):
    """One table builder serves triangles and quadrilaterals: after the name of the function the refusal reads the same."""
    said = []
    for cls, t in ((poisson2d.Poisson2dSolver, P.nodes_tables(2, 4, 3)[1]), (poisson2d.Poisson2dQuadSolver, Q.mesh_tables("shear", 2, 3, 2)[1])):
        kw = dict(tables=t)
        kw.update(SHARED_REFUSALS[name](t))
        with pytest.raises(C.BdgError) as e:
            cls(**kw)
        assert e.value.code == C.BDG_ERR_ARGUMENT
        _, named, text = str(e.value).partition(cls._CREATE + ": ")
        assert named and text
        said.append(text)
    print(f"{name}: {said[0]}")
    assert said[0] == said[1]
