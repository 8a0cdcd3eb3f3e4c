"""Set-up of the drifters of the quadrilateral solver, on the CPU: the element tables of bdg_quadnodes_drifter_tables, and the
NumPy restatement tests/quaddrift_ref.py held to a closed form and measured against itself in np.longdouble.

Measured here (test_measured_noise prints them), relative to the domain's size; the GPU tolerances of
tests/test_sw2d_quads_drifters_gpu.py are 16 x the recorded values:
  float64 restatement against the closed form of Heun on a solid-body rotation, 40 steps      3.22e-16   NOISE_CLOSED = 3.3e-16
  float64 restatement against the longdouble restatement on every GPU case                    5.76e-16   NOISE_LD = 5.8e-16
(the largest of the cases; the moving-flow cases, with states stepped by the float64 restatements of the solvers, give 1.7e-16
and flag no drifter).
test_measured_noise also asserts that what it measures stays within the recorded values, so they cannot go stale."""
import numpy as np
import pytest

import quaddrift_ref as D
import quadref_ld as ld

NOISE_CLOSED = 3.3e-16
NOISE_LD = 5.8e-16


def tables_both(nodes, mesh, mapO=None):
    return D.tables(nodes, mesh, mapO), D.tables(nodes, mesh, mapO, dtype=ld.LD)


@pytest.mark.parametrize("name,order", [("shear", 1), ("shear", 8), ("jitter", 4), ("jitter", 12), ("small", 5)])
def test_tables(name, order):
    nodes, t, mesh = D.mesh_case(name, order)
    T = D.tables(nodes, mesh)
    mapO = D.side_nodes(name, t, T)
    bil, neigh, bary = nodes.drifterTables(mapO)
    K, Nq, Np = T.K, order + 1, (order + 1) ** 2
    assert bil.shape == (K, 8) and neigh.shape == (4, K) and bary.shape == (Nq,)
    # the neighbour table against EToE, the boundary nodes (vmapP == vmapM) and mapO
    EToE = np.asarray(mesh.EToE).reshape(K, 4)
    boundary = (t["vmapP"] == t["vmapM"]).reshape(K, 4, Nq).all(axis=2)
    opened = np.zeros(K * 4 * Nq, dtype=bool)
    opened[mapO] = True
    opened = opened.reshape(K, 4, Nq).any(axis=2)
    assert opened.sum() > 0 and (opened & ~boundary).sum() == 0
    assert np.array_equal(neigh.T[~boundary], EToE[~boundary]) and (EToE[~boundary] != np.arange(K)[:, None].repeat(4, 1)[~boundary]).all()
    assert (neigh.T[boundary & opened] == -2).all() and (neigh.T[boundary & ~opened] == -1).all()
    assert np.array_equal(nodes.drifterTables()[1].T[boundary], np.full(boundary.sum(), -1))
    assert np.array_equal(neigh, D.tables(nodes, mesh, mapO).neigh)
    # the bilinear map reproduces the nodal coordinates (both geometry forms) and equals the restatement's bit for bit
    assert np.array_equal(bil, T.bil)
    r = np.repeat(T.r1d, Nq)
    s = np.tile(T.r1d, Nq)
    size = np.maximum(np.hypot(bil[:, 1], bil[:, 5]), np.hypot(bil[:, 2], bil[:, 6]))
    for c, g in ((0, t["x"]), (4, t["y"])):
        got = bil[:, c][None] + bil[:, c + 1][None] * r[:, None] + bil[:, c + 2][None] * s[:, None] + bil[:, c + 3][None] * (r * s)[:, None]
        assert np.abs(got - g).max() <= 1e-13 * size.max()
    # barycentric weights: the basis they give is the library's
    assert np.allclose(bary, T.bary, rtol=1e-15, atol=0)
    pts = np.array([-0.7, 0.1, 0.93, T.r1d[0], T.r1d[-1]])
    assert np.abs(D.basis(T, pts) - nodes.lagrangeBasis(pts)).max() < 1e-13
    assert np.array_equal(D.basis(T, T.r1d), np.eye(Nq))


@pytest.mark.parametrize("name,order,n", D.ROTATION_CASES)
def test_restatement_against_the_closed_form(name, order, n):
    """Heun on a solid-body rotation: z_n = z_0 (1 + i theta - theta^2 / 2)^n exactly; the velocity is of degree 1, so it is
    interpolated exactly and is continuous across the faces of any bilinear mesh."""
    nodes, t, mesh, T, q, pts, omega, dt, c, size = D.rotation_problem(name, order, n)
    d = D.Drifters(T, q, *pts)
    z0 = (d.x - c[0]) + 1j * (d.y - c[1])
    for _ in range(D.ROTATION_STEPS):
        d.advance(q, dt)
    z = D.heun_rotation(z0, omega * dt, D.ROTATION_STEPS)
    err = float(np.abs((d.x - c[0]) + 1j * (d.y - c[1]) - z).max()) / size
    print(f"{name} N={order} n={n}: float64 restatement against the closed form {err:.2e}")
    assert (d.status == 0).all() and not d.flag.any()
    assert (d.k != pts[0]).mean() > 0.9                                     # the quarter turn leaves the first element
    assert err <= NOISE_CLOSED


def run_pair(T, Tl, q_of_step, pts, dt, steps):
    """The float64 and longdouble restatements through the same states; q_of_step(i) is the state of advance i (and of the
    initial sample for i = -1). Returns (largest position difference, the two Drifters)."""
    a, b = D.Drifters(T, q_of_step(-1), *pts), D.Drifters(Tl, q_of_step(-1), *pts)
    worst = 0.0
    for i in range(steps):
        q = q_of_step(i)
        a.advance(q, dt)
        b.advance(q, dt)
        worst = max(worst, np.abs(a.xy() - b.xy()).max())
    return worst, a, b


def test_measured_noise():
    ld.require_extended_precision()
    worst = 0.0
    for name, order, n in D.ROTATION_CASES:
        nodes, t, mesh, T, q, pts, omega, dt, c, size = D.rotation_problem(name, order, n)
        err, a, b = run_pair(*tables_both(nodes, mesh), lambda i: q, pts, dt, D.ROTATION_STEPS)
        assert np.array_equal(a.status, b.status) and np.array_equal(a.k, b.k)
        print(f"rotation {name} N={order} n={n}: float64 against longdouble {err / size:.2e}")
        worst = max(worst, err / size)
    for name, order, n in D.WALL_CASES:
        nodes, t, mesh, q, pts, mapO, size = D.wall_problem(name, order, n)
        for mo in (None, mapO):
            err, a, b = run_pair(*tables_both(nodes, mesh, mo), lambda i: q, pts, D.WALL_DT, D.WALL_STEPS)
            assert np.array_equal(a.status, b.status) and np.array_equal(a.k, b.k)
            assert ((a.status & D.TOUCHED) != 0).any() and ((a.status & D.EXITED) != 0).any() == (mo is not None)
            assert not (a.status & D.LOST).any()
            print(f"walls {name} N={order} n={n} open={mo is not None}: float64 against longdouble {err / size:.2e}")
            worst = max(worst, err / size)
    for kind in D.MOVING_CASES:
        p = D.moving_problem(kind)
        states, q, time = [p["q0"]], p["q0"], p["t0"]
        for _ in range(p["steps"]):
            q, time = p["step"](q, time)
            states.append(q)
        size = D.domain(D.tables(p["nodes"], p["mesh"]), p["t"])[2]
        err, a, b = run_pair(*tables_both(p["nodes"], p["mesh"], p["mapO"]), lambda i: states[i + 1], p["points"], p["dt"], p["steps"])
        print(f"moving {kind}: float64 against longdouble {err / size:.2e}, flagged {int(b.flag.sum())}")
        assert (a.status == 0).all() and (b.status == 0).all()
        assert not a.flag.any() and not b.flag.any(), "choose other seeds: a drifter of the moving-flow case comes near an edge"
        worst = max(worst, err / size)
    print(f"largest float64 against longdouble difference, of the domain's size: {worst:.2e}")
    assert worst <= NOISE_LD
