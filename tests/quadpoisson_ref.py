"""Glue that puts tests/poisson_ref.py (the definition of the elliptic operator, its conjugate-gradient loop and its inputs) on
quadrilateral tables, for blitzdg_amd.poisson2d.Poisson2dQuadSolver. Nothing of the operator is restated here:
poisson_ref.apply, cg, right_hand_side, dense_operator, mass_dot and true_residual only index the tables, so they run unchanged
on a dict with the same keys -- quadref.tables plus J and Vinv = V1^-1 (x) V1^-1 from QuadNodesProvisioner.dgContext(), whose
Lift is built from the full 1-D mass matrix, so that <u, v> = sum_k J_k u_k^T (V V^T)^-1 v_k is the matching inner product.

The meshes:
  shear   quadref_ld.mesh_tables("shear", order): the 13 x 11 box, shuffled, each element's vertex order rotated, mapped by
          quadref_ld.SHEAR; K = 143 = tiles of 64, 32, 16 and 8 elements plus a tail; all four metric terms nonzero
  rect    the same shuffled, rotated 13 x 11 box of rectangles on [-1, 1]^2, for the problems whose closed form needs the square
  small   3 x 2 boxes of either kind (and quadref_ld's jitter map on it), where the (Np K, Np K) matrix of the operator is
          formed: at N = 12 the matrix of the 143-element mesh would take 4.7 GB
Sides are selected BY BOUNDARY FACE (poisson_ref.side_nodes thresholds the normals' components, and the sheared normals are
skew): a boundary face lies on the side of the unmapped box its midpoint is nearest to."""
import numpy as np

import blitzdg_amd.pyblitzdg as dg
import poisson_ref as P
import quadref
import quadref_ld

ORDERS = tuple(range(1, 13))
SOLVE_ORDERS = (1, 4, 8, 12)
SOLVE_MESH = {"harmonic": "shear", "euler": "shear", "sin": "rect", "cos": "rect"}
SOLVE_SIZE = {12: (6, 5)}    # at N = 12 poisson_ref.cg needs more than ten seconds on the 13 x 11 mesh (4864 iterations): 6 x 5 there
SIDES = {"harmonic": "lr", "euler": "lrb"}
_TABLES, _SOLVES = {}, {}


def tables(nodes):
    """Host tables of a QuadNodesProvisioner: quadref.tables plus J, Vinv and BCmap."""
    ctx = nodes.dgContext()
    t = quadref.tables(ctx)
    t["J"], t["Vinv"] = ctx.J, ctx.Vinv
    t["BCmap"] = {int(k): np.array(v, dtype=np.int32) for k, v in ctx.BCmap.items()}
    return t


def mesh_arrays(name, nx=quadref_ld.NX, ny=quadref_ld.NY):
    """(EToV, Vert, unmap): `shear`, `rect` or `jitter` on an nx x ny box; unmap is the 2 x 2 matrix that takes the mesh back to
    [-1, 1]^2."""
    if name == "shear":
        E, V = quadref_ld.shear_box(nx, ny, quadref_ld.SEED)
        return E, V, np.linalg.inv(quadref_ld.SHEAR)
    rng = np.random.default_rng(quadref_ld.SEED)
    E, V = quadref.quad_box(nx, ny)
    V = V.astype(np.float64)
    if name == "jitter":
        inner = (np.abs(V[:, 0]) < 1) & (np.abs(V[:, 1]) < 1)
        V[inner] += 0.15 * rng.uniform(-1, 1, (inner.sum(), 2)) * np.array([2 / nx, 2 / ny])
    else:
        assert name == "rect", name
    return quadref_ld.shuffle_and_rotate(E, rng), V, np.eye(2)


def mesh_tables(name, order, nx=quadref_ld.NX, ny=quadref_ld.NY):
    """(nodes, tables) of a mesh at an order, built once; tables["unmap"] as mesh_arrays gives it."""
    key = (name, order, nx, ny)
    if key not in _TABLES:
        if name == "shear" and (nx, ny) == (quadref_ld.NX, quadref_ld.NY):
            nodes = quadref_ld.mesh_tables("shear", order)[0]
            unmap = np.linalg.inv(quadref_ld.SHEAR)
        else:
            E, V, unmap = mesh_arrays(name, nx, ny)
            mesh = dg.MeshManager()
            mesh.buildMesh(E, V)
            nodes = dg.QuadNodesProvisioner(order, mesh)
            nodes._mesh = mesh
        t = tables(nodes)
        t["unmap"] = unmap
        _TABLES[key] = (nodes, t)
    return _TABLES[key]


def side_nodes(t, which):
    """Boundary face nodes of the faces on the sides named in `which` (a string of l, r, b, t) of the unmapped box, as a mapD."""
    Nfp = t["order"] + 1
    bnd = P.boundary_nodes(t).reshape(-1, Nfp)                 # one row per face (face-node index = Nfp (4 k + f) + n)
    vM = np.asarray(t["vmapM"]).reshape(-1, Nfp)
    xy = np.stack([t["x"].flatten("F")[vM].mean(axis=1), t["y"].flatten("F")[vM].mean(axis=1)]) # face midpoints
    X, Y = t["unmap"] @ xy
    near = {"l": np.abs(X + 1), "r": np.abs(X - 1), "b": np.abs(Y + 1), "t": np.abs(Y - 1)}
    on = np.zeros(len(X), dtype=bool)
    for c in which:
        on |= near[c] < 1e-9
    faces = bnd.all(axis=1) & on
    assert (bnd.all(axis=1) == bnd.any(axis=1)).all()
    return np.nonzero(np.repeat(faces, Nfp))[0].astype(np.int32)


def operator_cases(t):
    """poisson_ref.operator_cases' six cases on the tables `t`: Dirichlet, Neumann and mixed, with and without g / qn, with and
    without sigma, scalar and per-element kappa."""
    g, qn = P.face_data(t)
    everyD, mixed, none = P.all_boundary(t), side_nodes(t, "lb"), np.zeros(0, dtype=np.int32)
    ke = P.kappa_elements(t)
    return {
        "dirichlet": dict(mapD=everyD, kappa=P.KAPPA_SCALAR, sigma=0.0, g=None, qn=None),
        "dirichlet-data-sigma-kappaK": dict(mapD=everyD, kappa=ke, sigma=P.SIGMA, g=g, qn=None),
        "neumann": dict(mapD=none, kappa=P.KAPPA_SCALAR, sigma=0.0, g=None, qn=None),
        "neumann-data-sigma": dict(mapD=none, kappa=P.KAPPA_SCALAR, sigma=P.SIGMA, g=None, qn=qn),
        "mixed-kappaK": dict(mapD=mixed, kappa=ke, sigma=0.0, g=None, qn=None),
        "mixed-data-sigma": dict(mapD=mixed, kappa=P.KAPPA_SCALAR, sigma=P.SIGMA, g=g, qn=qn),
    }


def analytic_problem(name, t):
    """poisson_ref.analytic_problem on the tables `t`, the sides of `harmonic` and `euler` selected by boundary face."""
    p = P.analytic_problem(name, t)
    return dict(p, mapD=side_nodes(t, SIDES[name])) if name in SIDES else p


def solve_mesh(name, order):
    """The mesh of a solve input: shear for harmonic and euler, rect for sin and cos; 13 x 11, at N = 12 6 x 5 (K = 30: three
    tiles of 8 and a tail)."""
    return mesh_tables(SOLVE_MESH[name], order, *SOLVE_SIZE.get(order, (quadref_ld.NX, quadref_ld.NY)))[1]


def reference_solve(name, order):
    """(problem, u, info): poisson_ref.cg on analytic_problem(name, solve_mesh(name, order)) at poisson_ref.REL_TOL and
    CHECK_EVERY, once."""
    key = (name, order)
    if key not in _SOLVES:
        t = solve_mesh(name, order)
        p = analytic_problem(name, t)
        u, info = P.cg(p["f"], t, relTol=P.REL_TOL, checkEvery=P.CHECK_EVERY, **P.operator_args(p))
        _SOLVES[key] = (p, u, info)
    return _SOLVES[key]


_DISTANCE = {}


def apply_distance(order):
    """{case: max|apply - apply_ld| / max|apply_ld|} of float64 poisson_ref.apply from its np.longdouble evaluation on the shear
    mesh, u = poisson_ref.jumping_field, for the six operator cases with their data; computed once per order."""
    if order not in _DISTANCE:
        quadref_ld.require_extended_precision()
        t = mesh_tables("shear", order)[1]
        u = P.jumping_field(t)
        out = {}
        for name, case in operator_cases(t).items():
            ld = P.apply_ld(u, t, **case)
            out[name] = float(np.abs(P.apply(u, t, **case) - ld).max() / np.abs(ld).max())
        _DISTANCE[order] = out
    return _DISTANCE[order]


def apply_tolerance(order):
    """What the device operator is held to at an order, relative to max|A u|: max(1e-12, 8 x the largest apply_distance). The
    device's sum-factorised sums are another valid float64 order of evaluation, at a distance from longdouble comparable to
    NumPy's; 8 leaves room for both distances and the difference of the two orders."""
    return max(1e-12, 8 * max(apply_distance(order).values()))


def asymmetry(t, mapD, kappa, sigma=0.0):
    """max|M A - (M A)^T| / max|M A| with the dense matrices of poisson_ref, and (A, M)."""
    A = P.dense_operator(t, mapD, kappa, sigma)
    M = P.mass_matrix(t)
    MA = M @ A
    return np.abs(MA - MA.T).max() / np.abs(MA).max(), A, M


def bilinear_asymmetry(t, mapD, kappa, sigma=0.0, seed=4):
    """|<v, A u> - <u, A v>| / sqrt(<u, A u> <v, A v>) for two random fields: the asymmetry of M A without its matrix."""
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal(t["x"].shape), rng.standard_normal(t["x"].shape)
    Au, Av = P.apply(u, t, mapD, kappa, sigma), P.apply(v, t, mapD, kappa, sigma)
    return abs(P.mass_dot(v, Au, t) - P.mass_dot(u, Av, t)) / np.sqrt(P.mass_dot(u, Au, t) * P.mass_dot(v, Av, t))


# ---- backward Euler against explicit steps: poisson_ref.heat_reference's construction on a 5 x 4 sheared box at N = 3
_HEAT = {}


def heat_reference():
    """poisson_ref.heat_reference rebuilt on quadrilateral tables (its docstring derives `bound` and `allowance`): the same
    kappa, steps, ratio, data and start, sides by boundary face, on the 5 x 4 sheared box at N = HEAT_ORDER. The explicit step is
    dt_diff / 2 (c = 2, the step quaddiff_ref.step_size takes): dt_diff is the unpenalised tracer operator's step, and with the
    penalty the spectral radius on these quadrilaterals is 2.91 / dt_diff, beyond forward Euler's limit of 2 (on poisson_ref's
    triangles it is 1.62 / dt_diff)."""
    if not _HEAT:
        t = mesh_tables("shear", P.HEAT_ORDER, *P.HEAT_MESH)[1]
        x, y = t["x"], t["y"]
        p = dict(mapD=side_nodes(t, "lrb"), kappa=P.HEAT_KAPPA, sigma=0.0,
                 g=P.face_values(lambda x, y, nx, ny: 0.2 + 0.1 * x * y, t),
                 qn=P.face_values(lambda x, y, nx, ny: 0.02 * np.cos(2 * x), t))
        start = np.exp(-4 * (x * x + y * y))
        dte = P.diffusion_dt(P.HEAT_KAPPA, P.HEAT_ORDER, t, c=2.0)
        dt = P.HEAT_RATIO * dte
        A = P.dense_operator(t, p["mapD"], p["kappa"], 0.0)
        c = P.apply(np.zeros_like(start), t, **p).flatten("F")
        u = start.flatten("F")
        for _ in range(P.HEAT_STEPS * P.HEAT_RATIO):
            u = u - dte * (A @ u + c)
        B = np.eye(A.shape[0]) / dt + A
        v = start.flatten("F")
        for _ in range(P.HEAT_STEPS):
            v = np.linalg.solve(B, v / dt - c)
        lam, V = np.linalg.eig(A)
        steady = -np.linalg.solve(A, c)
        exact = steady + (V @ (np.exp(-P.HEAT_STEPS * dt * lam) * np.linalg.solve(V, start.flatten("F") - steady))).real
        back = lambda a: a.reshape(start.shape, order="F")
        lmin = np.linalg.eigvalsh(t["Vinv"].T @ t["Vinv"]).min() * t["J"].min()
        mnorm = lambda a: np.sqrt(P.mass_dot(back(a), back(a), t))
        allowance = P.HEAT_STEPS * P.HEAT_REL_TOL * (mnorm(start.flatten("F")) + dt * mnorm(c)) / np.sqrt(lmin)
        _HEAT.update(tables=t, problem=p, start=start, dt=dt, rho_dt=dte * np.abs(lam).max(), explicit=back(u), implicit=back(v),
                     exact=back(exact), allowance=allowance,
                     bound=np.abs(v - exact).max() + np.abs(u - exact).max() + allowance)
    return _HEAT
