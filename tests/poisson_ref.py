"""The elliptic operator of blitzdg_amd.poisson2d on straight-sided triangles: the definition the two passes of
csrc/hip/poisson2d_kernel.hpp and the device-resident conjugate-gradient loop are held to. Every function is
dtype-generic, so that it can be evaluated in np.longdouble.

  A u = sigma u - div(kappa grad u),   sigma >= 0 a scalar, kappa > 0 a scalar or one value per element, tau > 0 one scalar

in Hesthaven and Warburton's stabilised central flux form (local DG, both numerical fluxes the averages, plus a penalty on the
jump of u). A face node is INTERIOR (it has a neighbour, vmapP != vmapM), DIRICHLET (a boundary node listed in mapD) or NEUMANN
(any other boundary node):
  gradient    du = u- - u+ (interior), 2 (u- - g) (Dirichlet, g = 0 unless data is set), 0 (Neumann)
              qx = kappa_k (rx Dr u + sx Ds u - Lift(Fscale nx du / 2)),  qy likewise with ry, sy, ny
  divergence  dq = nx (qx- - qx+) + ny (qy- - qy+) (interior), 0 (Dirichlet), 2 (nx qx- + ny qy- - qn) (Neumann, qn = 0 unless set)
              A u = sigma u - [ rx Dr qx + sx Ds qx + ry Dr qy + sy Ds qy - Lift(Fscale (dq + tau du) / 2) ]
  tau         = tauScale Np max(Fscale) / 2 max(kappa)
qn is the prescribed outward normal flux kappa du/dn. With g = qn = 0, A is self-adjoint and positive semi-definite in the mass
inner product <u, v> = sum_k J_k u_k^T (V V^T)^-1 v_k (div_h is minus the adjoint of grad_h for this pairing of boundary fluxes,
kappa_k commutes with the element's mass matrix, the penalty adds tau/2 times the integral of [u][v] over the faces); it is
singular, with the constants as its kernel, exactly when sigma = 0 and no node is a Dirichlet node.

THE SIGN IS OPPOSITE to the operator of the project this one follows (poisson2d::PoissonOperator), which returns the Laplacian;
that operator also omits Fscale in its last lift, takes tau from J and averages grad u, not q, in its boundary flux, so it is
not the definition here (DESIGN.md 3.12 records the departures).

cg() is conjugate gradients in the mass inner product (PCG on J M A preconditioned by (J M)^-1) in NumPy, with the solver's
treatment of the singular case: the mass-weighted mean of the right-hand side is removed, the mean of the residual at every
convergence check, the mean of the solution at the end."""
import numpy as np

import blitzdg_amd.pyblitzdg as dg

LD = np.longdouble


def to_ld(t):
    """Tables with every floating-point array as np.longdouble."""
    return {k: (np.asarray(v).astype(LD) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in t.items()}


def tables(nodes):
    """Host tables of a TriangleNodesProvisioner, with J and Vinv for the mass inner product."""
    ctx = nodes.dgContext()
    t = {k: getattr(ctx, k) for k in
         ("Dr", "Ds", "Lift", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP", "x", "y", "J", "Vinv")}
    t["order"] = ctx.order
    t["BCmap"] = {int(k): np.array(v, dtype=np.int32) for k, v in ctx.BCmap.items()}
    return t


def boundary_nodes(t):
    """Boolean per face node, in the numbering of vmapM (j + 3 Nfp k)."""
    return np.asarray(t["vmapM"]) == np.asarray(t["vmapP"])


def all_boundary(t):
    """Every boundary face node, as a mapD."""
    return np.nonzero(boundary_nodes(t))[0].astype(np.int32)


def kinds(t, mapD):
    """(interior, dirichlet, neumann): three boolean arrays per face node. A mapD entry that is not a boundary node is refused."""
    bnd = boundary_nodes(t)
    mapD = np.asarray(mapD, dtype=np.int64).reshape(-1)
    if mapD.size and (mapD.min() < 0 or mapD.max() >= bnd.size or not bnd[mapD].all()):
        raise ValueError("mapD holds an entry that is not a boundary face node")
    dirichlet = np.zeros(bnd.size, dtype=bool)
    dirichlet[mapD] = True
    return ~bnd, dirichlet, bnd & ~dirichlet


def penalty(t, kappa, tauScale=1.0):
    """tau = tauScale Np max(Fscale) / 2 max(kappa)."""
    Np = t["rx"].shape[0]
    return tauScale * Np * np.abs(np.asarray(t["Fscale"], dtype=np.float64)).max() / 2 * np.max(np.asarray(kappa, dtype=np.float64))


def apply(u, t, mapD, kappa=1.0, sigma=0.0, tau=None, g=None, qn=None):
    """A u (with the data g, qn, each (3 Nfp, K), where given). kappa: a scalar or (K,)."""
    dtype = u.dtype.type
    half, two = dtype(0.5), dtype(2)
    if np.ndim(kappa) == 2:
        raise ValueError("a nodal kappa field does not commute with the mass matrix: one value per element at most")
    kap = np.asarray(kappa).astype(u.dtype)
    tau = dtype(penalty(t, kappa) if tau is None else tau)
    vM, vP = np.asarray(t["vmapM"]), np.asarray(t["vmapP"])
    interior, dirichlet, neumann = kinds(t, mapD)
    shape = t["nx"].shape
    uC = u.flatten("F")
    du = uC[vM] - uC[vP]
    gC = np.zeros(du.shape, dtype=u.dtype) if g is None else np.asarray(g).astype(u.dtype).flatten("F")
    du[dirichlet] = (two * (uC[vM] - gC))[dirichlet]
    du[neumann] = 0
    duM = du.reshape(shape, order="F")
    Dr, Ds, Lift, Fs = t["Dr"], t["Ds"], t["Lift"], t["Fscale"]
    Dru, Dsu = Dr @ u, Ds @ u
    qx = kap * (t["rx"] * Dru + t["sx"] * Dsu - Lift @ (Fs * t["nx"] * duM * half))
    qy = kap * (t["ry"] * Dru + t["sy"] * Dsu - Lift @ (Fs * t["ny"] * duM * half))
    qxC, qyC, nxC, nyC = qx.flatten("F"), qy.flatten("F"), t["nx"].flatten("F"), t["ny"].flatten("F")
    dq = nxC * (qxC[vM] - qxC[vP]) + nyC * (qyC[vM] - qyC[vP])
    qnC = np.zeros(du.shape, dtype=u.dtype) if qn is None else np.asarray(qn).astype(u.dtype).flatten("F")
    dq[dirichlet] = 0
    dq[neumann] = (two * (nxC * qxC[vM] + nyC * qyC[vM] - qnC))[neumann]
    flux = ((dq + tau * du) * half).reshape(shape, order="F")
    div = t["rx"] * (Dr @ qx) + t["sx"] * (Ds @ qx) + t["ry"] * (Dr @ qy) + t["sy"] * (Ds @ qy) - Lift @ (Fs * flux)
    return dtype(sigma) * u - div


def apply_ld(u, t, mapD, kappa=1.0, sigma=0.0, tau=None, g=None, qn=None):
    """The float64 inputs evaluated in np.longdouble."""
    k = np.asarray(kappa).astype(LD) if np.ndim(kappa) else LD(kappa)
    tau = penalty(t, kappa) if tau is None else tau
    return apply(u.astype(LD), to_ld(t), mapD, k, LD(sigma), LD(tau), None if g is None else g.astype(LD),
                 None if qn is None else qn.astype(LD))


def mass_apply(u, t):
    """J_k (V V^T)^-1 u_k."""
    Vinv = t["Vinv"]
    return t["J"][0] * ((Vinv.T @ Vinv) @ u)


def mass_dot(u, v, t):
    return (u * mass_apply(v, t)).sum()


def mass_mean(u, t):
    one = np.ones_like(u)
    return mass_dot(one, u, t) / mass_dot(one, one, t)


def mass_matrix(t):
    """Block-diagonal diag(J_k (V V^T)^-1), (Np K, Np K), nodes numbered n + Np k."""
    Np, K = t["rx"].shape
    Mref = t["Vinv"].T @ t["Vinv"]
    M = np.zeros((Np * K, Np * K))
    for k in range(K):
        M[k * Np:(k + 1) * Np, k * Np:(k + 1) * Np] = t["J"][0, k] * Mref
    return M


def dense_operator(t, mapD, kappa=1.0, sigma=0.0, tau=None):
    """The (Np K, Np K) matrix of the homogeneous operator, nodes numbered n + Np k."""
    Np, K = t["rx"].shape
    A = np.empty((Np * K, Np * K))
    e = np.zeros((Np, K))
    for i in range(Np * K):
        e[i % Np, i // Np] = 1.0
        A[:, i] = apply(e, t, mapD, kappa, sigma, tau).flatten("F")
        e[i % Np, i // Np] = 0.0
    return A


def is_singular(t, mapD, sigma):
    return sigma == 0 and np.asarray(mapD).size == 0


def right_hand_side(f, t, mapD, kappa=1.0, sigma=0.0, tau=None, g=None, qn=None):
    """b = f - A(0; g, qn), the mass-weighted mean removed in the singular case: what the iteration solves A u = b for."""
    b = f.copy()
    if g is not None or qn is not None:
        b = b - apply(np.zeros_like(f), t, mapD, kappa, sigma, tau, g, qn)
    if is_singular(t, mapD, sigma):
        b = b - mass_mean(b, t)
    return b


def cg(f, t, mapD, kappa=1.0, sigma=0.0, tau=None, g=None, qn=None, x0=None, relTol=1e-8, maxIterations=None, checkEvery=1):
    """Conjugate gradients in the mass inner product. Returns (u, info) with info = dict(iterations, relres (the recursive
    residual), trueres (|b - A u| / |b| in the mass norm), converged, projected)."""
    tau = penalty(t, kappa) if tau is None else tau
    singular = is_singular(t, mapD, sigma)
    A = lambda v: apply(v, t, mapD, kappa, sigma, tau)
    b = right_hand_side(f, t, mapD, kappa, sigma, tau, g, qn)
    bb = mass_dot(b, b, t)
    x = np.zeros_like(f) if x0 is None else np.array(x0, dtype=f.dtype)
    info = dict(iterations=0, relres=0.0, trueres=0.0, converged=True, projected=bool(singular))
    if bb == 0:
        return np.zeros_like(f), info
    maxIterations = f.size if maxIterations is None else maxIterations
    r = b - A(x) if np.any(x) else b.copy()
    if singular:
        r = r - mass_mean(r, t)
    s = mass_apply(r, t)
    rr = (r * s).sum()
    p = np.zeros_like(f)
    beta, it = 0.0, 0
    converged = np.sqrt(rr / bb) <= relTol
    while not converged and it < maxIterations:
        p = r + beta * p
        Ap = A(p)
        w = mass_apply(Ap, t)
        pAp = (p * w).sum()
        alpha = rr / pAp if pAp != 0 else 0.0
        x = x + alpha * p
        r = r - alpha * Ap
        s = s - alpha * w
        rrn = (r * s).sum()
        beta, rrPrev, rr = (rrn / rr if rr != 0 else 0.0), rr, rrn
        it += 1
        if it % checkEvery == 0 or it == maxIterations:
            if singular:
                r = r - mass_mean(r, t)
                s = mass_apply(r, t)
                rr = (r * s).sum()
                beta = rr / rrPrev if rrPrev != 0 else 0.0
            converged = np.sqrt(max(rr, 0.0) / bb) <= relTol
    if singular:
        x = x - mass_mean(x, t)
    res = b - A(x)
    if singular:
        res = res - mass_mean(res, t)
    info.update(iterations=it, relres=float(np.sqrt(max(rr, 0.0) / bb)), trueres=float(np.sqrt(mass_dot(res, res, t) / bb)),
                converged=bool(converged))
    return x, info


# ---- meshes and inputs shared by the CPU and GPU tests
def distorted_box(nx, ny, amount=0.25, seed=5):
    import tridiff_ref
    return tridiff_ref.distorted_box(nx, ny, amount, seed)


def box(nx=13, ny=11, seed=0):
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny, shuffleSeed=seed)
    return m


SHUFFLE_SEED = 7       # buildBoxMesh(13, 11) with a shuffled element order: 286 triangles, four full waves and a tail
KAPPA_SCALAR = 0.7
SIGMA = 2.5
_NODES, _PROBLEMS = {}, {}


def nodes_tables(order, nx=13, ny=11, seed=SHUFFLE_SEED):
    key = (order, nx, ny, seed)
    if key not in _NODES:
        nodes = dg.TriangleNodesProvisioner(order, box(nx, ny, seed))
        _NODES[key] = (nodes, tables(nodes))
    return _NODES[key]


def side_nodes(t, which):
    """Boundary face nodes on the sides named in `which` (a string of l, r, b, t) of the box [-1, 1]^2, as a mapD."""
    bnd = boundary_nodes(t)
    nx, ny = t["nx"].flatten("F"), t["ny"].flatten("F")
    on = np.zeros(bnd.size, dtype=bool)
    for c in which:
        on |= {"l": nx < -0.5, "r": nx > 0.5, "b": ny < -0.5, "t": ny > 0.5}[c]
    return np.nonzero(bnd & on)[0].astype(np.int32)


def kappa_elements(t, lo=0.4, hi=1.3):
    """One positive value per element."""
    xc, yc = t["x"].mean(axis=0), t["y"].mean(axis=0)
    return lo + (hi - lo) * (0.5 + 0.5 * np.sin(2 * xc + 0.3) * np.cos(3 * yc))


def jumping_field(t, seed=1):
    """A field that jumps at every face: smooth plus noise per node."""
    rng = np.random.default_rng(seed)
    return np.sin(2 * t["x"]) * np.cos(t["y"]) + 0.3 * rng.standard_normal(t["x"].shape)


def face_data(t, seed=2):
    """(g, qn): (3 Nfp, K) boundary data, nonzero at every face node (only the entries of the node's own kind are read)."""
    rng = np.random.default_rng(seed)
    shape = t["nx"].shape
    return 0.5 + rng.random(shape), -0.8 + 0.6 * rng.random(shape)


def operator_cases(order):
    """The GPU operator test's cases: name -> dict(mapD, kappa, sigma, g, qn), every one on nodes_tables(order), u = jumping_field."""
    _, t = nodes_tables(order)
    g, qn = face_data(t)
    everyD, mixed, none = all_boundary(t), side_nodes(t, "lb"), np.zeros(0, dtype=np.int32)
    ke = kappa_elements(t)
    return {
        "dirichlet": dict(mapD=everyD, kappa=KAPPA_SCALAR, sigma=0.0, g=None, qn=None),
        "dirichlet-data-sigma-kappaK": dict(mapD=everyD, kappa=ke, sigma=SIGMA, g=g, qn=None),
        "neumann": dict(mapD=none, kappa=KAPPA_SCALAR, sigma=0.0, g=None, qn=None),
        "neumann-data-sigma": dict(mapD=none, kappa=KAPPA_SCALAR, sigma=SIGMA, g=None, qn=qn),
        "mixed-kappaK": dict(mapD=mixed, kappa=ke, sigma=0.0, g=None, qn=None),
        "mixed-data-sigma": dict(mapD=mixed, kappa=KAPPA_SCALAR, sigma=SIGMA, g=g, qn=qn),
    }


def face_values(fn, t):
    """fn(x, y, nx, ny) at the face nodes, (3 Nfp, K)."""
    vM = np.asarray(t["vmapM"])
    x, y = t["x"].flatten("F")[vM], t["y"].flatten("F")[vM]
    return fn(x, y, t["nx"].flatten("F"), t["ny"].flatten("F")).reshape(t["nx"].shape, order="F")


def analytic_problem(name, t):
    """dict(mapD, kappa, sigma, f, g, qn, exact) of one of the analytic problems on [-1, 1]^2 (kappa = 1):
      sin       -lap u = 2 pi^2 sin(pi x) sin(pi y), u = 0 on all four sides
      cos       -lap u = 2 pi^2 cos(pi x) cos(pi y), du/dn = 0 on all four sides, mean 0
      harmonic  lap u = 0, u = exp(x) cos(y): Dirichlet data left and right, Neumann data top and bottom
      euler     one backward-Euler step (1/dt - kappa lap) u = u_old / dt, kappa = 0.05, dt = 0.1, u_old = exp(-4 (x^2 + y^2)),
                Dirichlet data on three sides (left, right, bottom) and Neumann data on the top; no closed form (exact = None)"""
    x, y = t["x"], t["y"]
    pi = np.pi
    if name == "sin":
        ex = np.sin(pi * x) * np.sin(pi * y)
        return dict(mapD=all_boundary(t), kappa=1.0, sigma=0.0, f=2 * pi * pi * ex, g=None, qn=None, exact=ex)
    if name == "cos":
        ex = np.cos(pi * x) * np.cos(pi * y)
        return dict(mapD=np.zeros(0, dtype=np.int32), kappa=1.0, sigma=0.0, f=2 * pi * pi * ex, g=None, qn=None, exact=ex)
    if name == "harmonic":
        ex = np.exp(x) * np.cos(y)
        g = face_values(lambda x, y, nx, ny: np.exp(x) * np.cos(y), t)
        qn = face_values(lambda x, y, nx, ny: nx * np.exp(x) * np.cos(y) - ny * np.exp(x) * np.sin(y), t)
        return dict(mapD=side_nodes(t, "lr"), kappa=1.0, sigma=0.0, f=np.zeros_like(x), g=g, qn=qn, exact=ex)
    if name == "euler":
        kappa, dt = 0.05, 0.1
        old = np.exp(-4 * (x * x + y * y))
        g = face_values(lambda x, y, nx, ny: np.exp(-4 * (x * x + y * y)), t)
        qn = face_values(lambda x, y, nx, ny: 0.02 * np.cos(2 * x), t)
        return dict(mapD=side_nodes(t, "lrb"), kappa=kappa, sigma=1.0 / dt, f=old / dt, g=g, qn=qn, exact=None)
    raise KeyError(name)


PROBLEMS = ("sin", "cos", "harmonic", "euler")
SOLVE_ORDERS = (1, 4, 8)
REL_TOL = 1e-10
CHECK_EVERY = 8


def solve_problem(name, order):
    """The GPU solve test's input, once per (name, order): analytic_problem on nodes_tables(order)."""
    key = (name, order)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = analytic_problem(name, nodes_tables(order)[1])
    return _PROBLEMS[key]


def operator_args(p):
    return dict(mapD=p["mapD"], kappa=p["kappa"], sigma=p["sigma"], g=p["g"], qn=p["qn"])


_REFERENCE_SOLVES = {}


def reference_solve(name, order):
    """cg() on solve_problem(name, order) at REL_TOL and CHECK_EVERY, once: (u, info). What the device solver's iteration count
    and true residual are held against."""
    key = (name, order)
    if key not in _REFERENCE_SOLVES:
        p = solve_problem(name, order)
        _REFERENCE_SOLVES[key] = cg(p["f"], nodes_tables(order)[1], relTol=REL_TOL, checkEvery=CHECK_EVERY, **operator_args(p))
    return _REFERENCE_SOLVES[key]


def true_residual(u, p, t):
    """|b - A u| / |b| in the mass norm (the mean of b - A u removed in the singular case), in the dtype of u."""
    b = right_hand_side(p["f"], t, p["mapD"], p["kappa"], p["sigma"], None, p["g"], p["qn"])
    res = b - apply(u, t, p["mapD"], p["kappa"], p["sigma"])
    if is_singular(t, p["mapD"], p["sigma"]):
        res = res - mass_mean(res, t)
    return float(np.sqrt(mass_dot(res, res, t) / mass_dot(b, b, t)))


# ---- backward Euler against explicit steps (the loop of examples/heat2d.py)
HEAT_ORDER, HEAT_MESH, HEAT_KAPPA, HEAT_STEPS, HEAT_RATIO, HEAT_REL_TOL = 3, (5, 4), 0.05, 10, 50, 1e-12
_HEAT = {}


def diffusion_dt(kappa, order, t, c=4.0):
    """The explicit tracer diffusion's step size, c / (kappa (N+1)^4 max(Fscale)^2) (tridiff_ref.diffusion_dt)."""
    return c / (kappa * (order + 1) ** 4 * np.abs(t["Fscale"]).max() ** 2)


def heat_reference():
    """dp/dt = -A(p; g, qn) with sigma = 0, kappa = HEAT_KAPPA on buildBoxMesh(5, 4) at N = 3, Dirichlet data on the left, right
    and bottom and Neumann data on the top, from a Gaussian: HEAT_STEPS backward-Euler steps of dt = HEAT_RATIO diffusionDt by
    direct solves with the dense operator (`implicit`), HEAT_STEPS HEAT_RATIO forward-Euler steps of diffusionDt (`explicit`), the
    exact exponential (`exact`), and `bound` = max|implicit - exact| + max|explicit - exact| + `allowance`: both schemes are
    first-order, so the first two terms are the time discretisation's first-order error between them. `allowance` is what steps
    solved iteratively to HEAT_REL_TOL may add: a residual of relative size eps in (1/dt + A) p = b moves p by at most
    dt eps |b| in the mass norm (the smallest eigenvalue of 1/dt + A is at least 1/dt), |b| <= |p_old| / dt + |c|, backward Euler
    does not amplify it, and max|v| <= |v|_M / sqrt(lambda_min(J M)): HEAT_STEPS eps (|start|_M + dt |c|_M) / sqrt(lambda_min). rho_dt = diffusionDt rho(A) must stay below 2 for the
    explicit steps to be stable (asserted by tests/test_poisson_reference.py)."""
    if not _HEAT:
        nodes = dg.TriangleNodesProvisioner(HEAT_ORDER, box(*HEAT_MESH, seed=3))
        t = tables(nodes)
        x, y = t["x"], t["y"]
        p = dict(mapD=side_nodes(t, "lrb"), kappa=HEAT_KAPPA, sigma=0.0,
                 g=face_values(lambda x, y, nx, ny: 0.2 + 0.1 * x * y, t), qn=face_values(lambda x, y, nx, ny: 0.02 * np.cos(2 * x), t))
        start = np.exp(-4 * (x * x + y * y))
        dte = diffusion_dt(HEAT_KAPPA, HEAT_ORDER, t)
        dt = HEAT_RATIO * dte
        A = dense_operator(t, p["mapD"], p["kappa"], 0.0)
        c = apply(np.zeros_like(start), t, **p).flatten("F")
        n = A.shape[0]
        u = start.flatten("F")
        for _ in range(HEAT_STEPS * HEAT_RATIO):
            u = u - dte * (A @ u + c)
        B = np.eye(n) / dt + A
        v = start.flatten("F")
        for _ in range(HEAT_STEPS):
            v = np.linalg.solve(B, v / dt - c)
        lam, V = np.linalg.eig(A)
        steady = -np.linalg.solve(A, c)
        T = HEAT_STEPS * dt
        exact = steady + (V @ (np.exp(-T * lam) * np.linalg.solve(V, start.flatten("F") - steady))).real
        shape = start.shape
        back = lambda a: a.reshape(shape, order="F")
        lmin = np.linalg.eigvalsh(t["Vinv"].T @ t["Vinv"]).min() * t["J"].min()
        mnorm = lambda a: np.sqrt(mass_dot(back(a), back(a), t))
        allowance = HEAT_STEPS * HEAT_REL_TOL * (mnorm(start.flatten("F")) + dt * mnorm(c)) / np.sqrt(lmin)
        _HEAT.update(tables=t, problem=p, start=start, dt=dt, rho_dt=dte * np.abs(lam).max(), explicit=back(u), implicit=back(v),
                     exact=back(exact), allowance=allowance,
                     bound=np.abs(v - exact).max() + np.abs(u - exact).max() + allowance)
    return _HEAT
