"""NumPy restatement of the drifters of the quadrilateral sw2d solver (csrc/hip/sw2d_quad_drifter_kernel.hpp), written from the
algorithm's text and not from the kernel; the dtype is a parameter (np.float64, or np.longdouble as tests/quadref_ld.py uses it).

Element tables (tables()): per element the bilinear map of its corner nodes 0, (N+1) N, N, Np - 1 (node (N+1) j + i sits at
r = r1d[j], s = r1d[i]), x(r, s) = xc + ax r + bx s + cx r s; neigh[f][k] for the faces f = 0..3 = (s = -1, r = +1, s = +1,
r = -1) from EToE: the neighbour, -1 for a wall, -2 for a boundary face with a node in mapO; the barycentric weights
c_a = 1 / prod_{b != a} (r1d[a] - r1d[b]).

locate: at most 32 hops; in each, Newton on the bilinear map of k from (0, 0), at most 12 iterations, stopped at
max(|dr|, |ds|) <= 1e-14; lost (2) on a determinant that is not positive and finite, an iterate that is not finite or a last step
above 1e-10. Violations (-1 - s, r - 1, s - 1, -1 - r): the largest <= 1e-12 is found; otherwise across the face of the largest
(lowest index on a tie): to the neighbour, clamped at a wall (bit 4, same element again), exited (1) at an open face.

velocity: u = hu / h, v = hv / h at the nodes, value = sum_i ls[i] (sum_j lr[j] f[(N+1) j + i]) with both sums ascending, lr and
ls by the second barycentric form (on a node the unit vector).

advance (Heun): predictor from (u0, v0), located from k, velocity there; corrector with the mean, located from the old k;
(u0, v0) sampled at the new position. An open face met by the predictor only ends its search. A lost drifter stays where it was.

Every decision records how close it came: a drifter is flagged when a violation of any face, at any decision, lay within 1e-9
of the 1e-12 threshold (a coordinate within 1e-9 of 1 + 1e-12): there the float64 device may decide the other way."""
import numpy as np

HOPS, NEWTON = 32, 12
EXITED, LOST, TOUCHED = 1, 2, 4
WALL, OPEN = -1, -2


class Tables:
    pass


def tables(nodes, mesh, mapO=None, dtype=np.float64):
    """The element tables of `nodes` (a QuadNodesProvisioner on `mesh`) in `dtype`."""
    ctx = nodes.dgContext()
    N, Np, Nq, K = nodes._dims()
    x, y = np.asarray(ctx.x, dtype=dtype), np.asarray(ctx.y, dtype=dtype)
    T = Tables()
    T.N, T.K, T.dtype = N, K, dtype
    T.r1d = np.asarray(ctx.r, dtype=dtype).reshape(Nq, Nq)[:, 0].copy()
    c00, c10, c01, c11 = 0, Nq * N, N, Np - 1
    four = dtype(4)
    bil = np.empty((K, 8), dtype=dtype)
    for c, g in enumerate((x, y)):
        bil[:, 4 * c + 0] = (g[c00] + g[c10] + g[c01] + g[c11]) / four
        bil[:, 4 * c + 1] = (g[c10] - g[c00] + g[c11] - g[c01]) / four
        bil[:, 4 * c + 2] = (g[c01] - g[c00] + g[c11] - g[c10]) / four
        bil[:, 4 * c + 3] = (g[c00] - g[c10] - g[c01] + g[c11]) / four
    T.bil = bil
    EToE = np.asarray(mesh.EToE).reshape(K, 4)
    boundary = EToE == np.arange(K)[:, None]
    opened = np.zeros((K, 4), dtype=bool)
    mo = np.asarray([] if mapO is None else mapO, dtype=np.int64).reshape(-1)
    opened[mo // (4 * Nq), mo % (4 * Nq) // Nq] = True
    T.neigh = np.where(boundary, np.where(opened, OPEN, WALL), EToE).T.astype(np.int64).copy()      # [f][k]
    T.bary = np.array([dtype(1) / np.prod([T.r1d[a] - T.r1d[b] for b in range(Nq) if b != a], dtype=dtype) for a in range(Nq)],
                      dtype=dtype)
    return T


def map_xy(T, k, r, s):
    c = T.bil[k]
    return c[:, 0] + (c[:, 1] * r + c[:, 2] * s + c[:, 3] * (r * s)), c[:, 4] + (c[:, 5] * r + c[:, 6] * s + c[:, 7] * (r * s))


def locate(T, x, y, k, flag):
    """(res, x, y, k, r, s, wall) for the points (x, y) searched from the elements k; res 0 found, EXITED or LOST. flag (bool per
    point) is or-ed in place."""
    dt = T.dtype
    n = len(x)
    x, y, k = x.copy(), y.copy(), k.copy()
    r, s = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    res = np.full(n, -1)
    wall = np.zeros(n, dtype=np.int64)
    one = dt(1)
    with np.errstate(all="ignore"):
        for _ in range(HOPS):
            act = np.nonzero(res < 0)[0]
            if not act.size:
                break
            xc, ax, bx, cx, yc, ay, by, cy = T.bil[k[act]].T
            dx, dy = x[act] - xc, y[act] - yc
            m = act.size
            rr, ss = np.zeros(m, dtype=dt), np.zeros(m, dtype=dt)
            step = np.full(m, np.inf, dtype=dt)
            lost, live = np.zeros(m, dtype=bool), np.ones(m, dtype=bool)
            for _ in range(NEWTON):
                if not live.any():
                    break
                fx = ax * rr + bx * ss + cx * (rr * ss) - dx
                fy = ay * rr + by * ss + cy * (rr * ss) - dy
                j11, j12, j21, j22 = ax + cx * ss, bx + cx * rr, ay + cy * ss, by + cy * rr
                det = j11 * j22 - j12 * j21
                bad = live & ~((det > 0) & np.isfinite(det))
                lost |= bad
                live &= ~bad
                dr, ds = (j12 * fy - j22 * fx) / det, (j21 * fx - j11 * fy) / det
                rr, ss = np.where(live, rr + dr, rr), np.where(live, ss + ds, ss)
                bad = live & ~(np.isfinite(rr) & np.isfinite(ss))
                lost |= bad
                live &= ~bad
                step = np.where(live, np.maximum(np.abs(dr), np.abs(ds)), step)
                live &= ~(step <= dt(1e-14))
            lost |= ~(step <= dt(1e-10))
            viol = np.stack([-one - ss, rr - one, ss - one, -one - rr], axis=1)
            f = np.argmax(viol, axis=1)                                   # the first maximum: the lowest face on a tie
            worst = viol[np.arange(m), f]
            flag[act] |= ~lost & (np.abs(viol - dt(1e-12)) < dt(1e-9)).any(axis=1)
            found = ~lost & (worst <= dt(1e-12))
            nb = T.neigh[f, k[act]]
            hop = ~lost & ~found & (nb >= 0)
            clamp = ~lost & ~found & (nb == WALL)
            out = ~lost & ~found & (nb == OPEN)
            ss = np.where(clamp & (f == 0), -one, np.where(clamp & (f == 2), one, ss))
            rr = np.where(clamp & (f == 1), one, np.where(clamp & (f == 3), -one, rr))
            r[act], s[act] = rr, ss
            xn = xc + (ax * rr + bx * ss + cx * (rr * ss))
            yn = yc + (ay * rr + by * ss + cy * (rr * ss))
            x[act] = np.where(clamp, xn, x[act])
            y[act] = np.where(clamp, yn, y[act])
            wall[act] |= np.where(clamp, TOUCHED, 0)
            k[act] = np.where(hop, nb, k[act])
            res[act] = np.where(lost, LOST, np.where(found, 0, np.where(out, EXITED, -1)))
    res[res < 0] = LOST
    return res, x, y, k, r, s, wall


def basis(T, r):
    """(n, N+1): second barycentric form at the abscissae r; on a node the unit vector."""
    with np.errstate(all="ignore"):
        d = r[:, None] - T.r1d[None, :]
        t = T.bary[None, :] / d
        tot = np.zeros(len(r), dtype=T.dtype)
        for a in range(t.shape[1]):
            tot = tot + t[:, a]
        b = t / tot[:, None]
    on = d == 0
    return np.where(on.any(axis=1)[:, None], on.astype(T.dtype), b)


def velocity(T, q, k, r, s):
    """(u, v, finite) at (k, r, s) from the state q = (h, hu, hv, ...), each (Np, K)."""
    Nq = T.N + 1
    h = np.asarray(q[0], dtype=T.dtype)[:, k]                              # (Np, n)
    lr, ls = basis(T, r), basis(T, s)
    out = []
    with np.errstate(all="ignore"):
        for c in (1, 2):
            f = (np.asarray(q[c], dtype=T.dtype)[:, k] / h).reshape(Nq, Nq, -1)   # [j][i][point]
            val = np.zeros(len(k), dtype=T.dtype)
            for i in range(Nq):
                acc = np.zeros(len(k), dtype=T.dtype)
                for j in range(Nq):
                    acc = acc + lr[:, j] * f[j, i]
                val = val + ls[:, i] * acc
            out.append(val)
    return out[0], out[1], np.isfinite(out[0]) & np.isfinite(out[1])


class Drifters:
    """The drifters' state (x, y, k, r, s, u0, v0, status) and the near-edge flag."""

    def __init__(self, T, q, element, r, s):
        dt = T.dtype
        self.T = T
        self.k = np.asarray(element, dtype=np.int64).copy()
        self.r, self.s = np.asarray(r, dtype=dt).copy(), np.asarray(s, dtype=dt).copy()
        self.x, self.y = map_xy(T, self.k, self.r, self.s)
        self.status = np.zeros(len(self.k), dtype=np.int64)
        self.flag = np.zeros(len(self.k), dtype=bool)
        self.u0, self.v0 = np.zeros(len(self.k), dtype=dt), np.zeros(len(self.k), dtype=dt)
        self.sample(q)

    def moving(self):
        return (self.status & (EXITED | LOST)) == 0

    def sample(self, q):
        """(u0, v0) from the state q (after the state under the drifters has been replaced)."""
        a = np.nonzero(self.moving())[0]
        u, v, ok = velocity(self.T, q, self.k[a], self.r[a], self.s[a])
        self.u0[a], self.v0[a] = u, v
        self.status[a] |= np.where(ok, 0, LOST)

    def advance(self, q, dt):
        """One Heun advance by dt in the state q."""
        T = self.T
        dt = T.dtype(dt)
        a = np.nonzero(self.moving())[0]
        if not a.size:
            return
        x, y, k, u0, v0 = self.x[a], self.y[a], self.k[a], self.u0[a], self.v0[a]
        flag = self.flag[a]
        res, _, _, kp, rp, sp, wall = locate(T, x + dt * u0, y + dt * v0, k, flag)
        up, vp, ok = velocity(T, q, kp, rp, sp)
        ok &= res != LOST
        half = T.dtype(0.5) * dt
        with np.errstate(all="ignore"):
            xn, yn = x + half * (u0 + up), y + half * (v0 + vp)
        sub = np.nonzero(ok)[0]                                            # the corrector of those the predictor kept
        res2 = np.full(len(a), LOST)
        kc, rn, sn, un, vn = k.copy(), self.r[a].copy(), self.s[a].copy(), u0.copy(), v0.copy()
        if sub.size:
            f2 = flag[sub]
            r2, xs, ys, ks, rs, ss, w2 = locate(T, xn[sub], yn[sub], k[sub], f2)
            flag[sub] = f2
            wall[sub] |= w2
            us, vs, fin = velocity(T, q, ks, rs, ss)
            keep = (r2 == EXITED) | ((r2 == 0) & fin)
            r2 = np.where(keep, r2, LOST)
            res2[sub] = r2
            xn[sub], yn[sub], kc[sub], rn[sub], sn[sub] = xs, ys, ks, rs, ss
            un[sub] = np.where(r2 == 0, us, u0[sub])
            vn[sub] = np.where(r2 == 0, vs, v0[sub])
        done = res2 != LOST
        self.x[a], self.y[a] = np.where(done, xn, x), np.where(done, yn, y)
        self.k[a] = np.where(done, kc, k)
        self.r[a], self.s[a] = np.where(done, rn, self.r[a]), np.where(done, sn, self.s[a])
        self.u0[a], self.v0[a] = np.where(done, un, u0), np.where(done, vn, v0)
        self.status[a] |= wall | np.where(done, res2, LOST)
        self.flag[a] = flag

    def xy(self):
        return np.stack([np.asarray(self.x, dtype=np.float64), np.asarray(self.y, dtype=np.float64)], axis=1)


def rotation_state(x, y, omega, h0=2.0):
    """Solid-body rotation about the origin: h constant, hu = -h omega y, hv = h omega x (degree 1: interpolated exactly)."""
    h = np.full_like(x, h0)
    return h, -h * omega * y, h * omega * x


def heun_rotation(z0, theta, n):
    """Heun on dz/dt = i omega z: z_n = z_0 (1 + i theta - theta^2 / 2)^n, theta = omega dt, in complex longdouble."""
    g = np.clongdouble(1 - np.longdouble(theta) ** 2 / 2 + 1j * np.longdouble(theta))
    return np.asarray(z0, dtype=np.clongdouble) * g ** n


# ---- the cases tests/test_quad_drifter_setup.py measures on the CPU and tests/test_sw2d_quads_drifters_gpu.py runs on the device

ROTATION_CASES = [("shear", 1, 63), ("shear", 4, 300), ("shear", 12, 1), ("jitter", 1, 300), ("jitter", 8, 63), ("jitter", 12, 63),
                  ("small", 4, 1), ("small", 8, 300)]
ROTATION_STEPS = 40                                                        # about a quarter turn
WALL_CASES = [("jitter", 4, 63), ("shear", 8, 300), ("small", 1, 63), ("small", 12, 1)]
WALL_STEPS, WALL_DT, WALL_UV = 45, 0.05, (1.0, 0.6)
MOVING_CASES = {"rk2": ("jitter", 4, 6), "lserk": ("shear", 8, 4), "heun3": ("jitter", 4, 5), "heun4": ("shear", 8, 4)}
MOVING_DRIFTERS = 63

_MESH = {}


def mesh_case(name, order):
    """(nodes, tables, mesh) of `shear`, `jitter` (tests/quadref_ld.py) or `small`, the jittered 5 x 4 box of tests/golden."""
    import blitzdg_amd.pyblitzdg as dg
    import quadref
    import quadref_ld
    key = (name, order)
    if key not in _MESH:
        if name == "small":
            d = np.load(f"{quadref.GOLDEN}/sw2dq_rhs_jitter_box5x4_N5.npz")
            mesh = dg.MeshManager()
            mesh.buildMesh(d["EToV"], d["Vert"])
            nodes = dg.QuadNodesProvisioner(order, mesh)
            nodes.buildFilter(0.99 * order, 4)
            _MESH[key] = (nodes, quadref.tables(nodes.dgContext()), mesh)
        else:
            nodes, t = quadref_ld.mesh_tables(name, order)
            _MESH[key] = (nodes, t, nodes._mesh)
    return _MESH[key]


def boundary_segments(T, t):
    """(f, k, a, b): the boundary faces and their end points a, b (each (m, 2))."""
    Nq = T.N + 1
    ends = [(0, Nq * T.N), (Nq * T.N, Nq * Nq - 1), (T.N, Nq * Nq - 1), (0, T.N)]     # faces s = -1, r = +1, s = +1, r = -1
    f, k = np.nonzero(T.neigh < 0)
    a = np.array([[t["x"][ends[i][0], j], t["y"][ends[i][0], j]] for i, j in zip(f, k)])
    b = np.array([[t["x"][ends[i][1], j], t["y"][ends[i][1], j]] for i, j in zip(f, k)])
    return f, k, a, b


def domain(T, t):
    """(centre, radius of the largest circle about it that stays clear of the boundary, size of the domain)."""
    _, _, a, b = boundary_segments(T, t)
    c = 0.5 * (a.mean(axis=0) + b.mean(axis=0))
    ab = b - a
    u = np.clip(((c - a) * ab).sum(axis=1) / (ab * ab).sum(axis=1), 0, 1)
    dist = np.hypot(*(a + u[:, None] * ab - c).T)
    size = max(np.ptp(t["x"]), np.ptp(t["y"]))
    return c, dist.min(), size


def side_nodes(name, t, T):
    """mapO of the open side of the wall cases: the flat face-node indices of the boundary faces on the side x = +1 of the box
    (of the box before the shear)."""
    import quadref_ld
    Nq = T.N + 1
    f, k, a, b = boundary_segments(T, t)
    if name == "shear":
        inv = np.linalg.inv(quadref_ld.SHEAR).T
        a, b = a @ inv, b @ inv
    xmax = max(a[:, 0].max(), b[:, 0].max())
    on = (np.abs(a[:, 0] - xmax) < 1e-9) & (np.abs(b[:, 0] - xmax) < 1e-9)
    return np.concatenate([(k[i] * 4 + f[i]) * Nq + np.arange(Nq) for i in np.nonzero(on)[0]]).astype(np.int32)


def disc_points(nodes, c, radius, n, seed, inner=0.15, outer=0.9):
    """(element, r, s) of n seeded points with inner radius <= |p - c| <= outer radius."""
    rng = np.random.default_rng([seed, n])
    rad, ang = radius * np.sqrt(rng.uniform(inner ** 2, outer ** 2, n)), rng.uniform(0, 2 * np.pi, n)
    el, r, s = nodes.locatePoints(c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang))
    assert (el >= 0).all()
    return el, r, s


def rotation_problem(name, order, n):
    """(nodes, t, mesh, T64, state, (element, r, s), omega, dt, centre, size) of a frozen-rotation case."""
    nodes, t, mesh = mesh_case(name, order)
    T = tables(nodes, mesh)
    c, radius, size = domain(T, t)
    omega = 1.0
    dt = 0.5 * np.pi / omega / ROTATION_STEPS
    q = rotation_state(t["x"] - c[0], t["y"] - c[1], omega)
    return nodes, t, mesh, T, q, disc_points(nodes, c, radius, n, seed=order), omega, dt, c, size


def uniform_state(t, uv=WALL_UV, h0=2.0):
    h = np.full_like(t["x"], h0)
    return h, h * uv[0], h * uv[1]


def wall_problem(name, order, n):
    """(nodes, t, mesh, state, (element, r, s), mapO of the side x = +1, size) of a wall case: a uniform oblique flow that
    carries every drifter to the top or the right side within WALL_STEPS steps of WALL_DT."""
    nodes, t, mesh = mesh_case(name, order)
    T = tables(nodes, mesh)
    c, radius, size = domain(T, t)
    return nodes, t, mesh, uniform_state(t), disc_points(nodes, c, radius, n, seed=100 + order), side_nodes(name, t, T), size


def bump_state(t):
    """A Gaussian bump on still water of depth 2 with a gentle swirl: the flow it starts is discontinuous at the faces."""
    x, y = t["x"], t["y"]
    h = 2.0 + 0.3 * np.exp(-6 * ((x - 0.1) ** 2 + (y + 0.05) ** 2))
    return [h, h * 0.3 * np.sin(2 * x + 1) * np.cos(y), h * 0.2 * np.cos(x) * np.sin(2 * y - 1)]


def moving_points(nodes, t, mesh):
    T = tables(nodes, mesh)
    c, radius, _ = domain(T, t)
    return disc_points(nodes, c, radius, MOVING_DRIFTERS, seed=7, inner=0.05, outer=0.8)


def moving_problem(kind):
    """The moving-flow case `kind` of MOVING_CASES: dict(nodes, t, mesh, q0, dt, steps, points, mapO, fields, t0, step), where
    step(q, time) -> (q, time) is one step of that case's scheme in the float64 NumPy restatement (quadref.py for stepRK2 and
    lserk4Stages, quadrefB.py / quadrefB4.py for variant B's stepSSPRK2 on three and four fields)."""
    import blitzdg_amd.pyblitzdg as dg
    import quadref
    import quadref4
    import quadref_ld
    name, order, steps = MOVING_CASES[kind]
    if kind in ("rk2", "lserk"):
        nodes, t, mesh = mesh_case(name, order)
        q0 = bump_state(t)
        dt = quadref4.compute_dt(*q0, quadref_ld.G, t, quadref_ld.CFL)[0]

        def rhs(q):
            return quadref.rhs(*q, quadref_ld.G, t)

        def step(q, time):
            if kind == "rk2":
                q1 = [a + 0.5 * dt * (t["Filter"] @ b) for a, b in zip(q, rhs(q))]
                return [a + dt * (t["Filter"] @ b) for a, b in zip(q, rhs(q1))], time + dt
            res = [np.zeros_like(a) for a in q]
            for i in range(5):
                res = [dg.LSERK4.rk4a[i] * x + dt * y for x, y in zip(res, rhs(q))]
                q = [x + dg.LSERK4.rk4b[i] * y for x, y in zip(q, res)]
            return q, time + dt
        mapO, t0, fields = None, 0.0, 3
    else:
        import quadrefB as B
        import quadrefB4 as B4
        import test_sw2d_quadsB4_gpu as vb4
        import test_sw2d_quadsB_gpu as vb3
        if kind == "heun3":
            nodes, t, vb, sp, q0, dt = vb3.problem(name, order)
            heun, fields = B.heun_steps, 3
        else:
            nodes, t, vb, sp, q0, dt, per_node = vb4.problem4(name, order)
            vb = dict(vb, tracer=per_node)
            heun, fields = B4.heun_steps, 4
        mesh, mapO, t0 = nodes._mesh, t["mapO"], vb3.T0

        def step(q, time):
            return heun(q, t, vb, dt, 1, time=time, sponge_coeff=sp)
    return dict(nodes=nodes, t=t, mesh=mesh, q0=[np.array(a) for a in q0], dt=dt, steps=steps, mapO=mapO, fields=fields, t0=t0,
                step=step, points=moving_points(nodes, t, mesh))
