"""NumPy restatement of the drifters of the triangle sw2d solver (csrc/hip/sw2d_drifter_kernel.hpp), written from the algorithm's
text in that header and not from the kernel; the dtype is a parameter (np.float64 or np.longdouble).

Element tables (tables()): per element the corner nodes v0, v1, v2 at (r, s) = (-1, -1), (1, -1), (-1, 1) (face 0, s = -1, runs
from v0 to v1, face 1, r + s = 0, from v1 to v2, face 2, r = -1, from v2 to v0), e1 = v1 - v0, e2 = v2 - v0 and the affine map
x(r, s) = x0 + ((0.5 (1 + r)) e1x + (0.5 (1 + s)) e2x); neigh[f][k] from EToE: the neighbour, -1 for a wall, -2 for a boundary
face with a node in mapO ((3 k + f) Nfp + i); Vinv; the recurrences p_0 = A_0, p_n = (A_n x + B_n) p_{n-1} + C_n p_{n-2} of
sqrt(2) P_n^(0,0) (row 0) and the orthonormal P_n^(2i+1,0) (row i + 1), formed in longdouble.

locate: at most 32 hops; in each the closed-form inverse of the affine map, r = 2 ((dx e2y - e2x dy) / det) - 1,
s = 2 ((e1x dy - dx e1y) / det) - 1; not finite: lost (2). Violations (-1 - s, r + s, -1 - r): the largest <= 1e-12 is found;
otherwise across the face of the largest (lowest index on a tie): to the neighbour; exited (1) at an open face; at a wall the
point is projected onto the face's line (t not clamped), bit 4, same element again -- unless an earlier wall crossing of the same
search was at another face than the first one crossed: then the point goes to the nearer end vertex of the face now crossed (the
first vertex on a tie). Hops used up: lost.

velocity: u = hu / h, v = hv / h at the nodes, value = sum_n row[n] f[n], row[n] = sum_m P_m Vinv[m, n], every sum ascending.
In float64 P is the header's recurrence ((L_i(a) (1 - b)^i) J^i_j(b), the power by repeated multiplication); in longdouble P and
the rows are trimon_ref.simplex_ld / rows_ld, the basis by its own recurrence with its own square roots: the longdouble run does
not depend on the coefficient table.

advance (Heun): predictor from (u0, v0), located from k, velocity there; corrector with the mean, located from the old k;
(u0, v0) sampled at the new position. An open face met by the predictor only ends its search. A lost drifter stays where it was.

Every decision records how close it came: a drifter is flagged when a violation of any face, at any decision, lay within 1e-9
of the 1e-12 threshold: there the float64 device may decide the other way."""
import numpy as np

import trimon_ref as tri
from quaddrift_ref import heun_rotation, rotation_state                     # noqa: F401  (geometry-agnostic)

LD = np.longdouble
HOPS = 32
EXITED, LOST, TOUCHED = 1, 2, 4
WALL, OPEN = -1, -2
G = 9.81


class Tables:
    pass


def corner_nodes(r, s):
    """The nodes nearest (-1, -1), (1, -1), (-1, 1)."""
    return [int(np.argmin(np.hypot(r - a, s - b))) for a, b in ((-1, -1), (1, -1), (-1, 1))]


def jacobi_table(N):
    """(N + 2, N + 1, 3) longdouble: (A, B, C) of sqrt(2) P_n^(0,0) (row 0) and the orthonormal P_n^(2i+1,0) (row i + 1)."""
    out = np.zeros((N + 2, N + 1, 3), dtype=LD)
    for g in range(N + 2):
        al = LD(0) if g == 0 else LD(2 * (g - 1) + 1)

        def a(m):
            h = 2 * LD(m) + al
            return 2 / h * (m * (m + al)) / np.sqrt((h - 1) * (h + 1))
        for n in range(N + 1):
            if n == 0:
                A = np.sqrt((al + 1) / LD(2) ** (al + 1)) * (np.sqrt(LD(2)) if g == 0 else 1)
                B = C = LD(0)
            elif n == 1:
                w = np.sqrt((al + 3) / (al + 1))
                A, B, C = (al + 2) / 2 * w, al / 2 * w, LD(0)
            else:
                h = 2 * LD(n - 1) + al
                A, B, C = 1 / a(n), al * al / (h * (h + 2)) / a(n), -a(n - 1) / a(n)
            out[g, n] = A, B, C
    return out


def tables(nodes, mesh, mapO=None, dtype=np.float64):
    """The element tables of `nodes` (a TriangleNodesProvisioner on `mesh`) in `dtype`."""
    ctx = nodes.dgContext()
    N, Np, Nfp, K = nodes._dims()
    T = Tables()
    T.N, T.Np, T.K, T.dtype = N, Np, K, dtype
    c = corner_nodes(np.asarray(ctx.r), np.asarray(ctx.s))
    x, y = np.asarray(ctx.x, dtype=dtype), np.asarray(ctx.y, dtype=dtype)
    T.vert = np.stack([x[c[0]], y[c[0]], x[c[1]], y[c[1]], x[c[2]], y[c[2]]], axis=1)
    EToE = np.asarray(mesh.EToE).reshape(K, 3)
    boundary = EToE == np.arange(K)[:, None]
    opened = np.zeros((K, 3), dtype=bool)
    mo = np.asarray([] if mapO is None else mapO, dtype=np.int64).reshape(-1)
    opened[mo // (3 * Nfp), mo % (3 * Nfp) // Nfp] = True
    T.neigh = np.where(boundary, np.where(opened, OPEN, WALL), EToE).T.astype(np.int64).copy()      # [f][k]
    T.Vinv64 = np.asarray(ctx.Vinv, dtype=np.float64)
    T.Vinv = T.Vinv64.astype(dtype)
    T.jac = np.asarray(jacobi_table(N), dtype=np.float64).astype(dtype)       # the device's table is the rounded one
    return T


def map_xy(T, k, r, s):
    v = T.vert[k]
    half, one = T.dtype(0.5), T.dtype(1)
    wr, ws = half * (one + r), half * (one + s)
    return v[:, 0] + (wr * (v[:, 2] - v[:, 0]) + ws * (v[:, 4] - v[:, 0])), v[:, 1] + (wr * (v[:, 3] - v[:, 1]) + ws * (v[:, 5] - v[:, 1]))


def locate(T, x, y, k, flag):
    """(res, x, y, k, r, s, wall) for the points (x, y) searched from the elements k; res 0 found, EXITED or LOST. flag (bool per
    point) is or-ed in place."""
    dt = T.dtype
    n = len(x)
    x, y, k = x.copy(), y.copy(), k.copy()
    r, s = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    res = np.full(n, -1)
    wall = np.zeros(n, dtype=np.int64)
    wk, wf = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    one, two = dt(1), dt(2)
    with np.errstate(all="ignore"):
        for _ in range(HOPS):
            act = np.nonzero(res < 0)[0]
            if not act.size:
                break
            m = act.size
            ka = k[act]
            x0, y0, x1, y1, x2, y2 = T.vert[ka].T
            e1x, e1y, e2x, e2y = x1 - x0, y1 - y0, x2 - x0, y2 - y0
            det = e1x * e2y - e2x * e1y
            px, py = x[act], y[act]
            dx, dy = px - x0, py - y0
            rr = two * ((dx * e2y - e2x * dy) / det) - one
            ss = two * ((e1x * dy - dx * e1y) / det) - one
            lost = ~(np.isfinite(rr) & np.isfinite(ss))
            viol = np.stack([-one - ss, rr + ss, -one - rr], axis=1)
            viol_cmp = np.where(np.isnan(viol), -np.inf, viol)
            f = np.argmax(viol_cmp, axis=1)                               # the first maximum: the lowest face on a tie
            worst = viol[np.arange(m), f]
            flag[act] |= ~lost & (np.abs(viol - dt(1e-12)) < dt(1e-9)).any(axis=1)
            found = ~lost & (worst <= dt(1e-12))
            nb = T.neigh[f, ka]
            go = ~lost & ~found
            hop = go & (nb >= 0)
            atwall = go & (nb == WALL)
            out = go & (nb == OPEN)
            ax = np.where(f == 0, x0, np.where(f == 1, x1, x2))
            ay = np.where(f == 0, y0, np.where(f == 1, y1, y2))
            bx = np.where(f == 0, x1, np.where(f == 1, x2, x0))
            by = np.where(f == 0, y1, np.where(f == 1, y2, y0))
            corner = atwall & (wk[act] >= 0) & ((wk[act] != ka) | (wf[act] != f))
            da = (px - ax) * (px - ax) + (py - ay) * (py - ay)
            db = (px - bx) * (px - bx) + (py - by) * (py - by)
            ex, ey = bx - ax, by - ay
            t = ((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey)
            xn = np.where(corner, np.where(da <= db, ax, bx), ax + t * ex)
            yn = np.where(corner, np.where(da <= db, ay, by), ay + t * ey)
            x[act], y[act] = np.where(atwall, xn, px), np.where(atwall, yn, py)
            first = atwall & (wk[act] < 0)
            wk[act], wf[act] = np.where(first, ka, wk[act]), np.where(first, f, wf[act])
            wall[act] |= np.where(atwall, TOUCHED, 0)
            r[act], s[act] = rr, ss
            k[act] = np.where(hop, nb, ka)
            res[act] = np.where(lost, LOST, np.where(found, 0, np.where(out, EXITED, -1)))
    res[res < 0] = LOST
    return res, x, y, k, r, s, wall


def basis(T, r, s):
    """(n, Np) in T.dtype: the header's recurrences in float64; trimon_ref.simplex_ld in longdouble."""
    if T.dtype is LD:
        return tri.simplex_ld(T.N, r, s)
    dt, N = T.dtype, T.N
    one, two = dt(1), dt(2)
    with np.errstate(all="ignore"):
        a = np.where(s != one, two * (one + r) / np.where(s != one, one - s, one) - one, -one)
        om = one - s
        pw = np.ones_like(r)
        lp, lc = np.zeros_like(r), np.zeros_like(r)
        cols = []
        for i in range(N + 1):
            cl = T.jac[0, i]
            ln = np.full_like(r, cl[0]) if i == 0 else (cl[0] * a + cl[1]) * lc + cl[2] * lp
            lp, lc = lc, ln
            if i > 0:
                pw = pw * om
            fa = lc * pw
            jp, jc = np.zeros_like(r), np.zeros_like(r)
            for j in range(N + 1 - i):
                cj = T.jac[i + 1, j]
                jn = np.full_like(r, cj[0]) if j == 0 else (cj[0] * s + cj[1]) * jc + cj[2] * jp
                jp, jc = jc, jn
                cols.append(fa * jc)
    return np.stack(cols, axis=1)


def rows(T, r, s):
    """(n, Np): row[n] = sum_m P_m Vinv[m, n], ascending from 0.0 (longdouble: trimon_ref.rows_ld)."""
    if T.dtype is LD:
        return tri.rows_ld(T.N, r, s, T.Vinv64)[0]
    P = basis(T, r, s)
    out = np.zeros_like(P)
    with np.errstate(all="ignore"):
        for m in range(T.Np):
            out = out + P[:, m:m + 1] * T.Vinv[m][None, :]
    return out


def velocity(T, q, k, r, s):
    """(u, v, finite) at (k, r, s) from the state q = (h, hu, hv, ...), each (Np, K)."""
    h = np.asarray(q[0], dtype=T.dtype)[:, k]                              # (Np, n)
    row = rows(T, r, s)
    out = []
    with np.errstate(all="ignore"):
        for c in (1, 2):
            f = np.asarray(q[c], dtype=T.dtype)[:, k] / h
            val = np.zeros(len(k), dtype=T.dtype)
            for n in range(T.Np):
                val = val + row[:, n] * f[n]
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


# ---- the cases tests/test_tri_drifter_setup.py measures on the CPU and tests/test_sw2d_drifters_gpu.py runs on the device.
# Meshes: the boxes of tests/test_sw2d_monitor_gpu.py on [-1, 1]^2 and `straight`, its 5 x 4 shuffled box with the interior
# vertices moved (straight-sided elements of uneven shape; the deformed box of that file has curved maps, which drifters refuse).

BOXES = {"box3x2": (3, 2, 0), "box9x7": (9, 7, 0), "shuffled10": (10, 10, 7), "straight": (5, 4, 77)}
SIZE = 2.0                                                                 # of the domain [-1, 1]^2
ROTATION_CASES = [("box3x2", 1, 1), ("box9x7", 4, 63), ("shuffled10", 5, 300), ("straight", 8, 63), ("box9x7", 8, 300),
                  ("straight", 1, 300)]
ROTATION_STEPS = 40                                                        # about a quarter turn
WALL_CASES = [("box9x7", 4, 63), ("straight", 5, 300), ("box3x2", 8, 1), ("shuffled10", 1, 63)]
WALL_STEPS, WALL_DT, WALL_UV = 45, 0.05, (1.0, 0.6)
# kind: (mesh, order, steps); rk2, lserk, adaptive: three fields; heun3: variant B; heun4: four fields with sources
MOVING_CASES = {"rk2": ("box9x7", 4, 6), "lserk": ("straight", 8, 4), "heun3": ("box9x7", 5, 5), "heun4": ("shuffled10", 4, 4),
                "adaptive": ("box9x7", 4, 5)}
MOVING_DRIFTERS = 63

_MESH = {}


def box_mesh(name):
    import blitzdg_amd.pyblitzdg as dg
    nx, ny, seed = BOXES[name]
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=seed)
    if name == "straight":
        vert = np.asarray(mesh.vertices).reshape(-1, 3)[:, :2].copy()
        etov = np.asarray(mesh.elements).reshape(-1, 3).copy()
        inner = (np.abs(vert[:, 0]) < 1 - 1e-9) & (np.abs(vert[:, 1]) < 1 - 1e-9)
        rng = np.random.default_rng(77)
        vert[inner] += rng.uniform(-0.09, 0.09, (int(inner.sum()), 2))     # cells are 0.4 x 0.5: no element turns over
        mesh = dg.MeshManager()
        mesh.buildMesh(etov, vert)
    return mesh


def mesh_case(name, order, variant_b=False):
    """(nodes, t, mesh[, vb]) on the mesh `name`; t the host tables of conftest.tables_from_nodes."""
    import blitzdg_amd.pyblitzdg as dg
    from conftest import tables_from_nodes, variant_b_setup
    key = (name, order, variant_b)
    if key not in _MESH:
        mesh = box_mesh(name)
        if variant_b:
            nodes, t, vb = variant_b_setup(order, mesh)
            _MESH[key] = (nodes, t, mesh, vb)
        else:
            nodes = dg.TriangleNodesProvisioner(order, mesh)
            nodes.buildFilter(0.9 * order, max(order, 2))
            _MESH[key] = (nodes, tables_from_nodes(nodes), mesh)
    return _MESH[key]


def disc_points(nodes, n, seed, inner=0.15, outer=0.9):
    """(element, r, s) of n seeded points with inner <= |p| <= outer."""
    rng = np.random.default_rng([seed, n])
    rad, ang = np.sqrt(rng.uniform(inner ** 2, outer ** 2, n)), rng.uniform(0, 2 * np.pi, n)
    el, r, s = nodes.locatePoints(rad * np.cos(ang), rad * np.sin(ang))
    assert (el >= 0).all()
    return el, r, s


def rotation_problem(name, order, n):
    """(nodes, t, mesh, state, (element, r, s), omega, dt) of a frozen-rotation case about the origin."""
    nodes, t, mesh = mesh_case(name, order)
    omega = 1.0
    dt = 0.5 * np.pi / omega / ROTATION_STEPS
    return nodes, t, mesh, rotation_state(t["x"], t["y"], omega), disc_points(nodes, n, seed=order), omega, dt


def uniform_state(t, uv=WALL_UV, h0=2.0):
    h = np.full_like(t["x"], h0)
    return h, h * uv[0], h * uv[1]


def side_nodes(T, nodes):
    """mapO of the open side of the wall cases: the flat face-node indices of the boundary faces on x = +1."""
    Nfp = nodes._dims()[2]
    ends = ((0, 2), (2, 4), (4, 0))
    out = []
    for f, k in zip(*np.nonzero(T.neigh < 0)):
        a, b = T.vert[k, ends[f][0]], T.vert[k, ends[f][1]]
        if abs(a - 1) < 1e-9 and abs(b - 1) < 1e-9:
            out.append((3 * k + f) * Nfp + np.arange(Nfp))
    return np.concatenate(out).astype(np.int32)


def wall_problem(name, order, n):
    """(nodes, t, mesh, state, (element, r, s), mapO of the side x = +1) of a wall case: a uniform oblique flow that carries
    every drifter to the top or the right side within WALL_STEPS steps of WALL_DT."""
    nodes, t, mesh = mesh_case(name, order)
    T = tables(nodes, mesh)
    return nodes, t, mesh, uniform_state(t), disc_points(nodes, n, seed=100 + order), side_nodes(T, nodes)


def bump_state(t):
    """A Gaussian bump on still water of depth 2 with a swirl: the flow it starts is discontinuous at the faces."""
    x, y = t["x"], t["y"]
    h = 2.0 + 0.3 * np.exp(-6 * ((x - 0.1) ** 2 + (y + 0.05) ** 2))
    return [h, h * 3.0 * np.sin(2 * x + 1) * np.cos(y), h * 2.0 * np.cos(x) * np.sin(2 * y - 1)]


def moving_problem(kind):
    """The moving-flow case `kind` of MOVING_CASES: dict(nodes, t, mesh, vb, q0, dt, steps, points, mapO, fields, t0)."""
    name, order, steps = MOVING_CASES[kind]
    vb = None
    if kind == "heun3":
        nodes, t, mesh, vb = mesh_case(name, order, True)
        q0, mapO, t0 = [vb["h"].copy(), vb["hu"].copy(), vb["hv"].copy()], vb["mapO"], vb["time"]
    else:
        nodes, t, mesh = mesh_case(name, order)
        q0, mapO, t0 = bump_state(t), None, 0.0
        if kind == "heun4":
            q0.append(q0[0] * (0.5 + 0.25 * np.sin(t["x"] - t["y"])))
    from conftest import oracle_from
    dt = float(oracle_from(t, g=G).dt(*q0[:3], 0.65, order))               # the drivers' CFL step of the initial state
    return dict(nodes=nodes, t=t, mesh=mesh, vb=vb, q0=[np.array(a) for a in q0], dt=dt, steps=steps, mapO=mapO,
                fields=len(q0), t0=t0, points=moving_points(nodes, order))


def moving_points(nodes, seed):
    """(element, r, s) of MOVING_DRIFTERS points: a third in a disc, the others within 5e-3 of an element edge in reference
    coordinates (s = -1 or r = -1) that is shared with a neighbour, where a few steps of the flow carry them across it."""
    n = MOVING_DRIFTERS
    el, r, s = disc_points(nodes, n, seed=seed, inner=0.05, outer=0.8)
    rng = np.random.default_rng([seed, 11])
    neigh = nodes.drifterTables()[1]
    for lo, hi, f in ((n // 3, 2 * n // 3, 0), (2 * n // 3, n, 2)):       # elements whose face f is no boundary face
        el[lo:hi] = rng.choice(np.nonzero(neigh[f] >= 0)[0], hi - lo)
    r[n // 3:], s[n // 3:] = tri.reference_points(n - n // 3, [seed, 12])
    near = -1.0 + rng.uniform(1e-4, 5e-3, n)
    s[n // 3:2 * n // 3] = near[n // 3:2 * n // 3]
    r[2 * n // 3:] = near[2 * n // 3:]
    return el, r, s


def cpu_moving_states(kind):
    """The states a CPU stepper gives for the moving case `kind` (rk2, lserk: oracle.Sw2dOracle; heun3: oracle_np.step_ssprk2_b),
    one per step: what tests/test_tri_drifter_setup.py measures the restatement's float64 noise on. The device runs its own
    steps; the drifters' arithmetic on them is the same."""
    from conftest import oracle_from
    from oracle import oracle_np as onp
    p = moving_problem(kind)
    q, out, time = p["q0"], [], p["t0"]
    if kind == "heun3":
        v = p["vb"]
        Hx, Hy = p["nodes"].bedSlopes(v["H"])
        for _ in range(p["steps"]):
            q = list(onp.step_ssprk2_b(*q, v["H"], Hx, Hy, G, v["f"], v["CD"], time, p["dt"], 1, p["t"], mapO=v["mapO"]))[:3]
            time += p["dt"]
            out.append([np.array(a) for a in q])
        return p, out
    orc = oracle_from(p["t"], g=G)
    for _ in range(p["steps"]):
        q = list(orc.step_rk2(*q, p["dt"], 1, filter=True) if kind == "rk2" else orc.step_lserk4(*q, p["dt"], 1))
        out.append([np.array(a) for a in q])
    return p, out
