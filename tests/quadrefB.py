"""NumPy restatement of the reference's tidal right-hand side ("variant B", src/sw2d/main.cpp:279-484 computeRHS) and of its
time loops, and the meshes, beds and states the variant-B tests run on.

rhsB reads the face count from the tables (nx has numFaces * Nfp rows), as the reference function reads dg.numFaces(), so the
same lines run on triangle and on quadrilateral tables; it is dtype-generic, so with tables, state and parameters cast to
np.longdouble (quadref_ld.to_ld, vb_ld) it is the extended-precision reference of the GPU tests. Quirks restated literally:
hM is overwritten by hMstar before the momentum rescale (:366-368), so the rescale divides by the star depth and the
hydrostatic correction of :420-421 is 0.5 g hM^2 - 0.5 g hMstar^2 with hM = hMstar already. The open-boundary assignment
(:348-353) comes after the wall assignment (:340-345) and wins where a node is in both lists.

heun_steps is the driver's SSP-RK2 loop body with the sponge division (:211-236, both evaluations at the old time level),
lserk4_stages freezes the tide over the five stages of a step and advances the time after the last, rk2_steps is the
sw2d-simple midpoint scheme (both evaluations at the old time level, as the device solvers run it).
tests/test_quadB_reference.py pins rhsB to fixtures made by the reference's Python RHS."""
import numpy as np

import blitzdg_amd.pyblitzdg as dg
import quadref
import quadref_ld as Q

LD = np.longdouble
G = 9.81
OUT = 2  # BCTag::Out


def tide_value(time, tide, dtype=np.float64):
    """amp cos(2 pi t / T) (tanh(ramp (t - T)) + 1) / 2 (main.cpp:352) in `dtype`."""
    amp, period, ramp = (dtype(v) for v in tide)
    time = dtype(time)
    pi = 4 * np.arctan(dtype(1))
    return amp * np.cos(2 * pi / period * time) * dtype(0.5) * (np.tanh(ramp * (time - period)) + 1)


def rhsB(h, hu, hv, t, vb, time=0.0, return_speed=False):
    """(RHS1, RHS2, RHS3) of main.cpp:279-484 on the tables `t`; vb: dict(g, H, Hx, Hy, mapO, CD, f, tide=(amp, period,
    ramp)); every floating-point input in one dtype."""
    dtype = h.dtype.type
    g, H, Hx, Hy = vb["g"], vb["H"], vb["Hx"], vb["Hy"]
    mapO = np.asarray(vb.get("mapO", []), dtype=np.int64)
    vM, vP, mapW = t["vmapM"], t["vmapP"], t["mapW"]
    nx, ny = t["nx"].ravel("F"), t["ny"].ravel("F")
    hC, huC, hvC, HC = h.ravel("F"), hu.ravel("F"), hv.ravel("F"), H.ravel("F")
    hM, hP = hC[vM], hC[vP].copy()
    huM, huP = huC[vM], huC[vP].copy()
    hvM, hvP = hvC[vM], hvC[vP].copy()
    HM, HP = HC[vM], HC[vP]
    # :340-345
    un = huM[mapW] * nx[mapW] + hvM[mapW] * ny[mapW]
    hP[mapW] = hM[mapW]
    huP[mapW] = huM[mapW] - 2 * nx[mapW] * un
    hvP[mapW] = hvM[mapW] - 2 * ny[mapW] * un
    # :348-353
    if mapO.size:
        huP[mapO] = huM[mapO]
        hvP[mapO] = hvM[mapO]
        hP[mapO] = HM[mapO] + tide_value(time, vb["tide"], dtype)
    # :356-368
    bM, bP = -HM, -HP
    zero = dtype(0)
    hMstar = np.maximum(zero, hM + bM - np.maximum(bP, bM))
    hPstar = np.maximum(zero, hP + bP - np.maximum(bP, bM))
    hM, hP = hMstar, hPstar
    huM, huP = hMstar * (huM / hM), hPstar * (huP / hP)
    hvM, hvP = hMstar * (hvM / hM), hPstar * (hvP / hP)
    dh, dhu, dhv = hM - hP, huM - huP, hvM - hvP
    half = dtype(0.5)
    F2M, G2M, G3M = (huM * huM) / hM + half * g * hM * hM, (huM * hvM) / hM, (hvM * hvM) / hM + half * g * hM * hM
    F2P, G2P, G3P = (huP * huP) / hP + half * g * hP * hP, (huP * hvP) / hP, (hvP * hvP) / hP + half * g * hP * hP
    F2, G2, G3 = (hu * hu) / h + half * g * h * h, (hu * hv) / h, (hv * hv) / h + half * g * h * h
    # :400-414
    uM, vMv, uP, vPv = huM / hM, hvM / hM, huP / hP, hvP / hP
    spdM = np.sqrt(uM * uM + vMv * vMv) + np.sqrt(g * hM)
    spdP = np.sqrt(uP * uP + vPv * vPv) + np.sqrt(g * hP)
    lam = np.maximum(spdM, spdP).max()
    # :419-421
    corr = half * g * hM * hM - half * g * hMstar * hMstar
    d1 = half * ((huM - huP) * nx + (hvM - hvP) * ny - lam * dh)
    d2 = half * ((F2M - F2P) * nx + (G2M - G2P) * ny - lam * dhu - corr * nx)
    d3 = half * ((G2M - G2P) * nx + (G3M - G3P) * ny - lam * dhv - corr * ny)
    shape = t["nx"].shape
    Dr, Ds, rx, sx, ry, sy = t["Dr"], t["Ds"], t["rx"], t["sx"], t["ry"], t["sy"]

    def div(F, Gf):
        return -(rx * (Dr @ F) + sx * (Ds @ F)) - (ry * (Dr @ Gf) + sy * (Ds @ Gf))

    lift = [t["Lift"] @ (t["Fscale"] * d.reshape(shape, order="F")) for d in (d1, d2, d3)]
    r1 = div(hu, hv) + lift[0]
    r2 = div(F2, G2) + lift[1]
    r3 = div(G2, G3) + lift[2]
    # :461-483
    u, v = hu / h, hv / h
    nrm = np.sqrt(u * u + v * v)
    r2 = r2 + g * h * Hx - vb["CD"] * u * nrm + vb["f"] * hv
    r3 = r3 + g * h * Hy - vb["CD"] * v * nrm - vb["f"] * hu
    return (r1, r2, r3, lam) if return_speed else (r1, r2, r3)


def _eval(q, t, vb, time, filt):
    r = rhsB(*q, t, vb, time)
    return [t["Filter"] @ a for a in r] if filt else list(r)


def sponge(x, c):
    return x / (1 + c * x * x)


def heun_steps(q, t, vb, dt, nsteps, time=0.0, sponge_coeff=0.0, filt=False):
    """main.cpp:211-236, nsteps times; sponge_coeff an (Np, K) array or a scalar. Returns (state, time)."""
    dtype = q[0].dtype.type
    dt, half = dtype(dt), dtype(0.5)
    c = sponge_coeff if np.ndim(sponge_coeff) else dtype(sponge_coeff)
    for _ in range(nsteps):
        r = _eval(q, t, vb, time, filt)
        q1 = [a + dt * b for a, b in zip(q, r)]
        q1 = [q1[0], sponge(q1[1], c), sponge(q1[2], c)]
        r = _eval(q1, t, vb, time, filt)
        q = [half * (a + a1 + dt * b) for a, a1, b in zip(q, q1, r)]
        q = [q[0], sponge(q[1], c), sponge(q[2], c)]
        time = time + float(dt)
    return q, time


def rk2_steps(q, t, vb, dt, nsteps, time=0.0, filt=True):
    dtype = q[0].dtype.type
    dt, half = dtype(dt), dtype(0.5)
    for _ in range(nsteps):
        r = _eval(q, t, vb, time, filt)
        q1 = [a + half * dt * b for a, b in zip(q, r)]
        r = _eval(q1, t, vb, time, filt)
        q = [a + dt * b for a, b in zip(q, r)]
        time = time + float(dt)
    return q, time


def lserk4_stages(q, t, vb, dt, nstages, time=0.0, first=0, res=None):
    """Stages first .. first + nstages - 1; the tide frozen over a step, the time advanced after stage 4. Returns
    (state, residual, time)."""
    dtype = q[0].dtype.type
    dt = dtype(dt)
    res = [np.zeros_like(a) for a in q] if res is None else res
    for i in range(first, first + nstages):
        a, b = dtype(dg.LSERK4.rk4a[i % 5]), dtype(dg.LSERK4.rk4b[i % 5])
        r = rhsB(*q, t, vb, time)
        res = [a * x + dt * y for x, y in zip(res, r)]
        q = [x + b * y for x, y in zip(q, res)]
        if i % 5 == 4:
            time = time + float(dt)
    return q, res, time


def vb_ld(vb):
    """vb with every floating-point entry as np.longdouble."""
    out = {}
    for k, v in vb.items():
        if k == "mapO":
            out[k] = v
        elif k == "tide":
            out[k] = tuple(LD(a) for a in v)
        else:
            out[k] = LD(v) if np.ndim(v) == 0 else np.asarray(v, dtype=LD)
    return out


def to_ld(q):
    return [np.asarray(a, dtype=LD) for a in q]


# ---- meshes with an open side, beds

def tag_open_side(mesh, EToV, Vert, x_min, tol=1e-12):
    """The bcType vector of `mesh` with every boundary face whose two vertices have x = x_min (in the coordinates `Vert`)
    tagged Out. Face f of an element joins its local vertices f and f + 1."""
    bc = np.array(mesh.bcType).reshape(len(EToV), -1)
    nf = bc.shape[1]
    onside = np.abs(Vert[:, 0] - x_min) < tol
    for k, e in enumerate(EToV):
        for f in range(nf):
            if bc[k, f] != 0 and onside[e[f]] and onside[e[(f + 1) % nf]]:
                bc[k, f] = OUT
    return bc.ravel()


def open_box(EToV, Vert, order, box_verts=None, filter_args=None):
    """(nodes, tables, mesh) of a quadrilateral mesh whose x = x_min side (x of `box_verts`, the vertices before any map;
    default Vert) is re-tagged Out the way the driver does it (main.cpp:160-174): buildBCHash is called again and appends,
    so those nodes stay in the wall list as well. tables["mapO"] holds them."""
    mesh = dg.MeshManager()
    mesh.buildMesh(EToV, Vert)
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(*(filter_args or (0.99 * order, 4)))
    bv = Vert if box_verts is None else box_verts
    bc = tag_open_side(mesh, np.asarray(mesh.elements).reshape(len(EToV), -1), bv, bv[:, 0].min())
    only_out = np.where(bc == OUT, OUT, 0)
    nodes.buildBCHash(only_out)
    t = quadref.tables(nodes.dgContext())
    t["mapO"] = np.asarray(nodes.dgContext().BCmap.get(OUT, []), dtype=np.int32)
    assert t["mapO"].size > 0
    return nodes, t, mesh


_TABLES = {}


def mesh_tables(name, order):
    """(nodes, tables) of quadref_ld's `shear` / `jitter` 13 x 11 box (K = 143) with the x = -1 side open; built once."""
    key = (name, order)
    if key not in _TABLES:
        E, V = Q.mesh_arrays(name)
        box = V @ np.linalg.inv(Q.SHEAR).T if name == "shear" else V  # (jitter leaves the boundary vertices where they were)
        _TABLES[key] = open_box(E, V, order, box_verts=box)
    return _TABLES[key][:2]


def jumping_bed(t, depth, jump, seed=5, flat=False):
    """Still-water depth with a discontinuity at every face: per-element constant offsets of at most `jump` / 2 (so a face sees
    at most `jump`) on depth (1 + 0.05 x - 0.03 y^2) (flat: on `depth`), rounded to float32 values."""
    x, y = t["x"], t["y"]
    rng = np.random.default_rng([seed, 31])
    off = 0.5 * jump * rng.uniform(-1, 1, x.shape[1])
    base = depth + 0 * x if flat else depth * (1 + 0.05 * x - 0.03 * y * y)
    return np.asarray(base + off[None, :], dtype=np.float32).astype(np.float64)


def min_edge(EToV, Vert):
    """Length of the shortest element edge."""
    E, V = np.asarray(EToV), np.asarray(Vert, dtype=np.float64)
    return min(np.linalg.norm(V[E[:, f]] - V[E[:, (f + 1) % E.shape[1]]], axis=1).min() for f in range(E.shape[1]))
