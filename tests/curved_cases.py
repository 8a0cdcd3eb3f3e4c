"""Problems and reference loops of the curved / over-integrated sw2d tests: plain NumPy on this repository's host builders and
oracle/oracle_np.py::sw2d_rhs_curved (float64; bit-identical to the reference function's stored output, tests/test_oracle.py).
Nothing here touches a GPU: solver(case) alone creates one, and only when a GPU test calls it.

A case is a deformed box: the deformation, fields and sources of test_sw2d_curved_gpu.big_problem (g = 0.0245, f = 0.0788,
depth 1 .. 1.3, 0.05 N(0,1) momentum, tracer, bed slope, drag array -- the parameters the project's 1e-12 / 1e-11 are known
to hold at). tests/test_curved_cases.py holds the conditions every case of CASES meets; run it before any GPU time is spent.
"""
import types

import numpy as np

import blitzdg_amd.pyblitzdg as dg

G, F = 0.0245, 0.0788
TILE = 16                       # elements per tile of the stage kernels
INSTANCE_MESH = (7, 6)          # K = 84: 6 tiles, the last of 4 elements; two workgroups of four waves
SMALL_MESH = (2, 2)             # K = 8: less than one tile
# shuffleSeed of the K = 84 mesh: the first seed whose shuffle leaves a full 16-element tile without a curved element
# (test_curved_cases.test_shuffle_seed_is_the_first_that_qualifies); a shuffle scatters the deformed corner over the tiles
INSTANCE_SHUFFLE = 4


def deform(x0, y0):
    rho2 = ((x0 - 0.4) ** 2 + (y0 + 1.0) ** 2) / 0.8 ** 2
    b = np.where(rho2 < 1.0, (1.0 - rho2) ** 3, 0.0)
    return x0 + 0.02 * b * np.cos(1.3 * y0), y0 + 0.05 * b * np.sin(1.7 * x0 + 0.4)


def fields(x, y, seed=7):
    rng = np.random.default_rng(seed)
    h = 1.0 + 0.3 * np.exp(-8 * x * x - 8 * y * y)
    hu, hv = 0.05 * rng.standard_normal(x.shape), 0.05 * rng.standard_normal(x.shape)
    hN = h * (0.5 + 0.3 * np.sin(2 * x) * np.cos(3 * y))
    return h, hu, hv, hN


def sources(x, y):
    return dict(zx=0.05 + 0 * x, zy=-0.04 * y, g=G, f=F, CD=2.5e-3 * (1.0 + 0.5 * np.cos(x)))


def rewired_gmapM(gmapM, gmapP, NG):
    """Two Gauss points of the first interior face exchange their interior-side entries: an interior map that is not the
    identity (test_contexts_without_face_structure_fall_back_to_the_general_form)."""
    inner = np.where(gmapP != np.arange(gmapP.size))[0]
    i0 = int(inner[0]) // NG * NG
    out = gmapM.copy()
    out[i0 + 2], out[i0 + 3] = out[i0 + 3], out[i0 + 2]
    return out


def pad_to_odd(deformed, K):
    """curvedEls: the deformed elements plus, when their number is even, one straight element (the fix-up kernel packs 4 / 2 / 1
    elements per wave: an odd count leaves its last wave part empty). The straight one comes from a tile that already holds a
    deformed element, so that no all-straight tile is lost."""
    deformed = np.asarray(deformed, dtype=np.int32)
    if deformed.size % 2 == 1 or deformed.size == 0:
        return deformed
    taken = set(int(k) for k in deformed)
    for k0 in deformed:
        t0 = int(k0) // TILE * TILE
        for k in range(t0, min(t0 + TILE, K)):
            if k not in taken:
                return np.sort(np.append(deformed, np.int32(k))).astype(np.int32)
    raise ValueError("every tile with a deformed element is all deformed")


def bump(x0, y0):
    """A deformation that moves the two triangles of the middle cell of a 3 x 3 box and nothing else."""
    b = np.clip(1.0 - (x0 ** 2 + y0 ** 2) / 0.3 ** 2, 0.0, None) ** 3
    return x0 + 0.02 * b * np.cos(1.3 * y0), y0 + 0.05 * b


def narrow_first_column(x0, y0):
    """The first column of cells of a 3 x 3 box 0.8 times as wide, the other two wider: piecewise linear in x with its kink on
    a mesh line, so every element stays straight-sided and the areas of the first column differ from the others' by 27 %."""
    kink = -1.0 + 2.0 / 3.0
    left = -1.0 + 0.8 * (x0 + 1.0)
    right = 1.0 - (1.0 - (-1.0 + 0.8 * (kink + 1.0))) / (1.0 - kink) * (1.0 - x0)
    return np.where(x0 <= kink, left, right), y0


def problem(order, nx, ny, ngauss=None, ncub=None, shuffle=0, rewire_gmapM=False, seed=7, odd_curved=True, deformation=None,
            listed=None):
    """A deformed nx x ny box (shuffleSeed = shuffle) at `order` with a Gauss rule of `ngauss` points per face (default 2 (N + 1))
    and a cubature rule of degree `ncub` (default 3 (N + 1)): contexts from this repository's builders and the oracle's tables.
    `seed` (of the momentum noise) and `odd_curved=False` (curvedEls = the deformed elements as they are, no straight one
    added) exist for test_sw2d_curved_gpu.big_problem alone, whose problems stay what they were; no case of CASES sets them.
    `deformation` replaces deform() of this module, `listed` the elements of curvedEls (default: the deformed ones)."""
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=shuffle)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, order)
    ctx = nodes.dgContext()
    x0, y0 = ctx.x, ctx.y
    x, y = (deformation or deform)(x0, y0)
    deformed = np.where((np.abs(x - x0) + np.abs(y - y0)).max(axis=0) > 0)[0].astype(np.int32)
    K = int(ctx.numElements)
    if listed is not None:
        curvedEls = np.asarray(listed, dtype=np.int32)
    else:
        curvedEls = pad_to_odd(deformed, K) if odd_curved else deformed
    nodes.setCoordinates(x, y)
    J = (ctx.Dr @ x) * (ctx.Ds @ y) - (ctx.Ds @ x) * (ctx.Dr @ y)
    NG = 2 * (order + 1) if ngauss is None else int(ngauss)
    gauss = nodes.buildGaussFaceNodes(NG)
    cub = nodes.buildCubatureVolumeMesh(3 * (order + 1) if ncub is None else int(ncub))
    gmapM, gmapP = gauss.mapM, gauss.mapP
    if rewire_gmapM:
        gmapM = rewired_gmapM(gmapM, gmapP, NG)
    q = fields(x, y, seed)
    ph = sources(x, y)
    t = dict(cubV=cub.V, cubDr=cub.Dr, cubDs=cub.Ds, cubW=cub.W, cubrx=cub.rx, cubry=cub.ry, cubsx=cub.sx, cubsy=cub.sy,
             gInterp=gauss.Interp, gW=gauss.W, gnx=gauss.nx, gny=gauss.ny, gmapM=gmapM, gmapP=gmapP,
             gmapW=np.array(gauss.BCmap[3], dtype=np.int32), V=ctx.V, J=J, MMChol=cub.MMChol, curvedEls=curvedEls,
             Filter=ctx.filter)
    return types.SimpleNamespace(order=order, nx=nx, ny=ny, K=K, NGauss=NG, nodes=nodes, ctx=ctx, cub=cub, gauss=gauss, x=x, y=y,
                                 J=J, gmapM=gmapM, gmapP=gmapP, deformed=deformed, curvedEls=curvedEls, t=t, q=q, ph=ph)


def kref_case(order=3):
    """Every element straight-sided, the first column of cells narrower than the rest, and the two triangles of the first cell
    listed in curvedEls (the reference takes any list): the general form's reference element is element 0, the nodal-trace
    form's the first unlisted one, of another area."""
    c = problem(order, 3, 3, deformation=narrow_first_column, listed=[0, 1])
    first_unlisted = 2
    a0, a1 = c.J[0, 0], c.J[0, first_unlisted]
    assert np.ptp(c.J, axis=0).max() < 1e-12 * a0                     # every element is geometrically straight
    assert abs(a1 - a0) >= 0.01 * a0, (a0, a1)
    return c


def solver(c):
    """The HIP solver of a case (needs a GPU)."""
    from blitzdg_amd.sw2d_curved import Sw2dCurvedSolver
    return Sw2dCurvedSolver(c.ctx, c.cub, c.gauss, c.curvedEls, c.J, c.gmapM, c.gmapP, g=c.ph["g"], zx=c.ph["zx"], zy=c.ph["zy"],
                            f=c.ph["f"], CD=c.ph["CD"])


def tiles(c):
    """(all straight, mixed, all curved) counts of the 16-element tiles, by membership in curvedEls."""
    member = np.zeros(c.K, dtype=bool)
    member[c.curvedEls] = True
    n = [0, 0, 0]
    for k0 in range(0, c.K, TILE):
        m = member[k0:k0 + TILE]
        n[0 if not m.any() else (2 if m.all() else 1)] += 1
    return tuple(n)


def full_straight_tiles(c):
    member = np.zeros(c.K, dtype=bool)
    member[c.curvedEls] = True
    return sum(1 for k0 in range(0, c.K - TILE + 1, TILE) if not member[k0:k0 + TILE].any())


# ---- reference loops (float64, on the oracle)

def rhs(c, q, filt=False):
    r = _oracle().sw2d_rhs_curved(*q, c.ph["zx"], c.ph["zy"], c.ph["g"], c.ph["f"], c.ph["CD"], c.t)
    return tuple(c.t["Filter"] @ a for a in r) if filt else tuple(r)


def _oracle():
    from oracle import oracle_np
    return oracle_np


def step_size(c, q=None):
    """0.25 (2 / max(nx, ny)) / ((N + 1)^2 (sqrt(g max h) + max(|hu / h|, |hv / h|))), from the host fields."""
    h, hu, hv, _ = c.q if q is None else q
    speed = np.sqrt(c.ph["g"] * h.max()) + max(np.abs(hu / h).max(), np.abs(hv / h).max())
    return 0.25 * (2.0 / max(c.nx, c.ny)) / ((c.order + 1) ** 2 * speed)


def _wet(q, where):
    """Every state a reference loop passes through keeps h > 0 (a condition on the case: tests/test_curved_cases.py)."""
    assert np.isfinite(q[0]).all() and q[0].min() > 0, f"{where}: min h = {q[0].min()}"
    return q


def rk2_steps(c, q, dt, n, filt):
    """The driver's loop (RHS, filter, predictor, RHS, filter, corrector), n times:
    test_sw2d_curved_gpu.test_driver_loop_rk2_with_filter_matches_the_oracle. Asserts h > 0 at every predictor and step."""
    q = _wet([a.copy() for a in q], "RK2 start")
    for i in range(n):
        r = rhs(c, q, filt)
        q1 = _wet([a + 0.5 * dt * b for a, b in zip(q, r)], f"RK2 predictor of step {i}")
        r = rhs(c, q1, filt)
        q = _wet([a + dt * b for a, b in zip(q, r)], f"RK2 step {i}")
    return tuple(q)


def lserk4_stages(c, q, dt, n, stage0=0, res=None):
    """n stages of the low-storage scheme (dg.LSERK4.rk4a / rk4b) from stage index stage0 with residual res (zero when None):
    res = a res + dt RHS(q); q += b res. Returns (state, residual)."""
    a, b = dg.LSERK4.rk4a, dg.LSERK4.rk4b
    q = [x.copy() for x in q]
    res = [np.zeros_like(x) for x in q] if res is None else [x.copy() for x in res]
    for i in range(stage0, stage0 + n):
        r = rhs(c, q)
        res = [a[i % 5] * x + dt * y for x, y in zip(res, r)]
        q = _wet([x + b[i % 5] * y for x, y in zip(q, res)], f"LSERK4 stage {i}")
    return tuple(q), tuple(res)


# ---- the case table: name -> arguments of problem()

def _inst(n, **kw):
    return dict(order=n, nx=INSTANCE_MESH[0], ny=INSTANCE_MESH[1], shuffle=INSTANCE_SHUFFLE, **kw)


# (order, NGauss, cubature degree) -> the nodal-trace shape (fb, live_steps) and image placement tests expect
SHAPES = [
    (3, 13, 8, (1, 4), "resident"),     # <1,4>, last step ragged (13 = 3 x 4 + 1)
    (2, 7, 9, (1, 2), "resident"),      # the default shape (1,2) with ng = 7, not the default 6
    (4, 21, 10, (2, 4), "resident"),
    (6, 19, 21, (2, 4), "resident"),
    (7, 11, 16, (1, 4), "streamed"),    # three live steps
    (8, 13, 27, (1, 4), "streamed"),
    (8, 25, 18, (2, 4), "streamed"),
    (5, 32, 18, (2, 4), "resident"),    # the limit of 32 Gauss points per face
]
REWIRED = (4, 8)
SMALL = (1, 4, 8)


def shape_name(order, ng, ncub):
    return f"shape-N{order}-g{ng}-c{ncub}"


def _cases():
    c = {f"inst-N{n}": _inst(n) for n in range(1, 9)}
    for order, ng, ncub, _, _ in SHAPES:
        c[shape_name(order, ng, ncub)] = _inst(order, ngauss=ng, ncub=ncub)
    for n in REWIRED:
        c[f"rewired-N{n}"] = _inst(n, rewire_gmapM=True)
    for n in SMALL:
        c[f"small-N{n}"] = dict(order=n, nx=SMALL_MESH[0], ny=SMALL_MESH[1], shuffle=0)
    return c


# What each group of cases is stepped through: ("rk2", steps, filter) and ("lserk", stages) runs from the case's fields q,
# ("lserk1", stages) from the second state q1 (fields with seed + 100); "rhs" and "rhs1" are single evaluations of q and q1.
RUNS = {
    "inst": [("rk2", 1, True), ("rk2", 3, True), ("rk2", 1, False), ("rk2", 3, False), ("rk2", 2, True), ("rk2", 2, False),
             ("lserk", 4), ("lserk", 7), ("lserk1", 5), ("lserk", 5)],
    "shape": [("rk2", 2, True), ("lserk", 5)],
    "rewired": [("rk2", 2, True), ("lserk", 5)],
    "small": [("rk2", 1, True)],
}

_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = problem(**CASES[name])
    return _CASE[name]


def second_state(c):
    return fields(c.x, c.y, seed=107)


def reference(name, what):
    """Reference results of a case, computed once and shared by the kernel forms and the switches. what: ("rhs", filt),
    ("rhs1", filt), ("rk2", n, filt), ("lserk", n), ("lserk1", n)."""
    key = (name, what)
    if key in _REF:
        return _REF[key]
    c = case(name)
    dt = step_size(c)
    kind = what[0]
    if kind == "rhs":
        r = rhs(c, c.q, what[1])
    elif kind == "rhs1":
        r = rhs(c, second_state(c), what[1])
    elif kind == "rk2":
        _, n, filt = what
        r = rk2_steps(c, c.q, dt, n, filt) if n == 1 else rk2_steps(c, reference(name, ("rk2", n - 1, filt)), dt, 1, filt)
    elif kind in ("lserk", "lserk1"):
        r = lserk4_stages(c, c.q if kind == "lserk" else second_state(c), dt, what[1])[0]
    else:
        raise KeyError(what)
    _REF[key] = r
    return r


CASES = _cases()
