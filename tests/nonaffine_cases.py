"""Per-node-geometry cases of the sw2d variants B, C and D and their np.longdouble reference (no GPU).

deformed_box_tables builds the tables of a smoothly deformed box mesh: metric terms per node, normals and Fscale per face
node, from this repository's Dr / Ds. case_tables is the one mesh of tests/test_sw2d_nonaffine_variants_gpu.py: a shuffled
13 x 11 box, K = 286 triangles -- five workgroups of 64 elements with a last wave of 30 for the stage kernels of
sw2d_vn_kernel.hpp, two blocks of 256 (the second holding 30) for sw2d_vn_speed_kernel. variant_b_inputs / source_inputs are
the fields the variants take; make_case binds a field set (B, D, C, T, D3) to its reference function.

The reference is oracle/oracle_np.py -- sw2d_rhs4 and sw2d_rhs_b, which are generic in the tables and in the dtype --
evaluated in np.longdouble on tables converted to np.longdouble and rounded to float64 at the comparison only. The right-hand
side is not restated here; the stepper loops are (LSERK4 stages, midpoint RK2, Heun with the sponge on hu and hv), each
asserting h > 0 at every intermediate state. reference() computes each group of results once per (order, set) and keeps it
for every test of the session."""
import functools

import numpy as np

import blitzdg_amd.pyblitzdg as dg
from conftest import oracle_from, seeded_fields, tables_from_nodes
from oracle import lserk4_coefficients
from oracle import oracle_np as onp
from regimes import regime_fields

LD = np.longdouble
G = 9.81
CFL = 0.65
NX, NY = 13, 11
SETS = ("B", "D", "C", "T", "D3")
TIME0 = 1.45 * onp.TIDE_PERIOD     # the ramp is up and the tide near its low: about -2.5 m
SPONGE_SCALAR = 0.3
F_SCALAR = 0.1                     # set C: scalar Coriolis parameter


def require_extended_precision():
    """The reference must be wider than what it judges: fail (never fall back to float64, never skip) where np.longdouble is
    not at least the x87 80-bit format."""
    eps = np.finfo(LD).eps
    assert eps < 1e-18, (f"np.longdouble has eps = {float(eps):.3e} on this platform: it is no wider than float64, so "
                         "tests/nonaffine_cases.py cannot serve as an extended-precision reference here")


def deformed_box_tables(order, nx, ny, shuffle_seed=77):
    """Tables that are NOT those of straight-sided elements: a shuffled nx x ny box, its nodes moved by a smooth map, the
    metric terms and normals of the deformed elements recomputed per node (what buildCubatureVolumeMesh leaves in the
    provisioner), as the reference's formulas give them (src/TriangleNodesProvisioner.cpp:810-892), from this repository's
    Dr / Ds. Returns the table dict (x, y: the deformed nodes; J: the Jacobian per node)."""
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=shuffle_seed)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, max(order, 2))
    ctx = nodes.dgContext()
    x0, y0 = ctx.x, ctx.y
    x = x0 + 0.06 * np.sin(2.1 * y0) * (1 - x0 * x0)
    y = y0 + 0.05 * np.sin(2.7 * x0 + 0.3) * (1 - y0 * y0)
    Dr, Ds = ctx.Dr, ctx.Ds
    xr, xs, yr, ys = Dr @ x, Ds @ x, Dr @ y, Ds @ y
    J = xr * ys - xs * yr
    assert J.min() > 0
    t = tables_from_nodes(nodes)
    t.update(rx=ys / J, sx=-yr / J, ry=-xs / J, sy=xr / J, x=x, y=y, J=J)
    Fm = ctx.Fmask.T.reshape(-1) if ctx.Fmask.shape[0] == order + 1 else ctx.Fmask.reshape(-1)
    Nfp = order + 1
    fxr, fxs, fyr, fys = xr[Fm], xs[Fm], yr[Fm], ys[Fm]
    nxf, nyf = np.empty_like(fxr), np.empty_like(fxr)
    nxf[:Nfp], nyf[:Nfp] = fyr[:Nfp], -fxr[:Nfp]
    nxf[Nfp:2 * Nfp], nyf[Nfp:2 * Nfp] = fys[Nfp:2 * Nfp] - fyr[Nfp:2 * Nfp], -fxs[Nfp:2 * Nfp] + fxr[Nfp:2 * Nfp]
    nxf[2 * Nfp:], nyf[2 * Nfp:] = -fys[2 * Nfp:], fxs[2 * Nfp:]
    sJ = np.hypot(nxf, nyf)
    t.update(nx=nxf / sJ, ny=nyf / sJ, Fscale=sJ / J[Fm])
    return t


@functools.lru_cache(maxsize=None)
def case_tables(order):
    """The module's mesh at `order`: K = 286 > 256, no multiple of 64 or 256 (blockIdx.x > 0, a ragged last wave and a
    second speed block at once; the smallest box that gives all three)."""
    t = deformed_box_tables(order, NX, NY)
    K = t["rx"].shape[1]
    assert K == 2 * NX * NY and K > 256 and K % 256 != 0 and K % 64 != 0
    return t


def to_ld(t):
    """The tables with every floating-point array as np.longdouble (index maps and the order as they are)."""
    return {k: (np.asarray(v, dtype=LD) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in t.items()}


def f64(fields):
    """Rounded to float64: only at the comparison."""
    return [np.asarray(a, dtype=np.float64) for a in fields]


# ---- inputs of the variants

def open_boundary_nodes(t):
    """The wall face nodes on the left edge (they stay in the wall list too, as the driver's second buildBCHash leaves them)."""
    x = t["x"]
    Nfp = t["nx"].shape[0] // 3
    xface = x.flatten("F")[t["vmapM"]].reshape(-1, Nfp)             # one row per (element, face)
    wall = np.zeros(xface.size, dtype=bool)
    wall[t["mapW"]] = True
    left = wall.reshape(-1, Nfp).all(axis=1) & (np.abs(xface - x.min()) < 1e-9).all(axis=1)
    mapO = np.where(np.repeat(left, Nfp))[0].astype(np.int32)
    assert mapO.size > 0 and mapO.size % Nfp == 0
    return mapO


def variant_b_inputs(t):
    """Variant B on the tables: open boundary on the left edge, a smooth bed plus an offset per element (the bed jumps at
    every face, so hMstar != hM), bed slopes, drag, Coriolis, a time at which the tide is far from zero, and a sponge array
    that vanishes on the right part of the mesh."""
    x, y = t["x"], t["y"]
    K = x.shape[1]
    rng = np.random.default_rng([int(t["order"]), 41])
    H = 12.0 + 1.5 * x - 0.8 * y * y + 0.3 * np.sin(3 * x) * np.cos(2 * y) + np.tile(rng.uniform(-0.4, 0.4, K), (x.shape[0], 1))
    Hx, Hy = 1.5 + 0.9 * np.cos(3 * x) * np.cos(2 * y), -1.6 * y - 0.6 * np.sin(3 * x) * np.sin(2 * y)
    sponge = np.maximum(0.0, -0.25 - x)
    assert (sponge == 0).any() and (sponge > 0).any()
    assert abs(onp.tide_elevation(TIME0)) > 0.1
    return dict(H=H, Hx=Hx, Hy=Hy, mapO=open_boundary_nodes(t), CD=2.5e-2, f=0.05, time=TIME0, sponge=sponge)


def source_inputs(t):
    """Variants C / D: bed slopes and Coriolis parameter as arrays, a drag coefficient."""
    x, y = t["x"], t["y"]
    return {"zx": -0.05 + 0.02 * np.sin(2 * y), "zy": 0.05 * y + 0.01 * np.cos(3 * x), "f": 0.1 * (1 + 0.5 * y), "CD": 2.5e-2}


def tracer(h, x, y, seed):
    """hN = h c(x, y) with a perturbation per node, so that hN jumps at every face (rounded to float32 values as the regime
    states are)."""
    rng = np.random.default_rng([seed, 77])
    hN = h * (1.0 + 0.3 * np.sin(2 * x) * np.cos(3 * y)) * (1.0 + 0.02 * rng.standard_normal(np.shape(x)))
    return np.asarray(hN, dtype=np.float32).astype(np.float64)


def state(t, fields, kind, seed):
    """`smooth` (conftest.seeded_fields) or a regime of tests/regimes.py, with the tracer where fields == 4."""
    x, y = t["x"], t["y"]
    q = list(seeded_fields(x, y, seed) if kind == "smooth" else regime_fields(x, y, kind, seed))
    if fields == 4:
        q.append(tracer(q[0], x, y, seed))
    return q


# ---- a field set and its reference

class Case:
    """Field set `fs` at `order`: what the solver is built from (fields, sources / variant-B inputs) and rhs(q, time, ld), the
    reference function on the float64 (ld = False) or longdouble tables."""

    def __init__(self, order, fs):
        assert fs in SETS
        self.order, self.fs = order, fs
        self.t = t = case_tables(order)
        self.tl = to_ld(t)
        self.fields = 3 if fs in ("B", "D3") else 4
        self.vb = variant_b_inputs(t) if fs == "B" else None
        self.sources = {"D": source_inputs(t), "D3": source_inputs(t), "C": {"f": F_SCALAR}, "T": None, "B": None}[fs]
        self.time0 = TIME0 if fs == "B" else 0.0
        self.last_speed = None

    def _keep_speed(self, top):
        self.last_speed = top
        return top

    def rhs(self, q, time=0.0, ld=True):
        """Right-hand side of every field of the set; variant B also leaves its global speed in last_speed."""
        cast = (lambda a: LD(a) if np.ndim(a) == 0 else np.asarray(a, dtype=LD)) if ld else (lambda a: a)
        t = self.tl if ld else self.t
        if ld:
            require_extended_precision()
            assert t["rx"].dtype == LD
        q = [cast(a) for a in q]
        if self.fs == "B":
            v = self.vb
            return onp.sw2d_rhs_b(*q, cast(v["H"]), cast(v["Hx"]), cast(v["Hy"]), cast(G), cast(v["f"]), cast(v["CD"]), cast(time),
                                  t, v["mapO"], reduce_speed=self._keep_speed)
        zero = np.zeros_like(q[0])
        s = self.sources or {}
        zx, zy = cast(s.get("zx", zero)), cast(s.get("zy", zero))
        f, CD = cast(s.get("f", 0.0)), cast(s.get("CD", 0.0))
        if self.fields == 3:    # the tracer takes no part in the other three fields
            return onp.sw2d_rhs4(*q, q[0], zx, zy, cast(G), f, CD, t)[:3]
        return onp.sw2d_rhs4(*q, zx, zy, cast(G), f, CD, t)

    def evaluate(self, q, time, filt, ld=True):
        r = self.rhs(q, time, ld)
        return [(self.tl if ld else self.t)["Filter"] @ a for a in r] if filt else list(r)

    def dt(self, q):
        """The reference's step size at CFL 0.65 on the host tables (three-field oracle)."""
        return oracle_from(self.t).dt(*q[:3], CFL, self.order)


@functools.lru_cache(maxsize=None)
def make_case(order, fs):
    return Case(order, fs)


# ---- stepper loops (the right-hand side stays in oracle_np). `time` is kept in float64, as the solver keeps it.

def _positive(q):
    assert q[0].min() > 0, "the depth left the positive range inside a reference loop"
    return q


def lserk4_stages(case, q, dt, nstages, time=0.0, ld=True):
    """LSERK4 stages 0 .. nstages - 1 from a zero residual, never filtered (lserk4Stages has no filter argument); the time
    is frozen over the five stages of a step and moves on after the fifth. Returns (q, time)."""
    T = LD if ld else np.float64
    a_, b_ = lserk4_coefficients()
    q = [np.asarray(a, dtype=T) for a in q]
    res = [np.zeros_like(a) for a in q]
    for i in range(nstages):
        r = case.evaluate(q, time, False, ld)
        res = [T(a_[i % 5]) * x + T(dt) * y for x, y in zip(res, r)]
        q = _positive([x + T(b_[i % 5]) * y for x, y in zip(q, res)])
        if i % 5 == 4:
            time = time + dt
    return q, time


def _relaxation(sponge, T):
    """S of the combine steps: hu, hv /= 1 + c hu^2 (c an array, a scalar or None); h and hN are not relaxed."""
    c = T(0.0) if sponge is None else (T(sponge) if np.ndim(sponge) == 0 else np.asarray(sponge, dtype=T))
    return lambda p: [a / (T(1.0) + c * a * a) if i in (1, 2) else a for i, a in enumerate(p)]


def midpoint_rk2(case, q, dt, nsteps, filt, time=0.0, ld=True, sponge=None):
    """q1 = q + dt/2 R(q); q = q + dt R(q1), both evaluations at the old time level. `sponge`: the sponge ARRAY of a variant-B
    solver, which relaxes every combine step, not only Heun's (sw2d_vb_kernel.hpp and sw2d_vn_kernel.hpp agree on that).
    Returns (q, time)."""
    T = LD if ld else np.float64
    q = [np.asarray(a, dtype=T) for a in q]
    relax = _relaxation(sponge, T)
    for _ in range(nsteps):
        r = case.evaluate(q, time, filt, ld)
        q1 = _positive(relax([x + T(0.5) * T(dt) * y for x, y in zip(q, r)]))
        r = case.evaluate(q1, time, filt, ld)
        q = _positive(relax([x + T(dt) * y for x, y in zip(q, r)]))
        time = time + dt
    return q, time


def heun(case, q, dt, nsteps, filt, sponge=None, time=0.0, ld=True):
    """q1 = S(q + dt R(q)); q = S((q + q1 + dt R(q1)) / 2), S: hu, hv /= 1 + c hu^2 (c an array, a scalar or None); both
    evaluations at the old time level, as oracle_np.step_ssprk2_b has them. h and hN are not relaxed. Returns (q, time)."""
    T = LD if ld else np.float64
    q = [np.asarray(a, dtype=T) for a in q]
    relax = _relaxation(sponge, T)
    for _ in range(nsteps):
        r = case.evaluate(q, time, filt, ld)
        q1 = _positive(relax([x + T(dt) * y for x, y in zip(q, r)]))
        r = case.evaluate(q1, time, filt, ld)
        q = _positive(relax([T(0.5) * (x + x1 + T(dt) * y) for x, x1, y in zip(q, q1, r)]))
        time = time + dt
    return q, time


# ---- results shared by the tests of a session

_REF = {}


def reference(order, fs, what, ld=True):
    """Results of group `what` (rhs, lserk, rk2, ssprk2, jumpy) for (order, set); longdouble ones rounded to float64."""
    key = (order, fs, what, ld)
    if key in _REF:
        return _REF[key]
    c = make_case(order, fs)
    r = {"time0": c.time0}
    q0 = r["q0"] = state(c.t, c.fields, "smooth", seed=order)
    qj = r["qj"] = state(c.t, c.fields, "jumpy", seed=order)
    dt = r["dt"] = c.dt(q0)
    dtj = r["dtj"] = 0.25 * c.dt(qj)
    sponges = {"scalar": SPONGE_SCALAR}
    if fs == "B":
        sponges["array"] = c.vb["sponge"]
    if what == "rhs":
        for kind, q in (("smooth", q0), ("jumpy", qj)):
            raw = c.rhs(q, c.time0, ld)
            r[kind, False] = f64(raw)
            r[kind, True] = f64([(c.tl if ld else c.t)["Filter"] @ a for a in raw])
            r[kind, "speed"] = None if c.last_speed is None else float(c.last_speed)
    elif what == "lserk":
        q13, t13 = lserk4_stages(c, q0, dt, 13, c.time0, ld)
        r[13], r["time13"] = f64(q13), t13
        r["time8"] = c.time0 + dt                              # after eight stages one step is complete
        r["q1"] = state(c.t, c.fields, "smooth", seed=order + 100)
        q7, t7 = lserk4_stages(c, r["q1"], dt, 7, t13, ld)     # after setState: stage 0, residual zero, the time goes on
        r[7], r["time7"] = f64(q7), t7
    elif what == "rk2":
        for filt in (False, True):
            q, tt = midpoint_rk2(c, q0, dt, 3, filt, c.time0, ld)
            r[filt], r["time"] = f64(q), tt
    elif what == "ssprk2":
        for name, sp in sponges.items():
            for filt in (False, True):
                q, tt = heun(c, q0, dt, 2, filt, sp, c.time0, ld)
                r[name, filt], r["time"] = f64(q), tt
    else:
        assert what == "jumpy"
        sp = sponges.get("array", SPONGE_SCALAR)
        r["sponge"] = "array" if "array" in sponges else "scalar"
        r["lserk"] = f64(lserk4_stages(c, qj, dtj, 5, c.time0, ld)[0])
        r["rk2"] = f64(midpoint_rk2(c, qj, dtj, 1, True, c.time0, ld, sponges.get("array"))[0])
        r["ssprk2"] = f64(heun(c, qj, dtj, 1, True, sp, c.time0, ld)[0])
    _REF[key] = r
    return r
