"""Variant B (the tidal driver's right-hand side, oracle_np.sw2d_rhs_b) with a passive tracer hN as a fourth field on
triangles: the definition the tracer pass of sw2d_vb_tracer_kernel.hpp is held to. The reference's tidal driver has no tracer;
this is tests/quadrefB4.py restated on oracle_np.sw2d_rhs_b.

rhsB4's components 1 to 3 ARE oracle_np.sw2d_rhs_b's (that function is called, so they are equal bit for bit) and the global
speed is the maximum of its speeds_only output. The fourth component is tracer_rhs, dtype-generic, with that speed as an
argument, so that it can be evaluated in np.longdouble:
  concentrations from the depths BEFORE the star states, NM = hN[vM] / h[vM], NP = hN[vP] / h[vP]; wall nodes NP = NM, then
  open-boundary nodes NP = tracer (a scalar, or one value per entry of mapO), which wins as hP does;
  star tracer hNM* = hM* NM, hNP* = hP* NP: a true rescale, so that a uniform concentration stays uniform over a bed that jumps;
  F4 = (hN* hu*) / h*, G4 = (hN* hv*) / h*, d4 = 1/2 ((F4M - F4P) nx + (G4M - G4P) ny - lam (hNM* - hNP*)) with the same global
  speed, which the tracer does not enter;
  r4 = -div((hN hu) / h, (hN hv) / h) + Lift(Fscale d4), no source term.
The steppers are oracle_np.step_ssprk2_b's and quadrefB4's with four fields: hN is updated like h (the sponge division touches
hu and hv only) and the filter applies to all four right-hand sides."""
import numpy as np

import blitzdg_amd.pyblitzdg as dg
from oracle import oracle_np

LD = np.longdouble


def tide_value(time, dtype=np.float64):
    """oracle_np.tide_elevation (main.cpp:352), the float64 number every evaluation is handed, in `dtype`."""
    return dtype(oracle_np.tide_elevation(time))


def global_speed(h, hu, hv, H, g, time, t, mapO):
    spdM, spdP = oracle_np.sw2d_rhs_b(h, hu, hv, H, H, H, g, 0.0, 0.0, time, t, mapO, speeds_only=True)
    return max(spdM.max(), spdP.max())


def tracer_rhs(h, hu, hv, hN, H, lam, time, t, mapO, tracer, return_terms=False, return_star=False):
    """The fourth component; every array in h's dtype. return_terms: also sum|terms| per node (what its rounding error scales
    with); return_star: also the smallest star depth."""
    dtype = h.dtype.type
    mapO = np.asarray(mapO, dtype=np.int64)
    mapW = np.asarray(t["mapW"], dtype=np.int64)
    vM, vP = np.asarray(t["vmapM"]), np.asarray(t["vmapP"])
    nx, ny = t["nx"].flatten("F"), t["ny"].flatten("F")
    hC, huC, hvC, hNC, HC = (a.flatten("F") for a in (h, hu, hv, hN, H))
    hM, hP = hC[vM], hC[vP].copy()
    huM, huP = huC[vM], huC[vP].copy()
    hvM, hvP = hvC[vM], hvC[vP].copy()
    HM, HP = HC[vM], HC[vP]
    NM, NP = hNC[vM] / hM, hNC[vP] / hP
    # walls, then the open boundary (main.cpp:340-353)
    un = huM[mapW] * nx[mapW] + hvM[mapW] * ny[mapW]
    hP[mapW] = hM[mapW]
    huP[mapW] = huM[mapW] - 2 * nx[mapW] * un
    hvP[mapW] = hvM[mapW] - 2 * ny[mapW] * un
    NP[mapW] = NM[mapW]
    if mapO.size:
        huP[mapO] = huM[mapO]
        hvP[mapO] = hvM[mapO]
        hP[mapO] = HM[mapO] + tide_value(time, dtype)
        NP[mapO] = np.asarray(tracer, dtype=h.dtype)
    # star states (:356-368)
    bM, bP = -HM, -HP
    zero, half = dtype(0), dtype(0.5)
    hMstar = np.maximum(zero, hM + bM - np.maximum(bP, bM))
    hPstar = np.maximum(zero, hP + bP - np.maximum(bP, bM))
    hM, hP = hMstar, hPstar
    huM, huP = hMstar * (huM / hM), hPstar * (huP / hP)
    hvM, hvP = hMstar * (hvM / hM), hPstar * (hvP / hP)
    hNM, hNP = hMstar * NM, hPstar * NP
    F4M, G4M = (hNM * huM) / hM, (hNM * hvM) / hM
    F4P, G4P = (hNP * huP) / hP, (hNP * hvP) / hP
    lam = dtype(lam)
    d4 = half * ((F4M - F4P) * nx + (G4M - G4P) * ny - lam * (hNM - hNP))
    shape = t["nx"].shape
    Dr, Ds, rx, sx, ry, sy = t["Dr"], t["Ds"], t["rx"], t["sx"], t["ry"], t["sy"]
    F4, G4 = (hN * hu) / h, (hN * hv) / h
    r4 = -(rx * (Dr @ F4) + sx * (Ds @ F4)) - (ry * (Dr @ G4) + sy * (Ds @ G4)) + t["Lift"] @ (t["Fscale"] * d4.reshape(shape, order="F"))
    out = (r4,)
    if return_terms:
        aDr, aDs, aF, aG = abs(Dr), abs(Ds), abs(F4), abs(G4)
        ad4 = half * ((abs(F4M) + abs(F4P)) * abs(nx) + (abs(G4M) + abs(G4P)) * abs(ny) + lam * (abs(hNM) + abs(hNP)))
        out += (abs(rx) * (aDr @ aF) + abs(sx) * (aDs @ aF) + abs(ry) * (aDr @ aG) + abs(sy) * (aDs @ aG) +
                abs(t["Lift"]) @ (abs(t["Fscale"]) * ad4.reshape(shape, order="F")),)
    if return_star:
        out += (min(hMstar.min(), hPstar.min()),)
    return out[0] if len(out) == 1 else out


def rhsB4(h, hu, hv, hN, H, Hx, Hy, g, f, CD, time, t, mapO, tracer, return_speed=False):
    """(RHS1, RHS2, RHS3, RHS4) in float64."""
    r = oracle_np.sw2d_rhs_b(h, hu, hv, H, Hx, Hy, g, f, CD, time, t, mapO)
    lam = global_speed(h, hu, hv, H, g, time, t, mapO)
    out = tuple(r) + (tracer_rhs(h, hu, hv, hN, H, lam, time, t, mapO, tracer),)
    return out + (lam,) if return_speed else out


def to_ld(t):
    """Tables with every floating-point array as np.longdouble."""
    return {k: (np.asarray(v).astype(LD) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in t.items()}


def rhs4_ld(h, hu, hv, hN, H, g, time, t, mapO, tracer):
    """The fourth component in np.longdouble, with the float64 global speed of the float64 state."""
    lam = global_speed(h, hu, hv, H, g, time, t, mapO)
    tr = np.asarray(tracer).astype(LD)
    return tracer_rhs(*(a.astype(LD) for a in (h, hu, hv, hN, H)), lam, time, to_ld(t), mapO, tr)


def _eval(q, p, time, filt):
    r = rhsB4(*q, p["H"], p["Hx"], p["Hy"], p["g"], p["f"], p["CD"], time, p["t"], p["mapO"], p["tracer"])
    return [p["t"]["Filter"] @ a for a in r] if filt else list(r)


def _sponged(q, c):
    return [q[0], q[1] / (1.0 + c * q[1] * q[1]), q[2] / (1.0 + c * q[2] * q[2]), q[3]]


def heun_steps(q, p, dt, nsteps, time=0.0, sponge=0.0, filt=False):
    """oracle_np.step_ssprk2_b with four fields; p: dict(H, Hx, Hy, g, f, CD, t, mapO, tracer); sponge: scalar or (Np, K).
    Both evaluations at the old time. Returns (state, time)."""
    for _ in range(nsteps):
        r = _eval(q, p, time, filt)
        q1 = _sponged([a + dt * b for a, b in zip(q, r)], sponge)
        r = _eval(q1, p, time, filt)
        q = _sponged([0.5 * (a + a1 + dt * b) for a, a1, b in zip(q, q1, r)], sponge)
        time = time + dt
    return q, time


def rk2_steps(q, p, dt, nsteps, time=0.0, filt=True):
    for _ in range(nsteps):
        r = _eval(q, p, time, filt)
        q1 = [a + 0.5 * dt * b for a, b in zip(q, r)]
        r = _eval(q1, p, time, filt)
        q = [a + dt * b for a, b in zip(q, r)]
        time = time + dt
    return q, time


def lserk4_stages(q, p, dt, nstages, time=0.0, first=0, res=None):
    """The tide frozen over the five stages of a step. Returns (state, residual, time)."""
    res = [np.zeros_like(a) for a in q] if res is None else res
    for i in range(first, first + nstages):
        a, b = dg.LSERK4.rk4a[i % 5], dg.LSERK4.rk4b[i % 5]
        r = _eval(q, p, time, False)
        res = [a * x + dt * y for x, y in zip(res, r)]
        q = [x + b * y for x, y in zip(q, res)]
        if i % 5 == 4:
            time = time + dt
    return q, res, time


def open_tracer(mapO, lo=0.2, hi=0.9):
    """One distinct concentration per entry of mapO, so that a wrong slot shows."""
    n = len(mapO)
    return lo + (hi - lo) * (np.random.default_rng(3).permutation(n) + 0.5) / n


def jumping_tracer(h, seed, lo=0.2, hi=0.9):
    """hN = h * (one random concentration per element in [lo, hi]): the tracer jumps at every face."""
    return h * np.random.default_rng([seed, 4]).uniform(lo, hi, h.shape[1])[None, :]


def problem(order, mesh, seed=3, g=9.81):
    """conftest.variant_b_setup with a tracer that jumps at every face and one concentration per open node:
    (nodes, tables, extras, q = [h, hu, hv, hN], p = the dict the steppers take)."""
    from conftest import variant_b_setup
    nodes, t, ex = variant_b_setup(order, mesh, seed)
    Hx, Hy = oracle_np.bed_slopes(ex["H"], t)
    q = [ex["h"], ex["hu"], ex["hv"], jumping_tracer(ex["h"], seed)]
    p = dict(H=ex["H"], Hx=Hx, Hy=Hy, g=g, f=ex["f"], CD=ex["CD"], t=t, mapO=ex["mapO"], tracer=open_tracer(ex["mapO"]))
    return nodes, t, ex, q, p
