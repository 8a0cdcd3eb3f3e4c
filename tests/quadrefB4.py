"""Variant B (the tidal driver's right-hand side, tests/quadrefB.py) with a passive tracer hN as a fourth field: the
definition the four-field variant-B kernels (sw2d_quadb4_kernel.hpp) are held to. The reference's tidal driver has no
tracer; this extends it the way swhelpers/rhs.py extends sw2d-simple.

rhsB4 is dtype-generic like quadrefB.rhsB. Components 1 to 3 are quadrefB.rhsB's own (that function is called, so they are
equal bit for bit); the lines it needs for the fourth component are restated here operation for operation. The fourth:
  concentrations from the depths BEFORE the star states, NM = hN[vM] / h[vM], NP = hN[vP] / h[vP]; wall nodes NP = NM, then
  open-boundary nodes NP = vb["tracer"] (a scalar, or one value per entry of mapO), which wins as hP does;
  star tracer hNM* = hM* NM, hNP* = hP* NP: a true rescale (the momentum lines' rescale is an identity, the reference's
  quirk), so that a uniform concentration stays uniform over a discontinuous bed;
  F4 = (hN* hu) / h*, G4 = (hN* hv) / h* in the form of G2, d4 = 1/2 ((F4M - F4P) nx + (G4M - G4P) ny - lam (hNM* - hNP*)) with
  the same global speed, which the tracer does not enter;
  r4 = div((hN hu) / h, (hN hv) / h) + Lift(Fscale d4), no source term.
The steppers are quadrefB's with four fields: hN is updated like h (the sponge division touches hu and hv only) and the filter
applies to all four right-hand sides."""
import numpy as np

import blitzdg_amd.pyblitzdg as dg
import quadrefB as B

LD = B.LD


def rhsB4(h, hu, hv, hN, t, vb, time=0.0, return_speed=False, return_terms=False):
    """(RHS1, RHS2, RHS3, RHS4); vb as quadrefB.rhsB's with "tracer" (the open-boundary concentration). return_terms: also
    sum|terms| of RHS4 per node (the magnitudes its rounding error scales with)."""
    dtype = h.dtype.type
    r1, r2, r3, lam = B.rhsB(h, hu, hv, t, vb, time, return_speed=True)
    g, H = vb["g"], vb["H"]
    mapO = np.asarray(vb.get("mapO", []), dtype=np.int64)
    vM, vP, mapW = t["vmapM"], t["vmapP"], t["mapW"]
    nx, ny = t["nx"].ravel("F"), t["ny"].ravel("F")
    hC, huC, hvC, hNC, HC = h.ravel("F"), hu.ravel("F"), hv.ravel("F"), hN.ravel("F"), H.ravel("F")
    hM, hP = hC[vM], hC[vP].copy()
    huM, huP = huC[vM], huC[vP].copy()
    hvM, hvP = hvC[vM], hvC[vP].copy()
    HM, HP = HC[vM], HC[vP]
    NM, NP = hNC[vM] / hM, hNC[vP] / hP
    # walls, then the open boundary (quadrefB.rhsB :340-353)
    un = huM[mapW] * nx[mapW] + hvM[mapW] * ny[mapW]
    hP[mapW] = hM[mapW]
    huP[mapW] = huM[mapW] - 2 * nx[mapW] * un
    hvP[mapW] = hvM[mapW] - 2 * ny[mapW] * un
    NP[mapW] = NM[mapW]
    if mapO.size:
        huP[mapO] = huM[mapO]
        hvP[mapO] = hvM[mapO]
        hP[mapO] = HM[mapO] + B.tide_value(time, vb["tide"], dtype)
        NP[mapO] = np.asarray(vb["tracer"], dtype=h.dtype)
    # star states (:356-368)
    bM, bP = -HM, -HP
    zero = dtype(0)
    hMstar = np.maximum(zero, hM + bM - np.maximum(bP, bM))
    hPstar = np.maximum(zero, hP + bP - np.maximum(bP, bM))
    hM, hP = hMstar, hPstar
    huM, huP = hMstar * (huM / hM), hPstar * (huP / hP)
    hvM, hvP = hMstar * (hvM / hM), hPstar * (hvP / hP)
    hNM, hNP = hMstar * NM, hPstar * NP
    half = dtype(0.5)
    F4M, G4M = (hNM * huM) / hM, (hNM * hvM) / hM
    F4P, G4P = (hNP * huP) / hP, (hNP * hvP) / hP
    d4 = half * ((F4M - F4P) * nx + (G4M - G4P) * ny - lam * (hNM - hNP))
    shape = t["nx"].shape
    Dr, Ds, rx, sx, ry, sy = t["Dr"], t["Ds"], t["rx"], t["sx"], t["ry"], t["sy"]
    F4, G4 = (hN * hu) / h, (hN * hv) / h
    r4 = -(rx * (Dr @ F4) + sx * (Ds @ F4)) - (ry * (Dr @ G4) + sy * (Ds @ G4)) + t["Lift"] @ (t["Fscale"] * d4.reshape(shape, order="F"))
    out = (r1, r2, r3, r4)
    if return_speed:
        out += (lam,)
    if return_terms:
        aDr, aDs, aF, aG = abs(Dr), abs(Ds), abs(F4), abs(G4)
        ad4 = half * ((abs(F4M) + abs(F4P)) * abs(nx) + (abs(G4M) + abs(G4P)) * abs(ny) + lam * (abs(hNM) + abs(hNP)))
        terms = abs(rx) * (aDr @ aF) + abs(sx) * (aDs @ aF) + abs(ry) * (aDr @ aG) + abs(sy) * (aDs @ aG) + \
            abs(t["Lift"]) @ (abs(t["Fscale"]) * ad4.reshape(shape, order="F"))
        out += (terms,)
    return out


def _eval(q, t, vb, time, filt):
    r = rhsB4(*q, t, vb, time)
    return [t["Filter"] @ a for a in r] if filt else list(r)


def _sponged(q, c):
    return [q[0], B.sponge(q[1], c), B.sponge(q[2], c), q[3]]


def heun_steps(q, t, vb, dt, nsteps, time=0.0, sponge_coeff=0.0, filt=False):
    """quadrefB.heun_steps with four fields. Returns (state, time)."""
    dtype = q[0].dtype.type
    dt, half = dtype(dt), dtype(0.5)
    c = sponge_coeff if np.ndim(sponge_coeff) else dtype(sponge_coeff)
    for _ in range(nsteps):
        r = _eval(q, t, vb, time, filt)
        q1 = _sponged([a + dt * b for a, b in zip(q, r)], c)
        r = _eval(q1, t, vb, time, filt)
        q = _sponged([half * (a + a1 + dt * b) for a, a1, b in zip(q, q1, r)], c)
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
    """quadrefB.lserk4_stages with four fields. Returns (state, residual, time)."""
    dtype = q[0].dtype.type
    dt = dtype(dt)
    res = [np.zeros_like(a) for a in q] if res is None else res
    for i in range(first, first + nstages):
        a, b = dtype(dg.LSERK4.rk4a[i % 5]), dtype(dg.LSERK4.rk4b[i % 5])
        r = rhsB4(*q, t, vb, time)
        res = [a * x + dt * y for x, y in zip(res, r)]
        q = [x + b * y for x, y in zip(q, res)]
        if i % 5 == 4:
            time = time + float(dt)
    return q, res, time


def vb_ld(vb):
    """vb with every floating-point entry as np.longdouble (quadrefB.vb_ld handles "tracer" as any other entry)."""
    return B.vb_ld(vb)


def open_tracer(t, lo=0.2, hi=0.9):
    """One distinct concentration per entry of mapO, so that a wrong slot shows."""
    n = len(t["mapO"])
    return lo + (hi - lo) * (np.random.default_rng(3).permutation(n) + 0.5) / n
