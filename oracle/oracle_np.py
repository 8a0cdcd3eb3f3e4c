"""NumPy restatement of the reference's four-field sw2d RHS with source terms ("variant D") --
TEST INFRASTRUCTURE ONLY (same rules as oracle_sw2d.c).

Follows swhelpers/rhs.py:178-311 and swhelpers/flux.py:1-22 step by step, including the
re-formation huM = hM*(hu/h)[vmapM] (rhs.py:229-233) and the sign pattern of the drag term in RHS3
(rhs.py:307: ``RHS3 -= f*hu - CD|u| v``). Pinned by tests/golden/sw2d_rhs4_*.npz, which hold the
output of the reference function itself (tests/golden/make_golden.py).
"""
import numpy as np


def fluxes(h, hu, hv, hN, g):
    """flux.py:1-22"""
    u, v = hu / h, hv / h
    return (hu, hu * u + 0.5 * g * h * h, hv * u, hN * u), (hv, hu * v, hv * v + 0.5 * g * h * h, hN * v)


def sw2d_rhs4(h, hu, hv, hN, zx, zy, g, f, CD, t):
    """t: mapping with Dr Ds Lift rx sx ry sy nx ny Fscale vmapM vmapP mapW (reference numbering)."""
    Nfp = t["nx"].shape[0] // 3
    K = t["rx"].shape[1]
    vM, vP, mapW = np.asarray(t["vmapM"]), np.asarray(t["vmapP"]), np.asarray(t["mapW"], dtype=np.int64)
    col = lambda a: a.flatten("F")  # noqa: E731  column-wise numbering n + Np*k
    hC, huC, hvC, hNC, nxC, nyC = col(h), col(hu), col(hv), col(hN), col(t["nx"]), col(t["ny"])
    hM, hP = hC[vM], hC[vP]
    uM, uP = huC[vM] / hC[vM], huC[vP] / hC[vP]
    vMv, vPv = hvC[vM] / hC[vM], hvC[vP] / hC[vP]
    hNM, hNP = hNC[vM], hNC[vP]
    huM, hvM, huP, hvP = hM * uM, hM * vMv, hP * uP, hP * vPv
    nxW, nyW = nxC[mapW], nyC[mapW]
    un = huM[mapW] * nxW + hvM[mapW] * nyW
    huP[mapW] = huM[mapW] - 2 * nxW * un
    hvP[mapW] = hvM[mapW] - 2 * nyW * un
    dq = (hM - hP, huM - huP, hvM - hvP, hNM - hNP)
    FM, GM = fluxes(hM, huM, hvM, hNM, g)
    FP, GP = fluxes(hP, huP, hvP, hNP, g)
    F, G = fluxes(h, hu, hv, hN, g)
    uM, vMv, uP, vPv = huM / hM, hvM / hM, huP / hP, hvP / hP
    spd = np.maximum(np.sqrt(uM * uM + vMv * vMv) + np.sqrt(g * hM), np.sqrt(uP * uP + vPv * vPv) + np.sqrt(g * hP))
    lam = np.repeat(spd.reshape(3 * K, Nfp).max(axis=1), Nfp)  # per-face maximum, broadcast to its nodes
    out = []
    for c in range(4):
        dflux = 0.5 * ((FM[c] - FP[c]) * nxC + (GM[c] - GP[c]) * nyC - lam * dq[c])
        surf = t["Fscale"] * dflux.reshape((3 * Nfp, K), order="F")
        r = -(t["rx"] * (t["Dr"] @ F[c]) + t["sx"] * (t["Ds"] @ F[c]))
        r += -(t["ry"] * (t["Dr"] @ G[c]) + t["sy"] * (t["Ds"] @ G[c]))
        out.append(r + t["Lift"] @ surf)
    u, v = hu / h, hv / h
    cdn = CD * np.hypot(u, v)
    out[1] += f * hv - cdn * u
    out[2] -= f * hu - cdn * v
    out[1] -= g * h * zx
    out[2] -= g * h * zy
    return tuple(out)


def sw2d_rhs_c(h, hu, hv, hN, g, f, t):
    """Variant C: the reference script's sw2dComputeRHS(h,hu,hv,hN,g,H,f,ctx), sw2d.py:37-146 -- traces
    taken directly (no hM*(hu/h) re-formation), F3 = G2 = hu*v (sw2d.py:24-27), Coriolis only.
    Pinned bit for bit by tests/golden/sw2d_rhsC_*.npz (outputs of the script's own functions)."""
    Nfp = t["nx"].shape[0] // 3
    K = t["rx"].shape[1]
    vM, vP, mapW = np.asarray(t["vmapM"]), np.asarray(t["vmapP"]), np.asarray(t["mapW"], dtype=np.int64)
    col = lambda a: a.flatten("F")  # noqa: E731
    hC, huC, hvC, hNC, nxC, nyC = col(h), col(hu), col(hv), col(hN), col(t["nx"]), col(t["ny"])
    hM, hP, huM, huP, hvM, hvP, hNM, hNP = hC[vM], hC[vP], huC[vM], huC[vP], hvC[vM], hvC[vP], hNC[vM], hNC[vP]
    nxW, nyW = nxC[mapW], nyC[mapW]
    huP[mapW] = huM[mapW] - 2 * nxW * (huM[mapW] * nxW + hvM[mapW] * nyW)
    hvP[mapW] = hvM[mapW] - 2 * nyW * (huM[mapW] * nxW + hvM[mapW] * nyW)
    dq = (hM - hP, huM - huP, hvM - hvP, hNM - hNP)

    def flux(h_, hu_, hv_, hN_):
        u, v = hu_ / h_, hv_ / h_
        G2 = hu_ * v
        return (hu_, hu_ * u + 0.5 * g * h_ * h_, G2, hN_ * u), (hv_, G2, hv_ * v + 0.5 * g * h_ * h_, hN_ * v)

    FM, GM = flux(hM, huM, hvM, hNM)
    FP, GP = flux(hP, huP, hvP, hNP)
    F, G = flux(h, hu, hv, hN)
    uM, vMv, uP, vPv = huM / hM, hvM / hM, huP / hP, hvP / hP
    spdM = np.sqrt(uM * uM + vMv * vMv) + np.sqrt(g * hM)
    spdP = np.sqrt(uP * uP + vPv * vPv) + np.sqrt(g * hP)
    spd = np.max(np.array([spdM, spdP]), axis=0)
    lam = np.reshape(spd, (Nfp, 3 * K), order="F")
    lam = np.outer(np.ones((Nfp, 1)), np.max(lam, axis=0)).flatten("F")
    out = []
    for c in range(4):
        dflux = 0.5 * ((FM[c] - FP[c]) * nxC + (GM[c] - GP[c]) * nyC - lam * dq[c])
        surf = t["Fscale"] * np.reshape(dflux, (3 * Nfp, K), order="F")
        r = -(t["rx"] * np.dot(t["Dr"], F[c]) + t["sx"] * np.dot(t["Ds"], F[c]))
        r += -(t["ry"] * np.dot(t["Dr"], G[c]) + t["sy"] * np.dot(t["Ds"], G[c]))
        r += np.dot(t["Lift"], surf)
        out.append(r)
    out[1] += f * hv
    out[2] -= f * hu
    return tuple(out)


# ------------------------------------------------------------------------------------------------
# Variant B: the reference's C++ "sw2d" driver (src/sw2d/main.cpp). PARITY UNPINNED for the parts
# only that file has (the C++ cannot be built here and holds no known-answer test): global
# Lax-Friedrichs speed, open-boundary tide, star states. The parts it shares with variants A/D are
# pinned by running this function with ``global_lf=False`` against the golden RHS fixtures
# (tests/test_oracle.py).

TIDE_PERIOD = 3600 * 12.42   # main.cpp:280
TIDE_AMPLITUDE = 3.0         # main.cpp:282
TIDE_RAMP = 0.15 / 3600      # main.cpp:352


def tide_elevation(t, amp=TIDE_AMPLITUDE, period=TIDE_PERIOD, ramp=TIDE_RAMP):
    """main.cpp:352: amp*cos(om t) * 1/2 (tanh(ramp (t - T)) + 1)"""
    om = 2.0 * np.pi / period
    return amp * np.cos(om * t) * 0.5 * (np.tanh(ramp * (t - period)) + 1)


def bed_slopes(H, t):
    """main.cpp:128-133: Hx, Hy = Filter * (rx Dr H + sx Ds H, ry Dr H + sy Ds H)"""
    Hx = t["rx"] * (t["Dr"] @ H) + t["sx"] * (t["Ds"] @ H)
    Hy = t["ry"] * (t["Dr"] @ H) + t["sy"] * (t["Ds"] @ H)
    return t["Filter"] @ Hx, t["Filter"] @ Hy


def build_sponge_coeff(t, mapO, strength, radius):
    """main.cpp:516-556 (buildSpongeCoeff): strength*(1 - d/radius), d = distance to the closest
    open-boundary node when d < radius, else 0."""
    x, y = t["x"], t["y"]
    vM = np.asarray(t["vmapM"])
    o = vM[np.asarray(mapO, dtype=np.int64)]
    xo, yo = x.flatten("F")[o], y.flatten("F")[o]
    out = np.zeros_like(x)
    if len(o) == 0:
        return out
    for k in range(x.shape[1]):
        for n in range(x.shape[0]):
            d = np.hypot(x[n, k] - xo, y[n, k] - yo)
            d = d[d < radius]
            if d.size:
                out[n, k] = strength * (1.0 - d.min() / radius)
    return out


def sw2d_rhs_b(h, hu, hv, H, Hx, Hy, g, f, CD, time, t, mapO=(), global_lf=True, tide=None, owned=None, reduce_speed=None,
               speeds_only=False):
    """main.cpp:279-484. t: tables as for sw2d_rhs4; mapO: open-boundary face nodes (BCmap[2]).
    Partitioned runs (tests): owned = number of owned elements of a rank-local mesh (the ghost elements behind them
    take no part in the speed maximum), reduce_speed = the all-rank maximum of this rank's value.
    speeds_only: return the two per-face-node speeds (:400-414) whose maximum is the global speed, (spdM, spdP), instead."""
    Nfp = t["nx"].shape[0] // 3
    K = t["rx"].shape[1]
    vM, vP = np.asarray(t["vmapM"]), np.asarray(t["vmapP"])
    mapW, mapO = np.asarray(t["mapW"], dtype=np.int64), np.asarray(mapO, dtype=np.int64)
    col = lambda a: a.flatten("F")  # noqa: E731
    hC, huC, hvC, HC, nxC, nyC = col(h), col(hu), col(hv), col(H), col(t["nx"]), col(t["ny"])
    hM, hP = hC[vM], hC[vP]
    huM, huP = huC[vM], huC[vP]
    hvM, hvP = hvC[vM], hvC[vP]
    HM, HP = HC[vM], HC[vP]
    # walls (:340-345) then open boundary (:348-353); the second overrides the first where both apply
    un = huM[mapW] * nxC[mapW] + hvM[mapW] * nyC[mapW]
    hP[mapW] = hM[mapW]
    huP[mapW] = huM[mapW] - 2 * nxC[mapW] * un
    hvP[mapW] = hvM[mapW] - 2 * nyC[mapW] * un
    huP[mapO] = huM[mapO]
    hvP[mapO] = hvM[mapO]
    hP[mapO] = HM[mapO] + (tide_elevation(time) if tide is None else tide)
    # star states (:356-368); hM is overwritten first, so the momentum rescale is hMstar*(huM/hMstar)
    bM, bP = -HM, -HP
    mx = np.maximum(bP, bM)
    hMstar = np.maximum(0.0, hM + bM - mx)
    hPstar = np.maximum(0.0, hP + bP - mx)
    hM, hP = hMstar, hPstar
    with np.errstate(divide="ignore", invalid="ignore"):
        huM, huP = hMstar * (huM / hM), hPstar * (huP / hP)
        hvM, hvP = hMstar * (hvM / hM), hPstar * (hvP / hP)
        dq = (hM - hP, huM - huP, hvM - hvP)
        F2M, G2M, G3M = (huM * huM) / hM + 0.5 * g * hM * hM, (huM * hvM) / hM, (hvM * hvM) / hM + 0.5 * g * hM * hM
        F2P, G2P, G3P = (huP * huP) / hP + 0.5 * g * hP * hP, (huP * hvP) / hP, (hvP * hvP) / hP + 0.5 * g * hP * hP
        uM, vMv, uP, vPv = huM / hM, hvM / hM, huP / hP, hvP / hP
    FM, GM = (huM, F2M, G2M), (hvM, G2M, G3M)
    FP, GP = (huP, F2P, G2P), (hvP, G2P, G3P)
    F2, G2, G3 = (hu * hu) / h + 0.5 * g * h * h, (hu * hv) / h, (hv * hv) / h + 0.5 * g * h * h
    F, G = (hu, F2, G2), (hv, G2, G3)
    spdM, spdP = np.sqrt(uM * uM + vMv * vMv) + np.sqrt(g * hM), np.sqrt(uP * uP + vPv * vPv) + np.sqrt(g * hP)
    if speeds_only:
        return spdM, spdP
    spd = np.maximum(spdM, spdP)
    if global_lf:
        top = spd.max() if owned is None else spd[:3 * Nfp * owned].max()
        lam = np.full_like(spd, top if reduce_speed is None else reduce_speed(top))   # :414
    else:
        lam = np.repeat(spd.reshape(3 * K, Nfp).max(axis=1), Nfp)     # variants A/D: per-face maximum
    corr = 0.5 * g * hM * hM - 0.5 * g * hMstar * hMstar              # :420-421, identically zero
    out = []
    for c in range(3):
        extra = 0.0 if c == 0 else corr * (nxC if c == 1 else nyC)
        dflux = 0.5 * ((FM[c] - FP[c]) * nxC + (GM[c] - GP[c]) * nyC - lam * dq[c] - extra)
        surf = t["Fscale"] * dflux.reshape((3 * Nfp, K), order="F")
        r = -(t["rx"] * (t["Dr"] @ F[c]) + t["sx"] * (t["Ds"] @ F[c]))
        r += -(t["ry"] * (t["Dr"] @ G[c]) + t["sy"] * (t["Ds"] @ G[c]))
        out.append(r + t["Lift"] @ surf)
    u, v = hu / h, hv / h
    out[1] += g * h * Hx                                              # :461-468
    out[2] += g * h * Hy
    norm_u = np.sqrt(u * u + v * v)
    out[1] += -CD * u * norm_u                                        # :473-474
    out[2] += -CD * v * norm_u
    out[1] += f * hv                                                  # :477-478
    out[2] += -f * hu
    return tuple(out)


def step_ssprk2_b(h, hu, hv, H, Hx, Hy, g, f, CD, time, dt, nsteps, t, mapO=(), sponge=None):
    """main.cpp:211-236: Heun steps with both RHS evaluations at the old time level and the sponge
    relaxation hu /= 1 + c hu^2 after each update."""
    sp = np.zeros_like(h) if sponge is None else sponge
    for _ in range(nsteps):
        r = sw2d_rhs_b(h, hu, hv, H, Hx, Hy, g, f, CD, time, t, mapO)
        h1, hu1, hv1 = h + dt * r[0], hu + dt * r[1], hv + dt * r[2]
        hu1 = hu1 / (1.0 + sp * hu1 * hu1)
        hv1 = hv1 / (1.0 + sp * hv1 * hv1)
        r = sw2d_rhs_b(h1, hu1, hv1, H, Hx, Hy, g, f, CD, time, t, mapO)
        h = 0.5 * (h + h1 + dt * r[0])
        hu = 0.5 * (hu + hu1 + dt * r[1])
        hv = 0.5 * (hv + hv1 + dt * r[2])
        hu = hu / (1.0 + sp * hu * hu)
        hv = hv / (1.0 + sp * hv * hv)
        time += dt
    return h, hu, hv, time


# ------------------------------------------------------------------------------------------------
# Curved / over-integrated RHS: the reference's swhelpers.rhs.sw2dComputeRHS_curved
# (swhelpers/rhs.py:6-176). Pinned bit for bit by tests/golden/sw2d_rhs_curved_*.npz, which hold the
# output of the reference function itself on tables built by this repository's
# buildGaussFaceNodes / buildCubatureVolumeMesh (tests/golden/make_golden.py).

def sw2d_rhs_curved(h, hu, hv, hN, zx, zy, g, f, CD, t):
    """t: mapping with the tables the reference function reads from its context arguments --
    cubV cubDr cubDs (Ncub, Np); cubW cubrx cubry cubsx cubsy (Ncub, K); gInterp (3NG, Np); gW gnx gny
    (3NG, K); gmapM gmapP gmapW (flat Gauss ids g + 3NG*k); V (Np, Np); J (Np, K); MMChol (Np, Np, K);
    curvedEls. Same operations in the same order as rhs.py:6-176 (cub_zx, cub_zy, cub_H and the Gauss
    trace of H are formed there but never used)."""
    from scipy.linalg import solve_triangular
    V_, Dr_, Ds_ = t["cubV"], t["cubDr"], t["cubDs"]
    q = (h, hu, hv, hN)
    cq = [np.dot(V_, a) for a in q]                                                    # rhs.py:8-11
    F, G = fluxes(cq[0], cq[1], cq[2], cq[3], g)                                        # rhs.py:18
    DrT, DsT = np.transpose(Dr_), np.transpose(Ds_)
    W, rx, ry, sx, sy = t["cubW"], t["cubrx"], t["cubry"], t["cubsx"], t["cubsy"]
    MM = []
    for c in range(4):                                                                  # rhs.py:23-49
        tmpr = W * (rx * F[c] + ry * G[c])
        tmps = W * (sx * F[c] + sy * G[c])
        MM.append(np.dot(DrT, tmpr) + np.dot(DsT, tmps))
    nx, ny = t["gnx"], t["gny"]
    mapW = np.asarray(t["gmapW"], dtype=np.int64)
    gmapM, gmapP = np.asarray(t["gmapM"]), np.asarray(t["gmapP"])
    nxW, nyW = nx.flatten("F")[mapW], ny.flatten("F")[mapW]                             # rhs.py:55-56
    NG3, K = nx.shape
    gq = [np.dot(t["gInterp"], a).flatten("F") for a in q]                              # rhs.py:61-75
    hM, huM, hvM, hNM = (a[gmapM] for a in gq)
    hP, huP, hvP, hNP = (a[gmapP] for a in gq)
    uM, uP, vM, vP = huM / hM, huP / hP, hvM / hM, hvP / hP                             # rhs.py:81-85 (before the wall BC)
    huP[mapW] = huM[mapW] - 2 * nxW * (huM[mapW] * nxW + hvM[mapW] * nyW)               # rhs.py:87-88
    hvP[mapW] = hvM[mapW] - 2 * nyW * (huM[mapW] * nxW + hvM[mapW] * nyW)
    FM, GM = fluxes(hM, huM, hvM, hNM, g)
    FP, GP = fluxes(hP, huP, hvP, hNP, g)
    spdM = np.sqrt(uM * uM + vM * vM) + np.sqrt(g * hM)
    spdP = np.sqrt(uP * uP + vP * vP) + np.sqrt(g * hP)
    spdMax = np.max(np.array([spdM, spdP]), axis=0)
    Nfp = NG3 // 3
    lam = np.reshape(spdMax, (Nfp, 3 * K), order="F")                                   # rhs.py:102-104
    spdMax = np.reshape(np.outer(np.ones((Nfp, 1)), np.max(lam, axis=0)), (NG3, K), order="F")
    shp = lambda a: np.reshape(a, (NG3, K), order="F")  # noqa: E731
    dq = [shp(a - b) for a, b in ((hM, hP), (huM, huP), (hvM, hvP), (hNM, hNP))]
    interpT = np.transpose(t["gInterp"])
    gW = t["gW"]
    for c in range(4):                                                                  # rhs.py:126-135
        flux = 0.5 * ((shp(FM[c]) + shp(FP[c])) * nx + (shp(GM[c]) + shp(GP[c])) * ny + spdMax * dq[c])
        MM[c] -= np.dot(interpT, gW * flux)
    V = t["V"]
    mmInv = np.dot(V, V.T)                                                              # rhs.py:150-156
    J = t["J"]
    out = [np.dot(mmInv, MM[c] / J) for c in range(4)]
    chol = t["MMChol"]
    for k in set(int(e) for e in np.asarray(t["curvedEls"]).reshape(-1)):               # rhs.py:157-162
        U = chol[:, :, k]
        for c in range(4):
            out[c][:, k] = solve_triangular(U, solve_triangular(U, MM[c][:, k], trans="T"))
    u, v = hu / h, hv / h                                                               # rhs.py:165-174
    cdn = CD * np.hypot(u, v)
    out[1] += f * hv - cdn * u
    out[2] -= f * hu - cdn * v
    out[1] -= g * h * zx
    out[2] -= g * h * zy
    return tuple(out)


# ---- burgers1d (reference src/burgers1d/main.cpp:119-226): the RHS in NumPy, operation for operation. Test infrastructure only.
# parity unpinned: the reference holds no vector for this solver and its C++ cannot be built here (blitz++, boost absent); the
# restatement and the host code are two independent readings of the same file, checked against each other and against the
# travelling-wave solution the driver itself prints its error against.

def burgers2(x, t, alpha, nu, c):
    """main.cpp:119-126."""
    return (c / alpha) - (c / alpha) * np.tanh(0.5 * (c / nu) * (x - c * t))


def burgers1d_rhs(u, x, t, c, alpha, nu, Dr, rx, Lift, Fscale, nx, vmapM, vmapP, mapI, mapO, vmapI, vmapO):
    """main.cpp:129-226; every (rows, K) table C-ordered, index maps on the column-wise flattening (byRows = false)."""
    F = lambda a: np.asarray(a).flatten("F")                      # noqa: E731  fullToVector(.., false)
    shape = np.asarray(nx).shape
    M = lambda v: np.reshape(v, shape, order="F")                 # noqa: E731  vectorToFull(.., false)
    uVec, xVec, nxVec = F(u), F(x), F(nx)
    uM, uP = uVec[vmapM], uVec[vmapP]
    maxvel = np.max(np.abs(u))
    uL, uR = burgers2(xVec[vmapI], t, alpha, nu, c), burgers2(xVec[vmapO], t, alpha, nu, c)
    du = uM - uP
    du[mapI] = 2 * (uVec[vmapI] - uL)
    du[mapO] = 2 * (uVec[vmapO] - uR)
    q = np.sqrt(nu) * (rx * np.dot(Dr, u) - np.dot(Lift, 0.5 * Fscale * nx * M(du)))
    qVec = F(q)
    dq = 0.5 * (qVec[vmapM] - qVec[vmapP])
    dq[mapI] = dq[mapO] = 0.0
    du2 = 0.5 * (uM * uM - uP * uP)
    du2[mapI] = uVec[vmapI] * uVec[vmapI] - uL * uL
    du2[mapO] = uVec[vmapO] * uVec[vmapO] - uR * uR
    flux = nxVec * (0.5 * du2 - np.sqrt(nu) * dq) - (0.5 * maxvel) * du
    return -rx * np.dot(Dr, 0.5 * u * u - np.sqrt(nu) * q) + np.dot(Lift, Fscale * M(flux))
