"""Shared pieces of the four-field quadrilateral tests: fixture loading and a NumPy restatement, with four faces, of the
reference's swhelpers.rhs.sw2dComputeRHS (rhs.py:178-311, fluxes of swhelpers/flux.py: tracer hN, Coriolis f, drag CD, bed
slope zx, zy; traces re-formed through the velocities, fluxes through velocities, one Lax-Friedrichs speed per face,
reflective walls on BCmap[3], strong form). tests/test_quad4_setup.py pins the restatement to the reference's own outputs
(the sw2dq_rhs4_* fixtures); the GPU tests then use it for multi-step loops."""
import os

import numpy as np

import blitzdg_amd.pyblitzdg as dg
from quadref import GOLDEN, tables  # noqa: F401

FIXTURES4 = ([f"coarse_box_quads_fine_N{n}" for n in range(1, 9)] + [f"jitter_box5x4_N{n}" for n in (2, 5, 8)]
             + ["box6x5_shuffled_N4", "box6x5_shuffled_N7", "shear_box6x5_N6", "scalarf_jitter_box5x4_N4",
                "nosrc_box6x5_shuffled_N5", "regime_coarse_box_quads_fine_N3"])
PARALLELOGRAM4 = {"box6x5_shuffled_N4", "box6x5_shuffled_N7", "shear_box6x5_N6", "nosrc_box6x5_shuffled_N5"}


def load_fixture4(name):
    """(npz, mesh, nodes, ctx): the fixture and this repository's tables rebuilt from its mesh; the filter is the
    quadrilateral script's (Nc = 0.99 N, s = 4)."""
    d = np.load(os.path.join(GOLDEN, f"sw2dq_rhs4_{name}.npz"))
    mesh = dg.MeshManager()
    mesh.buildMesh(d["EToV"], d["Vert"])
    N = int(d["order"])
    nodes = dg.QuadNodesProvisioner(N, mesh)
    nodes.buildFilter(0.99 * N, 4)
    return d, mesh, nodes, nodes.dgContext()


def sources(d):
    """The sources of a fixture as the solvers take them (f scalar or (Np, K))."""
    f = d["f"]
    return {"zx": d["zx"], "zy": d["zy"], "f": float(f) if f.ndim == 0 else f, "CD": float(d["CD"])}


def state(d):
    return [d[k].copy() for k in ("h", "hu", "hv", "hN")]


def reference(d):
    return [d[f"rhs{i}"] for i in (1, 2, 3, 4)]


def rhs4(h, hu, hv, hN, g, t, zx=0.0, zy=0.0, f=0.0, CD=0.0):
    """The reference function on the tables `t` (dict from `tables`), any number of faces of Nfp nodes."""
    Nfp = t["order"] + 1
    K = h.shape[1]
    nfaces = t["nx"].shape[0] // Nfp
    vM, vP, mapW = t["vmapM"], t["vmapP"], t["mapW"]
    hC, huC, hvC, hNC = (a.ravel("F") for a in (h, hu, hv, hN))
    nx, ny = t["nx"].ravel("F"), t["ny"].ravel("F")
    hM, hP = hC[vM], hC[vP]
    uM, uP = huC[vM] / hM, huC[vP] / hP
    vvM, vvP = hvC[vM] / hM, hvC[vP] / hP
    hNM, hNP = hNC[vM], hNC[vP]
    huM, hvM = hM * uM, hM * vvM
    huP, hvP = hP * uP, hP * vvP
    un = huM[mapW] * nx[mapW] + hvM[mapW] * ny[mapW]
    huP[mapW] = huM[mapW] - 2 * nx[mapW] * un
    hvP[mapW] = hvM[mapW] - 2 * ny[mapW] * un

    def flux(a, b, c, n):
        u, v = b / a, c / a
        return (b, b * u + 0.5 * g * a * a, c * u, n * u), (c, b * v, c * v + 0.5 * g * a * a, n * v)

    FM, GM = flux(hM, huM, hvM, hNM)
    FP, GP = flux(hP, huP, hvP, hNP)
    F, G = flux(h, hu, hv, hN)
    spM = np.sqrt((huM / hM) ** 2 + (hvM / hM) ** 2) + np.sqrt(g * hM)
    spP = np.sqrt((huP / hP) ** 2 + (hvP / hP) ** 2) + np.sqrt(g * hP)
    lam = np.maximum(spM, spP).reshape(Nfp, nfaces * K, order="F").max(axis=0)
    lam = np.repeat(lam, Nfp)
    jumps = (hM - hP, huM - huP, hvM - hvP, hNM - hNP)
    out = []
    for c in range(4):
        df = 0.5 * ((FM[c] - FP[c]) * nx + (GM[c] - GP[c]) * ny - lam * jumps[c])
        df = df.reshape(nfaces * Nfp, K, order="F")
        r = -(t["rx"] * (t["Dr"] @ F[c]) + t["sx"] * (t["Ds"] @ F[c]))
        r += -(t["ry"] * (t["Dr"] @ G[c]) + t["sy"] * (t["Ds"] @ G[c]))
        out.append(r + t["Lift"] @ (t["Fscale"] * df))
    u, v = hu / h, hv / h
    cdn = CD * np.hypot(u, v)
    out[1] += f * hv - cdn * u
    out[2] -= f * hu - cdn * v
    out[1] -= g * h * zx
    out[2] -= g * h * zy
    return tuple(out)


def compute_dt(h, hu, hv, g, t, CFL):
    """The drivers' time step (dt, speed): speed = max over face nodes of |Fscale| (sqrt(u^2 + v^2) + sqrt(g h))."""
    N = t["order"]
    u, v = hu / h, hv / h
    spd = (np.sqrt(u * u + v * v) + np.sqrt(g * h)).ravel("F")[t["vmapM"]]
    speed = (np.abs(t["Fscale"].ravel("F")) * spd).max()
    return CFL / ((N + 1) * (N + 1) * 0.5 * speed), speed


def gll_weights(ctx, N):
    """(Np, 1) tensor Gauss-Lobatto weights: node (N+1) j + i has w1[j] w1[i]."""
    V1 = dg.VandermondeBuilder().buildVandermondeMatrix(ctx.s[:N + 1])[0]
    w1 = np.linalg.inv(V1 @ V1.T).sum(axis=1)
    return np.outer(w1, w1).ravel()[:, None]
