"""Shared pieces of the quadrilateral tests: fixture loading and a NumPy restatement of the reference script's
sw2dComputeRHS (sw2dquads.py:24-133: local Lax-Friedrichs flux with one speed per face, reflective walls on BCmap[3],
strong form). tests/test_quad_setup.py pins the restatement to the reference's own outputs (the sw2dq_rhs_* fixtures);
the GPU tests then use it for multi-step loops."""
import os

import numpy as np

import blitzdg_amd.pyblitzdg as dg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FIXTURES = ([f"coarse_box_quads_fine_N{n}" for n in range(1, 9)] + [f"jitter_box5x4_N{n}" for n in (2, 5, 8)]
            + ["box6x5_shuffled_N4", "box6x5_shuffled_N7", "shear_box6x5_N3", "shear_box6x5_N8",
               "regime_coarse_box_quads_fine_N3"])


def load_fixture(name):
    """(npz, mesh, nodes, ctx): the fixture and this repository's tables rebuilt from its mesh; the filter is the
    script's (Nc = 0.99 N, s = 4)."""
    d = np.load(os.path.join(GOLDEN, f"sw2dq_rhs_{name}.npz"))
    mesh = dg.MeshManager()
    mesh.buildMesh(d["EToV"], d["Vert"])
    N = int(d["order"])
    nodes = dg.QuadNodesProvisioner(N, mesh)
    nodes.buildFilter(0.99 * N, 4)
    return d, mesh, nodes, nodes.dgContext()


def tables(ctx):
    """Host tables of a quad DGContext2D, as a dict (every access of a context property copies)."""
    t = {k: getattr(ctx, k) for k in ("Dr", "Ds", "Lift", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP",
                                      "filter", "x", "y")}
    t["Filter"] = t.pop("filter")
    t["order"] = ctx.numFacePoints - 1
    t["mapW"] = np.asarray(ctx.BCmap.get(3, []), dtype=np.int32)
    return t


def rhs(h, hu, hv, g, t):
    """The script's sw2dComputeRHS on the tables `t` (dict from `tables`)."""
    Nfp = t["order"] + 1
    K = h.shape[1]
    vM, vP, mapW = t["vmapM"], t["vmapP"], t["mapW"]
    hC, huC, hvC = h.ravel("F"), hu.ravel("F"), hv.ravel("F")
    nx, ny = t["nx"].ravel("F"), t["ny"].ravel("F")
    hM, hP = hC[vM], hC[vP]
    huM, huP = huC[vM], huC[vP].copy()
    hvM, hvP = hvC[vM], hvC[vP].copy()
    un = huM[mapW] * nx[mapW] + hvM[mapW] * ny[mapW]
    huP[mapW] = huM[mapW] - 2 * nx[mapW] * un
    hvP[mapW] = hvM[mapW] - 2 * ny[mapW] * un

    def flux(a, b, c):
        return (b, b * b / a + 0.5 * g * a * a, b * c / a), (c, b * c / a, c * c / a + 0.5 * g * a * a)

    FM, GM = flux(hM, huM, hvM)
    FP, GP = flux(hP, huP, hvP)
    F, G = flux(h, hu, hv)
    spM = np.sqrt((huM / hM) ** 2 + (hvM / hM) ** 2) + np.sqrt(g * hM)
    spP = np.sqrt((huP / hP) ** 2 + (hvP / hP) ** 2) + np.sqrt(g * hP)
    lam = np.maximum(spM, spP).reshape(Nfp, 4 * K, order="F").max(axis=0)
    lam = np.repeat(lam, Nfp)
    jumps = (hM - hP, huM - huP, hvM - hvP)
    out = []
    for c in range(3):
        df = 0.5 * ((FM[c] - FP[c]) * nx + (GM[c] - GP[c]) * ny - lam * jumps[c])
        df = df.reshape(4 * Nfp, K, order="F")
        r = -(t["rx"] * (t["Dr"] @ F[c]) + t["sx"] * (t["Ds"] @ F[c]))
        r -= t["ry"] * (t["Dr"] @ G[c]) + t["sy"] * (t["Ds"] @ G[c])
        out.append(r + t["Lift"] @ (t["Fscale"] * df))
    return tuple(out)


def quad_box(n, m=None, x0=-1.0, x1=1.0):
    """EToV (K, 4) and Vert of an n x m box of counter-clockwise quadrangles on [x0, x1]^2."""
    m = n if m is None else m
    xs, ys = np.linspace(x0, x1, n + 1), np.linspace(x0, x1, m + 1)
    X, Y = np.meshgrid(xs, ys)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(m)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    E = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    return E, V
