#!/usr/bin/env python3
"""The quadrilateral counterpart of examples/sw2d_tracer.py: shallow water with a passive tracer over a sloping bed, with
f-plane rotation and quadratic drag, on an n x m box of quadrangles with walls on every side, state resident in HBM
(Sw2dQuadSolver with fields=4 and sources: the arithmetic of the reference's swhelpers.rhs.sw2dComputeRHS).

    python examples/sw2d_quads_tracer.py [box:NXxNY | mesh.msh] [order] [finalTime] [outputDir]

Midpoint RK2 with the modal filter on every right-hand side; the time step is recomputed on the device every 10 steps
(computeDt: dt = CFL / ((N+1)^2 / 2 * max |Fscale| (|u| + sqrt(g h)))) and shortened to end at finalTime. Water mass
sum(w J h) and tracer mass sum(w J hN) are printed: the sources enter neither equation, so both hold to round-off. With an
output directory the state is written as .npy files and h, u, v, N as *.vtu files (eta = h: no still-water depth is
subtracted).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2dquads  # noqa: E402


def quad_box(nx, ny):
    xs, ys = np.linspace(-1, 1, nx + 1), np.linspace(-1, 1, ny + 1)
    X, Y = np.meshgrid(xs, ys)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    return np.stack([a, a + 1, a + nx + 2, a + nx + 1], axis=1), V


def setup(mesh_arg, NOrder):
    mesh = dg.MeshManager()
    if mesh_arg.startswith("box:"):
        nx, ny = (int(v) for v in mesh_arg[4:].split("x"))
        mesh.buildMesh(*quad_box(nx, ny))
    else:
        mesh.readMesh(mesh_arg)
    nodes = dg.QuadNodesProvisioner(NOrder, mesh)
    nodes.buildFilter(0.99 * NOrder, 4)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    g = 9.81
    h = 10.0 + 0.5 * np.exp(-10 * (x + 0.3) ** 2 - 10 * y * y)       # a hump released from rest
    hu, hv = np.zeros_like(h), np.zeros_like(h)
    hN = h * np.exp(-((x - 0.2) / 0.25) ** 2 - ((y + 0.1) / 0.25) ** 2)  # a tracer blob
    sources = {"zx": 0.02 + 0 * x, "zy": 0.01 * y, "f": 0.5 * (1.0 + 0.2 * y), "CD": 2.5e-3}
    V1 = dg.VandermondeBuilder().buildVandermondeMatrix(ctx.s[:NOrder + 1])[0]
    w1 = np.linalg.inv(V1 @ V1.T).sum(axis=1)                              # 1-D Gauss-Lobatto weights
    wJ = np.outer(w1, w1).ravel()[:, None] * ctx.J
    return nodes, (h, hu, hv, hN), g, sources, wJ


def main():
    mesh_arg = sys.argv[1] if len(sys.argv) > 1 else "box:24x24"
    NOrder = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    finalTime = float(sys.argv[3]) if len(sys.argv) > 3 else 0.05
    outdir = sys.argv[4] if len(sys.argv) > 4 else None
    nodes, q, g, sources, wJ = setup(mesh_arg, NOrder)
    solver = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=g, fields=4, sources=sources)
    solver.setState4(*q)
    m0, n0 = (wJ * q[0]).sum(), (wJ * q[3]).sum()
    outputter = None
    if outdir:
        os.makedirs(outdir, exist_ok=True)
        outputter = dg.VtkOutputter(nodes)
    t, step, CFL = 0.0, 0, 0.5
    while t < finalTime:
        dt, speed = solver.computeDt(CFL)
        n = min(10, int(np.ceil((finalTime - t) / dt)))
        dt = min(dt, (finalTime - t) / n)
        solver.stepRK2(dt, n, filter=True)          # raises NumericalInstability on max|h| > 1e8 or NaN
        step += n
        t += n * dt
        h, hu, hv, hN = solver.getState4()
        m1, n1 = (wJ * h).sum(), (wJ * hN).sum()
        print(f"t={t:.6g} step={step} dt={dt:.4g} speed={speed:.5g} |u|max={np.hypot(hu, hv).max() / 10:.4g} "
              f"N in [{(hN / h).min():.4f}, {(hN / h).max():.4f}] water {abs(m1 - m0) / m0:.2e} tracer {abs(n1 - n0) / n0:.2e}")
        if outdir:
            np.save(os.path.join(outdir, f"state{step:07d}.npy"), np.stack([h, hu, hv, hN]))
            outputter.writeSolverFields(solver, step, directory=outdir)
    assert abs(m1 - m0) <= 1e-12 * m0 and abs(n1 - n0) <= 1e-12 * n0, "mass is not conserved to round-off"
    return solver.getState4(), t


if __name__ == "__main__":
    main()
