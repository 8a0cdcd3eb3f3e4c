#!/usr/bin/env python3
"""A dye carried into a tidal basin: examples/sw2d_quads_tidal.py (the loop of the reference's C++ tidal driver,
src/sw2d/main.cpp:192-244, on a box of quadrilaterals, state resident in HBM) with a passive tracer as a fourth field. The
basin starts at concentration 0 and the open side feeds concentration 1 (enableVariantB(..., tracer=1.0) on a four-field solver).

    python examples/sw2d_quads_tidal_tracer.py [finalTime] [order] [cells] [outputDir]

A 10 km x 10 km basin of cells x cells quadrilaterals (default 24). The bed slopes from 12 m at the open side x = 0 to 8 m and
carries a 2 m bump; that side is tagged Out (MeshManager.setBCType before the provisioner builds its BC hash) and driven by a tide of 0.5 m amplitude and a
period of one hour; the other sides are walls. Drag, Coriolis, a sponge layer of 1.5 km around the open side. The loop is the
driver's: the time step from the state (computeDt, CFL 0.5), one Heun / SSP-RK2 step with the sponge division (stepSSPRK2),
eta and tracer statistics every 50 steps; the run monitor records int hN and the concentration N at three gauges on the
basin's axis after every step, on the device; with an output directory, eta, u, v and N as *.vtu files (writeSolverFields with H).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.sw2dquads import Sw2dQuadSolver  # noqa: E402

OUT = 2  # BCTag::Out


def box(n, length):
    xs = np.linspace(0.0, length, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    return np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1), V


def main():
    finalTime = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    outdir = sys.argv[4] if len(sys.argv) > 4 else None
    g, CD, f, CFL, L = 9.81, 2.5e-3, 1.0e-4, 0.5, 1.0e4
    mesh = dg.MeshManager()
    mesh.buildMesh(*box(n, L))
    bc = np.array(mesh.bcType).reshape(-1, 4)
    bc[np.arange(n) * n, 3] = OUT                       # face 3 of the first column of elements: the side x = 0
    mesh.setBCType(bc.ravel())
    nodes = dg.QuadNodesProvisioner(N, mesh)
    nodes.buildFilter(0.9 * N, N)                       # the tidal driver's filter; it enters through the bed slopes only
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    mapO = ctx.BCmap[OUT]
    H = 12.0 - 4.0 * x / L - 2.0 * np.exp(-((x - 0.6 * L) ** 2 + (y - 0.5 * L) ** 2) / (0.1 * L) ** 2)
    Hx, Hy = nodes.bedSlopes(H)
    sponge = nodes.buildSpongeCoeff(mapO, 1.0e-2, 1500.0)

    solver = Sw2dQuadSolver(nodes=nodes, g=g, fields=4)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tide=(0.5, 3600.0, 0.15 / 3600), sponge=sponge, tracer=1.0)
    gauges = np.array([[0.02 * L, 0.5 * L], [0.1 * L, 0.5 * L], [0.3 * L, 0.5 * L]])
    solver.enableMonitor(nodes, gauges=gauges, capacity=1 << 16)    # eta = h - H with the solver's own H
    solver.setState4(H.copy(), np.zeros_like(H), np.zeros_like(H), np.zeros_like(H))
    outputter = None
    if outdir:
        os.makedirs(outdir, exist_ok=True)
        outputter = dg.VtkOutputter(nodes)
        outputter.writeSolverFields(solver, 0, directory=outdir, H=H)
    t, step = 0.0, 0
    t0 = time.perf_counter()
    while t < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)                           # raises NumericalInstability as the driver's check would
        t = solver.getTime()
        step += 1
        if outputter and step % 50 == 0:
            outputter.writeSolverFields(solver, step, directory=outdir, H=H)
        if step % 50 == 0 or t >= finalTime:
            h, hu, hv, hN = solver.getState4()
            rec = solver.monitorRecords()
            solver.resetMonitor()
            print(f"t={t:.2f} step={step} dt={dt:.4f} speed={solver.globalSpeed():.4f} eta in [{(h - H).min():+.5f}, "
                  f"{(h - H).max():+.5f}] max|u|={np.hypot(hu, hv).max() / h.min():.4f} N in [{(hN / h).min():+.4f}, "
                  f"{(hN / h).max():+.4f}] int hN={rec['tracer'][-1]:.6e} N at the gauges "
                  + " ".join(f"{v:.4f}" for v in rec["gauges"][-1][:, 3]), flush=True)
    wall = time.perf_counter() - t0
    print(f"done: {step} steps to t={t:.2f} on {ctx.numElements} quadrilaterals at N={N} in {wall:.2f} s")


if __name__ == "__main__":
    main()
