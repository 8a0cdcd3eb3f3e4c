#!/usr/bin/env python3
"""Shallow water on quadrilaterals: the loop of the reference's sw2dquads.py driver on the MI355X path, state resident
in HBM.

    python examples/sw2d_quads.py [finalTime] [order] [outputDir]

The script's set-up: coarse_box_quads_fine.msh (a copy ships in tests/golden/), N = 4, the quad filter built with
Nc = 0.99 N and s = 4, a Gaussian hump of height 1 on still water of depth 10, u = v = 0, its fixed dt = 0.45 *
0.000724295, g = 9.81. The loop body (midpoint RK2 with the filter on both right-hand sides, then the blow-up check) runs
on the device, 20 steps per call; the driver prints eta statistics. With an output directory it also writes eta, u, v as
*.vtu files at step 0 and every 20 steps, as the script does (the fields are formed and interpolated to the output lattice on
the device).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.sw2dquads import Sw2dQuadSolver  # noqa: E402


def main():
    finalTime = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    outdir = sys.argv[3] if len(sys.argv) > 3 else None
    g = 9.81
    mesh = dg.MeshManager()
    mesh.readMesh(os.path.join(ROOT, "tests", "golden", "coarse_box_quads_fine.msh"))
    nodes = dg.QuadNodesProvisioner(N, mesh)
    nodes.buildFilter(0.99 * N, 4)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    H = 10.0 * np.ones_like(x)
    eta = np.exp(-10 * x * x - 10 * y * y)
    h = H + eta
    hu, hv = np.zeros_like(h), np.zeros_like(h)

    solver = Sw2dQuadSolver(nodes=nodes, g=g)
    solver.setState(h, hu, hv)
    dt = 0.45 * 0.000724295
    t, step, chunk = 0.0, 0, 20
    outputter = None
    if outdir:
        os.makedirs(outdir, exist_ok=True)
        outputter = dg.VtkOutputter(nodes)
        outputter.writeSolverFields(solver, 0, directory=outdir, H=H)
    t0 = time.perf_counter()
    while t < finalTime:
        n = min(chunk, int(np.ceil((finalTime - t) / dt)))
        solver.stepRK2(dt, n, filter=True)  # raises NumericalInstability as the script's check would
        t += n * dt
        step += n
        if outputter and step % 20 == 0:
            outputter.writeSolverFields(solver, step, directory=outdir, H=H)
        if step % 400 == 0 or t >= finalTime:
            h, hu, hv = solver.getState()
            print(f"t={t:.4f} step={step} eta in [{(h - H).min():+.5f}, {(h - H).max():+.5f}] "
                  f"max|u|={np.abs(hu / h).max():.4f}", flush=True)
    wall = time.perf_counter() - t0
    print(f"done: {step} steps to t={t:.4f} on {ctx.numElements} quadrilaterals at N={N} in {wall:.2f} s")


if __name__ == "__main__":
    main()
