#!/usr/bin/env python3
"""examples/heat2d.py on quadrilaterals: backward-Euler steps of the heat equation with mixed, inhomogeneous boundary data,

    (1/dt - kappa lap) p = p_old / dt,

each solved on the device by blitzdg_amd.poisson2d.Poisson2dQuadSolver, with Dirichlet data on three sides of the box and
Neumann data on the fourth. This is the step an explicit Sw2dQuadSolver(fields=4).enableTracerDiffusion(...) run cannot take:
its dt is bound by dt_diff = 4 / (kappa (N+1)^4 max(Fscale)^2), here dt is `ratio` (default 50) times that.

    python examples/heat2d_quads.py [NXxNY] [order] [steps] [ratio]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from blitzdg_amd import poisson2d  # noqa: E402
from heat2d import backward_euler_steps, diffusion_dt, face_nodes  # noqa: E402
from poisson2d_quads import box_nodes  # noqa: E402


def main():
    nx, ny = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "24x20").split("x"))
    order = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    ratio = float(sys.argv[4]) if len(sys.argv) > 4 else 50.0
    kappa = 0.05

    mesh, nodes = box_nodes(nx, ny, order)
    ctx = nodes.dgContext()
    Fx, Fy, nxf, nyf, boundary = face_nodes(ctx)          # (4 Nfp, K) here
    top = nyf.flatten("F")[boundary] > 0.5
    mapD, mapN = boundary[~top], boundary[top]          # Dirichlet on the left, right and bottom, Neumann on the top
    g = 0.25 * (np.exp(Fx - 1.0) - 1.0) * (1.0 - Fy)
    qn = 0.02 * np.cos(2 * Fx)                          # kappa dp/dn on the top

    solver = poisson2d.Poisson2dQuadSolver(nodes=nodes, mapD=mapD, kappa=kappa)
    solver.setBoundaryData(g, qn)
    dt = ratio * diffusion_dt(kappa, order, ctx.Fscale)
    p = np.exp(-4 * (ctx.x ** 2 + ctx.y ** 2))
    print(f"K = {ctx.numElements}, N = {order}, {mapD.size} Dirichlet and {mapN.size} Neumann nodes, dt = {dt:.4e} "
          f"({ratio:g} explicit steps), device bytes {solver.deviceBytes()}")
    t = 0.0
    for step in range(steps):
        p, its = backward_euler_steps(solver, p, dt, 1)
        t += dt
        print(f"step {step + 1:3d}  t = {t:.4f}  iterations {its[0]:4d}  min {p.min():+.4f}  max {p.max():+.4f}")
    solver.close()


if __name__ == "__main__":
    main()
