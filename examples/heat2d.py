#!/usr/bin/env python3
"""The reference's heat2d.py driver -- backward-Euler steps of the heat equation with mixed, inhomogeneous boundary data -- on
the MI355X path: every step solves

    (1/dt - kappa lap) p = p_old / dt

on the device (blitzdg_amd.poisson2d: the stabilised central flux operator, conjugate gradients in the mass inner product),
with Dirichlet data on three sides of the box and Neumann data on the fourth.

    python examples/heat2d.py [NXxNY] [order] [steps] [ratio]

Differences from the script: the mesh is buildBoxMesh (the script reads a .msh file with sides tagged 6 and 7), the step is
`ratio` (default 50) of the step an explicit diffusion step could take, dt_diff = 4 / (kappa (N+1)^4 max(Fscale)^2), and the
system is never assembled: the script factors a sparse matrix once, here every step is a matrix-free solve that starts from
the previous step's solution.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import poisson2d  # noqa: E402


def diffusion_dt(kappa, order, Fscale, c=4.0):
    """The step of the explicit tracer diffusion (Sw2dSolver.diffusionDt)."""
    return c / (kappa * (order + 1) ** 4 * np.abs(Fscale).max() ** 2)


def backward_euler_steps(solver, p, dt, nsteps, relTol=1e-10, checkEvery=8):
    """`nsteps` steps (1/dt + A) p = p_old / dt with the solver's operator A = -div(kappa grad) and its boundary data, each from
    the step before. Returns (p, iterations per step)."""
    solver.setShift(1.0 / dt)
    iterations = []
    for _ in range(nsteps):
        p, info = solver.solve(p / dt, x0=p, relTol=relTol, checkEvery=checkEvery)
        if not info.converged:
            raise RuntimeError(f"backward Euler step {len(iterations)}: no convergence in {info.iterations} iterations")
        iterations.append(info.iterations)
    return p, iterations


def face_nodes(ctx):
    """x, y, nx, ny at the face nodes, (3 Nfp, K), and the flat indices of the boundary ones."""
    vM, vP = np.asarray(ctx.vmapM), np.asarray(ctx.vmapP)
    shape = ctx.nx.shape
    Fx = ctx.x.flatten("F")[vM].reshape(shape, order="F")
    Fy = ctx.y.flatten("F")[vM].reshape(shape, order="F")
    return Fx, Fy, ctx.nx, ctx.ny, np.nonzero(vM == vP)[0]


def main():
    nx, ny = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "24x20").split("x"))
    order = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    ratio = float(sys.argv[4]) if len(sys.argv) > 4 else 50.0
    kappa = 0.05

    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    ctx = nodes.dgContext()
    Fx, Fy, nxf, nyf, boundary = face_nodes(ctx)
    top = nyf.flatten("F")[boundary] > 0.5
    mapD, mapN = boundary[~top], boundary[top]          # Dirichlet on the left, right and bottom, Neumann on the top
    g = 0.25 * (np.exp(Fx - 1.0) - 1.0) * (1.0 - Fy)    # the script's boundary profile, scaled to this box
    qn = 0.02 * np.cos(2 * Fx)                          # kappa dp/dn on the top

    solver = poisson2d.Poisson2dSolver(nodes=nodes, mapD=mapD, kappa=kappa)
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
