#!/usr/bin/env python3
"""The reference's two Poisson drivers on the MI355X path (blitzdg_amd.poisson2d), on buildBoxMesh:

  * src/poisson2d: -lap u = 2 pi^2 sin(pi x) sin(pi y) on [-1, 1]^2 with u = 0 on the walls (the driver solves with a
    matrix-free Laplacian and a Krylov solver; here the operator is -lap, positive definite, and the solver is conjugate
    gradients in the mass inner product);
  * poisson2d.py: the pure-Neumann problem -lap u = 2 pi^2 cos(pi x) cos(pi y), du/dn = 0 on all four sides. The script borders
    the assembled matrix with the constant to pin the mean; here the solver removes the mass-weighted mean of the right-hand
    side, of the residual and of the solution (the bordering trick without the border).

    python examples/poisson2d.py [NXxNY] [order]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import poisson2d  # noqa: E402


def main():
    nx, ny = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "24x20").split("x"))
    order = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    pi = np.pi

    # ---- walls are Dirichlet (the default mapD of a provisioner: BCmap[Wall] + BCmap[Dirichlet])
    exact = np.sin(pi * x) * np.sin(pi * y)
    solver = poisson2d.Poisson2dSolver(nodes=nodes)
    u, info = solver.solve(2 * pi * pi * exact, relTol=1e-10)
    print(f"Dirichlet: K = {ctx.numElements}, N = {order}: {info.iterations} iterations, relative residual "
          f"{info.relativeResidual:.2e}, max error {np.abs(u - exact).max():.3e}")
    ms = solver.timeIterations(20)
    print(f"           {ms:.4f} ms per iteration, {solver.timeApply(20):.4f} ms per operator application")
    solver.close()

    # ---- no Dirichlet node and no shift: the singular case
    exact = np.cos(pi * x) * np.cos(pi * y)
    solver = poisson2d.Poisson2dSolver(nodes=nodes, mapD=[])
    u, info = solver.solve(2 * pi * pi * exact, relTol=1e-10)
    w = np.asarray(nodes.quadratureWeights())
    exact = exact - (w * exact).sum() / w.sum()
    print(f"Neumann:   {info.iterations} iterations, relative residual {info.relativeResidual:.2e}, projected {info.projected}, "
          f"mean {(w * u).sum() / w.sum():+.1e}, max error {np.abs(u - exact).max():.3e}")
    solver.close()


if __name__ == "__main__":
    main()
