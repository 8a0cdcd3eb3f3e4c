#!/usr/bin/env python3
"""The two problems of examples/poisson2d.py on quadrilaterals (blitzdg_amd.poisson2d.Poisson2dQuadSolver):

  * -lap u = 2 pi^2 sin(pi x) sin(pi y) on [-1, 1]^2 with u = 0 on the walls;
  * the pure-Neumann problem -lap u = 2 pi^2 cos(pi x) cos(pi y), du/dn = 0 on all four sides, which the reference's src/ins2d
    driver solves for its pressure on a QuadNodesProvisioner context with a bordered Poisson2DSparseMatrix: here the solver
    removes the mass-weighted mean of the right-hand side, of the residual and of the solution (the bordered system without
    the border).

    python examples/poisson2d_quads.py [NXxNY] [order]

Without a mesh size the mesh is tests/golden/coarse_box_quads.msh if the solver takes it -- it takes quadrilaterals in
parallelogram form only and says so otherwise --, else a 24 x 20 box of rectangles.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import _capi as C  # noqa: E402
from blitzdg_amd import poisson2d  # noqa: E402


def quad_box(nx, ny):
    """EToV (K, 4) and Vert of an nx x ny box of counter-clockwise rectangles on [-1, 1]^2."""
    X, Y = np.meshgrid(np.linspace(-1.0, 1.0, nx + 1), np.linspace(-1.0, 1.0, ny + 1))
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    return np.stack([a, a + 1, a + nx + 2, a + nx + 1], axis=1), np.stack([X.ravel(), Y.ravel()], axis=1)


def box_nodes(nx, ny, order):
    mesh = dg.MeshManager()
    mesh.buildMesh(*quad_box(nx, ny))
    return mesh, dg.QuadNodesProvisioner(order, mesh)


def main():
    order = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    if len(sys.argv) > 1:
        mesh, nodes = box_nodes(*(int(v) for v in sys.argv[1].split("x")), order)
        solver = poisson2d.Poisson2dQuadSolver(nodes=nodes)
    else:
        mesh = dg.MeshManager()
        mesh.readMesh(os.path.join(ROOT, "tests", "golden", "coarse_box_quads.msh"))
        nodes = dg.QuadNodesProvisioner(order, mesh)
        try:
            solver = poisson2d.Poisson2dQuadSolver(nodes=nodes)
        except C.BdgError as e:
            if "parallelogram" not in str(e):
                raise
            print(f"coarse_box_quads.msh refused ({e}); using a 24 x 20 box")
            mesh, nodes = box_nodes(24, 20, order)
            solver = poisson2d.Poisson2dQuadSolver(nodes=nodes)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    pi = np.pi

    # ---- walls are Dirichlet (the default mapD of a provisioner: BCmap[Wall] + BCmap[Dirichlet])
    exact = np.sin(pi * x) * np.sin(pi * y)
    u, info = solver.solve(2 * pi * pi * exact, relTol=1e-10)
    print(f"Dirichlet: K = {ctx.numElements}, N = {order}: {info.iterations} iterations, relative residual "
          f"{info.relativeResidual:.2e}, max error {np.abs(u - exact).max():.3e}")
    print(f"           {solver.timeIterations(20):.4f} ms per iteration, {solver.timeApply(20):.4f} ms per operator application")
    solver.close()

    # ---- no Dirichlet node and no shift: the singular case
    exact = np.cos(pi * x) * np.cos(pi * y)
    solver = poisson2d.Poisson2dQuadSolver(nodes=nodes, mapD=[])
    u, info = solver.solve(2 * pi * pi * exact, relTol=1e-10)
    one = np.ones_like(u)
    area = solver.massDot(one, one)
    exact = exact - solver.massDot(one, exact) / area
    print(f"Neumann:   {info.iterations} iterations, relative residual {info.relativeResidual:.2e}, projected {info.projected}, "
          f"mean {solver.massDot(one, u) / area:+.1e}, max error {np.abs(u - exact).max():.3e}")
    solver.close()


if __name__ == "__main__":
    main()
