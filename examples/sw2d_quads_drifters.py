#!/usr/bin/env python3
"""Drifter tracks in the tidal basin of examples/sw2d_quads_tidal.py: a line of drifters across the basin, advanced on the
device after every Heun step of the tidal driver's loop, their tracks written as CSV.

    python examples/sw2d_quads_drifters.py [finalTime] [order] [cells] [drifters] [tracks.csv]

The basin, bed, tide, drag, Coriolis and sponge are those of sw2d_quads_tidal.py. The drifters start on the line x = 3 km,
1 km <= y <= 9 km; one that leaves through the open side x = 0 gets status 1 and stays where it left, one that reaches a wall
slides along it (status bit 4). A record is kept every 20 steps; the CSV has one row per record and drifter:
t, drifter, x, y, status (NumPy only)."""
import os
import sys

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
    count = int(sys.argv[4]) if len(sys.argv) > 4 else 17
    path = sys.argv[5] if len(sys.argv) > 5 else "drifter_tracks.csv"
    g, CD, f, CFL, L = 9.81, 2.5e-3, 1.0e-4, 0.5, 1.0e4
    stride, capacity = 20, 256
    mesh = dg.MeshManager()
    mesh.buildMesh(*box(n, L))
    bc = np.array(mesh.bcType).reshape(-1, 4)
    bc[np.arange(n) * n, 3] = OUT                       # the side x = 0
    mesh.setBCType(bc.ravel())
    nodes = dg.QuadNodesProvisioner(N, mesh)
    nodes.buildFilter(0.9 * N, N)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    mapO = ctx.BCmap[OUT]
    H = 12.0 - 4.0 * x / L - 2.0 * np.exp(-((x - 0.6 * L) ** 2 + (y - 0.5 * L) ** 2) / (0.1 * L) ** 2)
    Hx, Hy = nodes.bedSlopes(H)
    sponge = nodes.buildSpongeCoeff(mapO, 1.0e-2, 1500.0)

    solver = Sw2dQuadSolver(nodes=nodes, g=g)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tide=(0.5, 3600.0, 0.15 / 3600), sponge=sponge)
    solver.setState(H.copy(), np.zeros_like(H), np.zeros_like(H))
    start = np.stack([np.full(count, 0.3 * L), np.linspace(0.1 * L, 0.9 * L, count)], axis=1)
    solver.enableDrifters(nodes, start, mapO=mapO, stride=stride, capacity=capacity)

    rows = []

    def drain():                                        # the records so far, then room for the next ones
        t, xy, status = solver.drifterTracks()
        for i in range(len(t)):
            rows.append(np.column_stack([np.full(count, t[i]), np.arange(count), xy[i], status[i]]))
        solver.resetDrifterTracks()

    step = 0
    while solver.getTime() < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)
        step += 1
        if step % (stride * capacity) == 0:
            drain()
    drain()
    now = solver.drifterState()
    moved = np.hypot(*(now["xy"] - start).T)
    print(f"t={solver.getTime():.2f} after {step} steps: {count} drifters moved {moved.min():.2f} .. {moved.max():.2f} m, "
          f"status {np.unique(now['status']).tolist()}")
    table = np.concatenate(rows) if rows else np.empty((0, 5))
    np.savetxt(path, table, delimiter=",", header="t,drifter,x,y,status", comments="", fmt=["%.6f", "%d", "%.6f", "%.6f", "%d"])
    print(f"wrote {len(table)} rows to {path}")


if __name__ == "__main__":
    main()
