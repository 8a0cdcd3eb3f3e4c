#!/usr/bin/env python3
"""Drifter tracks in the tidal basin of examples/sw2d_gauges.py: a line of drifters across a variant-B run on triangles,
advanced on the device after every Heun step of the tidal driver's loop, their tracks written as CSV (the triangle counterpart
of examples/sw2d_quads_drifters.py).

    python examples/sw2d_drifters.py [finalTime] [order] [cells] [drifters] [tracks.csv]

A 10 km square basin of cells x cells x 2 triangles, open towards the tide on the side x = 0 and walled elsewhere, a sloping
bed with a shoal, drag, Coriolis and a sponge in front of the open side. The drifters start on the line x = 3 km,
1 km <= y <= 9 km; one that leaves through the open side gets status 1 and stays where it left, one that reaches a wall slides
along it (status bit 4). The loop never downloads the state. A record is kept every 20 steps; the CSV has one row per record
and drifter: t, drifter, x, y, status (NumPy only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.sw2d import Sw2dSolver  # noqa: E402

OUT = 2  # BCTag::Out


def main():
    finalTime = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    count = int(sys.argv[4]) if len(sys.argv) > 4 else 17
    path = sys.argv[5] if len(sys.argv) > 5 else "drifter_tracks.csv"
    g, CD, f, CFL, L = 9.81, 2.5e-3, 1.0e-4, 0.5, 1.0e4
    stride, capacity = 20, 256
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(n, n, 0.0, L, 0.0, L)
    # the wall faces on the side x = 0 become the open boundary
    verts = np.asarray(mesh.vertices).reshape(-1, 3)
    etov = np.asarray(mesh.elements).reshape(-1, 3)
    bc = np.array(mesh.bcType).reshape(-1, 3)
    for face, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
        left = (verts[etov[:, a], 0] < 1e-9 * L) & (verts[etov[:, b], 0] < 1e-9 * L)
        bc[left & (bc[:, face] != 0), face] = OUT
    mesh.setBCType(bc.ravel())
    nodes = dg.TriangleNodesProvisioner(N, mesh)
    nodes.buildFilter(0.9 * N, N)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    mapO = ctx.BCmap[OUT]
    H = 12.0 - 4.0 * x / L - 2.0 * np.exp(-((x - 0.6 * L) ** 2 + (y - 0.5 * L) ** 2) / (0.1 * L) ** 2)
    Hx, Hy = nodes.bedSlopes(H)
    sponge = nodes.buildSpongeCoeff(mapO, 1.0e-2, 1500.0)

    solver = Sw2dSolver(nodes=nodes, g=g)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tideAmplitude=0.5, tidePeriod=3600.0, tideRamp=0.15 / 3600,
                          sponge=sponge)
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
    while solver.time < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)
        step += 1
        if step % (stride * capacity) == 0:
            drain()
    drain()
    now = solver.drifterState()
    moved = np.hypot(*(now["xy"] - start).T)
    print(f"t={solver.time:.2f} after {step} steps: {count} drifters moved {moved.min():.2f} .. {moved.max():.2f} m, "
          f"status {np.unique(now['status']).tolist()}")
    table = np.concatenate(rows) if rows else np.empty((0, 5))
    np.savetxt(path, table, delimiter=",", header="t,drifter,x,y,status", comments="", fmt=["%.6f", "%d", "%.6f", "%.6f", "%d"])
    print(f"wrote {len(table)} rows to {path}")


if __name__ == "__main__":
    main()
