#!/usr/bin/env python3
"""Tide gauges and conservation diagnostics recorded on the device in a triangle run: a tidal variant-B set-up on a small
box with the run monitor switched on (the triangle counterpart of examples/sw2d_quads_gauges.py).

    python examples/sw2d_gauges.py [finalTime] [order] [cells] [csv]

A 10 km square basin of cells x cells x 2 triangles, open towards the tide on the side x = 0 and walled elsewhere, a sloping
bed with a shoal, drag, Coriolis and a sponge in front of the open side. Three gauges stand 1 km, 5 km and 9 km from the open
side on the basin's centre line. After every step the solver records mass, momentum, energy, the extrema and eta, u, v at the
gauges on the device (enableMonitor, stride 1): the loop never downloads the state. Every 50 steps the records are read and the
reference driver's report line is printed from them (src/sw2d/main.cpp:198-199: h_min / h_max / hu_max / hv_max); at the end
every record goes to `csv` (default gauges.csv): t, mass, energy, then eta, u, v per gauge.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.sw2d import Sw2dSolver  # noqa: E402

OUT = 2  # BCTag::Out
REPORT = 50


def main():
    finalTime = float(sys.argv[1]) if len(sys.argv) > 1 else 600.0
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    csv = sys.argv[4] if len(sys.argv) > 4 else "gauges.csv"
    g, CD, f, CFL, L = 9.81, 2.5e-3, 1.0e-4, 0.5, 1.0e4
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
    gauges = np.array([[0.1 * L, 0.5 * L], [0.5 * L, 0.5 * L], [0.9 * L, 0.5 * L]])

    solver = Sw2dSolver(nodes=nodes, g=g)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tideAmplitude=0.5, tidePeriod=3600.0, tideRamp=0.15 / 3600,
                          sponge=sponge)
    solver.enableMonitor(nodes, gauges=gauges, stride=1, capacity=REPORT)   # eta = h - H with the bed of variant B
    solver.setState(H.copy(), np.zeros_like(H), np.zeros_like(H))
    rows = []
    t, step = 0.0, 0
    t0 = time.perf_counter()
    while t < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)
        t = solver.time
        step += 1
        if step % REPORT == 0 or t >= finalTime:
            rec = solver.monitorRecords()               # the only download: REPORT records of a few doubles
            solver.resetMonitor()
            rows.append(np.column_stack([rec["t"], rec["mass"], rec["energy"], rec["gauges"].reshape(len(rec["t"]), -1)]))
            print(f"t={rec['t'][-1]:.2f} step={step} dt={dt:.4f} h_min={rec['hmin'][-1]:.5f} h_max={rec['hmax'][-1]:.5f} "
                  f"hu_max={rec['humax'][-1]:.5f} hv_max={rec['hvmax'][-1]:.5f} mass={rec['mass'][-1]:.8e} "
                  f"eta@gauges={' '.join(f'{v:+.5f}' for v in rec['gauges'][-1, :, 0])}", flush=True)
    wall = time.perf_counter() - t0
    table = np.concatenate(rows) if rows else np.zeros((0, 12))
    header = "t,mass,energy," + ",".join(f"{name}{i}" for i in range(len(gauges)) for name in ("eta", "u", "v"))
    np.savetxt(csv, table, delimiter=",", header=header, comments="")
    print(f"done: {step} steps to t={t:.2f} on {ctx.numElements} triangles at N={N} in {wall:.2f} s; "
          f"{len(table)} records in {os.path.abspath(csv) if os.path.isabs(csv) else csv}")


if __name__ == "__main__":
    main()
