#!/usr/bin/env python3
"""A tidal basin on triangles with a Smagorinsky eddy viscosity on the momentum: the set-up of examples/sw2d_tidal_tracer.py (variant
B with a passive tracer fed at the open side, state resident in HBM) plus Sw2dSolver.enableViscosity -- the horizontal mixing
div(nu h grad u), nu = nu0 + Cs^2 D^2 |S|, that shear layers behind the bump and along the walls call for.

    python examples/sw2d_tidal_viscosity.py [finalTime] [order] [cells] [csv] [outputDir] [nu0] [Cs]

The basin, bed, tide, drag, Coriolis and sponge are those of sw2d_tidal_tracer.py; nu0 defaults to 0.5 m^2/s and Cs to 0.2. The
loop is the driver's: the time step from the state (computeDt, CFL 0.5 -- now min(advective dt, CFL dt_visc) with the largest nu
of the current state), one Heun / SSP-RK2 step with the sponge division (stepSSPRK2; with viscosity on the division follows the
viscous term). Every 50 steps the monitor's records are read and a line is printed with the range of nu (eddyViscosity()); at
the end the records go to `csv` (default viscosity.csv) and nu at the nodes to the same name with .nu.npy in place of .csv. With
an output directory, eta, u, v and N as *.vtu files every 50 steps (VtkOutputter.writeSolverFields), as the tracer example writes.
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
    csv = sys.argv[4] if len(sys.argv) > 4 else "viscosity.csv"
    outdir = sys.argv[5] if len(sys.argv) > 5 else None
    nu0 = float(sys.argv[6]) if len(sys.argv) > 6 else 0.5
    Cs = float(sys.argv[7]) if len(sys.argv) > 7 else 0.2
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
    nodes.buildFilter(0.9 * N, N)                       # the tidal driver's filter; it enters through the bed slopes only
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    mapO = ctx.BCmap[OUT]
    H = 12.0 - 4.0 * x / L - 2.0 * np.exp(-((x - 0.6 * L) ** 2 + (y - 0.5 * L) ** 2) / (0.1 * L) ** 2)
    Hx, Hy = nodes.bedSlopes(H)
    sponge = nodes.buildSpongeCoeff(mapO, 1.0e-2, 1500.0)
    gauges = np.array([[0.02 * L, 0.5 * L], [0.1 * L, 0.5 * L], [0.3 * L, 0.5 * L]])

    solver = Sw2dSolver(nodes=nodes, g=g, fields=4)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tideAmplitude=0.5, tidePeriod=3600.0, tideRamp=0.15 / 3600,
                          sponge=sponge, tracer=1.0)
    solver.enableViscosity(nu0, Cs)
    solver.enableMonitor(nodes, gauges=gauges, stride=1, capacity=REPORT)   # eta = h - H with the bed of variant B
    solver.setState4(H.copy(), np.zeros_like(H), np.zeros_like(H), np.zeros_like(H))
    outputter = None
    if outdir:
        os.makedirs(outdir, exist_ok=True)
        outputter = dg.VtkOutputter(nodes)
        outputter.writeSolverFields(solver, 0, directory=outdir)     # eta = h - H with the bed of variant B
    rows = []
    t, step = 0.0, 0
    t0 = time.perf_counter()
    while t < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)                           # raises NumericalInstability as the driver's check would
        t = solver.time
        step += 1
        if outputter and step % REPORT == 0:
            outputter.writeSolverFields(solver, step, directory=outdir)
        if step % REPORT == 0 or t >= finalTime:
            rec = solver.monitorRecords()               # the only download: REPORT records of a few doubles
            solver.resetMonitor()
            gv = rec["gauges"]                          # (records, gauges, fields): eta, u, v, N
            rows.append(np.column_stack([rec["t"], rec["mass"], rec["tracer"], gv[:, :, 0], gv[:, :, 3]]))
            nu = solver.eddyViscosity()
            print(f"t={rec['t'][-1]:.2f} step={step} dt={dt:.4f} speed={solver.globalSpeed:.4f} h_min={rec['hmin'][-1]:.5f} "
                  f"h_max={rec['hmax'][-1]:.5f} nu in [{nu.min():.4f}, {nu.max():.4f}] int hN={rec['tracer'][-1]:.6e} N at the gauges "
                  + " ".join(f"{v:.4f}" for v in gv[-1, :, 3]), flush=True)
    wall = time.perf_counter() - t0
    table = np.concatenate(rows) if rows else np.zeros((0, 3 + 2 * len(gauges)))
    header = "t,mass,tracer," + ",".join(f"eta{i}" for i in range(len(gauges))) + "," + ",".join(f"N{i}" for i in range(len(gauges)))
    np.savetxt(csv, table, delimiter=",", header=header, comments="")
    np.save(os.path.splitext(csv)[0] + ".nu.npy", solver.eddyViscosity())
    print(f"done: {step} steps to t={t:.2f} on {ctx.numElements} triangles at N={N} in {wall:.2f} s; {len(table)} records in {csv}")


if __name__ == "__main__":
    main()
