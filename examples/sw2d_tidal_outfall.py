#!/usr/bin/env python3
"""An outfall in a tidal basin on triangles: the basin of examples/sw2d_tidal_tracer.py (variant B with a passive tracer, state
resident in HBM) with the tracer's diffusion and a source switched on (Sw2dSolver.enableTracerDiffusion). The basin starts clean
and the open side feeds clean water (concentration 0); a Gaussian source S of hN per second releases the tracer around a point
inside, a constant diffusivity kappa mixes it, decay is off.

    python examples/sw2d_tidal_outfall.py [finalTime] [order] [cells] [csv] [kappa]

A 10 km x 10 km basin of cells x cells x 2 triangles (default 24), bed, tide, drag, Coriolis and sponge as in
sw2d_tidal_tracer.py. The outfall sits at (0.4 L, 0.5 L) with a radius of 400 m and releases one unit of hN per second in all;
kappa defaults to 5 m^2/s. The loop is the tidal driver's: the time step from the state (computeDt, CFL 0.5 -- with diffusion
on, the smaller of the advective step and CFL * diffusionDt()), one Heun / SSP-RK2 step with the sponge division. After every
step the run monitor records int hN and the concentration N at three gauges -- at the outfall, 1 km down the axis towards the
open side, and 3 km -- on the device; every 50 steps the records are read and a line is printed; at the end they go to `csv`
(default outfall.csv): t, int hN, the amount released so far, then N per gauge. While nothing has reached the open side,
int hN equals the amount released.
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
    csv = sys.argv[4] if len(sys.argv) > 4 else "outfall.csv"
    kappa = float(sys.argv[5]) if len(sys.argv) > 5 else 5.0
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
    x0, y0, radius = 0.4 * L, 0.5 * L, 400.0
    gauges = np.array([[x0, y0], [x0 - 0.1 * L, y0], [x0 - 0.3 * L, y0]])
    w = np.asarray(nodes.quadratureWeights())
    S = np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / radius ** 2)
    S /= (w * S).sum()                                  # one unit of hN per second over the basin
    rate = (w * S).sum()

    solver = Sw2dSolver(nodes=nodes, g=g, fields=4)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tideAmplitude=0.5, tidePeriod=3600.0, tideRamp=0.15 / 3600,
                          sponge=sponge, tracer=0.0)
    solver.enableTracerDiffusion(kappa, source=S)       # after enableVariantB, before the first evaluation
    solver.enableMonitor(nodes, gauges=gauges, stride=1, capacity=REPORT)
    solver.setState4(H.copy(), np.zeros_like(H), np.zeros_like(H), np.zeros_like(H))
    print(f"kappa={kappa} diffusionDt={solver.diffusionDt():.4f} first dt={solver.computeDt(CFL)[0]:.4f} (CFL {CFL})")
    rows = []
    t, step = 0.0, 0
    t0 = time.perf_counter()
    while t < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)                           # raises NumericalInstability as the driver's check would
        t = solver.time
        step += 1
        if step % REPORT == 0 or t >= finalTime:
            rec = solver.monitorRecords()               # the only download: REPORT records of a few doubles
            solver.resetMonitor()
            gv = rec["gauges"]                          # (records, gauges, fields): eta, u, v, N
            rows.append(np.column_stack([rec["t"], rec["tracer"], rate * rec["t"], gv[:, :, 3]]))
            print(f"t={rec['t'][-1]:.2f} step={step} dt={dt:.4f} int hN={rec['tracer'][-1]:.6e} released={rate * rec['t'][-1]:.6e} "
                  "N at the gauges " + " ".join(f"{v:.3e}" for v in gv[-1, :, 3]), flush=True)
    wall = time.perf_counter() - t0
    table = np.concatenate(rows) if rows else np.zeros((0, 3 + len(gauges)))
    header = "t,tracer,released," + ",".join(f"N{i}" for i in range(len(gauges)))
    np.savetxt(csv, table, delimiter=",", header=header, comments="")
    print(f"done: {step} steps to t={t:.2f} on {ctx.numElements} triangles at N={N} in {wall:.2f} s; {len(table)} records in {csv}")


if __name__ == "__main__":
    main()
