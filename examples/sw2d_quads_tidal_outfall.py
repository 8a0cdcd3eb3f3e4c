#!/usr/bin/env python3
"""An outfall in a tidal basin on quadrilaterals: the basin of examples/sw2d_quads_tidal_tracer.py (variant B with a passive
tracer, state resident in HBM) with the tracer's diffusion and a source switched on (Sw2dQuadSolver.enableTracerDiffusion); the
quadrilateral twin of examples/sw2d_tidal_outfall.py. The basin starts clean and the open side feeds clean water
(concentration 0); a Gaussian source S of hN per second releases the tracer around a point inside, a constant diffusivity kappa
mixes it, decay is off.

    python examples/sw2d_quads_tidal_outfall.py [finalTime] [order] [cells] [csv] [kappa]

A 10 km x 10 km basin of cells x cells quadrilaterals (default 24), bed, tide, drag, Coriolis and sponge as in
sw2d_quads_tidal_tracer.py. The outfall sits at (0.4 L, 0.5 L) with a radius of 400 m and releases one unit of hN per second in
all; kappa defaults to 5 m^2/s. The loop is the tidal driver's: the time step from the state (computeDt, CFL 0.5 -- with diffusion
on, the smaller of the advective step and CFL * diffusionDt()), one Heun / SSP-RK2 step with the sponge division. After every
step the run monitor records int hN and the concentration N at three gauges -- at the outfall, 1 km down the axis towards the
open side, and 3 km -- on the device; every 50 steps the records are read and a line is printed; at the end they go to `csv`
(default outfall_quads.csv): t, int hN, the amount released so far, then N per gauge. While nothing has reached the open side,
int hN equals the amount released.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.sw2dquads import Sw2dQuadSolver  # noqa: E402

OUT = 2  # BCTag::Out
REPORT = 50


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
    csv = sys.argv[4] if len(sys.argv) > 4 else "outfall_quads.csv"
    kappa = float(sys.argv[5]) if len(sys.argv) > 5 else 5.0
    g, CD, f, CFL, L = 9.81, 2.5e-3, 1.0e-4, 0.5, 1.0e4
    mesh = dg.MeshManager()
    mesh.buildMesh(*box(n, L))
    bc = np.array(mesh.bcType).reshape(-1, 4)
    bc[np.arange(n) * n, 3] = OUT                       # face 3 of the first column of elements: the side x = 0
    mesh.setBCType(bc.ravel())
    nodes = dg.QuadNodesProvisioner(N, mesh)
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

    solver = Sw2dQuadSolver(nodes=nodes, g=g, fields=4)
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tide=(0.5, 3600.0, 0.15 / 3600), sponge=sponge, tracer=0.0)
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
        t = solver.getTime()
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
    print(f"done: {step} steps to t={t:.2f} on {ctx.numElements} quadrilaterals at N={N} in {wall:.2f} s; {len(table)} records in {csv}")


if __name__ == "__main__":
    main()
