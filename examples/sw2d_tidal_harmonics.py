#!/usr/bin/env python3
"""Co-tidal charts, residual currents and envelopes of a tidal run, accumulated on the device: the tidal variant-B set-up of
examples/sw2d_gauges.py with the field statistics switched on.

    python examples/sw2d_tidal_harmonics.py [periods] [order] [cells] [directory]

A 10 km square basin of cells x cells x 2 triangles, open towards the tide on the side x = 0 and walled elsewhere, a sloping
bed with a shoal, drag, Coriolis and a sponge in front of the open side, driven over `periods` (default 2) periods of its
tide. After every step the solver adds eta, u, v at every node to the sums, the envelopes and the harmonic sums of the tide's
period and of half of it (its first overtide, M4 beside M2) on the device (enableFieldStats): the loop never downloads the
state. At the end the accumulators are read once, harmonicFit solves the normal equations of the fit on the host, and the
amplitude and phase of both constituents of eta, the residual currents and the envelopes go to `directory` (default .) as
*.vtu files.
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


def main():
    periods = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    directory = sys.argv[4] if len(sys.argv) > 4 else "."
    g, CD, f, CFL, L = 9.81, 2.5e-3, 1.0e-4, 0.5, 1.0e4
    tidePeriod = 3600.0
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
    solver.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, tideAmplitude=0.5, tidePeriod=tidePeriod, tideRamp=0.15 / 3600,
                          sponge=sponge)
    solver.setState(H.copy(), np.zeros_like(H), np.zeros_like(H))
    solver.enableFieldStats(periods=(tidePeriod, tidePeriod / 2))   # eta = h - H with the bed of variant B
    finalTime = periods * tidePeriod
    t, step = 0.0, 0
    t0 = time.perf_counter()
    while t < finalTime:
        dt, _ = solver.computeDt(CFL)
        solver.stepSSPRK2(dt)
        t = solver.time
        step += 1
        if step % 500 == 0:
            print(f"t={t:.1f} step={step} dt={dt:.4f}", flush=True)
    wall = time.perf_counter() - t0
    stats = solver.fieldStats()                                     # the only download: the accumulator planes, once
    fit = solver.harmonicFit(stats)
    fields = {"M2_amplitude": fit["amplitude"][0, 0], "M2_phase": fit["phase"][0, 0],
              "M4_amplitude": fit["amplitude"][1, 0], "M4_phase": fit["phase"][1, 0],
              "residual_u": fit["mean"][1], "residual_v": fit["mean"][2],
              "eta_max": stats["etaMax"], "h_min": stats["hMin"], "speed_max": stats["speedMax"]}
    os.makedirs(directory, exist_ok=True)
    os.chdir(directory)                                             # the writer names its files after the fields
    dg.VtkOutputter(nodes).writeFieldsToFiles(fields, 0)
    a2 = fields["M2_amplitude"]
    print(f"done: {step} steps to t={t:.1f} on {ctx.numElements} triangles at N={N} in {wall:.2f} s; {stats['n']} samples, "
          f"cond {fit['cond']:.3g}; M2 amplitude {a2.min():.4f} .. {a2.max():.4f} m, M4 up to {fields['M4_amplitude'].max():.4f} m, "
          f"residual speed up to {np.hypot(fields['residual_u'], fields['residual_v']).max():.4f} m/s, "
          f"highest water {fields['eta_max'].max():.4f} m; {len(fields)} *.vtu files in {directory}")


if __name__ == "__main__":
    main()
