#!/usr/bin/env python3
"""Gauges, conservation integrals, residual currents and drifter tracks of the curved-channel run, all recorded on the device:
the set-up of examples/sw2d_curved.py (a geostrophic jet in an 8 km channel whose top wall carries a headland) with the script's
adaptive loop (examples/sw2d_curved_adaptive.py) and the run records switched on.

    python examples/sw2d_curved_records.py [box:NXxNY] [order] [final time, s] [output directory]

Two gauges sit up- and downstream of the headland, a line of 32 drifters upstream of it. The channel ends (ctx.BCmap[2]) are
open faces for the drifters: one that reaches an end has left (status 1); along the walls, the curved headland included, they
slide. After every 10th step the solver stores the integrals of h, hu, hv, hN and of the energy, the extrema and eta, u, v, N
at the gauges (enableMonitor, with the weights of the curved scheme: quadratureWeights) and the drifters' positions
(enableDrifters); after every step it adds eta, u, v to the sums and envelopes at every node (enableFieldStats). The loop never
downloads the state: the records are read between the chunks of runAdaptive and at the end go to `directory` (default .) as
gauges.csv, tracks.csv and *.vtu files of the residual currents and the envelopes.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from sw2d_curved import setup  # noqa: E402


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    mesh_arg = argv[0] if len(argv) > 0 else "box:32x8"
    NOrder = int(argv[1]) if len(argv) > 1 else 4
    finalTime = float(argv[2]) if len(argv) > 2 else 600.0
    directory = argv[3] if len(argv) > 3 else "."
    solver, ctx, cub, q, H, _, _, ncurved = setup(mesh_arg, NOrder)
    nodes = ctx._nodes                                 # the provisioner the context views: its coordinates are the deformed ones
    CFL, stride, chunk = 0.75, 10, 500
    solver.enableDriver(ctx, H=H)
    solver.setState(*q)

    gauges = np.array([[3000.0, 700.0], [5000.0, 700.0]])
    solver.enableMonitor(nodes, gauges=gauges, stride=stride, capacity=chunk // stride + 1)
    solver.enableFieldStats(stride=1)                  # eta = h - H with the driver's H; mean and envelopes
    line = np.stack([np.full(32, 2500.0), np.linspace(60.0, 940.0, 32)], axis=1)
    solver.enableDrifters(nodes, line, mapO=ctx.BCmap[2], stride=stride, capacity=chunk // stride + 1)
    solver.sampleMonitor()                             # the initial state

    dt, _ = solver.computeDt(CFL)
    print(f"K={ctx.numElements} Np={ctx.numLocalPoints} curved elements={ncurved} dt={dt:.6g}")
    t, step, records, tracks = 0.0, 0, [], []
    while t < finalTime:
        t, dt, done = solver.runAdaptive(CFL, finalTime, t=t, dt=dt, maxSteps=chunk - 1, filter=True)
        step += done
        records.append(solver.monitorRecordArray())    # read, then reset: the device holds one chunk's records
        solver.resetMonitor()
        tracks.append(solver.drifterTracks())
        solver.resetDrifterTracks()
        mass = records[-1][:, 1]
        print(f"t={t:.6g} step={step} dt={dt:.6g} mass drift={(mass[-1] - records[0][0, 1]) / records[0][0, 1]:.3e}")

    os.makedirs(directory, exist_ok=True)
    rec = np.concatenate(records)
    header = "t,mass,hu,hv,hN,energy,hmin,hmax,humax,hvmax,nan," + ",".join(f"{f}{g}" for g in range(len(gauges)) for f in ("eta", "u", "v", "N"))
    np.savetxt(os.path.join(directory, "gauges.csv"), rec, delimiter=",", header=header, comments="")
    with open(os.path.join(directory, "tracks.csv"), "w") as f:
        f.write("t,drifter,x,y,status\n")
        for tt, xy, st in tracks:
            for i in range(len(tt)):
                for d in range(xy.shape[1]):
                    f.write(f"{tt[i]:.9g},{d},{xy[i, d, 0]:.9g},{xy[i, d, 1]:.9g},{st[i, d]}\n")
    stats = solver.fieldStats()                        # the accumulator planes, once
    n = max(stats["n"], 1)
    fields = {"residual_u": stats["sum"][1] / n, "residual_v": stats["sum"][2] / n, "mean_eta": stats["sum"][0] / n,
              "eta_max": stats["etaMax"], "h_min": stats["hMin"], "speed_max": stats["speedMax"]}
    here = os.getcwd()
    os.chdir(directory)                                # the writer names its files after the fields
    dg.VtkOutputter(nodes).writeFieldsToFiles(fields, 0)
    os.chdir(here)
    state = solver.drifterState()
    print(f"done: steps={step} t={t:.6g}; {len(rec)} monitor records, {sum(len(tr[0]) for tr in tracks)} track records; "
          f"drifters moving {int(((state['status'] & 3) == 0).sum())}, left {int(((state['status'] & 1) != 0).sum())}, "
          f"lost {int(((state['status'] & 2) != 0).sum())}, touched a wall {int(((state['status'] & 4) != 0).sum())}; "
          f"residual speed up to {np.hypot(fields['residual_u'], fields['residual_v']).max():.4f} m/s")
    return step, t


if __name__ == "__main__":
    main()
