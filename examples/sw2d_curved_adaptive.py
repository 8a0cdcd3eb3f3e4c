#!/usr/bin/env python3
"""The reference's sw2d_curved.py driver with the script's actual time loop (sw2d_curved.py:231-302) on the MI355X path: the
set-up of examples/sw2d_curved.py, then -- all on the device, the state never downloaded --

    CFL 0.75; after every RK2 + filter step the time step is recomputed from the face-node speeds (:281) and the blow-up check
    runs (:284-286); every 50 steps and at the end the six fields eta, u, v, B, h, vort are written as *.vtu (:290-302).

    python examples/sw2d_curved_adaptive.py [box:NXxNY] [order] [final time, s] [output directory]
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
    nodes = ctx._nodes                                 # the provisioner the context views: its metrics are the deformed ones
    outputter = dg.VtkOutputter(nodes)
    os.makedirs(directory, exist_ok=True)

    CFL, outputInterval = 0.75, 50                     # sw2d_curved.py:231-240
    solver.enableDriver(ctx, H=H)                      # c = sqrt(g mean(H)), the script's
    solver.setState(*q)
    outputter.writeSolverFields(solver, 0, directory=directory)
    dt, h_max = solver.computeDt(CFL)
    print(f"K={ctx.numElements} Np={ctx.numLocalPoints} curved elements={ncurved} dt={dt:.6g} h_max={h_max:.6g}")
    numSteps = int(np.ceil(finalTime / dt))

    t, step = 0.0, 0
    while t < finalTime:
        t, dt, done = solver.runAdaptive(CFL, finalTime, t=t, dt=dt, maxSteps=outputInterval, filter=True)
        step += done
        _, h_max = solver.computeDt(CFL)
        print(f"Outputting at t={t:.6g} step={step} dt={dt:.6g} h_max={h_max:.6g}")
        outputter.writeSolverFields(solver, step, directory=directory)
    print(f"done: steps={step} (a fixed first dt would take {numSteps}) t={t:.6g}")
    return step, t


if __name__ == "__main__":
    main()
