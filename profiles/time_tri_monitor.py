#!/usr/bin/env python3
"""Times one sample of the triangle solver's run monitor beside the LSERK4 stage of the same process:
    python3 profiles/time_tri_monitor.py [count] [rounds]
on the benchmark mesh (1000 x 500 cells = 10^6 triangles, N = 4) and at N = 8 (500 x 250 cells = 250 000 triangles), 50
samples and 2 rounds by default. One JSON line per (round, order, variant): HIP-event ms per sample (both launches,
Sw2dSolver.timeMonitor) with H and 16 gauges and without H and gauges, HIP-event ms of the LSERK4 stage
(timeLSERK4Stages), the bytes a sample has to read (fields + 1 planes with the weights, + 1 with H) and the bandwidth that
makes."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d  # noqa: E402


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    gauges = np.random.default_rng(0).uniform(-0.99, 0.99, (16, 2))
    for N, (nx, ny) in ((4, (1000, 500)), (8, (500, 250))):
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(nx, ny)
        nodes = dg.TriangleNodesProvisioner(N, mesh)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        K, Np = ctx.numElements, ctx.numLocalPoints
        h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
        H = 10.0 + 0.1 * x
        z = np.zeros_like(h)
        dt = 0.1 * (2.0 / nx) / (N * N * 10.0)
        del ctx, x, y
        for rnd in range(rounds):
            for with_H, ng in ((True, 16), (False, 0)):
                s = sw2d.Sw2dSolver(nodes=nodes)
                s.setState(h, z, z)
                s.enableMonitor(nodes, H=H if with_H else None, gauges=gauges[:ng] if ng else None, stride=1, capacity=4)
                s.timeMonitor(10)                      # warm-up
                sample = s.timeMonitor(count)
                s.timeLSERK4Stages(dt, 10)            # warm-up
                stage = s.timeLSERK4Stages(dt, count)
                renumbered = s.isRenumbered
                s.close()
                nbytes = (5 if with_H else 4) * Np * K * 8   # h, hu, hv, weights (, H)
                print(json.dumps({"round": rnd, "order": N, "K": K, "with_H": with_H, "gauges": ng, "renumbered": renumbered,
                                  "sample_ms": round(sample, 4), "lserk4_stage_ms": round(stage, 4), "sample_bytes": nbytes,
                                  "sample_GBps": round(nbytes / sample / 1e6, 1), "sample_over_stage": round(sample / stage, 3)}),
                      flush=True)


if __name__ == "__main__":
    main()
