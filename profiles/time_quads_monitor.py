#!/usr/bin/env python3
"""Times one sample of the quadrilateral solver's run monitor beside the LSERK4 stage and the output launch of the same process:
    python3 profiles/time_quads_monitor.py [n] [orders] [count] [rounds]
defaults: n = 775 (600 625 elements, the mesh of time_quads4.py), orders 4,8, 50 samples, 2 rounds. One JSON line per (round,
order, geometry form): ms per sample with 0 and with 16 gauges (both launches: the reduction and the finish kernel; wall
clock over `count` back-to-back sampleMonitor calls between two stream synchronisations, so it includes their launch cost),
HIP-event ms of the LSERK4 stage (timeStages) and of the nodal and the lattice outputFields launch (timeOutput), and the
bytes a sample has to read (fields + 1 planes with the weights, + 1 with H) with the bandwidth that makes."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2dquads  # noqa: E402


def time_samples(s, count):
    s.resetMonitor()
    s.sampleMonitor()  # warm-up
    s.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        s.sampleMonitor()
    s.synchronize()
    return (time.perf_counter() - t0) / count * 1e3


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 775
    orders = [int(o) for o in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 8]
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    E = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    K = mesh.numElements
    rng = np.random.default_rng(0)
    gauges = rng.uniform(-0.99, 0.99, (16, 2))
    for N in orders:
        nodes = dg.QuadNodesProvisioner(N, mesh)
        nodes.buildFilter(0.99 * N, 4)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
        H = 10.0 + 0.1 * x
        z = np.zeros_like(h)
        dt = 0.1 * (2.0 / n) / (N * N * 10.0)
        Np = (N + 1) ** 2
        for rnd in range(rounds):
            for general in (False, True):
                ms = {}
                for ng in (0, 16):
                    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
                    s.setState(h, z, z)
                    s.enableMonitor(nodes, H=H, gauges=gauges[:ng] if ng else None, stride=1, capacity=count + 1)
                    ms[ng] = time_samples(s, count)
                    if ng == 16:
                        s.timeStages(dt, 10)  # warm-up
                        stage = s.timeStages(dt, count)
                        out_nodal = s.timeOutput(count, H=H, lattice=False)
                        out_lattice = s.timeOutput(count, H=H, lattice=True)
                    s.close()
                nbytes = 5 * Np * K * 8  # h, hu, hv, weights, H
                print(json.dumps({"round": rnd, "order": N, "K": K, "general": general, "sample_ms_0_gauges": round(ms[0], 4),
                                  "sample_ms_16_gauges": round(ms[16], 4), "lserk4_stage_ms": round(stage, 4),
                                  "output_nodal_ms": round(out_nodal, 4), "output_lattice_ms": round(out_lattice, 4),
                                  "sample_bytes": nbytes, "sample_GBps": round(nbytes / ms[0] / 1e6, 1),
                                  "sample_over_stage": round(ms[0] / stage, 3)}), flush=True)


if __name__ == "__main__":
    main()
