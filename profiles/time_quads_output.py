#!/usr/bin/env python3
"""Times the output step of the quadrilateral solver (bdg_sw2dq_output_fields: sw2d_quad_output_kernel) on an n x n box:
    python3 profiles/time_quads_output.py [n] [orders] [launches] [repeats]
defaults: n = 775 (600 625 elements), orders 4,8, 50 launches per timing, 5 timings. For every order, with the lattice
interpolation on and off, one JSON line: HIP-event ms of the launch for eta, u, v with a bathymetry H (median, minimum and
maximum over the repeats), its compulsory bytes ((3 + 1 + 1) planes in, 3 planes out), the resulting GB/s, one LSERK4 stage
of the same box timed in the same process and the ratio to it; and what the call costs a user end to end (launch, three
row downloads) beside the route without the kernel: getState() and NumPy on the host (perf_counter)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2dquads  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 775
    orders = [int(o) for o in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 8]
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    mesh = dg.MeshManager()
    mesh.buildMesh(np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1), V)
    K = mesh.numElements
    for N in orders:
        nodes = dg.QuadNodesProvisioner(N, mesh)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        H = 10.0 + 0.1 * x
        h = H + np.exp(-10 * x * x - 10 * y * y)
        s = sw2dquads.Sw2dQuadSolver(nodes=nodes)
        s.setState(h, 0.1 * np.sin(x), 0.1 * np.cos(y))
        dt = 0.1 * (2.0 / n) / (N * N * 10.0)
        s.timeStages(dt, 10)  # warm-up
        stage = sorted(s.timeStages(dt, launches) for _ in range(repeats))
        IM, I1, _ = nodes.splitOperators()
        plane = (N + 1) ** 2 * K * 8
        for lattice in (True, False):
            s.timeOutput(5, H=H, lattice=lattice)  # warm-up
            ms = sorted(s.timeOutput(launches, H=H, lattice=lattice) for _ in range(repeats))
            med = ms[len(ms) // 2]
            t0 = time.perf_counter()
            dev = s.outputFields(H=H, lattice=lattice)
            call = time.perf_counter() - t0
            t0 = time.perf_counter()
            q = s.getState()
            host = [q[0] - H, q[1] / q[0], q[2] / q[0]]
            if lattice:
                host = [IM @ f for f in host]
            route = time.perf_counter() - t0
            print(json.dumps({"order": N, "K": K, "lattice": lattice, "launch_ms_median": round(med, 4),
                              "launch_ms_min": round(ms[0], 4), "launch_ms_max": round(ms[-1], 4),
                              "compulsory_bytes": 8 * plane, "GBps": round(8 * plane / med / 1e6, 1),
                              "lserk4_stage_ms_median": round(stage[len(stage) // 2], 4),
                              "lserk4_stage_ms_min": round(stage[0], 4), "lserk4_stage_ms_max": round(stage[-1], 4),
                              "ratio_to_stage": round(med / stage[len(stage) // 2], 3),
                              "outputFields_call_s": round(call, 4), "getState_numpy_route_s": round(route, 4),
                              "max_dev_vs_host": float(max(np.abs(a - b).max() for a, b in zip(dev, host)))}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
