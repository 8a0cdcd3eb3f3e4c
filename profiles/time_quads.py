#!/usr/bin/env python3
"""Times the quadrilateral sw2d kernel (bdg_sw2dq_*) on an n x n box of quadrangles:
    python3 profiles/time_quads.py [n] [orders] [stages]
defaults: n = 775 (600 625 elements; 1.5e7 nodes at N = 4), orders 4,6,8, 50 stages. For every order and both geometry
forms it prints one JSON line: HIP-event ms per fused LSERK4 stage and per RK2 + filter step, the stage kernel's
compulsory bytes and the resulting TB/s, beside the measured STREAM triad of the device. Under
`rocprofv3 --kernel-trace --stats` the same command gives the per-kernel split."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d, sw2dquads  # noqa: E402


def stage_bytes(N, K, general):
    """Compulsory HBM bytes of one LSERK4 stage: q in, q out, residual in and out (3 fields each), the gather index,
    and the geometry (per node and face node, or 16 values per element)."""
    Np, nfn = (N + 1) ** 2, 4 * (N + 1)
    fields = 3 * Np * 8 * 4
    gather = nfn * 4
    geo = (4 * Np + 3 * nfn) * 8 if general else 16 * 8
    return K * (fields + gather + geo)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 775
    orders = [int(o) for o in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 6, 8]
    stages = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    E = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    K = mesh.numElements
    triad = sw2d.streamTriadGBps(0)
    for N in orders:
        nodes = dg.QuadNodesProvisioner(N, mesh)
        nodes.buildFilter(0.99 * N, 4)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
        z = np.zeros_like(h)
        dt = 0.1 * (2.0 / n) / (N * N * 10.0)
        for general in (False, True):
            s = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
            s.setState(h, z, z)
            s.timeStages(dt, 5)  # warm-up
            ms_stage = s.timeStages(dt, stages)
            ms_rk2 = s.timeStages(dt, max(stages // 5, 2), rk2=True)
            b = stage_bytes(N, K, general)
            print(json.dumps({"order": N, "K": K, "nodes": K * (N + 1) ** 2,
                              "geometry": "general" if general else "parallelogram",
                              "ms_per_lserk4_stage": round(ms_stage, 4), "ms_per_rk2_filter_step": round(ms_rk2, 4),
                              "stage_bytes": b, "stage_TBps": round(b / ms_stage / 1e9, 3),
                              "stream_triad_TBps": round(triad / 1e3, 3),
                              "fraction_of_triad": round(b / ms_stage / 1e6 / triad, 3)}), flush=True)
            s.close()


if __name__ == "__main__":
    main()
