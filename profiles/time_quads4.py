#!/usr/bin/env python3
"""Times the three-field and the four-field quadrilateral stage kernels side by side on an n x n box of quadrangles:
    python3 profiles/time_quads4.py [n] [orders] [stages] [label] [rounds]
defaults: n = 775 (600 625 elements, the mesh of time_quads.py), orders 4,8, 50 stages, label "this", 2 rounds. One JSON line
per (round, order, geometry form, kind): kind "fields3" (LSERK4 stage and RK2 + filter step of the three-field solver: what
a build of the parent commit also runs, selected with BDG_HIP_LIBRARY and labelled with `label`), "fields4" (four fields, no
sources) and "fields4_sources" (Coriolis array, drag, bed slope); the kinds a library lacks are skipped. Compulsory bytes of a
parallelogram-form LSERK4 stage per element: state in, residual in and out, state out = 4 fields Np doubles, plus 2 Np (3 Np
with an f array) for the sources, plus the gather index (4 bytes per face node) and 16 geometry values. Each line also
carries the node count and the picoseconds per node of both timings, the figure that compares orders (9 to 12 beside 8:
profiles/quads_high_order.jsonl)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2dquads  # noqa: E402


def stage_bytes(N, K, general, fields, src_planes):
    Np, nfn = (N + 1) ** 2, 4 * (N + 1)
    geo = (4 * Np + 3 * nfn) * 8 if general else 16 * 8
    return K * ((4 * fields + src_planes) * Np * 8 + nfn * 4 + geo)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 775
    orders = [int(o) for o in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 8]
    stages = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    label = sys.argv[4] if len(sys.argv) > 4 else "this"
    rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 2
    has4 = hasattr(sw2dquads.Sw2dQuadSolver, "computeRHS4")
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    E = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    K = mesh.numElements
    for N in orders:
        nodes = dg.QuadNodesProvisioner(N, mesh)
        nodes.buildFilter(0.99 * N, 4)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
        z = np.zeros_like(h)
        dt = 0.1 * (2.0 / n) / (N * N * 10.0)
        src = {"zx": -0.05 + 0 * x, "zy": 0.05 * y, "f": 0.1 * (1 + 0.5 * y), "CD": 2.5e-2}
        kinds = [("fields3", 3, None, 0)] + ([("fields4", 4, None, 0), ("fields4_sources", 4, src, 3)] if has4 else [])
        for rnd in range(rounds):
            for general in (False, True):
                for kind, fields, sources, planes in kinds:
                    kw = {"fields": fields, "sources": sources} if has4 else {}
                    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, **kw)
                    s.setState4(h, z, z, 0.5 * h) if fields == 4 else s.setState(h, z, z)
                    s.timeStages(dt, 10)  # warm-up
                    ms_stage = s.timeStages(dt, stages)
                    ms_rk2 = s.timeStages(dt, max(stages // 5, 2), rk2=True)
                    b = stage_bytes(N, K, general, fields, planes)
                    nodes_total = K * (N + 1) ** 2
                    print(json.dumps({"build": label, "round": rnd, "kind": kind, "order": N, "K": K, "nodes": nodes_total,
                                      "geometry": "general" if general else "parallelogram",
                                      "ms_per_lserk4_stage": round(ms_stage, 4), "ms_per_rk2_filter_step": round(ms_rk2, 4),
                                      "ps_per_node_lserk4_stage": round(ms_stage * 1e9 / nodes_total, 2),
                                      "ps_per_node_rk2_filter_step": round(ms_rk2 * 1e9 / nodes_total, 2),
                                      "stage_bytes": b, "stage_TBps": round(b / ms_stage / 1e9, 3)}), flush=True)
                    s.close()


if __name__ == "__main__":
    main()
