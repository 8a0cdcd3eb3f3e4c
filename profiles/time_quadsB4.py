#!/usr/bin/env python3
"""Times variant B with the passive tracer (four fields) beside three-field variant B and four-field variant A (tracer and
sources) of the same build, the solvers interleaved in one process, on an n x n box (the protocol of profiles/time_quadsB.py):
    python3 profiles/time_quadsB4.py [n] [orders] [stages] [out.jsonl]
defaults: n = 775 (600 625 elements), orders 4,8,12, 30 stages, profiles/quadsB4_time.jsonl. For every order and both geometry
forms one JSON line: HIP-event ms per LSERK4 stage and per Heun step of three-field B and of four-field B (each evaluation =
speed pass + stage launch), and per LSERK4 stage of four-field A with sources (variant A has no Heun step). The x = -1 side is
open and feeds a concentration that varies along it, the bed slopes and jumps from element to element, drag and Coriolis are
on. Every solver is timed twice, in turn (the second round is reported as *_again)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2dquads  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 775
    orders = [int(o) for o in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 8, 12]
    stages = int(sys.argv[3]) if len(sys.argv) > 3 else 30
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "quadsB4_time.jsonl")
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    E = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    K = mesh.numElements
    bc = np.array(mesh.bcType).reshape(K, 4)
    bc[np.arange(n) * n, 3] = 2          # face 3 (local vertices 3 and 0) of the first column of elements: the x = -1 side
    mesh.setBCType(bc.ravel())
    rng = np.random.default_rng(0)
    with open(out, "a") as log:
        for N in orders:
            nodes = dg.QuadNodesProvisioner(N, mesh)
            nodes.buildFilter(0.99 * N, 4)
            ctx = nodes.dgContext()
            x, y = ctx.x, ctx.y
            mapO = np.asarray(ctx.BCmap.get(2, []))
            assert len(mapO) == n * (N + 1) and np.allclose(x.ravel("F")[ctx.vmapM[mapO]], -1.0)
            H = 10.0 * (1 + 0.05 * x - 0.03 * y * y) + 0.2 * rng.uniform(-1, 1, (1, K))
            Hx, Hy = 0.5 + 0 * x, -0.6 * y
            h = H + 0.3 * np.exp(-10 * x * x - 10 * y * y)
            z = np.zeros_like(h)
            hN = 0.3 * h
            tracer = 0.5 + 0.4 * np.sin(3 * y.ravel("F")[ctx.vmapM[mapO]])
            dt = 0.1 * (2.0 / n) / (N * N * 10.0)
            vb = dict(mapO=mapO, CD=2.5e-3, f=1e-4, tide=(0.5, 40.0, 0.05))
            for general in (False, True):
                flags = sw2dquads.GENERAL_GEOMETRY if general else 0
                b3 = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=flags)
                b3.enableVariantB(H, Hx, Hy, **vb)
                b4 = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=flags, fields=4)
                b4.enableVariantB(H, Hx, Hy, tracer=tracer, **vb)
                a4 = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=flags, fields=4, sources=dict(zx=-Hx, zy=-Hy, f=1e-4, CD=2.5e-3))
                b3.setState(h, z, z)
                b4.setState4(h, z, z, hN)
                a4.setState4(h, z, z, hN)
                for s in (b3, b4, a4):
                    s.timeStages(dt, 5)  # warm-up
                r = {"order": N, "K": K, "geometry": "general" if general else "parallelogram"}
                for tag in ("", "_again"):
                    r["ms_B3_lserk4_stage" + tag] = round(b3.timeStages(dt, stages), 4)
                    r["ms_B4_lserk4_stage" + tag] = round(b4.timeStages(dt, stages), 4)
                    r["ms_A4_lserk4_stage" + tag] = round(a4.timeStages(dt, stages), 4)
                    r["ms_B3_heun_step" + tag] = round(b3.timeHeun(dt, max(stages // 2, 2)), 4)
                    r["ms_B4_heun_step" + tag] = round(b4.timeHeun(dt, max(stages // 2, 2)), 4)
                line = json.dumps(r)
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
                for s in (b3, b4, a4):
                    s.close()


if __name__ == "__main__":
    main()
