#!/usr/bin/env python3
"""Times variant B of the quadrilateral sw2d solver beside variant A of the same build, in one process, on an n x n box:
    python3 profiles/time_quadsB.py [n] [orders] [stages] [out.jsonl]
defaults: n = 775 (600 625 elements), orders 4,8,12, 30 stages, profiles/quadsB_time.jsonl. For every order and both geometry
forms one JSON line: HIP-event ms per LSERK4 stage of variant A (three fields), per LSERK4 stage and per Heun step of variant
B (each evaluation = speed pass + stage launch), and of the speed pass alone. The x = -1 side is open, the bed slopes and
jumps from element to element, drag and Coriolis are on. A first, then B, then A and B again (the second pair is reported
as *_again). Under `rocprofv3 --kernel-trace --stats` the same command gives the per-kernel split."""
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
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "quadsB_time.jsonl")
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
            mapO = ctx.BCmap.get(2, [])
            assert len(mapO) == n * (N + 1) and np.allclose(x.ravel("F")[ctx.vmapM[mapO]], -1.0)
            H = 10.0 * (1 + 0.05 * x - 0.03 * y * y) + 0.2 * rng.uniform(-1, 1, (1, K))
            Hx, Hy = 0.5 + 0 * x, -0.6 * y
            h = H + 0.3 * np.exp(-10 * x * x - 10 * y * y)
            z = np.zeros_like(h)
            dt = 0.1 * (2.0 / n) / (N * N * 10.0)
            for general in (False, True):
                flags = sw2dquads.GENERAL_GEOMETRY if general else 0
                sa = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=flags)
                sb = sw2dquads.Sw2dQuadSolver(nodes=nodes, flags=flags)
                sb.enableVariantB(H, Hx, Hy, mapO=mapO, CD=2.5e-3, f=1e-4, tide=(0.5, 40.0, 0.05))
                for s in (sa, sb):
                    s.setState(h, z, z)
                    s.timeStages(dt, 5)  # warm-up
                r = {"order": N, "K": K, "geometry": "general" if general else "parallelogram"}
                for tag in ("", "_again"):
                    r["ms_A_lserk4_stage" + tag] = round(sa.timeStages(dt, stages), 4)
                    r["ms_B_lserk4_stage" + tag] = round(sb.timeStages(dt, stages), 4)
                    r["ms_B_heun_step" + tag] = round(sb.timeHeun(dt, max(stages // 2, 2)), 4)
                    r["ms_B_speed_pass" + tag] = round(sb.timeSpeedPass(stages), 4)
                line = json.dumps(r)
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()
                sa.close()
                sb.close()


if __name__ == "__main__":
    main()
