#!/usr/bin/env python3
"""Times the drifter advance of the quadrilateral sw2d solver (bdg_sw2dq_drifters_*) on an n x n box of quadrangles:
    python3 profiles/time_quad_drifters.py [n] [orders] [counts] [advances]
defaults: n = 775 (600 625 elements), orders 4,8, 10^4, 10^5 and 10^6 drifters spread uniformly, 50 advances after 5 of warm-up.
For every order and count it prints one JSON line (and appends it to profiles/quad_drifters_time.jsonl): HIP-event ms per
advance in a solid-body rotation, with the step's own dt (a drifter stays in its element) and with a dt that carries the
fastest drifter across about one element per advance, beside the ms per RK2 + filter step of the same process."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2dquads  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 775
    orders = [int(o) for o in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 8]
    counts = [int(float(c)) for c in sys.argv[3].split(",")] if len(sys.argv) > 3 else [10 ** 4, 10 ** 5, 10 ** 6]
    advances = int(sys.argv[4]) if len(sys.argv) > 4 else 50
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    E = np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    K = mesh.numElements
    out = open(os.path.join(ROOT, "profiles", "quad_drifters_time.jsonl"), "a")
    for N in orders:
        nodes = dg.QuadNodesProvisioner(N, mesh)
        nodes.buildFilter(0.99 * N, 4)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
        omega = 0.5                                          # |u| <= 0.5 sqrt(2) inside the box
        dt = 0.1 * (2.0 / n) / (N * N * 10.0)
        dt_cross = (2.0 / n) / (omega * np.sqrt(2.0))
        for count in counts:
            rng = np.random.default_rng(count)
            # inside the disc of radius 0.6: the rotation keeps them clear of the walls
            rad, ang = 0.6 * np.sqrt(rng.uniform(0, 1, count)), rng.uniform(0, 2 * np.pi, count)
            ix = np.minimum(((rad * np.cos(ang) + 1) / 2 * n).astype(np.int64), n - 1)
            iy = np.minimum(((rad * np.sin(ang) + 1) / 2 * n).astype(np.int64), n - 1)
            el = (iy * n + ix).astype(np.int32)
            r, sref = rng.uniform(-1, 1, count), rng.uniform(-1, 1, count)
            s = sw2dquads.Sw2dQuadSolver(nodes=nodes)
            s.setState(h, -h * omega * y, h * omega * x)
            s.enableDrifters(nodes, (el, r, sref), capacity=1)
            s.timeDrifters(dt, 5)                            # warm-up
            ms_small = s.timeDrifters(dt, advances)
            s.timeDrifters(dt_cross, 5)
            ms_cross = s.timeDrifters(dt_cross, advances)
            st = s.drifterState()["status"]
            s.timeStages(dt, 2, rk2=True)
            ms_rk2 = s.timeStages(dt, 10, rk2=True)
            line = json.dumps({"order": N, "K": K, "drifters": count, "advances": advances,
                               "ms_per_advance": round(ms_small, 4), "ms_per_advance_crossing": round(ms_cross, 4),
                               "ms_per_rk2_filter_step": round(ms_rk2, 4), "advance_over_step": round(ms_small / ms_rk2, 4),
                               "crossing_over_step": round(ms_cross / ms_rk2, 4), "moving": int((st == 0).sum())})
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            s.close()


if __name__ == "__main__":
    main()
