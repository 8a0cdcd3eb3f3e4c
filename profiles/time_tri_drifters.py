#!/usr/bin/env python3
"""Times the drifter advance of the triangle sw2d solver (bdg_sw2d_drifters_*) on an n x n box of 2 n^2 triangles:
    python3 profiles/time_tri_drifters.py [cases] [counts] [advances]
defaults: cases 4:707,8:354 (order:n -- 999 698 triangles at N = 4, 250 632 at N = 8), 10^5 drifters spread uniformly over the
disc of radius 0.6, 50 advances after 5 of warm-up. For every case and count it prints one JSON line (and appends it to
profiles/tri_drifters_time.jsonl): HIP-event ms per advance in a solid-body rotation, with the step's own dt (a drifter stays
in its element) and with a dt that carries the fastest drifter across about one element per advance, beside the ms per LSERK4
stage (HIP events) and per RK2 + filter step (host clock around 20 steps) of the same process."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d  # noqa: E402


def main():
    cases = [tuple(int(v) for v in c.split(":")) for c in (sys.argv[1] if len(sys.argv) > 1 else "4:707,8:354").split(",")]
    counts = [int(float(c)) for c in sys.argv[2].split(",")] if len(sys.argv) > 2 else [10 ** 5]
    advances = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    out = open(os.path.join(ROOT, "profiles", "tri_drifters_time.jsonl"), "a")
    for N, n in cases:
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(n, n)
        nodes = dg.TriangleNodesProvisioner(N, mesh)
        nodes.buildFilter(0.9 * N, max(N, 2))
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        K = x.shape[1]
        h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
        omega = 0.5                                          # |u| <= 0.5 sqrt(2) inside the box
        dt = 0.1 * (2.0 / n) / (N * N * 10.0)
        dt_cross = (2.0 / n) / (omega * np.sqrt(2.0))
        inside = np.nonzero(np.hypot(x.mean(axis=0), y.mean(axis=0)) < 0.6)[0]   # the rotation keeps them clear of the walls
        # the stage and the step of a solver without drifters (with them a step is followed by an advance)
        plain = sw2d.Sw2dSolver(nodes=nodes)
        plain.setState(h, -h * omega * y, h * omega * x)
        plain.timeLSERK4Stages(dt, 5)
        ms_stage = plain.timeLSERK4Stages(dt, 20)
        plain.setState(h, -h * omega * y, h * omega * x)
        plain.stepRK2(dt, 3, filter=True)
        plain.synchronize()
        t0 = time.perf_counter()
        plain.stepRK2(dt, 20, filter=True)
        plain.synchronize()
        ms_rk2 = (time.perf_counter() - t0) * 1e3 / 20
        plain.close()
        for count in counts:
            rng = np.random.default_rng(count)
            el = rng.choice(inside, count).astype(np.int32)
            a, b = rng.uniform(0, 1, count), rng.uniform(0, 1, count)
            flip = a + b > 1
            a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
            s = sw2d.Sw2dSolver(nodes=nodes)
            s.setState(h, -h * omega * y, h * omega * x)
            s.enableDrifters(nodes, (el, 2 * a - 1, 2 * b - 1), capacity=1)
            s.timeDrifters(dt, 5)                            # warm-up
            ms_small = s.timeDrifters(dt, advances)
            s.timeDrifters(dt_cross, 5)
            ms_cross = s.timeDrifters(dt_cross, advances)
            st = s.drifterState()["status"]
            line = json.dumps({"order": N, "K": K, "drifters": count, "advances": advances, "renumbered": bool(s.isRenumbered),
                               "ms_per_advance": round(ms_small, 4), "ms_per_advance_crossing": round(ms_cross, 4),
                               "ms_per_lserk4_stage": round(ms_stage, 4), "ms_per_rk2_filter_step": round(ms_rk2, 4),
                               "advance_over_step": round(ms_small / ms_rk2, 4),
                               "crossing_over_step": round(ms_cross / ms_rk2, 4), "moving": int((st == 0).sum())})
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            s.close()


if __name__ == "__main__":
    main()
