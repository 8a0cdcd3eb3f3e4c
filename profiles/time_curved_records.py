#!/usr/bin/env python3
"""Times the run records of the curved sw2d solver (bdg_sw2d_curved_monitor_*, _field_stats_*, _drifters_*) beside its step, in
one process on one GPU:
    python3 profiles/time_curved_records.py [out.json] [drifters] [count]
at the two README configurations of the curved solver (profiles/time_curved.py's deformed box: 250 000 triangles at N = 4 and
60 000 at N = 8, 5 % of the elements curved, a curved bottom wall), 10^5 drifters, 50 timed launches after warm-up. One entry
per configuration in profiles/curved_records.json, HIP-event milliseconds:
  ms_rk2_step                     an RK2 + filter step, two RHS evaluations (bdg_sw2d_curved_time_rk2), nothing enabled
  ms_monitor_sample               both launches of a monitor sample with 8 gauges
  ms_field_stats_sample           one sample with the mean, the envelopes and two periods
  ms_drifter_advance              one advance, every drifter in a straight-sided element
  ms_drifter_advance_curved       one advance, every drifter in a curved element (12 Newton iterations at most per hop)
  ms_drifter_advance_straight     the advance of Sw2dSolver (sw2d_drifter_kernel.hpp) on the undeformed mesh of the same size and
                                  order with the same reference coordinates: the cost of the curved path is the difference
The advances use the step's own dt, at which a drifter stays in its element."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d  # noqa: E402
from blitzdg_amd.sw2d_curved import Sw2dCurvedSolver  # noqa: E402

G = 9.81


def reference_points(rng, n):
    a, b = rng.uniform(0.02, 0.96, n), rng.uniform(0.02, 0.96, n)
    flip = a + b > 0.98
    a[flip], b[flip] = 0.98 - a[flip], 0.98 - b[flip]
    return 2 * a - 1, 2 * b - 1


def measure(order, nx, ny, drifters, count):
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, order)
    ctx = nodes.dgContext()
    x0, y0 = ctx.x.copy(), ctx.y.copy()
    b = np.clip(1.0 - (y0 + 1.0) / 0.1, 0.0, 1.0) ** 3
    x, y = x0, y0 + 0.02 * b * np.sin(3 * x0)
    curvedEls = np.where(np.abs(y - y0).max(axis=0) > 0)[0].astype(np.int32)
    # the straight solver first, on the undeformed coordinates
    K = int(ctx.numElements)
    rng = np.random.default_rng(drifters)
    straightEls = np.setdiff1d(np.arange(K), curvedEls)
    r, s = reference_points(rng, drifters)
    el = {"straight": rng.choice(straightEls, drifters).astype(np.int32), "curved": rng.choice(curvedEls, drifters).astype(np.int32)}
    h0 = 1.0 + 0.1 * np.exp(-10 * x0 * x0 - 10 * y0 * y0)
    q3 = (h0, 0.01 * np.sin(3 * x0) * h0, 0.01 * np.cos(2 * y0) * h0)
    dt = 0.1 * (2.0 / max(nx, ny)) / ((order + 1) ** 2 * np.sqrt(G * 1.1))
    plain = sw2d.Sw2dSolver(nodes=nodes, g=G)
    plain.setState(*q3)
    plain.enableDrifters(nodes, (el["straight"], r, s), capacity=1)
    plain.timeDrifters(dt, 5)
    ms_straight = min(plain.timeDrifters(dt, count) for _ in range(3))
    plain.close()

    nodes.setCoordinates(x, y)
    J = (ctx.Dr @ x) * (ctx.Ds @ y) - (ctx.Ds @ x) * (ctx.Dr @ y)
    gauss = nodes.buildGaussFaceNodes(2 * (order + 1))
    cub = nodes.buildCubatureVolumeMesh(3 * (order + 1))
    h = 1.0 + 0.1 * np.exp(-10 * x * x - 10 * y * y)
    z = np.zeros_like(h)
    q0 = (h, 0.01 * np.sin(3 * x) * h, 0.01 * np.cos(2 * y) * h, 0.5 * h)
    out = {"order": order, "elements": K, "curved_elements": int(curvedEls.size), "drifters": drifters, "launches": count,
           "ms_drifter_advance_straight": ms_straight}
    for where in ("straight", "curved"):
        sv = Sw2dCurvedSolver(ctx, cub, gauss, curvedEls, J, gauss.mapM, gauss.mapP, g=G, zx=z, zy=z, f=1e-4, CD=2.5e-3 + z)
        sv.enableDriver(ctx, H=np.ones_like(h))
        sv.setState(*q0)
        if where == "straight":                              # the step with nothing enabled, then the monitor and the statistics
            sv.stepRK2(dt, 5, True)
            out["ms_rk2_step"] = 2.0 * min(sv.timeRK2(dt, 20, True) for _ in range(3))
            gel = rng.choice(K, 8).astype(np.int32)
            gr, gs = reference_points(rng, 8)
            sv.enableMonitor(nodes, gauges=(gel, gr, gs), capacity=4)
            sv.timeMonitor(5)
            out["ms_monitor_sample"] = min(sv.timeMonitor(count) for _ in range(3))
            sv.enableFieldStats(periods=(44712.0, 22356.0))
            sv.timeFieldStats(5)
            out["ms_field_stats_sample"] = min(sv.timeFieldStats(count) for _ in range(3))
        sv.enableDrifters(nodes, (el[where], r, s), capacity=1)
        sv.timeDrifters(dt, 5)
        ms = min(sv.timeDrifters(dt, count) for _ in range(3))
        st = sv.drifterState()["status"]
        assert (st == 0).all(), np.unique(st)
        out["ms_drifter_advance" + ("_curved" if where == "curved" else "")] = ms
        sv.close()
    for key in ("ms_monitor_sample", "ms_field_stats_sample", "ms_drifter_advance", "ms_drifter_advance_curved"):
        out[key.replace("ms_", "") + "_over_step"] = out[key] / out["ms_rk2_step"]
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "curved_records.json")
    drifters = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10 ** 5
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    cases = [tuple(int(v) for v in c.split(":")) for c in os.environ.get("BDG_CURVED_RECORDS_CASES", "4:500:250,8:200:150").split(",")]
    results = []
    for order, nx, ny in cases:
        results.append(measure(order, nx, ny, drifters, count))
        print(json.dumps(results[-1]), flush=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
