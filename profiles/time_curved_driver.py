#!/usr/bin/env python3
"""Times the curved solver's driver kernels (sw2d_curved_driver_kernel.hpp) beside what they replace, in one process on one GPU:
    python3 profiles/time_curved_driver.py [out.jsonl]
at the two README configurations of the curved solver (profiles/time_curved.py's deformed box: 250 000 triangles at N = 4 and
60 000 at N = 8, 5 % of the elements curved). One JSON line per configuration, appended to profiles/curved_driver_timings.jsonl:
  ms_dt_pass                 the dt kernel and its finish kernel (HIP events; bdg_sw2d_curved_time_driver)
  ms_output_nodal, _lattice  one launch for the six fields, and the GB/s of its compulsory bytes (4 state planes + H + 4 metric
                             planes in, 6 planes out: 15 Np 8 bytes per element)
  ms_rk2_step                an RK2 + filter step, two RHS evaluations (bdg_sw2d_curved_time_rk2)
  ms_compute_dt_call         a computeDt() call by wall clock: the pass plus its 24-byte copy and the wait
  ms_adaptive_step           wall clock per step of runAdaptive over `steps` steps
  ms_host_dt                 the host alternative without the driver: getState() plus the NumPy dt expression, by wall clock
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.sw2d_curved import Sw2dCurvedSolver  # noqa: E402

G = 9.81


def numpy_dt(ctx, order, q, c, cfl):
    h, hu, hv = q[0], q[1], q[2]
    vmapM = np.asarray(ctx["vmapM"]).reshape(-1)
    u, v = hu / h, hv / h
    return cfl / np.max(((order + 1) ** 2) * 0.5 * np.abs(ctx["Fscale"].flatten("F")) *
                        (c + np.sqrt(u.flatten("F")[vmapM] ** 2 + v.flatten("F")[vmapM] ** 2)))


def measure(order, nx, ny, steps=20, count=50):
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, order)
    ctx = nodes.dgContext()
    x0, y0 = ctx.x, ctx.y
    b = np.clip(1.0 - (y0 + 1.0) / 0.1, 0.0, 1.0) ** 3
    x, y = x0, y0 + 0.02 * b * np.sin(3 * x0)
    curvedEls = np.where(np.abs(y - y0).max(axis=0) > 0)[0].astype(np.int32)
    nodes.setCoordinates(x, y)
    J = (ctx.Dr @ x) * (ctx.Ds @ y) - (ctx.Ds @ x) * (ctx.Dr @ y)
    gauss = nodes.buildGaussFaceNodes(2 * (order + 1))
    cub = nodes.buildCubatureVolumeMesh(3 * (order + 1))
    h = 1.0 + 0.1 * np.exp(-10 * x * x - 10 * y * y)
    z = np.zeros_like(h)
    s = Sw2dCurvedSolver(ctx, cub, gauss, curvedEls, J, gauss.mapM, gauss.mapP, g=G, zx=z, zy=z, f=1e-4, CD=2.5e-3 + z)
    H = np.ones_like(h)
    s.enableDriver(ctx, H=H)
    IM, _ = nodes.splitOperators()
    K, Np = ctx.numElements, ctx.numLocalPoints
    q0 = (h, 0.01 * np.sin(3 * x) * h, 0.01 * np.cos(2 * y) * h, 0.5 * h)
    s.setState(*q0)
    cfl = 0.25
    dt, _ = s.computeDt(cfl)
    s.stepRK2(dt, 5, True)
    s.synchronize()

    def wall(fn, n):
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        s.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    host = {"vmapM": ctx.vmapM, "Fscale": ctx.Fscale}
    c = float(np.sqrt(G * H.mean()))
    ms_dt = min(s.timeDriver("dt", count) for _ in range(3))
    ms_nodal = min(s.timeDriver("output", count) for _ in range(3))
    ms_lat = min(s.timeDriver("output", count, IM) for _ in range(3))
    ms_rk2 = 2.0 * min(s.timeRK2(dt, steps, True) for _ in range(3))
    ms_call = min(wall(lambda: s.computeDt(cfl), count) for _ in range(3))
    ms_host = min(wall(lambda: numpy_dt(host, order, s.getState(), c, cfl), 3) for _ in range(2))
    assert s.computeDt(cfl)[0] == numpy_dt(host, order, s.getState(), c, cfl)
    s.setState(*q0)
    s.synchronize()
    t0 = time.perf_counter()
    _, _, done = s.runAdaptive(cfl, np.inf, dt=dt, maxSteps=steps)
    ms_adaptive = (time.perf_counter() - t0) / done * 1e3
    assert np.isfinite(s.getState()[0]).all()
    out_bytes = 15 * Np * 8 * K
    return {"order": order, "elements": K, "Np": Np, "curved_elements": int(curvedEls.size),
            "ms_dt_pass": ms_dt, "ms_output_nodal": ms_nodal, "ms_output_lattice": ms_lat,
            "output_compulsory_bytes": out_bytes, "GBps_output_nodal": out_bytes / (ms_nodal * 1e-3) / 1e9,
            "GBps_output_lattice": out_bytes / (ms_lat * 1e-3) / 1e9,
            "ms_rk2_step": ms_rk2, "ms_compute_dt_call": ms_call, "ms_adaptive_step": ms_adaptive, "ms_host_dt": ms_host,
            "adaptive_steps": done}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "curved_driver_timings.jsonl")
    with open(path, "a") as f:
        for order, nx, ny in ((4, 500, 250), (8, 200, 150)):
            line = json.dumps(measure(order, nx, ny))
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
