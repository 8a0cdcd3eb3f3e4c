#!/usr/bin/env python3
"""Times one sample of the field statistics (bdg_sw2d_field_stats_time / bdg_sw2dq_field_stats_time):
    python3 profiles/time_field_stats.py [tri4] [tri8] [quad4]
defaults: all three -- 707 x 707 cells (999 698 triangles) at N = 4, 354 x 353 (249 924) at N = 8, 775 x 775 quadrilaterals
(600 625) at N = 4. For every mesh and each of four sets of groups (mean + envelope; with one period; with two periods; envelope
only) it prints one JSON line: HIP-event ms per sample over 50 samples after 10 of warm-up, the bytes moved by the formula of
sw2d_stats_kernel.hpp over that time in GB/s, and their ratio to the STREAM triad of the same process; on the first line of a
mesh also, from a solver of their own that has neither statistics nor a monitor while it steps, the ms per LSERK4 stage and per
RK2 + filter step (triangles: host clock around 50 steps) and, on triangles, per monitor sample (enabled after those) with its GB/s
by the same accounting (4 planes). The lines of the run quoted in DESIGN are in
profiles/field_stats_time.jsonl."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
import quadref  # noqa: E402
from blitzdg_amd import sw2d, sw2dquads  # noqa: E402

M2 = 3600 * 12.42
CONFIGS = [("mean+envelope", dict()), ("one period", dict(periods=(M2,))), ("two periods", dict(periods=(M2, M2 / 2))),
           ("envelope only", dict(mean=False))]


def planes(H, mean, envelope, m):
    return 3 + (1 if H else 0) + 2 * (3 * mean + 3 * envelope + 6 * m)


def run(label, make, Np, K, triad, extra):
    ld = (K + 63) // 64 * 64
    rows = []
    for name, kw in CONFIGS:
        s, q = make()
        s.setState(*q)
        s.enableFieldStats(**kw)
        s.timeFieldStats(10)
        ms = s.timeFieldStats(50)
        moved = planes(False, kw.get("mean", True), kw.get("envelope", True), len(kw.get("periods", ()))) * Np * ld * 8
        gbps = moved / (ms * 1e-3) / 1e9
        rows.append(dict(config=name, ms=ms, gbps=gbps, ratio=gbps / triad))
        s.close()
        if name == "mean+envelope":
            rows[-1].update(extra())  # the yardsticks, on a solver of their own: no statistics, no monitor in the timed steps
        print(json.dumps(dict(mesh=label, **rows[-1])), flush=True)
    return rows


def tri(nx, ny, order):
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, max(order, 2))
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
    q = [h, np.zeros_like(h), np.zeros_like(h)]
    Np, K = x.shape

    def make():
        return sw2d.Sw2dSolver(nodes=nodes, g=9.81), q

    def extra():
        s = sw2d.Sw2dSolver(nodes=nodes, g=9.81)
        s.setState(*q)
        dt = 0.3 * s.computeDt(0.65)[0]
        s.timeLSERK4Stages(dt, 20)
        stage = s.timeLSERK4Stages(dt, 50)
        s.setState(*q)
        s.stepRK2(dt, 5)
        s.synchronize()
        t0 = time.perf_counter()
        s.stepRK2(dt, 50)
        s.synchronize()
        rk2 = (time.perf_counter() - t0) / 50 * 1e3
        s.enableMonitor(nodes)                 # only now: the steps above carried no sample of any kind
        s.timeMonitor(5)
        mon = s.timeMonitor(50)
        s.close()
        ld = (K + 63) // 64 * 64
        return dict(stage_ms=stage, rk2_filter_ms=rk2, monitor_ms=mon, monitor_gbps=4 * Np * ld * 8 / (mon * 1e-3) / 1e9)
    return make, Np, K, extra


def quad(n, order):
    mesh = dg.MeshManager()
    mesh.buildMesh(*quadref.quad_box(n))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
    q = [h, np.zeros_like(h), np.zeros_like(h)]
    Np, K = x.shape

    def make():
        return sw2dquads.Sw2dQuadSolver(nodes=nodes, g=9.81), q

    def extra():
        s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=9.81)
        s.setState(*q)
        dt = 0.3 * s.computeDt(0.5)[0]
        s.timeStages(dt, 20)
        out = dict(stage_ms=s.timeStages(dt, 50), rk2_filter_ms=s.timeStages(dt, 20, rk2=True))
        s.close()
        return out
    return make, Np, K, extra


if __name__ == "__main__":
    triad = sw2d.streamTriadGBps(0)
    print(json.dumps(dict(triad_gbps=triad)), flush=True)
    which = sys.argv[1:] or ["tri4", "tri8", "quad4"]
    if "tri4" in which:
        make, Np, K, extra = tri(707, 707, 4)
        run(f"tri N=4 K={K}", make, Np, K, triad, extra)
    if "tri8" in which:
        make, Np, K, extra = tri(354, 353, 8)
        run(f"tri N=8 K={K}", make, Np, K, triad, extra)
    if "quad4" in which:
        make, Np, K, extra = quad(775, 4)
        run(f"quad N=4 K={K}", make, Np, K, triad, extra)
