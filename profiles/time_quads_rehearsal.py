#!/usr/bin/env python3
"""Loop-back rehearsal of a partitioned run of the quadrilateral solver on ONE GPU:
    python3 profiles/time_quads_rehearsal.py [order] [n] [world] [rank] [steps]
defaults: N = 4, the n = 775 box of profiles/time_quads.py (600 625 quadrangles), 8-way, rank 6, 50 steps. This process
computes `rank`'s share of a `world`-way split; every neighbour exchange is a real RCCL send-to-self of the true size
(NativeDistributedSw2dQuad(loopback=True)). Timing only: the ghosts then hold this rank's own boundary elements. The rank
must receive from each neighbour as many elements as it sends (else a send-to-self leaves ghosts at zero depth and the
blow-up check stops the run): on the 775 box, rank 1 of a 2- or 4-way split and rank 6 (four neighbours) of an 8-way one.
Prints one JSON line: ms per LSERK4 stage and per RK2 + filter step on the two-chain schedule, with every element in
stream order (BDG_SW2DQ_NO_OVERLAP), and of the whole mesh on the same GPU in the same process (host clock around
whole calls that end in a device synchronise, best of three)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.halo import build_plan  # noqa: E402
from blitzdg_amd.sw2dquads import NativeDistributedSw2dQuad, Sw2dQuadSolver  # noqa: E402


def box(n):
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    return np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1), V


def state(x, y):
    h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
    z = np.zeros_like(h)
    return h, z, z.copy()


def timed(run, sync, count):
    """Best of three: ms per unit of `count` units, one call each."""
    run(2)
    sync()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        run(count)
        sync()
        best = min(best, (time.perf_counter() - t0) / count * 1e3)
    return best


def main():
    a = [int(v) for v in sys.argv[1:]]
    order, n, world, rank, steps = (a + [4, 775, 8, 6, 50][len(a):])[:5]
    mesh = dg.MeshManager()
    mesh.buildMesh(*box(n))
    total = mesh.numElements
    mesh.partitionMesh(world)
    plan = build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, rank, world, bctype=mesh.bcType)
    _, _, sc, _, rc = plan.peer_tables()
    if (sc != rc).any():
        raise SystemExit(f"rank {rank} of a {world}-way split sends {sc.tolist()} and receives {rc.tolist()} elements: pick a "
                         "rank whose counts agree for the send-to-self rehearsal")
    filt = (0.99 * order, 4)
    dt = 0.1 * (2.0 / n) / (order * order * 10.0)
    d = NativeDistributedSw2dQuad(plan, order, filter_args=filt, loopback=True)
    d.set_initial_state(state)
    out = {"order": order, "elements": total, "world": world, "rank": rank, "owned": int(plan.num_owned),
           "interior": int(plan.num_interior), "ghost": int(plan.num_halo),
           "parallelogram_geometry": bool(d.solver.usesParallelogramGeometry)}
    sync = d.solver.synchronize
    for key, env in (("two_chains", None), ("stream_order", "1")):
        if env:
            os.environ["BDG_SW2DQ_NO_OVERLAP"] = env
        out[f"ms_per_lserk4_stage_{key}"] = round(timed(lambda k: d.lserk4_stages(dt, k), sync, 5 * steps), 4)
        out[f"ms_per_rk2_filter_step_{key}"] = round(timed(lambda k: d.step_rk2(dt, k, filter=True), sync, steps), 4)
    os.environ.pop("BDG_SW2DQ_NO_OVERLAP", None)
    d.close()
    # the whole mesh on this GPU
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(*filt)
    ctx = nodes.dgContext()
    s = Sw2dQuadSolver(nodes=nodes)
    s.setState(*state(ctx.x, ctx.y))
    out["ms_per_lserk4_stage_whole_mesh"] = round(timed(lambda k: s.lserk4Stages(dt, k), s.synchronize, 5 * steps), 4)
    out["ms_per_rk2_filter_step_whole_mesh"] = round(timed(lambda k: s.stepRK2(dt, k, filter=True), s.synchronize, steps), 4)
    s.close()
    for kind in ("lserk4_stage", "rk2_filter_step"):
        for key in ("two_chains", "stream_order"):
            out[f"speedup_{kind}_{key}"] = round(out[f"ms_per_{kind}_whole_mesh"] / out[f"ms_per_{kind}_{key}"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
