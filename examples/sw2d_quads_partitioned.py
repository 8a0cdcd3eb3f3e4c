#!/usr/bin/env python3
"""The loop of examples/sw2d_quads.py on an element partition: one process per GPU, each owning a share of the mesh
plus one layer of ghost elements, the ghosts refreshed by the library over RCCL before every evaluation.

    RANK=r WORLD_SIZE=w python examples/sw2d_quads_partitioned.py [finalTime] [order] [box n] [outputDir]

Rank and world come from RANK / WORLD_SIZE (LOCAL_RANK picks the GPU; default RANK), as bench.py --gpus passes them to
its child processes; rank 0's RCCL id reaches the others through a private file (blitzdg_amd.halo.file_rendezvous), so
every rank must be a child of the same launcher. The script's set-up: coarse_box_quads_fine.msh (or an n x n box of
[-1, 1]^2 with a third argument), N = 4, the filter with Nc = 0.99 N and s = 4, a Gaussian hump of height 1 on still water
of depth 10, dt = 0.45 * 0.000724295 (scaled with the element size on a box), g = 9.81; midpoint RK2 with the filter, 20
steps per call, the blow-up check on every rank together. At the end rank 0 prints the global eta range and the relative
mass drift (each rank leaves its four numbers in the rendezvous directory; rank 0 combines them). With an output directory
(box n = 0 keeps the Gmsh file) every rank writes its owned elements' eta, u, v as <field><step>.<rank>.vtu at step 0 and every
20 steps, and rank 0 the <field><step>.pvtu index of the pieces.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd.halo import build_plan  # noqa: E402
from blitzdg_amd.sw2dquads import NativeDistributedSw2dQuad  # noqa: E402


def box(n):
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    return np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1), V


def main():
    finalTime = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    outdir = sys.argv[4] if len(sys.argv) > 4 else None
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = int(os.environ.get("LOCAL_RANK", rank))
    g, H = 9.81, 10.0
    mesh = dg.MeshManager()
    if n:
        mesh.buildMesh(*box(n))
        dt = 0.45 * 0.000724295 * (2.0 / n) / 0.25   # (coarse_box_quads_fine.msh: 8 x 8 elements of side 0.25)
    else:
        mesh.readMesh(os.path.join(ROOT, "tests", "golden", "coarse_box_quads_fine.msh"))
        dt = 0.45 * 0.000724295
    total = mesh.numElements
    mesh.partitionMesh(world)
    plan = build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, rank, world, bctype=mesh.bcType)
    del mesh
    d = NativeDistributedSw2dQuad(plan, N, g=g, filter_args=(0.99 * N, 4), device=device)
    d.set_initial_state(lambda x, y: (H + np.exp(-10 * x * x - 10 * y * y), np.zeros_like(x), np.zeros_like(x)))
    m0 = d.owned_mass()
    Hloc = None
    if outdir:
        os.makedirs(outdir, exist_ok=True)
        Hloc = H * np.ones_like(d.nodes.dgContext().x)
        d.write_piece(0, outdir, H=Hloc)
    t, step, chunk = 0.0, 0, 20
    t0 = time.perf_counter()
    while t < finalTime:
        k = min(chunk, int(np.ceil((finalTime - t) / dt)))
        d.step_rk2(dt, k, filter=True)  # raises NumericalInstability on every rank together
        t += k * dt
        step += k
        if outdir and step % 20 == 0:
            d.write_piece(step, outdir, H=Hloc)
    d.barrier()
    wall = time.perf_counter() - t0
    _, h, _, _ = d.owned_state()
    mine = {"rank": rank, "eta_min": float((h - H).min()), "eta_max": float((h - H).max()), "m0": m0, "m1": d.owned_mass()}
    d.close()
    # the end-of-run numbers of every rank meet in the launcher's private directory (no collective needed for four floats)
    out = os.path.join(os.environ.get("BDG_RENDEZVOUS_DIR", "/tmp"), f"bdg_rccl_{os.getuid()}",
                       f"quads_{os.getppid()}_{os.environ.get('MASTER_PORT', '0')}_{world}")
    os.makedirs(os.path.dirname(out), mode=0o700, exist_ok=True)
    with open(f"{out}.{rank}.tmp", "w") as f:
        json.dump(mine, f)
    os.replace(f"{out}.{rank}.tmp", f"{out}.{rank}")
    if rank != 0:
        return
    deadline = time.time() + 120
    while not all(os.path.exists(f"{out}.{r}") for r in range(world)) and time.time() < deadline:
        time.sleep(0.05)
    parts = []
    for r in range(world):
        with open(f"{out}.{r}") as f:
            parts.append(json.load(f))
        os.remove(f"{out}.{r}")
    m0 = sum(p["m0"] for p in parts)
    m1 = sum(p["m1"] for p in parts)
    print(f"done: {step} steps to t={t:.4f} on {total} quadrilaterals at N={N}, {world} rank(s), in {wall:.2f} s")
    print(f"eta in [{min(p['eta_min'] for p in parts):+.5f}, {max(p['eta_max'] for p in parts):+.5f}], "
          f"relative mass drift {(m1 - m0) / m0:+.3e}")


if __name__ == "__main__":
    main()
