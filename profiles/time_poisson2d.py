#!/usr/bin/env python3
"""Times the elliptic solver (blitzdg_amd.poisson2d) on triangle boxes and sets the times beside the tracer's two diffusion passes
on the same mesh and beside the bytes an iteration must move:
    python3 profiles/time_poisson2d.py [cases] [count] [rounds] [out.json]
cases: order:cells,... of n x n x 2 triangle boxes; default 4:354,8:173 (250 632 triangles at N = 4, 59 858 at N = 8); 30 runs per
timing; 3 rounds; profiles/poisson2d.json. Per case one record: HIP-event ms per operator application (two launches,
bdg_poisson2d_time_apply) and per conjugate-gradient iteration (six launches, bdg_poisson2d_time_iterations) in every round; the
tracer's two diffusion launches on the same mesh (scalar kappa, no source, no decay: a four-field LSERK4 stage with diffusion
minus one without, best of each, as profiles/time_tri_diffusion.py measures them -- those kernels are the ones of the commit
before the elliptic solver, which changes none of them); bytes per element by accounting and the rate against streamTriadGBps of
the same process; and one solve of -lap u = exp(-40 ((x - 0.3)^2 + (y + 0.2)^2)) with Dirichlet walls to relTol 1e-8 (iterations,
wall seconds; a smooth eigenfunction such as sin(pi x) sin(pi y) would converge in a few dozen iterations at any size and say
nothing about the conditioning). Recorded, not asserted."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import poisson2d, sw2d  # noqa: E402


def apply_bytes(N):
    """Bytes per element of one operator application by accounting, 8 per double, 4 per gather index, 1 per kind. Gradient pass: u
    Np, qx and qy written 2 Np, geometry 13 and kappa 1, index and kind 3 Nfp each. Divergence pass: qx, qy 2 Np, u Np, A u written
    Np, geometry 13, index and kind 3 Nfp each. Neighbour traces come through L2."""
    Np, Nfp = (N + 1) * (N + 2) // 2, N + 1
    return 8 * (3 * Np + 14) + 15 * Nfp + 8 * (4 * Np + 13) + 15 * Nfp


def iteration_bytes(N):
    """... of one iteration: the application with the direction update fused into its first pass (r and p_old read instead of u,
    p written: + 2 Np), the mass product (A p and p read, w written, J: 3 Np + 1) and the update (x, r, s read and written, p, A p,
    w read: 9 Np). 21 Np + 28 doubles + 30 Nfp bytes."""
    Np = (N + 1) * (N + 2) // 2
    return apply_bytes(N) + 8 * 2 * Np + 8 * (3 * Np + 1) + 8 * 9 * Np


def main():
    cases = [tuple(int(v) for v in c.split(":")) for c in (sys.argv[1] if len(sys.argv) > 1 else "4:354,8:173").split(",")]
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "poisson2d.json")
    triad = sw2d.streamTriadGBps()
    records = []
    for N, n in cases:
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(n, n)
        nodes = dg.TriangleNodesProvisioner(N, mesh)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        K = x.shape[1]
        r = {"order": N, "K": K, "streamTriadGBps": round(triad, 1), "ms_apply": [], "ms_iteration": []}

        solver = poisson2d.Poisson2dSolver(nodes=nodes)
        solver.timeApply(5)
        solver.timeIterations(5)  # warm-up
        for _ in range(rounds):
            r["ms_apply"].append(round(solver.timeApply(count), 4))
            r["ms_iteration"].append(round(solver.timeIterations(count), 4))
        r["device_bytes"] = solver.deviceBytes()
        for key, ms, nbytes in (("apply", min(r["ms_apply"]), apply_bytes(N)), ("iteration", min(r["ms_iteration"]), iteration_bytes(N))):
            r[f"{key}_bytes_per_element"] = nbytes
            r[f"{key}_GBps"] = round(nbytes * K / (ms * 1e-3) / 1e9, 1)
            r[f"{key}_fraction_of_triad"] = round(r[f"{key}_GBps"] / triad, 3)
        t0 = time.perf_counter()
        u, info = solver.solve(np.exp(-40 * ((x - 0.3) ** 2 + (y + 0.2) ** 2)), relTol=1e-8, maxIterations=100000, checkEvery=32)
        r["solve"] = {"relTol": 1e-8, "iterations": info.iterations, "converged": info.converged,
                      "relative_residual": float(f"{info.relativeResidual:.3e}"), "seconds": round(time.perf_counter() - t0, 3),
                      "max_u": float(f"{np.abs(u).max():.4e}")}
        solver.close()

        # ---- the tracer's two diffusion launches on the same mesh
        h = 10.0 + 0.3 * np.exp(-10 * x * x - 10 * y * y)
        z = np.zeros_like(h)
        hN = h * (0.3 + 0.1 * np.sin(5 * x) * np.cos(4 * y))
        dt = 0.1 * (2.0 / n) / ((N + 1) ** 2 * 10.0)
        plain, diff = sw2d.Sw2dSolver(nodes=nodes, fields=4), sw2d.Sw2dSolver(nodes=nodes, fields=4)
        diff.enableTracerDiffusion(1e-4)
        r["ms_stage"], r["ms_stage_with_diffusion"] = [], []
        for s in (plain, diff):
            s.setState4(h, z, z, hN)
            s.timeLSERK4Stages(dt, 5)
        for _ in range(rounds):
            r["ms_stage"].append(round(plain.timeLSERK4Stages(dt, count), 4))
            r["ms_stage_with_diffusion"].append(round(diff.timeLSERK4Stages(dt, count), 4))
        r["ms_tracer_diffusion_launches"] = round(min(r["ms_stage_with_diffusion"]) - min(r["ms_stage"]), 4)
        r["apply_over_tracer_diffusion"] = round(min(r["ms_apply"]) / r["ms_tracer_diffusion_launches"], 3)
        plain.close()
        diff.close()
        print(json.dumps(r), flush=True)
        records.append(r)
    with open(out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
