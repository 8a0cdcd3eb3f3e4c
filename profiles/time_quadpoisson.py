#!/usr/bin/env python3
"""Times the elliptic solver on quadrilaterals (blitzdg_amd.poisson2d.Poisson2dQuadSolver) and sets the times beside the quad
tracer's two diffusion launches on the same mesh, beside the bytes an iteration must move and beside the triangle solver at an
equal node count:
    python3 profiles/time_quadpoisson.py [cases] [count] [rounds] [out.json] [triangles: 1 | 0]
cases: order:cells,... of n x n boxes of squares; default 4:775,8:775,12:400 (600 625 quadrilaterals at N = 4 and N = 8, 160 000
at N = 12); 30 runs per timing; best of 3 rounds; profiles/quadpoisson.json. Per case one record: HIP-event ms per operator
application (two launches) and per conjugate-gradient iteration (six launches) in every round, one process, the clocks ramped by
the triad probe and by untimed launches; the quad tracer's two diffusion launches on the same mesh (scalar kappa, no source, no
decay: a four-field LSERK4 stage with diffusion minus one without, best of each -- kernels this solver does not touch); bytes
per element by the accounting of profiles/time_poisson2d.py with Np = (N+1)^2, four faces and 16 geometry numbers, and the rate
against streamTriadGBps of the same process; one solve of -lap u = exp(-40 ((x - 0.3)^2 + (y + 0.2)^2)) with Dirichlet walls to
relTol 1e-8; and the triangle solver's ms per iteration on a box with about as many nodes (at its own order min(N, 8)). The record
is written after every case. Recorded, not asserted."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import poisson2d, sw2d, sw2dquads  # noqa: E402


def apply_bytes(N):
    """Bytes per element of one operator application, 8 per double, 4 per gather index, 1 per kind. Gradient pass: u Np, qx and qy
    written 2 Np, geometry 16 and kappa 1, index and kind 4 Nfp each. Divergence pass: qx, qy 2 Np, u Np, A u written Np, geometry
    16, index and kind 4 Nfp each. Neighbour traces come through L2."""
    Np, NFN = (N + 1) ** 2, 4 * (N + 1)
    return 8 * (3 * Np + 17) + 5 * NFN + 8 * (4 * Np + 16) + 5 * NFN


def iteration_bytes(N):
    """... of one iteration: + 2 Np for the fused direction update, 3 Np + 1 for the mass product, 9 Np for the update."""
    Np = (N + 1) ** 2
    return apply_bytes(N) + 8 * 2 * Np + 8 * (3 * Np + 1) + 8 * 9 * Np


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def quad_box(n):
    xs = np.linspace(-1, 1, n + 1)
    X, Y = np.meshgrid(xs, xs)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    mesh = dg.MeshManager()
    mesh.buildMesh(np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1), np.stack([X.ravel(), Y.ravel()], axis=1))
    return mesh


def main():
    cases = [tuple(int(v) for v in c.split(":")) for c in (sys.argv[1] if len(sys.argv) > 1 else "4:775,8:775,12:400").split(",")]
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "quadpoisson.json")
    triangles = (sys.argv[5] if len(sys.argv) > 5 else "1") != "0"
    triad = sw2d.streamTriadGBps()
    records = []
    for N, n in cases:
        mesh = quad_box(n)
        nodes = dg.QuadNodesProvisioner(N, mesh)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        K = x.shape[1]
        r = {"order": N, "K": K, "nodes": x.size, "streamTriadGBps": round(triad, 1), "ms_apply": [], "ms_iteration": []}

        note(f"N = {N}: K = {K}, tables built")
        solver = poisson2d.Poisson2dQuadSolver(nodes=nodes)
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
        note(f"N = {N}: operator and iteration timed")
        t0 = time.perf_counter()
        u, info = solver.solve(np.exp(-40 * ((x - 0.3) ** 2 + (y + 0.2) ** 2)), relTol=1e-8, maxIterations=100000, checkEvery=32)
        r["solve"] = {"relTol": 1e-8, "iterations": info.iterations, "converged": info.converged,
                      "relative_residual": float(f"{info.relativeResidual:.3e}"), "seconds": round(time.perf_counter() - t0, 3),
                      "max_u": float(f"{np.abs(u).max():.4e}")}
        solver.close()

        note(f"N = {N}: solved in {info.iterations} iterations")
        # ---- the quad tracer's two diffusion launches on the same mesh
        h = 10.0 + 0.3 * np.exp(-10 * x * x - 10 * y * y)
        z = np.zeros_like(h)
        hN = h * (0.3 + 0.1 * np.sin(5 * x) * np.cos(4 * y))
        dt = 0.1 * (2.0 / n) / ((N + 1) ** 2 * 10.0)
        plain, diff = sw2dquads.Sw2dQuadSolver(nodes=nodes, fields=4), sw2dquads.Sw2dQuadSolver(nodes=nodes, fields=4)
        diff.enableTracerDiffusion(1e-4)
        r["ms_stage"], r["ms_stage_with_diffusion"] = [], []
        for s in (plain, diff):
            s.setState4(h, z, z, hN)
            s.timeStages(dt, 5)
        for _ in range(rounds):
            r["ms_stage"].append(round(plain.timeStages(dt, count), 4))
            r["ms_stage_with_diffusion"].append(round(diff.timeStages(dt, count), 4))
        r["ms_tracer_diffusion_launches"] = round(min(r["ms_stage_with_diffusion"]) - min(r["ms_stage"]), 4)
        r["apply_over_tracer_diffusion"] = round(min(r["ms_apply"]) / r["ms_tracer_diffusion_launches"], 3)
        plain.close()
        diff.close()
        del nodes, ctx, mesh, h, z, hN, u

        note(f"N = {N}: tracer diffusion timed")
        # ---- the triangle solver on about as many nodes
        if triangles:
            Nt = min(N, 8)
            m = int(round(np.sqrt(x.size / ((Nt + 1) * (Nt + 2) / 2) / 2)))
            tmesh = dg.MeshManager()
            tmesh.buildBoxMesh(m, m)
            tnodes = dg.TriangleNodesProvisioner(Nt, tmesh)
            ts = poisson2d.Poisson2dSolver(nodes=tnodes)
            ts.timeIterations(5)
            tms = [round(ts.timeIterations(count), 4) for _ in range(rounds)]
            r["triangles"] = {"order": Nt, "K": 2 * m * m, "nodes": 2 * m * m * (Nt + 1) * (Nt + 2) // 2, "ms_iteration": tms}
            r["iteration_per_node_over_triangles"] = round((min(r["ms_iteration"]) / r["nodes"]) / (min(tms) / r["triangles"]["nodes"]), 3)
            ts.close()
            del tnodes, tmesh
        print(json.dumps(r), flush=True)
        records.append(r)
        with open(out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
