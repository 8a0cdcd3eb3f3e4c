#!/usr/bin/env python3
"""Times a four-field LSERK4 stage on quadrilaterals with and without the tracer's diffusion passes
(sw2d_quad_diffusion_kernel.hpp), the solvers interleaved in one process (the protocol of profiles/time_tri_diffusion.py):
    python3 profiles/time_quad_diffusion.py [cases] [stages] [rounds] [out.json]
cases: order:cells,... of n x n boxes of squares, which take the parallelogram form; default 4:775,8:775,12:400 (600 625
quadrilaterals at N = 4 and N = 8, 160 000 at N = 12); 30 stages per timing; 3 rounds; profiles/quad_diffusion.json. Per case and
per kind of solver -- "A" (variant A with bed slope, Coriolis and drag) and "B" (variant B with a tracer, the x = -1 side open) --
one record: HIP-event ms per LSERK4 stage (bdg_sw2dq_time) of the solver without and with diffusion in every round (the timings
without diffusion are those of the kernels that existed before the passes), the two diffusion launches as the difference of the
best of each, their bytes per element by accounting and their rate against streamTriadGBps of the same process. kappa is an
(Np, K) plane, a source is on, decay is on. The clocks are ramped by the triad probe and by a warm-up of five stages per solver.
The record is written after every case, so a run that is cut short leaves what it measured."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d, sw2dquads  # noqa: E402


def pass_bytes(N):
    """Bytes per element and LSERK4 stage of the two launches by accounting, 8 per double, 4 per index, parallelogram form.
    Gradient pass: h and hN Np each, kappa Np, fx and fy written 2 Np, geometry 16, gather index NFN (h again at the output rows
    comes through L2: not counted). Divergence pass: fx and fy 2 Np, the source Np, hN Np, residual and state read and written
    4 Np, geometry 16, gather index NFN. Neighbour traces come through L2. Together 13 Np doubles (10 Np without source, decay
    and a kappa plane) + 32 + 2 NFN indices."""
    Np, NFN = (N + 1) ** 2, 4 * (N + 1)
    gradient = 8 * (2 * Np + Np + 2 * Np + 16) + 4 * NFN
    divergence = 8 * (2 * Np + Np + Np + 4 * Np + 16) + 4 * NFN
    return gradient + divergence


def main():
    cases = [tuple(int(v) for v in c.split(":")) for c in (sys.argv[1] if len(sys.argv) > 1 else "4:775,8:775,12:400").split(",")]
    stages = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "quad_diffusion.json")
    triad = sw2d.streamTriadGBps()
    records = []
    for N, n in cases:
        xs = np.linspace(-1, 1, n + 1)
        X, Y = np.meshgrid(xs, xs)
        V = np.stack([X.ravel(), Y.ravel()], axis=1)
        a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
        mesh = dg.MeshManager()
        mesh.buildMesh(np.stack([a, a + 1, a + n + 2, a + n + 1], axis=1), V)
        K = mesh.numElements
        bc = np.array(mesh.bcType).reshape(K, 4)
        bc[np.arange(n) * n, 3] = 2          # face 3 of the first column of elements: the x = -1 side
        mesh.setBCType(bc.ravel())
        nodes = dg.QuadNodesProvisioner(N, mesh)
        nodes.buildFilter(0.99 * N, 4)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        mapO = np.asarray(ctx.BCmap.get(2, []), dtype=np.int32)
        H = 10.0 * (1 + 0.05 * x - 0.03 * y * y)
        Hx, Hy = 0.5 + 0 * x, -0.6 * y
        h = H + 0.3 * np.exp(-10 * x * x - 10 * y * y)
        z = np.zeros_like(h)
        hN = h * (0.3 + 0.1 * np.sin(5 * x) * np.cos(4 * y))
        kappa = 1e-4 * (1 + 0.5 * np.sin(3 * x))
        source = np.exp(-30 * (x - 0.2) ** 2 - 30 * y * y)
        dt = 0.1 * (2.0 / n) / ((N + 1) ** 2 * 10.0)

        def make(kind, diffusion):
            if kind == "A":
                s = sw2dquads.Sw2dQuadSolver(nodes=nodes, fields=4, sources=dict(zx=-0.01 * Hx, zy=-0.01 * Hy, f=1e-4, CD=2.5e-3))
            else:
                s = sw2dquads.Sw2dQuadSolver(nodes=nodes, fields=4)
                s.enableVariantB(H, Hx, Hy, mapO=mapO, CD=2.5e-3, f=1e-4, tide=(0.5, 40.0, 0.05), tracer=0.5)
            assert s.usesParallelogramGeometry
            if diffusion:
                s.enableTracerDiffusion(kappa, source=source, decay=1e-3)
                assert dt < s.diffusionDt()
            s.setState4(h, z, z, hN)
            return s

        for kind in ("A", "B"):
            plain, diff = make(kind, False), make(kind, True)
            for s in (plain, diff):
                s.timeStages(dt, 5)  # warm-up
            r = {"order": N, "K": K, "solver": kind, "streamTriadGBps": round(triad, 1), "ms_stage": [], "ms_stage_with_diffusion": []}
            for _ in range(rounds):
                r["ms_stage"].append(round(plain.timeStages(dt, stages), 4))
                r["ms_stage_with_diffusion"].append(round(diff.timeStages(dt, stages), 4))
            ms = min(r["ms_stage_with_diffusion"]) - min(r["ms_stage"])
            r["ms_diffusion_launches"] = round(ms, 4)
            r["ratio_stage"] = round(min(r["ms_stage_with_diffusion"]) / min(r["ms_stage"]), 3)
            r["diffusion_bytes_per_element"] = pass_bytes(N)
            r["diffusion_GBps"] = round(pass_bytes(N) * K / (ms * 1e-3) / 1e9, 1) if ms > 0 else None
            r["diffusion_fraction_of_triad"] = round(r["diffusion_GBps"] / triad, 3) if ms > 0 else None
            assert all(np.isfinite(a).all() for a in diff.getState4())
            print(json.dumps(r), flush=True)
            records.append(r)
            plain.close()
            diff.close()
            with open(out, "w") as f:
                json.dump(records, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
