#!/usr/bin/env python3
"""Times a four-field LSERK4 stage on triangles with and without the eddy-viscosity passes (sw2d_viscosity_kernel.hpp), the
solvers interleaved in one process (the protocol of profiles/time_tri_diffusion.py):
    python3 profiles/time_tri_viscosity.py [cases] [stages] [rounds] [out.json]
cases: order:cells,... of n x n x 2 triangle boxes; default 4:707,8:354 (10^6 triangles at N = 4, 2.5 10^5 at N = 8); 30 stages
per timing; 3 rounds; profiles/tri_viscosity.json. Per case, on variant B with a tracer (the x = -1 side open), one record: HIP-event
ms per LSERK4 stage (bdg_sw2d_time_lserk4_stages) in every round of the solver without viscosity (the kernels that existed
before the passes), with a constant viscosity field (Cs = 0), with Smagorinsky on top (Cs > 0), and with the tracer's diffusion
alone (scalar kappa, no source, no decay: its two launches, twice, are what two one-field passes per momentum component would
cost). The viscosity launches are the difference of the best of each; their bytes per element by accounting and their rate against
streamTriadGBps of the same process. The clocks are ramped by the triad probe and by a warm-up of five stages per solver."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d  # noqa: E402


def pass_bytes(N, field=True):
    """Bytes per element and LSERK4 stage of the two launches by accounting, 8 per double, 4 per index. Gradient pass: h, hu, hv
    3 Np, nu0 Np if it is a field, the four flux planes written 4 Np (the raw gradients written first are overwritten in cache),
    geometry 13, gather index 3 Nfp (the second component's re-reads of h, geometry and index come through L1 / L2: not counted).
    Divergence pass: the four flux planes 4 Np, residual and state of hu and hv read and written 8 Np, geometry 13, gather index
    3 Nfp. Neighbour traces come through L2. Together (19 + field) Np doubles + 26 + 6 Nfp indices."""
    Np, Nfp = (N + 1) * (N + 2) // 2, N + 1
    gradient = 8 * ((3 + (1 if field else 0)) * Np + 4 * Np + 13) + 4 * 3 * Nfp
    divergence = 8 * (4 * Np + 8 * Np + 13) + 4 * 3 * Nfp
    return gradient + divergence


def tracer_pass_bytes(N):
    """The tracer's two launches with a scalar kappa and no pointwise part (profiles/time_tri_diffusion.py: 10 Np doubles + 26 +
    6 Nfp indices)."""
    Np, Nfp = (N + 1) * (N + 2) // 2, N + 1
    return 8 * (10 * Np + 26) + 4 * 6 * Nfp


def main():
    cases = [tuple(int(v) for v in c.split(":")) for c in (sys.argv[1] if len(sys.argv) > 1 else "4:707,8:354").split(",")]
    stages = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_viscosity.json")
    triad = sw2d.streamTriadGBps()
    records = []
    for N, n in cases:
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(n, n)
        verts = np.asarray(mesh.vertices).reshape(-1, 3)
        etov = np.asarray(mesh.elements).reshape(-1, 3)
        bc = np.array(mesh.bcType).reshape(-1, 3)
        for face, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
            left = (verts[etov[:, a], 0] < -1 + 1e-9) & (verts[etov[:, b], 0] < -1 + 1e-9)
            bc[left & (bc[:, face] != 0), face] = 2
        mesh.setBCType(bc.ravel())
        nodes = dg.TriangleNodesProvisioner(N, mesh)
        nodes.buildFilter(0.9 * N, N)
        ctx = nodes.dgContext()
        x, y = ctx.x, ctx.y
        K = x.shape[1]
        mapO = np.asarray(ctx.BCmap.get(2, []), dtype=np.int32)
        H = 10.0 * (1 + 0.05 * x - 0.03 * y * y)
        Hx, Hy = 0.5 + 0 * x, -0.6 * y
        h = H + 0.3 * np.exp(-10 * x * x - 10 * y * y)
        hu = 0.5 * h * np.sin(3 * x) * np.cos(2 * y)
        hv = -0.5 * h * np.cos(3 * x) * np.sin(2 * y)
        hN = h * (0.3 + 0.1 * np.sin(5 * x) * np.cos(4 * y))
        nu0 = 1e-4 * (1 + 0.5 * np.sin(3 * x))
        dt = 0.1 * (2.0 / n) / ((N + 1) ** 2 * 10.0)

        def make(what):
            s = sw2d.Sw2dSolver(nodes=nodes, fields=4)
            s.enableVariantB(H, Hx, Hy, mapO=mapO, CD=2.5e-3, f=1e-4, tideAmplitude=0.5, tidePeriod=40.0, tideRamp=0.05, tracer=0.5)
            if what == "diffusion":
                s.enableTracerDiffusion(1e-4)
            elif what != "plain":
                s.enableViscosity(nu0, 0.2 if what == "smagorinsky" else 0.0)
            s.setState4(h, hu, hv, hN)
            if what in ("constant", "smagorinsky"):
                assert dt < s.viscosityDt()
            return s

        kinds = ("plain", "constant", "smagorinsky", "diffusion")
        solvers = {k: make(k) for k in kinds}
        for s in solvers.values():
            s.timeLSERK4Stages(dt, 5)  # warm-up
        r = {"order": N, "K": K, "solver": "B4", "streamTriadGBps": round(triad, 1)}
        ms = {k: [] for k in kinds}
        for _ in range(rounds):
            for k in kinds:
                ms[k].append(round(solvers[k].timeLSERK4Stages(dt, stages), 4))
        r["ms_stage"] = ms["plain"]
        r["ms_stage_with_viscosity"] = ms["constant"]
        r["ms_stage_with_smagorinsky"] = ms["smagorinsky"]
        r["ms_stage_with_tracer_diffusion"] = ms["diffusion"]
        best = {k: min(v) for k, v in ms.items()}
        for k, name in (("constant", "viscosity"), ("smagorinsky", "smagorinsky")):
            d = best[k] - best["plain"]
            r[f"ms_{name}_launches"] = round(d, 4)
            r[f"ratio_stage_{name}"] = round(best[k] / best["plain"], 3)
            r[f"{name}_GBps"] = round(pass_bytes(N) * K / (d * 1e-3) / 1e9, 1) if d > 0 else None
            r[f"{name}_fraction_of_triad"] = round(r[f"{name}_GBps"] / triad, 3) if d > 0 else None
        r["viscosity_bytes_per_element"] = pass_bytes(N)
        d = best["diffusion"] - best["plain"]
        r["ms_twice_tracer_diffusion_launches"] = round(2 * d, 4)
        r["twice_tracer_diffusion_bytes_per_element"] = 2 * tracer_pass_bytes(N)
        for s in solvers.values():
            assert all(np.isfinite(a).all() for a in s.getState4())
            s.close()
        print(json.dumps(r), flush=True)
        records.append(r)
    with open(out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
