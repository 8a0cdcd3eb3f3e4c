#!/usr/bin/env python3
"""Times variant B with the passive tracer (four fields) beside three-field variant B of the same build on triangles, the two
solvers interleaved in one process (the protocol of profiles/time_quadsB4.py):
    python3 profiles/time_tri_vb4.py [cases] [stages] [out.json]
cases: order:cells,... of n x n x 2 triangle boxes; default 4:707,6:500,8:354 (10^6 triangles at N = 4, 5 10^5 at N = 6,
2.5 10^5 at N = 8); 30 stages; profiles/tri_vb4.json. Per case one record: HIP-event ms per LSERK4 stage of three-field B and
of four-field B (bdg_sw2d_time_lserk4_stages), ms per Heun step of both (wall clock around stepSSPRK2 + synchronize: the
library has no event timer for that stepper), the tracer pass alone as the difference of the two stage times, its bytes per
element by accounting and its rate against streamTriadGBps of the same process. The x = -1 side is open and feeds a
concentration that varies along it, the bed slopes, drag and Coriolis are on. Every solver is timed twice, in turn (the second
round is reported as *_again); the clocks are ramped by a warm-up of five stages each and by the triad probe."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blitzdg_amd.pyblitzdg as dg  # noqa: E402
from blitzdg_amd import sw2d  # noqa: E402


def pass_bytes(N):
    """Bytes per element and LSERK4 stage of the tracer pass by accounting: own state 4 Np, H on the 3 Nfp face nodes, residual
    Np, writes 2 Np (residual and state), geometry 13, gather index 3 Nfp ints, open-boundary mask (and table index): 8 bytes
    per double. Neighbour traces come through L2. The general form reads the own state a second time at the face nodes
    (through L1 / L2: not counted)."""
    Np, Nfp = (N + 1) * (N + 2) // 2, N + 1
    return 8 * (4 * Np + 3 * Nfp + Np + 2 * Np + 13) + 4 * (3 * Nfp + 2)


def heun_ms(s, dt, steps):
    s.synchronize()
    t0 = time.perf_counter()
    s.stepSSPRK2(dt, steps)
    s.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    cases = [tuple(int(v) for v in c.split(":")) for c in (sys.argv[1] if len(sys.argv) > 1 else "4:707,6:500,8:354").split(",")]
    stages = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_vb4.json")
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
        assert len(mapO) == n * (N + 1)
        H = 10.0 * (1 + 0.05 * x - 0.03 * y * y)
        Hx, Hy = 0.5 + 0 * x, -0.6 * y
        h = H + 0.3 * np.exp(-10 * x * x - 10 * y * y)
        z = np.zeros_like(h)
        hN = 0.3 * h
        tracer = 0.5 + 0.4 * np.sin(3 * y.flatten("F")[np.asarray(ctx.vmapM).reshape(-1)[mapO]])
        dt = 0.1 * (2.0 / n) / ((N + 1) ** 2 * 10.0)
        vb = dict(mapO=mapO, CD=2.5e-3, f=1e-4, tideAmplitude=0.5, tidePeriod=40.0, tideRamp=0.05)
        b3 = sw2d.Sw2dSolver(nodes=nodes)
        b3.enableVariantB(H, Hx, Hy, **vb)
        b4 = sw2d.Sw2dSolver(nodes=nodes, fields=4)
        b4.enableVariantB(H, Hx, Hy, tracer=tracer, **vb)
        b3.setState(h, z, z)
        b4.setState4(h, z, z, hN)
        for s in (b3, b4):
            s.timeLSERK4Stages(dt, 5)  # warm-up
        r = {"order": N, "K": K, "streamTriadGBps": round(triad, 1)}
        for tag in ("", "_again"):
            r["ms_B3_lserk4_stage" + tag] = round(b3.timeLSERK4Stages(dt, stages), 4)
            r["ms_B4_lserk4_stage" + tag] = round(b4.timeLSERK4Stages(dt, stages), 4)
            r["ms_B3_heun_step" + tag] = round(heun_ms(b3, dt, max(stages // 2, 2)), 4)
            r["ms_B4_heun_step" + tag] = round(heun_ms(b4, dt, max(stages // 2, 2)), 4)
        ms_pass = min(r["ms_B4_lserk4_stage"], r["ms_B4_lserk4_stage_again"]) - min(r["ms_B3_lserk4_stage"], r["ms_B3_lserk4_stage_again"])
        r["ms_tracer_pass"] = round(ms_pass, 4)
        r["ratio_lserk4_stage"] = round(min(r["ms_B4_lserk4_stage"], r["ms_B4_lserk4_stage_again"]) /
                                        min(r["ms_B3_lserk4_stage"], r["ms_B3_lserk4_stage_again"]), 3)
        r["ratio_heun_step"] = round(min(r["ms_B4_heun_step"], r["ms_B4_heun_step_again"]) /
                                     min(r["ms_B3_heun_step"], r["ms_B3_heun_step_again"]), 3)
        r["tracer_pass_bytes_per_element"] = pass_bytes(N)
        r["tracer_pass_GBps"] = round(r["tracer_pass_bytes_per_element"] * K / (ms_pass * 1e-3) / 1e9, 1) if ms_pass > 0 else None
        r["tracer_pass_fraction_of_triad"] = round(r["tracer_pass_GBps"] / triad, 3) if ms_pass > 0 else None
        assert all(np.isfinite(a).all() for a in b4.getState4())
        print(json.dumps(r), flush=True)
        records.append(r)
        for s in (b3, b4):
            s.close()
    with open(out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
