"""The conditions the cases of tests/test_sw2d_curved_driver_gpu.py meet, checked on the CPU before any GPU time is spent
(tests/curved_driver_ref.py), and the compiler's report on the driver kernels (sw2d_curved_driver_kernel.hpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import curved_driver_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(ref.ADAPTIVE_CASES))
def test_adaptive_cases_stay_wet_and_finite_and_change_dt_every_step(name):
    """H = 1, c = sqrt(g), CFL = 0.25: the adaptive steps keep h > 0.5, stay finite, and use a different dt on every step (a
    fixed-dt implementation would pass otherwise). Measured: min h 0.61, 0.63, 0.65; 6, 6, 4 distinct dts."""
    steps, last_dt = ref.adaptive_loop(name)
    assert len(steps) == ref.ADAPTIVE_CASES[name][1]
    hmin = min(q[0].min() for _, _, q in steps)
    dts = [dt for dt, _, _ in steps] + [last_dt]
    print(name, "min h", hmin, "dts", dts)
    assert hmin > 0.5
    assert all(np.isfinite(a).all() for _, _, q in steps for a in q)
    assert len(set(dts[:-1])) == len(steps) and dts[-1] != dts[-2]
    assert all(np.isfinite(dts)) and min(dts) > 0


def test_dt_formula_reads_face_nodes_of_the_own_element():
    """What enableDriver validates: vmapM[j + 3 Nfp k] is a node of element k and the local part is one list for all k."""
    c = ref.case("N3-7x6")
    Np, K = c.ctx.numLocalPoints, c.K
    vm = np.asarray(c.ctx.vmapM).reshape(K, -1)
    assert (vm // Np == np.arange(K)[:, None]).all()
    assert (vm % Np == (vm % Np)[0]).all()


def test_rigid_rotation_has_vorticity_two_on_the_deformed_mesh():
    """hu = -y, hv = x on h = 1: the map is isoparametric, so the nodal derivative is exact and vort = 2 within the bound, curved
    elements included (what the GPU test asks of the device)."""
    c = ref.case("N4-7x6-shuffled")
    u, v = -c.y, c.x
    assert c.deformed.size > 0
    err = np.abs(ref.vorticity(c.ctx, u, v) - 2.0)
    assert (err <= ref.vorticity_bound(c.ctx, u, v)).all(), (err / ref.vorticity_bound(c.ctx, u, v)).max()


def test_driver_kernels_use_no_scratch_and_at_most_64k_of_lds(tmp_path):
    """Every instance of the driver kernels (run-time Np: the dt kernels serve orders 1 to 8 with one instance each, the output
    kernel with one per LDS size class, with and without the lattice) reports ScratchSize 0, and the output kernel at most
    64 KB of LDS (in the manner of test_quad_high_order.test_output_kernel_uses_no_scratch_at_orders_9_to_12)."""
    hip = os.path.join(ROOT, "blitzdg_amd", "csrc", "hip")
    lines = ['#include "sw2d_curved_driver_kernel.hpp"', "namespace bdg_dev {",
             *[f"template __global__ void sw2d_curved_output_kernel<{lat}, {cls}>(CurvedOutParams);"
               for lat in ("true", "false") for cls in (15, 28, 45)], "}",
             # the two dt kernels are not templates: referenced, so that they are emitted
             "void* bdg_curved_driver_instances[] = {(void*)bdg_dev::sw2d_curved_dt_kernel, (void*)bdg_dev::sw2d_curved_dt_finish_kernel};"]
    src = tmp_path / "curved_driver_instances.hip"
    src.write_text("\n".join(lines) + "\n")
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + hip, "--cuda-device-only", "-S", str(src),
           "-o", str(tmp_path / "curved_driver_instances.s"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    report = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        if "sw2d_curved_" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))  # noqa: E731
        report[name] = (get(r" VGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"Occupancy \[waves/SIMD\]"),
                        get(r"LDS Size \[bytes/block\]"))
    for key in sorted(report):
        print(key, "VGPRs %d scratch %d occupancy %d LDS %d" % report[key])
    out = [k for k in report if "output_kernel" in k]
    assert len(out) == 6 and len(report) == 8, sorted(report)
    assert all(v[1] == 0 for v in report.values()), report
    assert all(0 < report[k][3] <= 64 * 1024 for k in out), report
    assert sorted(report[k][3] for k in out) == sorted(2 * [2 * cls * 512 for cls in (15, 28, 45)])
