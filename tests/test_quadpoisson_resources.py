"""Register and LDS use of the elliptic operator's passes and of the mass product on quadrilaterals
(csrc/hip/poisson2d_quad_kernel.hpp), from the compiler's own report: the twin of tests/test_poisson2d_resources.py.
poisson2d_quad_order.hip is cross-compiled for gfx950, device side only, with -Rpass-analysis=kernel-resource-usage at orders
1..12; no GPU. The numbers themselves are recorded in DESIGN.md 3.13; what is held here is the instance set -- the gradient pass
plain, with data and with the direction update fused in, the divergence pass with and without data, the mass product --,
ScratchSize = 0, at most 256 VGPRs, an occupancy of at least one wave per SIMD and at most 64 KB of LDS for each of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "blitzdg_amd", "csrc", "hip")


def resource_usage(order, out):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", f"-DBDG_ORDER={order}",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "blitzdg_amd", "csrc", "host"), "-I" + HIP,
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(HIP, "poisson2d_quad_order.hip"),
           "-o", str(out)]
    run = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    kernels = {}
    for block in run.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        kernels[name] = {key: int(value) for key, value in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", block)}
    return kernels


@pytest.mark.parametrize("order", range(1, 13))
def test_no_instance_of_the_quadrilateral_elliptic_passes_uses_scratch(order, tmp_path):
    kernels = resource_usage(order, tmp_path / "poisson2d_quad.o")
    forms = {"gradient": 0, "divergence": 0, "mass": 0}
    for name, use in kernels.items():
        assert "poisson2d_quad_" in name, name
        forms["gradient" if "quad_gradient" in name else ("mass" if "quad_mass" in name else "divergence")] += 1
        assert use["ScratchSize"] == 0, (name, use)
        assert use["VGPRs"] <= 256 and use["Occupancy"] >= 1, (name, use)
        assert use["LDS Size"] <= 64 * 1024, (name, use)
    assert forms == {"gradient": 3, "divergence": 2, "mass": 1}, sorted(kernels)
    print(f"N{order}: " + "; ".join(f"{n[12:50]} VGPRs {u['VGPRs']} occ {u['Occupancy']} LDS {u['LDS Size']}" for n, u in sorted(kernels.items())))
