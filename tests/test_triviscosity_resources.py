"""Register use of the eddy-viscosity passes (csrc/hip/sw2d_viscosity_kernel.hpp), from the compiler's own report: no instance may
use scratch. sw2d_viscosity_order.hip is cross-compiled for gfx950, device side only, with
-Rpass-analysis=kernel-resource-usage at every order; no GPU. The numbers themselves (VGPRs, waves per SIMD) are recorded in
DESIGN.md 3.7; what is held here is the instance set -- the gradient pass on both geometry forms, the divergence pass in three
modes on both geometry forms and once per geometry form writing the unfiltered terms, the filter step in three modes, the
reduction of max nu -- and ScratchSize = 0, VGPRs <= 256 and at least one wave per SIMD for each of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "blitzdg_amd", "csrc", "hip")


def resource_usage(order, out):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", f"-DBDG_ORDER={order}",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "blitzdg_amd", "csrc", "host"), "-I" + HIP,
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(HIP, "sw2d_viscosity_order.hip"),
           "-o", str(out)]
    run = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    kernels = {}
    for block in run.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        kernels[name] = {key: int(value) for key, value in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", block)}
    return kernels


@pytest.mark.parametrize("order", range(1, 9))
def test_no_instance_of_the_viscosity_passes_uses_scratch(order, tmp_path):
    kernels = resource_usage(order, tmp_path / "viscosity.o")
    forms = {"gradient": 0, "divergence": 0, "filter": 0, "max": 0}
    for name, use in kernels.items():
        form = next(f for f in forms if f"viscosity_{f}_kernel" in name)
        forms[form] += 1
        assert use["ScratchSize"] == 0, (name, use)
        assert use["VGPRs"] <= 256 and use["Occupancy"] >= 1, (name, use)
    assert forms == {"gradient": 2, "divergence": 8, "filter": 3, "max": 1}, sorted(kernels)
    print(f"N{order}: " + "; ".join(f"{n[:60]} VGPRs {u['VGPRs']} AGPRs {u.get('AGPRs', 0)} occ {u['Occupancy']}" for n, u in sorted(kernels.items())))
