"""Register use of variant B's tracer pass (csrc/hip/sw2d_vb_tracer_kernel.hpp), from the compiler's own report: no instance
may use scratch. sw2d_vb4_order.hip is cross-compiled for gfx950, device side only, with -Rpass-analysis=kernel-resource-usage
at every order; no GPU. The numbers themselves (VGPRs, waves per SIMD) are recorded in DESIGN.md 3.7; what is held here is the
instance set -- the unrolled form in three modes at N <= 4, the general form in three modes on both geometry forms and the filter
pass in three modes at every order -- and ScratchSize = 0 for each of them."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "blitzdg_amd", "csrc", "hip")


@pytest.mark.parametrize("order", range(1, 9))
def test_no_instance_of_the_tracer_pass_uses_scratch(order, tmp_path):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", f"-DBDG_ORDER={order}",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "blitzdg_amd", "csrc", "host"), "-I" + HIP,
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(HIP, "sw2d_vb4_order.hip"),
           "-o", str(tmp_path / "vb4.o")]
    run = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    kernels = {}
    for block in run.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        kernels[name] = {key: int(value) for key, value in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", block)}
    forms = {"unrolled": 0, "general": 0, "filter": 0}
    for name, use in kernels.items():
        forms["unrolled" if "tracer_unrolled" in name else ("filter" if "tracer_filter" in name else "general")] += 1
        assert use["ScratchSize"] == 0, (name, use)
        assert use["VGPRs"] <= 256 and use["Occupancy"] >= 1, (name, use)
    assert forms == {"unrolled": 3 if order <= 4 else 0, "general": 6, "filter": 3}, sorted(kernels)
