"""Child of tests/test_sw2d_curved_instances_gpu.py::test_process_switches: one case of tests/curved_cases.py in a fresh process,
so that the switches the library reads once per process (BDG_SW2D_CURVED_STREAM, BDG_SW2D_CURVED_WAVES) are those of this
process's environment from its first launch on.

    python tests/curved_instance_worker.py <case name> <out.npz>

Runs RHS +- filter, 2 RK2 steps +- filter and 5 LSERK4 stages from the case's fields and writes the results and kernelInfo()
to <out.npz>; the parent compares them with the cached reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import curved_cases as cc  # noqa: E402


def run(c, s):
    """The runs of one case on solver s: {name: 4 fields}."""
    dt = cc.step_size(c)
    out = {}
    for filt in (False, True):
        out[f"rhs{int(filt)}"] = s.computeRHS(*c.q, filter=filt)
        s.setState(*c.q)
        s.stepRK2(dt, 2, filter=filt)
        out[f"rk2{int(filt)}"] = s.getState()
    s.setState(*c.q)
    s.lserk4Stages(dt, 5)
    out["lserk"] = s.getState()
    return out


def main(name, path):
    c = cc.case(name)
    s = cc.solver(c)
    info = {filt: s.kernelInfo(filter=filt) for filt in (False, True)}   # before the first launch: the same static is read
    out = run(c, s)
    assert s.kernelInfo() == info[False] and s.kernelInfo(filter=True) == info[True]
    arrays = {f"{k}_{i}": a for k, fields in out.items() for i, a in enumerate(fields)}
    for filt, d in info.items():
        for k, v in d.items():
            arrays[f"info{int(filt)}_{k}"] = np.int64(-1 if v is None else v)
    np.savez(path, **arrays)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
