"""CPU side of the quadrilateral sw2d path at orders 9 to 12 (tiles of 8 elements, csrc/hip/sw2d_quad_kernel.hpp).

  * The N = 10 fixtures (tests/golden/make_golden_quads_high_order.py: the reference's sw2dquads.sw2dComputeRHS and
    swhelpers.rhs.sw2dComputeRHS on coarse_box_quads.msh with this repository's tables) are reproduced by the float64
    restatements and by the longdouble reference to 1e-12 per field, the bound of test_quad_setup.py.
  * The float64 restatement stays within LD_TOL = 2.5e-13 per field of the longdouble one (a quarter of the 1e-12 the GPU is
    held to) at orders 9 to 12 on both 13 x 11 meshes, all four regimes, three field sets, plain and filtered. Measured maxima
    over both meshes (the test prints them per regime): N = 9 8.6e-15, N = 10 9.2e-15, N = 11 8.8e-15, N = 12 9.7e-15 (deep
    regime each time; the other regimes stay below 2.5e-15), so no order needs a wider GPU tolerance than 1e-12.
  * Mesh checks: the shear mesh passes the solver's parallelogram test, the jitter mesh fails it, K = 143 is ragged for the
    tiles of 8 and 16, and the provisioner's tables have the tensor form that tensorOperators (csrc/host/element_tables.cpp) demands.
  * bdg_sw2dq_create refuses orders 0 and 13 before it touches a device, and says 1..12.
  * sw2d_quad_output_kernel<9..12> compiled alone: no scratch, 512 (N+1)^2 bytes of LDS with the lattice, none without.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import quadref
import quadref4
import quadref_ld as Q
from blitzdg_amd import _capi as C
from regimes import REGIMES, assert_fields_close
from test_quad_reference_ld import LD_TOL, _spreads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (9, 10, 11, 12)
FIXTURE = "coarse_box_quads_N10"

assert LD_TOL == 2.5e-13


# ---- 1. the reference's own results at N = 10

def test_three_field_fixture_is_reproduced_in_float64_and_longdouble():
    d, _, _, ctx = quadref.load_fixture(FIXTURE)
    assert int(d["order"]) == 10 and d["h"].shape == (121, 16)
    assert sorted(d.files) == sorted(["EToV", "Vert", "order", "g", "h", "hu", "hv", "rhs1", "rhs2", "rhs3"])
    t = quadref.tables(ctx)
    ref = [d[f"rhs{i}"] for i in (1, 2, 3)]
    e64 = assert_fields_close(quadref.rhs(d["h"], d["hu"], d["hv"], float(d["g"]), t), ref, 1e-12, what="float64")
    got = Q.rhs_ld([d["h"], d["hu"], d["hv"]], float(d["g"]), Q.to_ld(t))
    assert all(a.dtype == Q.LD for a in got)
    eld = assert_fields_close(Q.f64(got), ref, 1e-12, what="longdouble")
    print("N=10 three fields: float64 " + " ".join(f"{e:.2e}" for e in e64) + "; longdouble " + " ".join(f"{e:.2e}" for e in eld))


def test_four_field_fixture_is_reproduced_in_float64_and_longdouble():
    d, _, _, ctx = quadref4.load_fixture4(FIXTURE)
    assert int(d["order"]) == 10 and d["h"].shape == (121, 16) and d["f"].shape == (121, 16)
    t = quadref.tables(ctx)
    src = quadref4.sources(d)
    e64 = assert_fields_close(quadref4.rhs4(*quadref4.state(d), float(d["g"]), t, **src), quadref4.reference(d), 1e-12,
                              what="float64")
    got = Q.rhs_ld(quadref4.state(d), float(d["g"]), Q.to_ld(t), src)
    assert all(a.dtype == Q.LD for a in got)
    eld = assert_fields_close(Q.f64(got), quadref4.reference(d), 1e-12, what="longdouble")
    print("N=10 four fields: float64 " + " ".join(f"{e:.2e}" for e in e64) + "; longdouble " + " ".join(f"{e:.2e}" for e in eld))


# ---- 2. float64 against longdouble

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mesh", Q.MESHES)
def test_float64_restatement_is_within_a_quarter_of_the_gpu_tolerance(mesh, order):
    _, t = Q.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    F = t["Filter"]
    worst = {}
    for regime in REGIMES:
        for fs in Q.FIELD_SETS:
            fields, src = Q.field_set(t, fs)
            q = Q.state(t, fields, regime, seed=order)
            r64 = quadref.rhs(*q, Q.G, t) if fields == 3 else quadref4.rhs4(*q, Q.G, t, **(src or {}))
            assert all(a.dtype == np.float64 for a in r64)
            for filt in (False, True):
                ref = Q.f64(Q.rhs_ld(q, Q.G, tl, src, filt))
                got = [F @ a for a in r64] if filt else r64
                # (measured first, asserted after the line below is printed)
                errs = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(got, ref)]
                worst[regime] = max(worst.get(regime, 0.0), max(errs))
    print(f"float64 against longdouble, {mesh} N={order}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= LD_TOL, worst


# ---- 3. meshes and tables

@pytest.mark.parametrize("order", ORDERS)
def test_shear_mesh_is_a_parallelogram_mesh_to_the_solver(order):
    _, t = Q.mesh_tables("shear", order)
    metric, face = _spreads(t)
    print(f"shear N={order}: metric spread {metric:.2e}, face spread {face:.2e}")
    assert metric < 1e-11 and face < 1e-11            # the solver's test asks 1e-10
    assert min(np.abs(t[k]).min() for k in ("rx", "sx", "ry", "sy")) > 1.0       # oblique: no metric term vanishes
    assert min(np.abs(t["nx"]).min(), np.abs(t["ny"]).min()) > 0.19


@pytest.mark.parametrize("order", ORDERS)
def test_jitter_mesh_is_refused_by_the_parallelogram_test(order):
    _, t = Q.mesh_tables("jitter", order)
    metric, face = _spreads(t)
    assert metric > 1e-3 and face > 1e-3


@pytest.mark.parametrize("mesh", Q.MESHES)
def test_meshes_are_ragged_at_the_tiles_of_8_and_16(mesh):
    E, _ = Q.mesh_arrays(mesh)
    K = len(E)
    assert K == 143 and K % 8 == 7 and K % 16 == 15
    assert -(-K // 8) >= 3 and -(-K // 16) >= 3


def tensor_form_errors(t):
    """tensorOperators of csrc/host/element_tables.cpp in NumPy: (errD, tolD, errL, tolL)."""
    Nq = t["order"] + 1
    Dr, Ds, L = t["Dr"], t["Ds"], t["Lift"]
    D1 = Dr[::Nq, ::Nq]                               # D1[j, m] = Dr[Nq j, Nq m]
    l0, lN = L[:Nq, 0], L[::Nq, Nq]                   # face 0 at j = 0; face 1 at i = 0
    I = np.eye(Nq)
    errD = max(np.abs(Dr - np.kron(D1, I)).max(), np.abs(Ds - np.kron(I, D1)).max())
    faces = np.hstack([np.kron(I, l0[:, None]), np.kron(lN[:, None], I), np.kron(I, lN[:, None]), np.kron(l0[:, None], I)])
    errL = np.abs(L - faces).max()
    return errD, 1e-13 * max(np.abs(Dr).max(), np.abs(Ds).max()), errL, 1e-13 * np.abs(L).max()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mesh", Q.MESHES)
def test_provisioner_tables_have_the_tensor_form(mesh, order):
    _, t = Q.mesh_tables(mesh, order)
    Nq = order + 1
    assert t["Dr"].shape == (Nq * Nq, Nq * Nq) and t["Lift"].shape == (Nq * Nq, 4 * Nq) and t["Filter"].shape == t["Dr"].shape
    errD, tolD, errL, tolL = tensor_form_errors(t)
    print(f"{mesh} N={order}: Dr/Ds deviation {errD:.2e} (tolerance {tolD:.2e}), Lift {errL:.2e} ({tolL:.2e})")
    assert errD <= tolD and errL <= tolL


# ---- 4. refusals (the order is checked before any table or device is touched)

@pytest.mark.parametrize("order", [0, 13, -1, 100])
@pytest.mark.parametrize("fields", [3, 4])
def test_create_refuses_orders_outside_1_to_12(order, fields):
    desc = C.Sw2dqDesc()
    desc.order, desc.num_elements = order, 16
    out = ctypes.c_void_p()
    if fields == 3:
        rc = C.lib.bdg_sw2dq_create(ctypes.byref(desc), ctypes.byref(out))
    else:
        rc = C.lib.bdg_sw2dq_create_fields(ctypes.byref(desc), 4, ctypes.byref(out))
    assert rc == C.BDG_ERR_ARGUMENT and not out.value
    msg = C.lib.bdg_last_error().decode()
    assert f"order {order}" in msg and "1..12" in msg, msg


@pytest.mark.parametrize("order", ORDERS)
def test_create_accepts_the_new_orders_as_far_as_the_tables(order):
    """Orders 9 to 12 pass the order check: with no tables the next refusal is the NULL table, not the order."""
    desc = C.Sw2dqDesc()
    desc.order, desc.num_elements = order, 16
    out = ctypes.c_void_p()
    assert C.lib.bdg_sw2dq_create(ctypes.byref(desc), ctypes.byref(out)) == C.BDG_ERR_ARGUMENT
    msg = C.lib.bdg_last_error().decode()
    assert "NULL table" in msg and "outside" not in msg, msg


# ---- 5. the output kernel alone

def test_output_kernel_uses_no_scratch_at_orders_9_to_12(tmp_path):
    """As test_quad_output.test_output_kernel_uses_no_scratch: a workgroup is N + 1 waves (832 threads at N = 12), a thread
    holds 3 (N + 1) doubles at the most, and the compiler reports zero scratch for all 16 instances."""
    hip = os.path.join(ROOT, "blitzdg_amd", "csrc", "hip")
    sig = "(const double*, const double*, const double*, double*, long long, int, int)"
    lines = ['#include "sw2d_quad_output_kernel.hpp"', "namespace bdg_dev {"]
    for n in ORDERS:
        for nf in (3, 4):
            for lat in ("true", "false"):
                lines.append(f"template __global__ void sw2d_quad_output_kernel<{n}, {nf}, {lat}>{sig};")
    lines.append("}")
    src = tmp_path / "quad_output_instances.hip"
    src.write_text("\n".join(lines) + "\n")
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + hip, "--cuda-device-only", "-S", str(src),
           "-o", str(tmp_path / "quad_output_instances.s"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    report = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_ZN7bdg_dev23sw2d_quad_output_kernelILi(\d+)ELi(\d)ELb(\d)EEE", blk)
        if not m:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))  # noqa: E731
        report[tuple(int(v) for v in m.groups())] = (get(r" VGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                                                    get(r"Occupancy \[waves/SIMD\]"), get(r"LDS Size \[bytes/block\]"))
    assert len(report) == 16 and {k[0] for k in report} == set(ORDERS), sorted(report)
    for key in sorted(report):
        print(key, "VGPRs %d scratch %d occupancy %d LDS %d" % report[key])
    assert all(v[1] == 0 for v in report.values()), {k: v for k, v in report.items() if v[1]}
    assert all(v[3] == (512 * (k[0] + 1) ** 2 if k[2] else 0) for k, v in report.items())
    assert report[12, 3, 1][3] == 86528


def test_create_refuses_zero_operators_of_an_allowed_order():
    """Dr = Ds = Lift = 0 would pass a tolerance of 1e-13 of their own largest entry; they are no element's operators."""
    order, K = 9, 4
    Np, nfn = (order + 1) ** 2, 4 * (order + 1)
    a = {"Dr": np.zeros((Np, Np)), "Ds": np.zeros((Np, Np)), "Lift": np.zeros((Np, nfn)),
         **{k: np.ones((Np, K)) for k in ("rx", "sx", "ry", "sy")}, **{k: np.ones((nfn, K)) for k in ("nx", "ny", "Fscale")}}
    vmapP = np.zeros(nfn * K, np.int32)
    desc = C.Sw2dqDesc()
    desc.order, desc.num_elements, desc.g = order, K, 9.81
    for k, v in a.items():
        setattr(desc, k, v.ctypes.data)
    desc.vmapP = vmapP.ctypes.data
    out = ctypes.c_void_p()
    assert C.lib.bdg_sw2dq_create(ctypes.byref(desc), ctypes.byref(out)) == C.BDG_ERR_ARGUMENT and not out.value
    msg = C.lib.bdg_last_error().decode()
    assert "identically zero" in msg and "order 9" in msg, msg
