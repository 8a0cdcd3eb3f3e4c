"""tests/nonaffine_cases.py is what it claims to be (no GPU): the mesh has the element counts the per-node variant kernels
need, the bed jump and the sponges change the result, the float64 evaluation of each reference stays close to the longdouble
one, and the depth stays positive through every loop at the step sizes the GPU module uses.

Distance of the float64 evaluation of oracle_np.sw2d_rhs4 / sw2d_rhs_b from the longdouble one on these cases, per field and
relative to the field's size (printed by the tests below, sets B and D, orders 1..8): at most 6.5e-14 for one right-hand side
(N = 7, set D; set B stays below 6.0e-15) and 8.1e-14 for a state after 13 LSERK4 stages (N = 8, set D) -- a fifteenth and a
hundredth of the bounds of the GPU module."""
import numpy as np
import pytest

import nonaffine_cases as C
from conftest import relmax

RHS_TOL = 1e-12      # the GPU module's bounds
STATE_TOL = 1e-11
ORDERS = range(1, 9)


@pytest.mark.parametrize("order", ORDERS)
def test_case_table(order):
    C.require_extended_precision()
    t = C.case_tables(order)
    K = t["rx"].shape[1]
    Nfp = order + 1
    assert K > 256 and K % 256 != 0 and K % 64 != 0
    assert (K + 63) // 64 == 5 and K % 64 == 30 and (K + 255) // 256 == 2
    assert t["J"].min() > 0
    mapO = C.open_boundary_nodes(t)
    assert mapO.size > 0 and mapO.size % Nfp == 0
    assert set(mapO) <= set(t["mapW"])
    if order > 1:    # the deformed elements are not straight-sided: the metric varies within an element
        assert np.ptp(t["rx"], axis=0).max() > 1e-3
    v = C.variant_b_inputs(t)
    assert abs(C.onp.tide_elevation(v["time"])) > 0.1
    assert (v["sponge"] == 0).any() and (v["sponge"] > 0).any()
    hN = C.state(t, 4, "smooth", order)[3]
    jump = np.abs(hN.flatten("F")[t["vmapM"]] - hN.flatten("F")[t["vmapP"]])
    interior = np.asarray(t["vmapM"]) != np.asarray(t["vmapP"])
    assert (jump[interior] > 0).all()


@pytest.mark.parametrize("order", ORDERS)
def test_bed_jump_reaches_the_star_states(order):
    """hMstar = hM - max(0, HM - HP) (main.cpp:356-368): somewhere it differs from hM by more than 1e-3 of the depth."""
    c = C.make_case(order, "B")
    t, H = c.t, c.vb["H"]
    h = C.state(t, 3, "smooth", order)[0]
    HM, HP = H.flatten("F")[t["vmapM"]], H.flatten("F")[t["vmapP"]]
    hM = h.flatten("F")[t["vmapM"]]
    interior = np.asarray(t["vmapM"]) != np.asarray(t["vmapP"])
    assert (HM != HP)[interior].all(), "the bed does not jump at every interior face node"
    drop = np.maximum(0.0, HM - HP) / hM
    assert drop.max() > 1e-3
    assert (hM - np.maximum(0.0, HM - HP)).min() > 0


@pytest.mark.parametrize("fs", ["B", "D"])
@pytest.mark.parametrize("order", ORDERS)
def test_float64_reference_is_close_to_the_longdouble_one(order, fs):
    a, b = C.reference(order, fs, "rhs", ld=False), C.reference(order, fs, "rhs", ld=True)
    worst = 0.0
    for kind in ("smooth", "jumpy"):
        for filt in (False, True):
            worst = max(worst, max(relmax(x, y) for x, y in zip(a[kind, filt], b[kind, filt])))
    a, b = C.reference(order, fs, "lserk", ld=False), C.reference(order, fs, "lserk", ld=True)
    state = max(relmax(x, y) for x, y in zip(a[13], b[13]))
    print(f"N{order} {fs}: float64 to longdouble distance, RHS {worst:.2e}, 13 LSERK4 stages {state:.2e}")
    assert worst < 0.1 * RHS_TOL and state < 0.1 * STATE_TOL


@pytest.mark.parametrize("order", [2, 5])
def test_sponges_change_the_result(order):
    c = C.make_case(order, "B")
    q0 = C.state(c.t, 3, "smooth", order)
    dt = c.dt(q0)
    out = {name: C.f64(C.heun(c, q0, dt, 2, False, sp, c.time0)[0])
           for name, sp in (("none", None), ("scalar", C.SPONGE_SCALAR), ("array", c.vb["sponge"]))}
    for a, b in (("none", "scalar"), ("none", "array"), ("scalar", "array")):
        for i in (1, 2):
            assert relmax(out[a][i], out[b][i]) > 1e4 * STATE_TOL, (a, b, i)


@pytest.mark.parametrize("fs", C.SETS)
@pytest.mark.parametrize("order", ORDERS)
def test_depth_stays_positive_through_every_loop(order, fs):
    """Every loop asserts h > 0 at each intermediate state; here at the reference dt at CFL 0.65 (smooth) and a quarter of it
    (jumpy), as the GPU module runs them. The states also move by far more than the tolerance."""
    for what in ("lserk", "rk2", "ssprk2", "jumpy"):
        r = C.reference(order, fs, what)
        for key, val in r.items():
            if isinstance(val, list) and key not in ("q0", "qj", "q1"):
                assert val[0].min() > 0
                start = r["qj"] if what == "jumpy" else (r["q1"] if key == 7 else r["q0"])
                for a, b in zip(val, start):
                    assert relmax(a, b) > 1e4 * STATE_TOL, (what, key)
