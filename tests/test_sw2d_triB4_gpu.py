"""Variant B with a passive tracer on the triangle solver (bdg_sw2d_enable_variant_b4, the tracer pass of
csrc/hip/sw2d_vb_tracer_kernel.hpp behind the three-field variant-B launches) against tests/trirefB4.py.

The problem is conftest.variant_b_setup on buildBoxMesh(13, 11) -- K = 286: more than one 64-lane workgroup, ragged against 64
and against 16; the left edge open (its nodes stay in the wall list too), sloping bed, drag, Coriolis, a time where the tide is
not zero -- with a tracer that jumps at every face and an open-boundary concentration that is a scalar or one distinct value per
node (a wrong slot would show). Orders 1 to 8 on straight-sided tables (flags = 0: the unrolled form at N <= 4, the general form
on 13 numbers per element above) and on per-node tables (NODAL_GEOMETRY: the general form, the filter as a second pass). Per
(order, geometry):

  test_rhs_and_speed      RHS (per-node and scalar Nopen) and Filter . RHS, globalSpeed; components 1-3 equal the three-field
                          solver's bit for bit                                                          RHS_TOL per field
  test_heun_steps         3 Heun steps with the sponge array (per-node Nopen), 3 with a scalar sponge (scalar Nopen)   STATE_TOL
  test_lserk4_stages      7 stages as 4 + 3: frozen tide, time advanced after the fifth                  STATE_TOL
  test_rk2_filter_steps   2 midpoint-RK2 + filter steps                                                  STATE_TOL

then a renumbered mesh (the per-node table goes through the element permutation), a uniform concentration over a bed that jumps
at every face, tracer mass in a closed basin, the monitor and the output step, a mesh smaller than a tile, and the refusals.
Tolerances are the project's: one RHS 1e-12 of max|field|, stepped states 1e-11 (tests/test_triB4_reference.py: the float64
definition is within 2.5e-13 of its longdouble evaluation). References are computed once per order and shared by the geometry
forms.

Measured on one MI355X: largest RHS error 1.2e-13 (N = 8, straight-sided; the tracer's own 6.0e-14), largest state error 3.5e-14
(N = 8, three Heun steps); per-node form at most 4.8e-15; the global speed exact; max|hN / h - c| 3.9e-16 over the jumping bed;
83 tests in 2.4 s."""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import nonaffine_cases as na
import quadmon_ref as mon
import trimon_ref as tri
import trirefB4 as T
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2d
from conftest import relmax, tables_from_nodes
from oracle import oracle_np as onp
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
G = 9.81
ORDERS = tuple(range(1, 9))
FORMS = {"affine": 0, "nodal": sw2d.NODAL_GEOMETRY}
N_SCALAR = 0.55
SPONGE_SCALAR = 1e-3

cases = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

_PROBLEM, _REF = {}, {}


def box(nx=13, ny=11, seed=0):
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny, shuffleSeed=seed)
    return m


def problem(order, nx=13, ny=11, seed=0):
    """(nodes, tables, extras, q of four fields, p for the steppers of trirefB4, sponge array, dt)."""
    key = (order, nx, ny, seed)
    if key not in _PROBLEM:
        nodes, t, ex, q, p = T.problem(order, box(nx, ny, seed), seed=order, g=G)
        assert abs(onp.tide_elevation(ex["time"])) > 0.1
        sp = onp.build_sponge_coeff(t, p["mapO"], 2e-3, 0.6)
        assert sp.max() > 0
        lam = T.global_speed(*q[:3], p["H"], G, ex["time"], t, p["mapO"])
        dt = 0.1 * (2.0 / max(nx, ny)) / ((order + 1) ** 2 * lam)
        _PROBLEM[key] = (nodes, t, ex, q, p, sp, dt)
    nodes, t, ex, q, p, sp, dt = _PROBLEM[key]
    return nodes, t, ex, [a.copy() for a in q], p, sp, dt


def solver(order, flags, tracer, fields=4, sponge=False, **kw):
    nodes, t, ex, q, p, sp, dt = problem(order, **kw)
    s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=flags, fields=fields)
    s.enableVariantB(p["H"], p["Hx"], p["Hy"], mapO=p["mapO"], CD=p["CD"], f=p["f"], sponge=sp if sponge else None,
                     **({"tracer": tracer} if fields == 4 else {}))
    assert s.usesAffineGeometry == (not flags & sw2d.NODAL_GEOMETRY)
    s.time = ex["time"]
    return s


def reference(order, what, **kw):
    key = (order, what, tuple(sorted(kw.items())))
    if key not in _REF:
        nodes, t, ex, q, p, sp, dt = problem(order, **kw)
        time = ex["time"]
        pn, ps = p, dict(p, tracer=N_SCALAR)
        a3 = (p["H"], p["Hx"], p["Hy"], G, p["f"], p["CD"], time, t, p["mapO"])
        if what == "rhs":
            r = T.rhsB4(*q, *a3, p["tracer"], return_speed=True)
            rs = T.rhsB4(*q, *a3, N_SCALAR)
            _REF[key] = (list(r[:4]), [t["Filter"] @ a for a in r[:4]], r[4], list(rs))
        elif what == "heun":
            a, ta = T.heun_steps(q, pn, dt, 3, time=time, sponge=sp)
            b, _ = T.heun_steps(q, ps, dt, 3, time=time, sponge=SPONGE_SCALAR)
            _REF[key] = (a, b, ta)
        elif what == "lserk":
            a, _, ta = T.lserk4_stages(q, pn, dt, 7, time=time)
            _REF[key] = (a, ta)
        else:
            a, ta = T.rk2_steps(q, ps, dt, 2, time=time, filt=True)
            _REF[key] = (a, ta)
        assert all(np.isfinite(a).all() for a in _REF[key][0])
    return _REF[key]


@cases
def test_rhs_and_speed(order, form):
    flags = FORMS[form]
    _, _, ex, q, p, _, _ = problem(order)
    plain, filtered, lam, plain_scalar = reference(order, "rhs")
    assert relmax(plain[3], plain_scalar[3]) > 1e-6 and len(set(p["tracer"])) == len(p["tracer"])   # the two forms of Nopen differ
    s = solver(order, flags, p["tracer"])
    got = s.computeRHS4(*q)
    errs = assert_fields_close(got, plain, RHS_TOL, what="RHS")
    got_lam = s.globalSpeed
    errs += assert_fields_close(s.computeRHS4(*q, filter=True), filtered, RHS_TOL, what="Filter . RHS")
    assert abs(got_lam - lam) <= RHS_TOL * lam
    assert s.time == ex["time"]
    s.close()
    s3 = solver(order, flags, None, fields=3)
    for a, b in zip(got[:3], s3.computeRHS(*q[:3])):
        assert np.array_equal(a, b)                    # the three-field launches are the three-field solver's
    s3.close()
    s = solver(order, flags, N_SCALAR)
    errs += assert_fields_close(s.computeRHS4(*q), plain_scalar, RHS_TOL, what="RHS, scalar Nopen")
    s.close()
    print(f"N{order} {form}: " + " ".join(f"{e:.2e}" for e in errs) + f" speed {abs(got_lam - lam) / lam:.2e}")


@cases
def test_heun_steps(order, form):
    flags = FORMS[form]
    _, _, _, q, p, _, dt = problem(order)
    with_array, with_scalar, t_end = reference(order, "heun")
    errs = []
    for sponge, tracer, ref in ((True, p["tracer"], with_array), (False, N_SCALAR, with_scalar)):
        s = solver(order, flags, tracer, sponge=sponge)
        s.setState4(*q)
        s.stepSSPRK2(dt, 1, sponge=SPONGE_SCALAR)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)
        got = s.getState4()
        assert relmax(got[1], q[1]) > 1e-5 and relmax(got[3], q[3]) > 1e-5              # the state moved, the tracer too
        errs += assert_fields_close(got, ref, STATE_TOL, what=f"Heun, sponge {'array' if sponge else 'scalar'}")
        assert abs(s.time - t_end) <= 1e-12 * t_end
        s.close()
    assert relmax(with_array[1], with_scalar[1]) > 1e-9                                 # the two sponges differ
    print(f"N{order} {form} heun: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_lserk4_stages(order, form):
    _, _, ex, q, p, _, dt = problem(order)
    ref, t_end = reference(order, "lserk")
    s = solver(order, FORMS[form], p["tracer"])
    s.setState4(*q)
    s.lserk4Stages(dt, 4)
    assert s.time == ex["time"]                                                         # the tide is frozen inside a step
    s.lserk4Stages(dt, 3)
    got = s.getState4()
    assert relmax(got[1], q[1]) > 1e-5 and relmax(got[3], q[3]) > 1e-5
    errs = assert_fields_close(got, ref, STATE_TOL, what="7 LSERK4 stages")
    assert abs(s.time - t_end) <= 1e-12 * t_end and t_end > ex["time"]
    print(f"N{order} {form} lserk: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@cases
def test_rk2_filter_steps(order, form):
    _, _, _, q, _, _, dt = problem(order)
    ref, t_end = reference(order, "rk2")
    s = solver(order, FORMS[form], N_SCALAR)
    s.setState4(*q)
    s.stepRK2(dt, 2, filter=True)
    got = s.getState4()
    assert relmax(got[1], q[1]) > 1e-5 and relmax(got[3], q[3]) > 1e-5
    errs = assert_fields_close(got, ref, STATE_TOL, what="2 RK2 + filter steps")
    assert abs(s.time - t_end) <= 1e-12 * t_end
    print(f"N{order} {form} rk2: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [2, 4, 6])
def test_renumbered_mesh(order, form):
    """A shuffled box, renumbered on the device: the per-node concentrations go through the element permutation as the
    open-boundary bit masks do."""
    kw = dict(seed=11)
    _, _, _, q, p, _, dt = problem(order, **kw)
    plain = reference(order, "rhs", **kw)[0]
    s = solver(order, FORMS[form] | sw2d.REORDER, p["tracer"], **kw)
    assert s.isRenumbered
    errs = assert_fields_close(s.computeRHS4(*q), plain, RHS_TOL, what="RHS, renumbered")
    s.setState4(*q)
    s.lserk4Stages(dt, 7)
    errs += assert_fields_close(s.getState4(), reference(order, "lserk", **kw)[0], STATE_TOL, what="7 LSERK4 stages, renumbered")
    print(f"N{order} {form} renumbered: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [2, 4, 6])
def test_a_uniform_concentration_stays_uniform_over_a_bed_that_jumps(order, form):
    """H constant per element (it jumps at every face), hN = c h and Nopen = c: after 10 LSERK4 stages and 2 Heun steps of a
    moving state hN / h is c to 1e-12; with another Nopen it is not."""
    nodes, t, ex, q, p, _, _ = problem(order)
    K = t["x"].shape[1]
    H = np.tile(9.0 + 3.0 * np.random.default_rng(4).random(K), (t["x"].shape[0], 1))
    zero = 0 * H
    c = 0.37
    h = H + (q[0] - p["H"])
    assert np.abs(H.ravel("F")[t["vmapM"]] - H.ravel("F")[t["vmapP"]]).max() > 0.1
    dev = {}
    for n_open in (c, c + 0.4):
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=FORMS[form], fields=4)
        s.enableVariantB(H, zero, zero, mapO=p["mapO"], CD=p["CD"], f=p["f"], tracer=n_open)
        s.time = ex["time"]
        s.setState4(h, q[1], q[2], c * h)
        dt = 0.2 * s.computeDt(0.5)[0]
        s.lserk4Stages(dt, 10)
        s.stepSSPRK2(dt, 2, False, SPONGE_SCALAR)
        hh, hu, _, hN = s.getState4()
        assert relmax(hh, h) > 1e-6 and relmax(hu, q[1]) > 1e-5                        # a moving state
        dev[n_open] = np.abs(hN / hh - c).max()
        s.close()
    print(f"N{order} {form}: max|hN / h - c| {dev[c]:.2e} (Nopen = c), {dev[c + 0.4]:.2e} (Nopen = c + 0.4)")
    assert dev[c] <= 1e-12
    assert dev[c + 0.4] > 1e-6


class _Basin:
    """What tests/nonaffine_cases.midpoint_rk2 steps: trirefB4.rhsB4 on a closed basin."""

    def __init__(self, p):
        self.p = p

    def evaluate(self, q, time, filt, ld):
        assert not filt and not ld
        p = self.p
        return list(T.rhsB4(*q, p["H"], p["Hx"], p["Hy"], G, p["f"], p["CD"], time, p["t"], (), 0.0))


def test_tracer_mass_is_conserved_in_a_closed_basin():
    """Walls on every side of a 9 x 7 box, N = 4, 20 unfiltered RK2 steps with the monitor on. tests/test_sw2d_monitor_gpu.py holds
    the drift of int h to 4 x the drift of the float64 CPU reference plus the summation bound of one sample (it names no
    constant for it); int hN is held to the same expression with the tracer's own reference drift and summation bound."""
    na.require_extended_precision()
    steps, dt = 20, 2e-4
    nodes = dg.TriangleNodesProvisioner(4, box(9, 7))
    nodes.buildFilter(0.9 * 4, 4)
    t = tables_from_nodes(nodes)
    assert t["mapW"].size == 2 * (9 + 7) * 5                                       # walls on every side
    ex = dict(CD=2.5e-3, f=1.0070e-4)
    x, y = t["x"], t["y"]
    H = 12.0 + 1.5 * x - 0.8 * y * y + 0.3 * np.sin(3 * x) * np.cos(2 * y)
    Hx, Hy = onp.bed_slopes(H, t)
    h = H + 0.3 * np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    q0 = [h, 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1), h * (0.5 + 0.4 * np.sin(2 * x) * np.cos(3 * y))]
    p = dict(H=H, Hx=Hx, Hy=Hy, f=ex["f"], CD=ex["CD"], t=t)
    w = nodes.quadratureWeights()
    wl = np.asarray(w, dtype=mon.LD)
    total = lambda q: (wl * np.asarray(q[3], dtype=mon.LD)).sum()
    case, q, m0, ref_drift = _Basin(p), q0, total(q0), 0.0
    for _ in range(steps):
        q, _ = na.midpoint_rk2(case, q, dt, 1, False, ld=False)
        ref_drift = max(ref_drift, abs(float(total(q) - m0)))
    summation = mon.integral_bounds(mon.record_ld(w, q0, G, H))["tracer"]
    s = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    s.enableVariantB(H, Hx, Hy, CD=ex["CD"], f=ex["f"], tracer=0.0)
    s.enableMonitor(nodes, stride=1, capacity=steps + 1)
    s.setState4(*q0)
    s.sampleMonitor()
    s.stepRK2(dt, steps, filter=False)
    rec = s.monitorRecords()
    assert rec["tracer"].shape == (steps + 1,) and rec["nan"].max() == 0
    drift = np.abs(rec["tracer"] - rec["tracer"][0]).max()
    print(f"tracer drift over {steps} steps: {drift:.3e}; float64 CPU reference {ref_drift:.3e}; summation bound {summation:.3e}")
    assert relmax(s.getState4()[3], q0[3]) > 1e-6
    assert drift <= 4 * ref_drift + summation
    s.close()


@pytest.mark.parametrize("order,stride", [(4, 3), (6, 1)])
def test_monitor_and_output_carry_the_tracer(order, stride):
    """After tests/test_sw2d_monitor_gpu.py::test_records_taken_during_heun_steps_of_variant_b: int hN and the gauge N recorded
    during Heun steps against the same quantities of getState4(), within the monitor's own bounds; outputTracer is hN / h."""
    na.require_extended_precision()
    nodes, t, ex, q, p, _, dt = problem(order, 9, 7)
    gauges = tri.gauge_points(t["x"].shape[1], 5, 3, 1)
    rows = nodes.interpolationRows(gauges[1], gauges[2])
    s = solver(order, 0, p["tracer"], nx=9, ny=7)
    s.enableMonitor(nodes, gauges=gauges, stride=stride)                   # no H: the variant-B solver's own
    s.setState4(*q)
    s.stepSSPRK2(dt, 6)
    recs = s.monitorRecordArray()
    assert recs.shape[0] == 6 // stride and recs[-1, 0] == s.time
    final = s.getState4()
    tri.check_record(recs[-1], nodes.quadratureWeights(), final, G, p["H"], 4, gauges=(gauges[0], rows), Np=t["x"].shape[0])
    conc = s.outputTracer()
    assert np.abs(conc - final[3] / final[0]).max() <= 2.0 ** -52 * np.abs(conc).max()  # one division (or reciprocal and product)
    assert relmax(final[3], q[3]) > 1e-6
    s.close()


@pytest.mark.parametrize("order,form", [(1, "affine"), (3, "nodal"), (5, "affine")])
def test_mesh_smaller_than_a_tile(order, form):
    """buildBoxMesh(2, 2): K = 8 < 64 (and < 16)."""
    kw = dict(nx=2, ny=2)
    _, t, ex, q, p, _, dt = problem(order, **kw)
    assert t["x"].shape[1] == 8 and p["mapO"].size > 0
    s = solver(order, FORMS[form], p["tracer"], **kw)
    assert_fields_close(s.computeRHS4(*q), reference(order, "rhs", **kw)[0], RHS_TOL, what="RHS")
    s.setState4(*q)
    s.lserk4Stages(dt, 7)
    assert_fields_close(s.getState4(), reference(order, "lserk", **kw)[0], STATE_TOL, what="7 LSERK4 stages")
    s.close()


def test_refusals_leave_the_solvers_usable():
    order = 2
    nodes, t, ex, q, p, _, _ = problem(order)
    a3 = (p["H"], p["Hx"], p["Hy"])
    want4 = reference(order, "rhs")[0]
    E = C.BDG_ERR_ARGUMENT
    mo = np.ascontiguousarray(p["mapO"], dtype=np.int32)
    desc = C.Sw2dVbDesc(C.ptr(a3[0]), C.ptr(a3[1]), C.ptr(a3[2]), C.ptr(mo), mo.size, p["CD"], p["f"], 3.0, 3600 * 12.42, 0.15 / 3600, None)
    per_node = np.ascontiguousarray(p["tracer"])
    # a three-field solver: ValueError from Python, BDG_ERR_ARGUMENT from the library; it stays a variant-A solver
    s3 = sw2d.Sw2dSolver(nodes=nodes, g=G)
    plain3 = s3.computeRHS(*q[:3])
    with pytest.raises(ValueError):
        s3.enableVariantB(*a3, mapO=mo, tracer=0.5)
    assert C.lib.bdg_sw2d_enable_variant_b4(s3._h, C.byref(desc), C.ptr(per_node), mo.size) == E
    assert b"bdg_sw2d_enable_variant_b4" in C.lib.bdg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(plain3, s3.computeRHS(*q[:3])))
    s3.close()
    # a solver with sources
    src = dict(zx=0 * q[0], zy=0 * q[0], f=1e-4, CD=1e-3)
    ss = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4, sources=src)
    with pytest.raises(C.BdgError) as e:
        ss.enableVariantB(*a3, mapO=mo, tracer=0.5)
    assert e.value.code == E
    with_sources = ss.computeRHS4(*q)
    assert all(np.isfinite(a).all() for a in with_sources)
    ss.close()
    # bad counts, NULL n_open, NULL descriptor on a live four-field handle; wrong lengths through Python
    s4 = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    for bad in (np.ones(2), np.ones(mo.size + 1), np.ones((mo.size, 1))):
        with pytest.raises(ValueError):
            s4.enableVariantB(*a3, mapO=mo, tracer=bad)
    big = np.ones(mo.size + 1)
    for n_open, count in ((C.ptr(big), 2), (C.ptr(big), mo.size + 1), (C.ptr(big), 0), (C.ptr(big), -1), (None, 1), (None, mo.size)):
        assert C.lib.bdg_sw2d_enable_variant_b4(s4._h, C.byref(desc), n_open, count) == E
    assert C.lib.bdg_sw2d_enable_variant_b4(s4._h, None, C.ptr(big), 1) == E
    with pytest.raises(C.BdgError):
        s4.globalSpeed                                                           # variant B was not enabled by any of these
    with pytest.raises(C.BdgError):
        s4.enableVariantB(*a3, mapO=mo)                                          # without tracer: refused as before
    assert b"tracer / variant-D sources" in C.lib.bdg_last_error()
    # ... and then the call that is right goes through, once
    s4.enableVariantB(*a3, mapO=mo, CD=p["CD"], f=p["f"], tracer=per_node)
    s4.time = ex["time"]
    assert_fields_close(s4.computeRHS4(*q), want4, RHS_TOL, what="after the refusals")
    for again in (0.25, per_node):                                               # a second call, scalar or per node
        with pytest.raises(C.BdgError) as e:
            s4.enableVariantB(*a3, mapO=mo, tracer=again)
        assert e.value.code == E
    assert_fields_close(s4.computeRHS4(*q), want4, RHS_TOL, what="after a second call")
    s4.close()
    # a closed basin: a count of 0 with NULL n_open is accepted
    s5 = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    closed = C.Sw2dVbDesc(C.ptr(a3[0]), C.ptr(a3[1]), C.ptr(a3[2]), None, 0, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    assert C.lib.bdg_sw2d_enable_variant_b4(s5._h, C.byref(closed), None, 0) == 0
    assert all(np.isfinite(a).all() for a in s5.computeRHS4(*q))
    s5.close()
    # after the first evaluation: refused, and the solver goes on as the four-field solver without sources it was
    s6 = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    before = s6.computeRHS4(*q)
    with pytest.raises(C.BdgError) as e:
        s6.enableVariantB(*a3, mapO=mo, tracer=0.5)
    assert e.value.code == E
    assert all(np.array_equal(a, b) for a, b in zip(before, s6.computeRHS4(*q)))
    s6.close()
