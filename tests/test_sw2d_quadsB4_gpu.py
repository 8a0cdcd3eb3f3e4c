"""Variant B with a passive tracer on the quadrilateral solver (bdg_sw2dq_enable_variant_b4, sw2d_quadb4_stage_kernel) against
tests/quadrefB4.py in np.longdouble, rounded at the comparison.

The problems are tests/test_sw2d_quadsB_gpu.py's (13 x 11 box, K = 143, ragged against every tile size; sheared in both geometry
forms or jittered; the x = x_min side open, a bed that jumps at every face, drag, Coriolis, a time where the tide is not zero)
with a tracer that jumps at every face and an open-boundary concentration that is a scalar or one distinct value per node (a
wrong slot would show). Orders 1 to 12, every one a compiled object of its own: every tile size, the unrolled / rolled phase C
(N <= 6 / N >= 7), the filter from registers / streamed from LDS planes of its own (N <= 6 / N >= 7), the rolled flux-array loop
(N > 8). Per (order, form):

  test_rhs_and_speed      RHS (per-node and scalar Nopen) and Filter . RHS, globalSpeed()               RHS_TOL per field / relative
  test_heun_steps         3 Heun steps with the sponge array (per-node Nopen), 3 with a scalar sponge (scalar Nopen)   STATE_TOL
  test_lserk4_stages      7 stages as 4 + 3: frozen tide, time advanced after the fifth                  STATE_TOL
  test_rk2_filter_steps   2 midpoint-RK2 + filter steps                                                  STATE_TOL

then a uniform concentration over the jumping bed, tracer mass in a closed basin, the monitor and the output step, a mesh
smaller than a tile, and the refusals. Tolerances are the project's: one RHS 1e-12 of max|field|, stepped states 1e-11
(tests/test_quadB4_reference.py: the float64 definition is within 2.5e-13 of the longdouble one).
References are computed once per (order, mesh) and shared by the geometry forms.

Measured on one MI355X: largest RHS error 4.0e-13, largest state error 6.9e-13 (Heun), both at N = 12 in the parallelogram form
(of the orders 3, 5, 10, 11: RHS 2.3e-13 at N = 10, state 3.6e-13 at N = 11, Heun, the same form); per-node form at most
6.4e-14 (N = 12); global speed 1.6e-16 relative (N = 11); 157 tests in 36 s."""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadref
import quadref4
import quadref_ld as Q
import quadrefB as B
import quadrefB4 as B4
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2dquads
from conftest import relmax
from quadref4 import compute_dt
from regimes import assert_fields_close
from test_sw2d_quads_monitor_gpu import DRIFT_TOL
from test_sw2d_quadsB_gpu import CD, FCOR, FORMS, SPONGE_SCALAR, T0, TIDE, problem

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
ORDERS = tuple(range(1, 13))
N_SCALAR = 0.55

cases = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

_REF = {}


def problem4(mesh, order):
    """test_sw2d_quadsB_gpu.problem with the tracer: (nodes, tables, vb, sponge array, state of four fields, dt, per-node Nopen)."""
    nodes, t, vb, sp, q, dt = problem(mesh, order)
    hN = Q.tracer(q[0], t["x"], t["y"], seed=order)
    return nodes, t, vb, sp, list(q) + [hN], dt, B4.open_tracer(t)


def solver(order, form, tracer, sponge=False):
    mesh, general = FORMS[form]
    _, t, vb, sp, _, _, _ = problem4(mesh, order)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=B.G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=4)
    s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], mapO=vb["mapO"], CD=CD, f=FCOR, tide=TIDE, sponge=sp if sponge else None,
                     tracer=tracer)
    assert s.usesParallelogramGeometry == (form == "shear-auto") and s.K == 143
    return s


def reference(mesh, order, what):
    key = (mesh, order, what)
    if key not in _REF:
        Q.require_extended_precision()
        _, t, vb, sp, q, dt, per_node = problem4(mesh, order)
        tl, ql = Q.to_ld(t), B.to_ld(q)
        vn, vs = B4.vb_ld(dict(vb, tracer=per_node)), B4.vb_ld(dict(vb, tracer=N_SCALAR))
        if what == "rhs":
            r = B4.rhsB4(*ql, tl, vn, time=T0, return_speed=True)
            rs = B4.rhsB4(*ql, tl, vs, time=T0)
            _REF[key] = (Q.f64(r[:4]), Q.f64([tl["Filter"] @ a for a in r[:4]]), float(r[4]), Q.f64(rs))
        elif what == "heun":
            a, ta = B4.heun_steps(ql, tl, vn, dt, 3, time=T0, sponge_coeff=np.asarray(sp, dtype=B.LD))
            b, _ = B4.heun_steps(ql, tl, vs, dt, 3, time=T0, sponge_coeff=SPONGE_SCALAR)
            _REF[key] = (Q.f64(a), Q.f64(b), ta)
        elif what == "lserk":
            a, _, ta = B4.lserk4_stages(ql, tl, vn, dt, 7, time=T0)
            _REF[key] = (Q.f64(a), ta)
        else:
            a, ta = B4.rk2_steps(ql, tl, vs, dt, 2, time=T0, filt=True)
            _REF[key] = (Q.f64(a), ta)
        assert all(np.isfinite(a).all() for a in _REF[key][0])
    return _REF[key]


@cases
def test_rhs_and_speed(order, form):
    mesh = FORMS[form][0]
    q, per_node = problem4(mesh, order)[4], problem4(mesh, order)[6]
    plain, filtered, lam, plain_scalar = reference(mesh, order, "rhs")
    assert relmax(plain[3], plain_scalar[3]) > 1e-6 and len(set(per_node)) == len(per_node)     # the two forms of Nopen differ
    s = solver(order, form, per_node)
    s.setTime(T0)
    errs = assert_fields_close(s.computeRHS4(*q), plain, RHS_TOL, what="RHS")
    got_lam = s.globalSpeed()
    errs += assert_fields_close(s.computeRHS4(*q, filter=True), filtered, RHS_TOL, what="Filter . RHS")
    assert abs(got_lam - lam) <= RHS_TOL * lam
    assert s.getTime() == T0
    s.close()
    s = solver(order, form, N_SCALAR)
    s.setTime(T0)
    errs += assert_fields_close(s.computeRHS4(*q), plain_scalar, RHS_TOL, what="RHS, scalar Nopen")
    s.close()
    print(f"N{order} {form}: " + " ".join(f"{e:.2e}" for e in errs) + f" speed {abs(got_lam - lam) / lam:.2e}")


@cases
def test_heun_steps(order, form):
    mesh = FORMS[form][0]
    _, _, _, _, q, dt, per_node = problem4(mesh, order)
    with_array, with_scalar, t_end = reference(mesh, order, "heun")
    errs = []
    for sponge, tracer, ref in ((True, per_node, with_array), (False, N_SCALAR, with_scalar)):
        s = solver(order, form, tracer, sponge=sponge)
        s.setTime(T0)
        s.setState4(*q)
        s.stepSSPRK2(dt, 1, sponge=SPONGE_SCALAR)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)
        got = s.getState4()
        assert relmax(got[1], q[1]) > 1e-4 and relmax(got[3], q[3]) > 1e-5              # the state moved, the tracer too
        errs += assert_fields_close(got, ref, STATE_TOL, what=f"Heun, sponge {'array' if sponge else 'scalar'}")
        assert abs(s.getTime() - t_end) <= 1e-12 * t_end
        s.close()
    assert relmax(with_array[1], with_scalar[1]) > 1e-6                                 # the two sponges differ
    print(f"N{order} {form} heun: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_lserk4_stages(order, form):
    mesh = FORMS[form][0]
    _, _, _, _, q, dt, per_node = problem4(mesh, order)
    ref, t_end = reference(mesh, order, "lserk")
    s = solver(order, form, per_node)
    s.setTime(T0)
    s.setState4(*q)
    s.lserk4Stages(dt, 4)
    assert s.getTime() == T0                                                            # the tide is frozen inside a step
    s.lserk4Stages(dt, 3)
    errs = assert_fields_close(s.getState4(), ref, STATE_TOL, what="7 LSERK4 stages")
    assert abs(s.getTime() - t_end) <= 1e-12 * t_end and t_end > T0
    print(f"N{order} {form} lserk: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@cases
def test_rk2_filter_steps(order, form):
    mesh = FORMS[form][0]
    _, _, _, _, q, dt, _ = problem4(mesh, order)
    ref, t_end = reference(mesh, order, "rk2")
    s = solver(order, form, N_SCALAR)
    s.setTime(T0)
    s.setState4(*q)
    s.stepRK2(dt, 2, filter=True)
    errs = assert_fields_close(s.getState4(), ref, STATE_TOL, what="2 RK2 + filter steps")
    assert abs(s.getTime() - t_end) <= 1e-12 * t_end
    print(f"N{order} {form} rk2: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [2, 4, 9])
def test_a_uniform_concentration_stays_uniform_over_a_jumping_bed(order, form):
    """hN = c h, Nopen = c: hN - c h stays at rounding. Both hN and c h are stepped states held to STATE_TOL, so their
    difference is held to the two tolerances added."""
    mesh = FORMS[form][0]
    _, t, vb, _, q, dt, _ = problem4(mesh, order)
    c = 0.37
    H = vb["H"].ravel("F")
    assert np.abs(H[t["vmapM"]] - H[t["vmapP"]]).max() > 0.1 and abs(B.tide_value(T0, TIDE)) > 0.1
    s = solver(order, form, c)
    s.setTime(T0)
    s.setState4(q[0], q[1], q[2], c * q[0])
    s.stepSSPRK2(dt, 10, sponge=SPONGE_SCALAR)
    h, hu, _, hN = s.getState4()
    assert relmax(h, q[0]) > 1e-5 and relmax(hu, q[1]) > 1e-4
    dev = np.abs(hN - c * h).max() / np.abs(hN).max()
    print(f"N{order} {form}: max|hN - c h| / max|hN| {dev:.2e}")
    assert dev <= 2 * STATE_TOL
    s.close()


def test_tracer_mass_is_conserved_in_a_closed_basin():
    """Walls on every side of the sheared box (parallelograms), a jumping bed, N = 4, 20 Heun steps: the drift of int hN within
    the bound tests/test_sw2d_quads_monitor_gpu.py applies to int h, scaled by int |hN| / int h."""
    nodes, t = Q.mesh_tables("shear", 4)
    assert t["mapW"].size == 2 * (Q.NX + Q.NY) * 5
    x, y = t["x"], t["y"]
    H = B.jumping_bed(t, 10.0, 1.0, seed=4)
    Hx, Hy = nodes.bedSlopes(H)
    h = H + 0.3 * np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    q = [h, 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1), h * (0.5 + 0.4 * np.sin(2 * x) * np.cos(3 * y))]
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=B.G, fields=4)
    s.enableVariantB(H, Hx, Hy, CD=CD, f=FCOR, tide=TIDE, tracer=0.0)
    assert s.usesParallelogramGeometry
    s.enableMonitor(nodes, stride=1)
    s.setState4(*q)
    s.sampleMonitor()
    s.stepSSPRK2(2e-4, 20)
    rec = s.monitorRecords()
    assert rec["tracer"].shape == (21,) and rec["nan"].max() == 0
    w = nodes.quadratureWeights()
    mass, abs_tracer = (w * q[0]).sum(), (w * np.abs(q[3])).sum()
    assert abs(rec["tracer"][0] - (w * q[3]).sum()) <= 1e-13 * abs_tracer
    drift = np.abs(rec["tracer"] - rec["tracer"][0]).max() / mass
    bound = DRIFT_TOL * abs_tracer / mass
    print(f"tracer drift over 20 Heun steps: {drift:.2e} of the mass (bound {bound:.2e}); "
          f"mass drift {np.abs(rec['mass'] - rec['mass'][0]).max() / mass:.2e}")
    assert relmax(s.getState4()[3], q[3]) > 1e-6
    assert drift <= bound
    s.close()


def test_monitor_and_output_carry_the_tracer(tmp_path):
    order = 4
    nodes, t, vb, _, q, dt, per_node = problem4("jitter", order)
    Nq = order + 1
    r1d = nodes.dgContext().r[::Nq]
    rng = np.random.default_rng(order)
    el = rng.integers(0, 143, 5).astype(np.int32)
    j, i = rng.integers(0, Nq, 5), rng.integers(0, Nq, 5)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=B.G, fields=4)
    s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], mapO=vb["mapO"], CD=CD, f=FCOR, tide=TIDE, tracer=per_node)
    s.enableMonitor(nodes, gauges=(el, r1d[j], r1d[i]))              # no H: the variant-B solver's own
    s.setTime(T0)
    s.setState4(*q)
    s.stepSSPRK2(dt, 3, sponge=SPONGE_SCALAR)
    rec = s.monitorRecords()
    assert rec["tracer"].shape == (3,) and rec["t"][-1] == s.getTime()
    state = s.getState4()
    w = nodes.quadratureWeights()
    assert abs(rec["tracer"][-1] - (w * state[3]).sum()) <= 1e-13 * (w * np.abs(state[3])).sum()
    out = s.outputFields(H=vb["H"], lattice=False)
    g = rec["gauges"][-1]
    for c in range(4):
        assert np.array_equal(g[:, c], out[c][Nq * j + i, el]), f"field {c}"
    assert np.array_equal(out[3], state[3] / state[0])
    paths = dg.VtkOutputter(nodes).writeSolverFields(s, 3, directory=str(tmp_path), H=vb["H"])
    assert [os.path.basename(p) for p in paths] == [f"{n}0000003.vtu" for n in ("eta", "u", "v", "N")]
    assert all(os.path.getsize(p) > 1000 for p in paths)
    s.close()


def test_mesh_smaller_than_a_tile():
    """A 3 x 1 box at N = 1: K = 3 < E = 64."""
    E, V = quadref.quad_box(3, 1)
    nodes, t, _ = B.open_box(E, V.astype(np.float64), 1)
    x, y = t["x"], t["y"]
    H = B.jumping_bed(t, 10.0, 1.0)
    Hx, Hy = nodes.bedSlopes(H)
    per_node = B4.open_tracer(t)
    vb = {"g": B.G, "H": H, "Hx": Hx, "Hy": Hy, "mapO": t["mapO"], "CD": CD, "f": FCOR, "tide": TIDE, "tracer": per_node}
    h = H + 0.2 * np.cos(x + y)
    q = [h, 2.0 * np.sin(2 * x + 1) + 0 * y, 1.5 * np.cos(x) * np.sin(2 * y - 1), h * (0.6 + 0.3 * np.sin(3 * x - y))]
    dt = compute_dt(*q[:3], B.G, t, Q.CFL)[0]
    tl, vl = Q.to_ld(t), B4.vb_ld(vb)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=B.G, fields=4)
    assert s.K == 3
    s.enableVariantB(H, Hx, Hy, mapO=t["mapO"], CD=CD, f=FCOR, tide=TIDE, tracer=per_node)
    s.setTime(T0)
    assert_fields_close(s.computeRHS4(*q), Q.f64(B4.rhsB4(*B.to_ld(q), tl, vl, time=T0)), RHS_TOL, what="RHS")
    s.setState4(*q)
    s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)
    ref, _ = B4.heun_steps(B.to_ld(q), tl, vl, dt, 2, time=T0, sponge_coeff=SPONGE_SCALAR)
    assert_fields_close(s.getState4(), Q.f64(ref), STATE_TOL, what="2 Heun steps")
    s.close()


def test_refusals_leave_the_solvers_usable():
    d4, _, nodes4, _ = quadref4.load_fixture4("jitter_box5x4_N2")
    z = np.zeros_like(d4["h"])
    q4, ref4 = quadref4.state(d4), quadref4.reference(d4)
    # tracer= on three fields
    d, _, nodes, _ = quadref.load_fixture("jitter_box5x4_N2")
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]))
    with pytest.raises(ValueError):
        s.enableVariantB(z + 10, z, z, tracer=0.5)
    one = np.ones(1)
    vbd = C.Sw2dVbDesc(C.ptr(z + 10), C.ptr(z), C.ptr(z), None, 0, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    assert C.lib.bdg_sw2dq_enable_variant_b4(s._h, C.byref(vbd), C.ptr(one), 1) == C.BDG_ERR_ARGUMENT
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), [d["rhs1"], d["rhs2"], d["rhs3"]], RHS_TOL, what="variant A")
    s.close()
    # after setSources
    s4 = sw2dquads.Sw2dQuadSolver(nodes=nodes4, g=float(d4["g"]), fields=4, sources=quadref4.sources(d4))
    with pytest.raises(C.BdgError) as e:
        s4.enableVariantB(z + 10, z, z, tracer=0.5)
    assert e.value.code == C.BDG_ERR_ARGUMENT
    # a wrong tracer length: ValueError before the library is called; a bad count and a NULL array through the C ABI
    mapO = np.arange(3, dtype=np.int32)
    for bad in (np.ones(2), np.ones(4), np.ones((3, 1))):
        with pytest.raises(ValueError):
            s4.enableVariantB(z + 10, z, z, mapO=mapO, tracer=bad)
    hb = z + 10
    vbd = C.Sw2dVbDesc(C.ptr(hb), C.ptr(z), C.ptr(z), C.ptr(mapO), 3, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    s5 = sw2dquads.Sw2dQuadSolver(nodes=nodes4, g=float(d4["g"]), fields=4)
    four = np.ones(4)
    for n_open, count in ((C.ptr(four), 2), (C.ptr(four), 4), (C.ptr(four), 0), (C.ptr(four), -1), (None, 1)):
        assert C.lib.bdg_sw2dq_enable_variant_b4(s5._h, C.byref(vbd), n_open, count) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2dq_enable_variant_b4(s5._h, None, C.ptr(four), 1) == C.BDG_ERR_ARGUMENT
    with pytest.raises(C.BdgError):
        s5.globalSpeed()                                                         # variant B was not enabled by any of these
    closed = C.Sw2dVbDesc(C.ptr(hb), C.ptr(z), C.ptr(z), None, 0, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    assert C.lib.bdg_sw2dq_enable_variant_b4(s5._h, C.byref(closed), None, 0) == 0   # no open node: nothing is read
    assert all(np.isfinite(a).all() for a in s5.computeRHS4(*q4))
    s5.close()
    assert_fields_close(s4.computeRHS4(*q4), ref4, RHS_TOL, what="four fields with sources, after the refusals")
    # after an evaluation
    with pytest.raises(C.BdgError) as e:
        s4.enableVariantB(z + 10, z, z, tracer=0.5)
    assert e.value.code == C.BDG_ERR_ARGUMENT
    s4.close()
    s6 = sw2dquads.Sw2dQuadSolver(nodes=nodes4, g=float(d4["g"]), fields=4)
    plain = s6.computeRHS4(*q4)
    with pytest.raises(C.BdgError) as e:
        s6.enableVariantB(z + 10, z, z, tracer=0.5)
    assert e.value.code == C.BDG_ERR_ARGUMENT
    again = s6.computeRHS4(*q4)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    # without tracer a four-field solver is refused by the library, as before; with it, set_sources is refused afterwards
    s7 = sw2dquads.Sw2dQuadSolver(nodes=nodes4, g=float(d4["g"]), fields=4)
    with pytest.raises(C.BdgError):
        s7.enableVariantB(z + 10, z, z)
    s7.enableVariantB(z + 10, z, z, tracer=0.5)
    with pytest.raises(C.BdgError):
        s7.setSources(**quadref4.sources(d4))
    for again in (0.25, np.full(3, 0.25)):                                       # a second call, scalar or per node: refused
        with pytest.raises(C.BdgError) as e:
            s7.enableVariantB(z + 10, z, z, mapO=mapO if np.ndim(again) else None, tracer=again)
        assert e.value.code == C.BDG_ERR_ARGUMENT
    assert all(np.isfinite(a).all() for a in s7.computeRHS4(*q4))
    s6.close()
    s7.close()
