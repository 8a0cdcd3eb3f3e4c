"""Variant B (the tidal driver's right-hand side, src/sw2d/main.cpp:279-484) on the quadrilateral solver against
tests/quadrefB.py in np.longdouble, rounded at the comparison.

The 13 x 11 box of the instance tests (K = 143: ragged last tiles of 64 / 32 / 16 / 8 elements), shuffled with rotated local
vertex order, sheared (both geometry forms) or jittered; the x = x_min side tagged Out, a bed that jumps at every face, drag,
Coriolis, an evaluation time where the tide is not zero. Orders 1 to 12, every one a compiled object of its own (register
allocation and all): every tile size, the rolled phase C (N >= 7) and the streamed filter (N > 8). Per (order, form):

  test_rhs_and_speed      RHS and Filter . RHS (RHS and filtered RHS instances), globalSpeed()        RHS_TOL per field / relative
  test_heun_steps         3 Heun steps with the sponge array, 3 with a scalar sponge (HEUN)            STATE_TOL
  test_lserk4_stages      7 stages as 4 + 3: frozen tide, time advanced after the fifth (LSERK)         STATE_TOL
  test_rk2_filter_steps   2 midpoint-RK2 + filter steps (filtered COMBINE)                             STATE_TOL

and the reference's own quadrilateral fixtures through the C ABI, still water over the jumping bed, a mesh smaller than a
tile, and the refusals. Tolerances are the project's: one RHS 1e-12 of max|field|, stepped states 1e-11.
References are computed once per (order, mesh) and shared by the geometry forms.

Measured on one MI355X: largest RHS error 4.0e-13, largest state error 6.9e-13 (Heun), both at N = 12 in the parallelogram form
(of the orders 3, 5, 6, 10, 11: RHS 2.3e-13 at N = 10, state 3.6e-13 at N = 11, Heun, the same form); per-node form at most
6.4e-14 (N = 12); global speed 1.6e-16 relative (N = 11); still water: max|hu| 9.7e-14, |h - H| 3.6e-15 at most; 164 tests in 27 s."""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadref
import quadref4
import quadref_ld as Q
import quadrefB as B
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2dquads
from conftest import relmax
from quadref4 import compute_dt
from regimes import assert_fields_close
from test_quadB_reference import QUAD_FIXTURES, fixture_vb, quad_fixture

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
FORMS = {"shear-auto": ("shear", False), "shear-general": ("shear", True), "jitter": ("jitter", True)}
ORDERS = tuple(range(1, 13))
TIDE, T0 = (0.5, 40.0, 0.05), 37.0
CD, FCOR = 2.5e-2, 0.1
SPONGE_SCALAR = 2.0

cases = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

_PROBLEM, _REF = {}, {}


def problem(mesh, order):
    """(nodes, tables, vb, sponge array, state, dt) on a mesh at an order; built once."""
    key = (mesh, order)
    if key not in _PROBLEM:
        nodes, t = B.mesh_tables(mesh, order)
        x, y = t["x"], t["y"]
        H = B.jumping_bed(t, 10.0, 1.0, seed=order)
        Hx, Hy = nodes.bedSlopes(H)
        vb = {"g": B.G, "H": H, "Hx": Hx, "Hy": Hy, "mapO": t["mapO"], "CD": CD, "f": FCOR, "tide": TIDE}
        sp = nodes.buildSpongeCoeff(t["mapO"], 5.0, 0.8)
        assert 0 < (sp > 0).sum() < sp.size
        h = H + 0.3 * np.exp(-4 * (x - 0.2) ** 2 - 4 * (y + 0.1) ** 2)
        q = [h, h * 0.6 * np.sin(2 * x + 1) * np.cos(y), h * 0.4 * np.cos(x) * np.sin(2 * y - 1)]
        dt = compute_dt(*q, B.G, t, Q.CFL)[0]
        _PROBLEM[key] = (nodes, t, vb, sp, q, dt)
    return _PROBLEM[key]


def solver(order, form, sponge=False):
    mesh, general = FORMS[form]
    _, t, vb, sp, _, _ = problem(mesh, order)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=B.G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], mapO=vb["mapO"], CD=CD, f=FCOR, tide=TIDE, sponge=sp if sponge else None)
    assert s.usesParallelogramGeometry == (form == "shear-auto") and s.K == 143
    return s


def reference(mesh, order, what):
    key = (mesh, order, what)
    if key not in _REF:
        Q.require_extended_precision()
        _, t, vb, sp, q, dt = problem(mesh, order)
        tl, vl, ql = Q.to_ld(t), B.vb_ld(vb), B.to_ld(q)
        if what == "rhs":
            r = B.rhsB(*ql, tl, vl, time=T0, return_speed=True)
            _REF[key] = (Q.f64(r[:3]), Q.f64([tl["Filter"] @ a for a in r[:3]]), float(r[3]))
        elif what == "heun":
            a, ta = B.heun_steps(ql, tl, vl, dt, 3, time=T0, sponge_coeff=np.asarray(sp, dtype=B.LD))
            b, _ = B.heun_steps(ql, tl, vl, dt, 3, time=T0, sponge_coeff=SPONGE_SCALAR)
            _REF[key] = (Q.f64(a), Q.f64(b), ta)
        elif what == "lserk":
            a, _, ta = B.lserk4_stages(ql, tl, vl, dt, 7, time=T0)
            _REF[key] = (Q.f64(a), ta)
        else:
            a, ta = B.rk2_steps(ql, tl, vl, dt, 2, time=T0, filt=True)
            _REF[key] = (Q.f64(a), ta)
    return _REF[key]


@cases
def test_rhs_and_speed(order, form):
    mesh = FORMS[form][0]
    q = problem(mesh, order)[4]
    plain, filtered, lam = reference(mesh, order, "rhs")
    assert abs(B.tide_value(T0, TIDE)) > 0.1
    s = solver(order, form)
    s.setTime(T0)
    errs = assert_fields_close(s.computeRHS(*q), plain, RHS_TOL, what="RHS")
    got_lam = s.globalSpeed()
    errs += assert_fields_close(s.computeRHS(*q, filter=True), filtered, RHS_TOL, what="Filter . RHS")
    print(f"N{order} {form}: " + " ".join(f"{e:.2e}" for e in errs) + f" speed {abs(got_lam - lam) / lam:.2e}")
    assert abs(got_lam - lam) <= RHS_TOL * lam
    assert s.getTime() == T0
    s.close()


@cases
def test_heun_steps(order, form):
    mesh = FORMS[form][0]
    _, _, _, _, q, dt = problem(mesh, order)
    with_array, with_scalar, t_end = reference(mesh, order, "heun")
    errs = []
    for sponge, ref in ((True, with_array), (False, with_scalar)):
        s = solver(order, form, sponge=sponge)
        s.setTime(T0)
        s.setState(*q)
        s.stepSSPRK2(dt, 1, sponge=SPONGE_SCALAR)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)
        got = s.getState()
        assert relmax(got[1], q[1]) > 1e-4                          # the state moved
        errs += assert_fields_close(got, ref, STATE_TOL, what=f"Heun, sponge {'array' if sponge else 'scalar'}")
        assert abs(s.getTime() - t_end) <= 1e-12 * t_end
        s.close()
    assert relmax(with_array[1], with_scalar[1]) > 1e-6             # the two sponges differ
    print(f"N{order} {form} heun: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_lserk4_stages(order, form):
    mesh = FORMS[form][0]
    _, _, _, _, q, dt = problem(mesh, order)
    ref, t_end = reference(mesh, order, "lserk")
    s = solver(order, form)
    s.setTime(T0)
    s.setState(*q)
    s.lserk4Stages(dt, 4)
    assert s.getTime() == T0                                        # the tide is frozen inside a step
    s.lserk4Stages(dt, 3)
    errs = assert_fields_close(s.getState(), ref, STATE_TOL, what="7 LSERK4 stages")
    assert abs(s.getTime() - t_end) <= 1e-12 * t_end and t_end > T0
    print(f"N{order} {form} lserk: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@cases
def test_rk2_filter_steps(order, form):
    mesh = FORMS[form][0]
    _, _, _, _, q, dt = problem(mesh, order)
    ref, t_end = reference(mesh, order, "rk2")
    s = solver(order, form)
    s.setTime(T0)
    s.setState(*q)
    s.stepRK2(dt, 2, filter=True)
    errs = assert_fields_close(s.getState(), ref, STATE_TOL, what="2 RK2 + filter steps")
    assert abs(s.getTime() - t_end) <= 1e-12 * t_end
    print(f"N{order} {form} rk2: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@pytest.mark.parametrize("name", QUAD_FIXTURES)
def test_reference_fixtures_through_the_c_abi(name):
    d, _, nodes = quad_fixture(name)
    vb = fixture_vb(d)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]))
    s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], CD=vb["CD"], f=vb["f"])
    got = s.computeRHS(d["h"], d["hu"], d["hv"])
    errs = assert_fields_close(got, [d["rhs1"], d["rhs2"], d["rhs3"]], RHS_TOL, what=name)
    print(name, " ".join(f"{e:.2e}" for e in errs))
    s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [1, 4, 9])
def test_still_water_over_a_jumping_bed_stays_at_rest(order, form):
    mesh, general = FORMS[form]
    nodes, t = B.mesh_tables(mesh, order)
    H = B.jumping_bed(t, 10.0, 2.0, flat=True)
    Hx, Hy = nodes.bedSlopes(H)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=B.G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    s.enableVariantB(H, Hx, Hy, mapO=t["mapO"], CD=CD, f=FCOR, tide=(0.0, 40.0, 0.05))     # an open side whose tide is zero
    zero = np.zeros_like(H)
    s.setState(H, zero, zero)
    dt = compute_dt(H, zero, zero, B.G, t, Q.CFL)[0]
    s.stepSSPRK2(dt, 20, sponge=SPONGE_SCALAR)
    h, hu, hv = s.getState()
    Hmax = H.max()
    print(f"N{order} {form}: max|hu| {np.abs(hu).max():.2e} max|hv| {np.abs(hv).max():.2e} max|h - H| {np.abs(h - H).max():.2e}")
    assert max(np.abs(hu).max(), np.abs(hv).max()) <= 1e-11 * np.sqrt(B.G * Hmax) * Hmax
    assert np.abs(h - H).max() <= 1e-12 * Hmax
    s.close()


def test_mesh_smaller_than_a_tile():
    """A 2 x 2 box at N = 1: K = 4 < E = 64."""
    E, V = quadref.quad_box(2)
    nodes, t, _ = B.open_box(E, V.astype(np.float64), 1)
    x, y = t["x"], t["y"]
    H = B.jumping_bed(t, 10.0, 1.0)
    Hx, Hy = nodes.bedSlopes(H)
    vb = {"g": B.G, "H": H, "Hx": Hx, "Hy": Hy, "mapO": t["mapO"], "CD": CD, "f": FCOR, "tide": TIDE}
    q = [H + 0.2 * np.cos(x + y), 2.0 * np.sin(2 * x + 1) + 0 * y, 1.5 * np.cos(x) * np.sin(2 * y - 1)]
    dt = compute_dt(*q, B.G, t, Q.CFL)[0]
    tl, vl = Q.to_ld(t), B.vb_ld(vb)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=B.G)
    assert s.K == 4
    s.enableVariantB(H, Hx, Hy, mapO=t["mapO"], CD=CD, f=FCOR, tide=TIDE)
    s.setTime(T0)
    assert_fields_close(s.computeRHS(*q), Q.f64(B.rhsB(*B.to_ld(q), tl, vl, time=T0)), RHS_TOL, what="RHS")
    s.setState(*q)
    s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)
    ref, _ = B.heun_steps(B.to_ld(q), tl, vl, dt, 2, time=T0, sponge_coeff=SPONGE_SCALAR)
    assert_fields_close(s.getState(), Q.f64(ref), STATE_TOL, what="2 Heun steps")
    s.close()


def test_refusals_leave_the_solvers_usable():
    # four fields: refused, and the solver still reproduces its variant-A fixture
    d4, _, nodes4, _ = quadref4.load_fixture4("jitter_box5x4_N2")
    s4 = sw2dquads.Sw2dQuadSolver(nodes=nodes4, g=float(d4["g"]), fields=4, sources=quadref4.sources(d4))
    z = np.zeros_like(d4["h"])
    with pytest.raises(C.BdgError) as e:
        s4.enableVariantB(z + 10, z, z)
    assert e.value.code == C.BDG_ERR_ARGUMENT
    assert_fields_close(s4.computeRHS4(*quadref4.state(d4)), quadref4.reference(d4), RHS_TOL, what="four fields")
    s4.close()
    # three fields: wrong shapes, a NULL descriptor, variant B without the Heun step's precondition, a late call
    d, _, nodes, _ = quadref.load_fixture("jitter_box5x4_N2")
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]))
    z = np.zeros_like(d["h"])
    with pytest.raises(ValueError):
        s.enableVariantB(z[:, :-1] + 10, z[:, :-1], z[:, :-1])
    with pytest.raises(ValueError):
        s.enableVariantB(z + 10, z, z, sponge=z[:-1])
    assert C.lib.bdg_sw2dq_enable_variant_b(s._h, None) == C.BDG_ERR_ARGUMENT
    with pytest.raises(C.BdgError):
        s.enableVariantB(z + 10, z, z, mapO=[4 * s.Nfp * s.K])                # an open-boundary node out of range
    with pytest.raises(C.BdgError):
        s.stepSSPRK2(1e-4)                                                    # variant B is not enabled
    with pytest.raises(C.BdgError):
        s.globalSpeed()
    ref = [d["rhs1"], d["rhs2"], d["rhs3"]]
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), ref, RHS_TOL, what="variant A")
    with pytest.raises(C.BdgError) as e:
        s.enableVariantB(z + 10, z, z)                                        # after the first evaluation
    assert e.value.code == C.BDG_ERR_ARGUMENT
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), ref, RHS_TOL, what="variant A after the refusal")
    t = ctypes.c_double()
    assert C.lib.bdg_sw2dq_get_time(s._h, None) == C.BDG_ERR_ARGUMENT and C.lib.bdg_sw2dq_get_time(s._h, ctypes.byref(t)) == 0
    s.close()
