"""Every quadrilateral stage-kernel instance against the np.longdouble reference (tests/quadref_ld.py).

sw2d_quad_order.hip compiles, per order, sw2d_quad_stage_kernel<N, MODE, FILT, GEN> ten times and
sw2d_quad4_stage_kernel<N, MODE, FILT, GEN, SRC> twenty times: (RHS, COMBINE) x filter x geometry form and LSERK x geometry form,
with four fields once more for sources on and off. Each has its own epilogue, LDS layout and unrolling (above N = 6 the
unfiltered phase C stays rolled, and with sources forms them there from a second read of the node). A wrong RK coefficient, a
filter on the wrong plane or two swapped metric slots conserve mass and keep every symmetry, so each instance is launched
here by an assertion against the reference, on meshes where no term of the geometry vanishes and no tile is full:

  form     shear-auto      oblique parallelograms (tests/quadref_ld.py), the solver picks the parallelogram form  GEN = false
           shear-general   the same mesh with GENERAL_GEOMETRY                                                    GEN = true
           jitter          general bilinear quadrilaterals                                                        GEN = true
  fields   3 | 4 (tracer, SRC = false) | 4src (tracer, Coriolis array, drag, bed slopes: SRC = true)
  order    1 .. 8; K = 143: 3, 5, 9 tiles of 64, 32, 16 elements, the last of 15 (k0 > 0 and the ragged tile)

  instance (per order, form, fields)   test
  RHS, plain and filtered              test_rhs_in_every_regime (computeRHS[4], filter False / True, four regimes)
  COMBINE, plain and filtered          test_midpoint_rk2_steps (3 steps as 1 + 2, filter False / True), test_jumpy_state
  LSERK                                test_lserk4_stages (8 + 5 stages, setState, 7 more), test_jumpy_state
so that test id [N-form-fields] of these three covers the ten (twenty) instances of that order, form and field set, and the
8 x 3 x 3 ids cover all 240; test_geometry_forms_agree_on_parallelograms holds GEN = false to GEN = true directly in every
mode, test_scalar_coriolis runs the fconst branch of the sources, test_compute_dt holds computeDt.

Step sizes come from quadref4.compute_dt on the host tables, not from the solver (the parallelogram form's computeDt carries
the 1e-10 face mean of Fscale). References are computed once per (order, mesh, fields) and shared by the forms.

Tolerances as tests/test_sw2d_quads_gpu.py: one RHS 1e-12 of max|RHS| per field, multi-step states 1e-11. Measured on one
MI355X: largest RHS error 9.0e-14 (N = 8, supercritical), largest state error 9.7e-14 (N = 8, LSERK4); 393 tests in 40 s.

Arithmetic-only edits tried against this module, one at a time, in a scratch build (first test that failed; unedited: all pass):
  sx and ry exchanged in phase C of the three-field GEN = false kernel     test_rhs_in_every_regime[N1-shear-auto-3]
  ny for nx in the F3 term of jt[2], four fields                            test_rhs_in_every_regime[N1-shear-auto-4]
  per-face lambda maximum stopped one node early, three fields              test_rhs_in_every_regime[N1-shear-auto-3]
  l0 for lN in the lift of face 2, four fields                              test_rhs_in_every_regime[N1-shear-auto-4]
  cb applied to v1 instead of the residual in LSERK, three fields           test_lserk4_stages[N1-shear-auto-3]
  filter on two of four planes in COMBINE                                   test_midpoint_rk2_steps[N1-shear-auto-4]
  drag sign in RHS3 with SRC                                                test_rhs_in_every_regime[N1-shear-auto-4src]
  late source add to RHS3 dropped in the rolled branch (N >= 7, no filter)  test_rhs_in_every_regime[N7-shear-auto-4src]"""
import numpy as np
import pytest

import quadref_ld as Q
from blitzdg_amd import sw2dquads
from conftest import relmax
from quadref4 import compute_dt
from regimes import REGIMES, assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
FORMS = {"shear-auto": ("shear", False), "shear-general": ("shear", True), "jitter": ("jitter", True)}
ORDERS = range(1, 9)

cases = pytest.mark.parametrize("order,form,fs", [pytest.param(n, f, s, id=f"N{n}-{f}-{s}")
                                                  for n in ORDERS for f in FORMS for s in Q.FIELD_SETS])


def _solver(order, form, fs, scalar_f=False):
    mesh, general = FORMS[form]
    nodes, t = Q.mesh_tables(mesh, order)
    fields, src = Q.field_set(t, fs, scalar_f)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=Q.G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=fields,
                                 sources=src)
    assert s.usesParallelogramGeometry == (form == "shear-auto")
    assert s.K == 143 and s.K % {1: 64, 2: 32}.get(order, 16) == 15
    return s, t


def _set(s, q):
    (s.setState4 if len(q) == 4 else s.setState)(*q)


def _get(s):
    return s.getState4() if s.fields == 4 else s.getState()


def _rhs(s, q, filt):
    return (s.computeRHS4 if len(q) == 4 else s.computeRHS)(*q, filter=filt)


_REF = {}


def _reference(order, mesh, fs, what):
    """Longdouble results on (order, mesh, fields), rounded to float64; each group computed once and shared by the forms."""
    key = (order, mesh, fs, what)
    if key in _REF:
        return _REF[key]
    _, t = Q.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    fields, src = Q.field_set(t, fs)
    r = {}
    if what == "rhs":
        for regime in REGIMES:
            q = r["q", regime] = Q.state(t, fields, regime, seed=order)
            for filt in (False, True):
                r[regime, filt] = Q.f64(Q.rhs_ld(q, Q.G, tl, src, filt))
    else:
        q0 = r["q0"] = Q.state(t, fields, "smooth", seed=order)
        r["dt"] = dt = compute_dt(*q0[:3], Q.G, t, Q.CFL)[0]
        if what == "rk2":
            for filt in (False, True):
                r[filt] = Q.f64(Q.rk2_steps(q0, Q.G, tl, dt, 3, filt, src))
        elif what == "lserk":
            r["q1"] = Q.state(t, fields, "smooth", seed=order + 100)
            r[13] = Q.f64(Q.lserk4_stages(q0, Q.G, tl, dt, 13, src))
            r[7] = Q.f64(Q.lserk4_stages(r["q1"], Q.G, tl, dt, 7, src))     # after setState: stage 0, residual zero
        else:
            assert what == "jumpy"
            qj = r["qj"] = Q.state(t, fields, "jumpy", seed=order)
            dtj = r["dtj"] = 0.25 * compute_dt(*qj[:3], Q.G, t, Q.CFL)[0]
            r["rk2"] = Q.f64(Q.rk2_steps(qj, Q.G, tl, dtj, 1, True, src))
            r["lserk"] = Q.f64(Q.lserk4_stages(qj, Q.G, tl, dtj, 4, src))
            for k in ("rk2", "lserk"):
                assert r[k][0].min() > 0
    _REF[key] = r
    return r


@cases
def test_rhs_in_every_regime(order, form, fs):
    """RHS and Filter . RHS on the four regimes of tests/regimes.py (contrast: single evaluations only, as on triangles)."""
    s, _ = _solver(order, form, fs)
    r = _reference(order, FORMS[form][0], fs, "rhs")
    for regime in REGIMES:
        for filt in (False, True):
            got = _rhs(s, r["q", regime], filt)
            errs = assert_fields_close(got, r[regime, filt], RHS_TOL, what=f"{regime} filter={filt}")
            print(f"N{order} {form} {fs} {regime} filter={filt}: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@cases
def test_midpoint_rk2_steps(order, form, fs):
    """3 steps of the script's midpoint RK2 on the smooth state, given as 1 + 2, with and without the filter."""
    s, _ = _solver(order, form, fs)
    r = _reference(order, FORMS[form][0], fs, "rk2")
    for filt in (True, False):
        _set(s, r["q0"])
        s.stepRK2(r["dt"], 1, filter=filt)
        s.stepRK2(r["dt"], 2, filter=filt)
        got = _get(s)
        assert relmax(got[0], r["q0"][0]) > 1e-6                # the state moved
        errs = assert_fields_close(got, r[filt], STATE_TOL, what=f"RK2 filter={filt}")
        print(f"N{order} {form} {fs} rk2 filter={filt}: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@cases
def test_lserk4_stages(order, form, fs):
    """13 stages given as 8 + 5 (the residual and the stage index carry over the calls), then setState part-way through a step
    (stage 0 again, residual zero) and 7 more."""
    s, _ = _solver(order, form, fs)
    r = _reference(order, FORMS[form][0], fs, "lserk")
    _set(s, r["q0"])
    s.lserk4Stages(r["dt"], 8)
    s.lserk4Stages(r["dt"], 5)
    errs = assert_fields_close(_get(s), r[13], STATE_TOL, what="13 LSERK4 stages")
    _set(s, r["q1"])
    s.lserk4Stages(r["dt"], 7)
    errs += assert_fields_close(_get(s), r[7], STATE_TOL, what="7 LSERK4 stages after setState")
    print(f"N{order} {form} {fs} lserk: " + " ".join(f"{e:.2e}" for e in errs))
    s.close()


@cases
def test_jumpy_state(order, form, fs):
    """A depth that jumps at every face: one RK2 + filter step and 4 LSERK4 stages at a quarter of the CFL step."""
    s, _ = _solver(order, form, fs)
    r = _reference(order, FORMS[form][0], fs, "jumpy")
    qj, dtj = r["qj"], r["dtj"]
    for name, run in (("rk2", lambda: s.stepRK2(dtj, 1, filter=True)), ("lserk", lambda: s.lserk4Stages(dtj, 4))):
        _set(s, qj)
        run()
        got = _get(s)
        assert got[0].min() > 0
        assert relmax(got[1], qj[1]) > 1e-3                      # the state moved
        assert_fields_close(got, r[name], STATE_TOL, what=f"jumpy {name}")
    s.close()


@cases
def test_compute_dt(order, form, fs):
    """As test_sw2d_quads4_gpu.test_compute_dt_matches_numpy_formula: the per-node tables to 1 ulp, the parallelogram form
    within the 1e-10 of its face mean."""
    s, t = _solver(order, form, fs)
    fields, _ = Q.field_set(t, fs)
    for kind in ("smooth", "jumpy", "supercritical"):
        q = Q.state(t, fields, kind, seed=order)
        _set(s, q)
        dt, speed = s.computeDt(Q.CFL)
        want_dt, want_speed = compute_dt(*q[:3], Q.G, t, Q.CFL)
        if FORMS[form][1]:
            assert abs(speed - want_speed) <= np.spacing(want_speed) and abs(dt - want_dt) <= np.spacing(want_dt)
        else:
            assert abs(speed - want_speed) <= 1e-10 * want_speed + np.spacing(want_speed)
            assert abs(dt - want_dt) <= 1e-10 * want_dt + np.spacing(want_dt)
    s.close()


@pytest.mark.parametrize("fs", Q.FIELD_SETS)
@pytest.mark.parametrize("order", ORDERS)
def test_geometry_forms_agree_on_parallelograms(order, fs):
    """On the shear mesh the 16 constants per element and the per-node tables describe the same geometry (to 1e-11, which
    tests/test_quad_reference_ld.py holds): both forms give the same RHS, RK2 step and LSERK4 stages."""
    a, t = _solver(order, "shear-auto", fs)
    b, _ = _solver(order, "shear-general", fs)
    fields, _ = Q.field_set(t, fs)
    q = Q.state(t, fields, "jumpy", seed=order + 7)
    dt = 0.25 * compute_dt(*q[:3], Q.G, t, Q.CFL)[0]
    for filt in (False, True):
        assert_fields_close(_rhs(a, q, filt), _rhs(b, q, filt), RHS_TOL, what=f"RHS filter={filt}")
        for s in (a, b):
            _set(s, q)
            s.stepRK2(dt, 1, filter=filt)
        assert_fields_close(_get(a), _get(b), RHS_TOL, what=f"RK2 filter={filt}")
    for s in (a, b):
        _set(s, q)
        s.lserk4Stages(dt, 6)
    assert_fields_close(_get(a), _get(b), RHS_TOL, what="LSERK4")
    a.close()
    b.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [2, 5, 8])
def test_scalar_coriolis(order, form):
    """Sources with a scalar f (the fconst branch of sources4): RHS, Filter . RHS and two unfiltered RK2 steps."""
    s, t = _solver(order, form, "4src", scalar_f=True)
    tl = Q.to_ld(t)
    src = Q.sources(t, scalar_f=True)
    q = Q.state(t, 4, "jumpy", seed=order + 3)
    for filt in (False, True):
        assert_fields_close(_rhs(s, q, filt), Q.f64(Q.rhs_ld(q, Q.G, tl, src, filt)), RHS_TOL, what=f"filter={filt}")
    dt = 0.25 * compute_dt(*q[:3], Q.G, t, Q.CFL)[0]
    _set(s, q)
    s.stepRK2(dt, 2, filter=False)
    assert_fields_close(_get(s), Q.f64(Q.rk2_steps(q, Q.G, tl, dt, 2, False, src)), STATE_TOL, what="RK2")
    s.close()
