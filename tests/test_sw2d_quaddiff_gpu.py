"""Diffusion, sources and decay of the tracer on the quadrilateral solver (bdg_sw2dq_enable_tracer_diffusion, the two passes of
csrc/hip/sw2d_quad_diffusion_kernel.hpp behind every evaluation's stage launch) against tests/quaddiff_ref.py -- the definition
of tests/tridiff_ref.py over quadref4.rhs4 and quadrefB4.rhsB4 -- in np.longdouble, rounded at the comparison.

Orders 1 to 12 on the three forms of test_sw2d_quadsB_gpu.FORMS (the sheared 13 x 11 box in the parallelogram and in the per-node
form, the jittered one), K = 143: ragged against tiles of 64, 32, 16 and 8; the meshes are shuffled and rotated, so the gathers
are not trivial. Three kinds of four-field solver: "Asrc" (variant A with bed slope, Coriolis and drag; kappa plane, S, k), "A"
(variant A without sources; a scalar kappa alone, so the path without S and k runs) and "B" (variant B with a per-node open-
boundary tracer at T0; kappa plane, S, k). Per (order, form):

  test_rhs              computeRHS4 and its filtered form on the three kinds: component 4 against advective reference + T
                        (+ Filter T), RHS_TOL of max|field|; components 1-3 and B's globalSpeed() BIT FOR BIT those of the
                        same solver without diffusion
  test_lserk4_stages    7 stages as 4 + 3 on Asrc and B                                      STATE_TOL
  test_rk2_filter_steps 2 midpoint-RK2 + filter steps on A and B                             STATE_TOL
  test_heun_steps       3 Heun steps with the sponge array on B                              STATE_TOL
  test_tracer_mass      5 unfiltered RK2 steps in the closed basin, from the monitor's int hN: constant with S = k = 0, growing
                        by dt sum(w S) per step with a source, within DRIFT_TOL of int |hN| (test_sw2d_quads_monitor_gpu's
                        bound, scaled as test_sw2d_quadsB4_gpu scales it); not on the jittered form at N = 1, where the
                        definition itself does not conserve (tests/test_quaddiff_reference.py)

with dt = min(the problem's dt, diffusionDt() / 2); then meshes smaller than a tile (a 2 x 2 box at N = 1 and N = 9), the step
size, device bytes and the refusals. Tolerances are the project's: one evaluation 1e-12 of max|field|, stepped states 1e-11
(tests/test_quaddiff_reference.py: the float64 definition is within 4.2e-15 of max|T| of the longdouble one). References are
computed once per (order, mesh) and shared by the geometry forms.

Measured on one MI355X: largest error of component 4 of one evaluation 2.3e-13 of max|field| (N = 12, parallelogram form), per-
node forms at most 3.5e-15 (N = 8, jitter); largest state error 7.4e-14 (N = 12, parallelogram form, three Heun steps; LSERK4
3.8e-14, RK2 + filter 2.4e-14), per-node forms at most 3.7e-14 (N = 4, LSERK4); drift of int hN in the closed basin 2.1e-16,
deviation from the source's rate 3.9e-16 of int |hN| (DRIFT_TOL is 2.1e-15); 184 tests in 65 s, most of it the longdouble
references (tracer diffusion)."""
import numpy as np
import pytest

import quaddiff_ref as QD
import quadref_ld as Q
import quadrefB as B
import tridiff_ref as R
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2dquads
from conftest import relmax
from regimes import assert_fields_close
from test_sw2d_quads_monitor_gpu import DRIFT_TOL
from test_sw2d_quadsB_gpu import CD, FCOR, FORMS, SPONGE_SCALAR, T0, TIDE

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
ORDERS = tuple(range(1, 13))
KINDS = ("Asrc", "A", "B")

cases = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

_REF = {}


def inputs(kind, mesh, order):
    """(nodes, tables, state, dt, d) of a kind."""
    if kind == "B":
        nodes, t, _, _, q, dt, d = QD.inputs_b(mesh, order)
    else:
        nodes, t, q, _, dt, d = QD.inputs_a(mesh, order)
    return nodes, t, q, dt, d


def model(kind, mesh, order):
    """The longdouble model of a kind: "Asrc" and "B" with the kappa plane, S and k, "A" with the scalar kappa alone."""
    if kind == "B":
        _, t, vb, _, _, _, d = QD.inputs_b(mesh, order)
        return QD.model_b(Q.to_ld(t), vb, d["kappa_field"], d["source"], d["decay"])
    _, t, _, src, _, d = QD.inputs_a(mesh, order)
    if kind == "A":
        return QD.model_a(Q.to_ld(t), d["kappa"])
    return QD.model_a(Q.to_ld(t), d["kappa_field"], d["source"], d["decay"], src=src)


def solver(kind, order, form, diffusion=True, sponge=False):
    mesh, general = FORMS[form]
    flags = sw2dquads.GENERAL_GEOMETRY if general else 0
    if kind == "B":
        _, t, vb, sp, _, _, d = QD.inputs_b(mesh, order)
        s = sw2dquads.Sw2dQuadSolver(tables=t, g=B.G, flags=flags, fields=4)
        s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], mapO=vb["mapO"], CD=CD, f=FCOR, tide=TIDE, sponge=sp if sponge else None,
                         tracer=vb["tracer"])
        s.setTime(T0)
    else:
        nodes, t, _, src, _, d = QD.inputs_a(mesh, order)
        s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, flags=flags, fields=4, sources=src if kind == "Asrc" else None)
    assert s.usesParallelogramGeometry == (form == "shear-auto") and s.K == 143
    if diffusion and kind == "A":
        s.enableTracerDiffusion(d["kappa"])
    elif diffusion:
        s.enableTracerDiffusion(d["kappa_field"], source=d["source"], decay=d["decay"])
    return s


def reference(what, kind, mesh, order):
    key = (what, kind, mesh, order)
    if key not in _REF:
        Q.require_extended_precision()
        _, _, q, dt, _ = inputs(kind, mesh, order)
        m, ql = model(kind, mesh, order), B.to_ld(q)
        if what == "rhs":
            adv = m.adv(ql, T0)
            T, FT = m.term(ql), m.term(ql, True)
            plain = list(adv[:3]) + [adv[3] + T]
            filtered = [m.t["Filter"] @ a for a in adv[:3]] + [m.t["Filter"] @ adv[3] + FT]
            _REF[key] = (Q.f64(plain), Q.f64(filtered), float(np.abs(T).max()), float(np.abs(adv[3]).max()))
        elif what == "lserk":
            a, ta = QD.lserk4_stages(m, ql, dt, 7, time=T0)
            _REF[key] = (Q.f64(a), ta)
        elif what == "rk2":
            a, ta = QD.rk2_steps(m, ql, dt, 2, time=T0, filt=True)
            _REF[key] = (Q.f64(a), ta)
        else:
            sp = np.asarray(QD.inputs_b(mesh, order)[3], dtype=R.LD)
            a, ta = QD.heun_steps(m, ql, dt, 3, time=T0, sponge=sp)
            _REF[key] = (Q.f64(a), ta)
        assert all(np.isfinite(a).all() for a in _REF[key][0])
    return _REF[key]


def rhs_checks(kind, order, form):
    mesh = FORMS[form][0]
    q = inputs(kind, mesh, order)[2]
    plain, filtered, tmax, advmax = reference("rhs", kind, mesh, order)
    assert tmax > 1e-3 * advmax                                                      # the term is no rounding of the sum
    s = solver(kind, order, form)
    got = s.computeRHS4(*q)
    lam = s.globalSpeed() if kind == "B" else None
    got_f = s.computeRHS4(*q, filter=True)
    s.close()
    errs = assert_fields_close(got[3:], plain[3:], RHS_TOL, what=f"{kind} RHS4")
    errs += assert_fields_close(got_f[3:], filtered[3:], RHS_TOL, what=f"{kind} Filter . RHS4")
    assert_fields_close(got[:3], plain[:3], RHS_TOL, what=f"{kind} RHS1-3")
    off = solver(kind, order, form, diffusion=False)
    for a, b in zip(got[:3], off.computeRHS4(*q)[:3]):
        assert np.array_equal(a, b)                                                  # planes 0-2 are the solver's without diffusion
    if kind == "B":
        assert lam == off.globalSpeed()
    without = off.computeRHS4(*q, filter=True)
    for a, b in zip(got_f[:3], without[:3]):
        assert np.array_equal(a, b)
    assert relmax(got_f[3], without[3]) > 1e-6                                       # ... and plane 3 is not
    off.close()
    return errs


@cases
def test_rhs(order, form):
    errs = [e for kind in KINDS for e in rhs_checks(kind, order, form)]
    print(f"N{order} {form}: " + " ".join(f"{e:.2e}" for e in errs))


def stepped(kind, order, form, what, run, sponge=False):
    mesh = FORMS[form][0]
    _, _, q, dt, d = inputs(kind, mesh, order)
    ref, t_end = reference(what, kind, mesh, order)
    s = solver(kind, order, form, sponge=sponge)
    assert dt <= 0.5 * s.diffusionDt() * (1 + 1e-12) or kind == "A"                  # ("A" diffuses with the smaller scalar kappa)
    s.setState4(*q)
    run(s, dt)
    got = s.getState4()
    assert relmax(got[1], q[1]) > 1e-6 and relmax(got[3], q[3]) > 1e-6              # the state moved, the tracer too
    errs = assert_fields_close(got, ref, STATE_TOL, what=f"{kind} {what}")
    if kind == "B":
        assert abs(s.getTime() - t_end) <= 1e-12 * t_end
    s.close()
    return errs


@cases
def test_lserk4_stages(order, form):
    def run(s, dt):
        s.lserk4Stages(dt, 4)
        s.lserk4Stages(dt, 3)

    errs = [e for kind in ("Asrc", "B") for e in stepped(kind, order, form, "lserk", run)]
    print(f"N{order} {form} lserk: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_rk2_filter_steps(order, form):
    errs = [e for kind in ("A", "B") for e in stepped(kind, order, form, "rk2", lambda s, dt: s.stepRK2(dt, 2, filter=True))]
    print(f"N{order} {form} rk2: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_heun_steps(order, form):
    def run(s, dt):
        s.stepSSPRK2(dt, 1, sponge=SPONGE_SCALAR)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)

    errs = stepped("B", order, form, "heun", run, sponge=True)
    print(f"N{order} {form} heun: " + " ".join(f"{e:.2e}" for e in errs))


@pytest.mark.parametrize("order", (1, 9))
def test_mesh_smaller_than_a_tile(order):
    """A 2 x 2 box: K = 4 < 64 (N = 1) and < 8 (N = 9). One evaluation, plain and filtered, and 7 LSERK4 stages."""
    Q.require_extended_precision()
    nodes, t = QD.small_box(order)
    assert t["x"].shape[1] == 4
    q = Q.state(t, 4, "smooth", order)
    d = QD.diffusion_inputs(t)
    dt = QD.step_size(QD.quadref4.compute_dt(*q[:3], Q.G, t, Q.CFL)[0], order, t, d)
    m, ql = QD.model_a(Q.to_ld(t), d["kappa_field"], d["source"], d["decay"]), B.to_ld(q)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
    s.enableTracerDiffusion(d["kappa_field"], source=d["source"], decay=d["decay"])
    assert_fields_close(s.computeRHS4(*q), Q.f64(m.evaluate(ql, 0.0)), RHS_TOL, what="RHS")
    assert_fields_close(s.computeRHS4(*q, filter=True), Q.f64(m.evaluate(ql, 0.0, True)), RHS_TOL, what="Filter . RHS")
    s.setState4(*q)
    s.lserk4Stages(dt, 7)
    ref, _ = QD.lserk4_stages(m, ql, dt, 7)
    assert_fields_close(s.getState4(), Q.f64(ref), STATE_TOL, what="7 LSERK4 stages")
    s.close()


def _monitored(order, form, source, steps=5):
    mesh, general = FORMS[form]
    nodes, t, q, _, dt, d = QD.inputs_a(mesh, order)
    assert t["mapW"].size == 2 * (Q.NX + Q.NY) * (order + 1)                            # walls on every side
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=4)
    s.enableTracerDiffusion(d["kappa_field"], source=source)
    s.enableMonitor(nodes, stride=1, capacity=steps + 1)
    s.setState4(*q)
    s.sampleMonitor()
    s.stepRK2(dt, steps, filter=False)
    rec = s.monitorRecords()
    moved = relmax(s.getState4()[3], q[3])
    s.close()
    assert rec["tracer"].shape == (steps + 1,) and rec["nan"].max() == 0 and moved > 1e-6
    w = np.asarray(nodes.quadratureWeights())
    return rec["tracer"], w, dt, (w * np.abs(q[3])).sum()


MASS_CASES = [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS if not (f == "jitter" and n == 1)]


@pytest.mark.parametrize("order,form", MASS_CASES)
def test_tracer_mass(order, form):
    """S = k = 0: int hN is constant; S != 0, k = 0: it grows by dt sum(w S) per step. Both within DRIFT_TOL of int |hN|."""
    mass, _, _, scale = _monitored(order, form, None)
    drift = np.abs(mass - mass[0]).max() / scale
    S = 50.0 * QD.inputs_a(FORMS[form][0], order)[5]["source"]
    fed, w, dt, _ = _monitored(order, form, S)
    rate = dt * (w * S).sum()
    dev = np.abs(np.diff(fed) - rate).max() / scale
    print(f"N{order} {form}: drift of int hN over 5 steps {drift:.2e}; growth per step {rate / scale:.3e}, largest deviation {dev:.2e} of int |hN|")
    assert rate > 100 * DRIFT_TOL * scale                                               # far above the tolerance
    assert drift <= DRIFT_TOL
    assert dev <= DRIFT_TOL


def test_step_size():
    order = 4
    nodes, t, q, _, _, _ = QD.inputs_a("jitter", order)
    cfl = 0.75
    plain = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
    plain.setState4(*q)
    advective_dt, speed = plain.computeDt(cfl)
    with pytest.raises(C.BdgError):
        plain.diffusionDt()                                                             # no diffusion: refused
    plain.close()
    fs = np.abs(t["Fscale"]).max()
    plane = 5.0 * np.ones_like(q[0])
    plane[3, 7] = 6.0                                                                   # kappa_max of a plane
    for kappa, bound in ((1e-6, False), (5.0, True), (plane, True), (0.0, False)):
        s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
        s.enableTracerDiffusion(kappa)
        s.setState4(*q)
        kmax = float(np.max(kappa))
        want = R.DT_CONSTANT / (kmax * (order + 1) ** 4 * fs ** 2) if kmax > 0 else np.inf
        assert s.diffusionDt() == pytest.approx(want, rel=1e-14) and want == (R.diffusion_dt(R.DT_CONSTANT, kmax, order, t) if kmax else np.inf)
        dt, sp = s.computeDt(cfl)
        assert sp == speed
        assert (cfl * want < advective_dt) == bound
        assert dt == (cfl * s.diffusionDt() if bound else advective_dt)                 # bit for bit the advective value otherwise
        s.close()


def test_device_bytes():
    order = 4
    _, t, _, _, _, d = QD.inputs_a("shear", order)
    Np, K = t["x"].shape
    plane = Np * ((K + 63) // 64 * 64) * 8
    off = solver("A", order, "shear-auto", diffusion=False)
    scalar = solver("A", order, "shear-auto")
    full = solver("Asrc", order, "shear-auto")
    full_off = solver("Asrc", order, "shear-auto", diffusion=False)
    assert scalar.deviceBytes - off.deviceBytes == 2 * plane                            # the two flux planes
    assert full.deviceBytes - full_off.deviceBytes == 4 * plane                         # ... and the planes of kappa and S
    for s in (off, scalar, full, full_off):
        s.close()


def test_refusals_leave_the_solvers_usable():
    order = 2
    nodes, t, q, _, _, d = QD.inputs_a("jitter", order)
    E = C.BDG_ERR_ARGUMENT
    desc = lambda kappa=0.1, field=None, source=None, decay=0.0: C.Sw2dDiffusionDesc(kappa, C.ptr(field), C.ptr(source), decay)
    enable = lambda s, dd: C.lib.bdg_sw2dq_enable_tracer_diffusion(s._h, C.byref(dd))
    # three fields: ValueError from Python, BDG_ERR_ARGUMENT from the library; the solver goes on as it was
    s3 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G)
    before3 = s3.computeRHS(*q[:3])
    with pytest.raises(ValueError):
        s3.enableTracerDiffusion(0.1)
    assert enable(s3, desc()) == E and b"bdg_sw2dq_enable_tracer_diffusion" in C.lib.bdg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(before3, s3.computeRHS(*q[:3])))
    s3.close()
    # the undiffused right-hand side of a four-field solver
    s0 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
    undiffused = s0.computeRHS4(*q)
    s0.close()
    # bad numbers on a live four-field handle: none of them enables anything, and the solver still evaluates its undiffused RHS
    bad_field = d["kappa_field"].copy()
    bad_field[1, 5] = -1e-3
    nan_field = d["kappa_field"].copy()
    nan_field[0, 0] = np.nan
    inf_source = d["source"].copy()
    inf_source[0, 3] = np.inf
    neg_source = d["source"].copy()
    neg_source[2, 1] = -1e-3
    for dd in (desc(-0.1), desc(np.nan), desc(np.inf), desc(field=bad_field), desc(field=nan_field), desc(decay=-1.0),
               desc(decay=np.nan), desc(decay=np.inf), desc(source=inf_source), desc(source=neg_source), None):
        s4 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
        bytes_before = s4.deviceBytes
        assert C.lib.bdg_sw2dq_enable_tracer_diffusion(s4._h, C.byref(dd) if dd is not None else None) == E
        assert s4.deviceBytes == bytes_before
        assert all(np.array_equal(a, b) for a, b in zip(undiffused, s4.computeRHS4(*q)))      # after each: the undiffused RHS
        s4.close()
    s4 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
    for dd in (desc(-0.1), desc(field=nan_field), desc(source=neg_source)):                   # several on one live handle
        assert enable(s4, dd) == E
    for bad in (-0.1, np.nan):
        with pytest.raises(C.BdgError) as e:
            s4.enableTracerDiffusion(bad)
        assert e.value.code == E
    with pytest.raises(C.BdgError):
        s4.diffusionDt()                                                                # none of these enabled it
    assert all(np.array_equal(a, b) for a, b in zip(undiffused, s4.computeRHS4(*q)))
    # ... which was its first evaluation: refused from now on
    with pytest.raises(C.BdgError) as e:
        s4.enableTracerDiffusion(0.1)
    assert e.value.code == E and "first evaluation" in str(e.value)
    assert all(np.array_equal(a, b) for a, b in zip(undiffused, s4.computeRHS4(*q)))
    s4.close()
    # the right call goes through once; a second call and a partition are refused and change nothing
    s5 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
    s5.enableTracerDiffusion(d["kappa_field"], source=d["source"], decay=d["decay"])
    first = s5.computeRHS4(*q)
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], undiffused[:3])) and relmax(first[3], undiffused[3]) > 1e-6
    with pytest.raises(C.BdgError) as e:
        s5.enableTracerDiffusion(0.2)
    assert e.value.code == E
    K = t["x"].shape[1]
    assert C.lib.bdg_sw2dq_set_partition(s5._h, K, K, None, 0) == E and b"diffusion" in C.lib.bdg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(first, s5.computeRHS4(*q)))
    s5.close()
    # a solver with a partition set
    s6 = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=4)
    assert C.lib.bdg_sw2dq_set_partition(s6._h, K, K, None, 0) == 0
    with pytest.raises(C.BdgError) as e:
        s6.enableTracerDiffusion(0.1)
    assert e.value.code == E and "partition" in str(e.value)
    assert all(np.array_equal(a, b) for a, b in zip(undiffused, s6.computeRHS4(*q)))
    s6.close()
    # the partitioned front end says so itself (a Python-level check: no ranks)
    with pytest.raises(NotImplementedError, match="partitioned"):
        sw2dquads.NativeDistributedSw2dQuad.enable_tracer_diffusion(None, 0.1)
    with pytest.raises(NotImplementedError, match="partitioned"):
        sw2dquads.NativeDistributedSw2dQuad.enableTracerDiffusion(None, 0.1)
